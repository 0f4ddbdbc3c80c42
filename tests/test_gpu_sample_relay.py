"""GPU: the sample relay (CGRT_GRID_SAMPLE_RELAY / CGRT_GRID_NO_SAMPLE_RELAY, sample_relay=True / False).

A tile-order launch of a glass sphere scene renders the tiles some primary ray of which may meet a refracting sphere by K
workgroups, each with a chunk of the samples; chunks >= 1 park their Hitpoint values in the handle's relay area and the last
workgroup of a tile to finish adds them to chunk 0's sums in chunk order -- the additions of the unsplit loop in their order.
So every launch here is rendered with the relay on and off in one process and compared bit for bit: rgb, per-pixel nhit, rays
(counter 0) and Hitpoints (counter 1).  CGRT_CNT_WAVE_ITERS is a measurement of the launch as it ran and differs by design."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32
from test_deep_trees_host import DEEP_SCENES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
SIZES = [(96, 40), (200, 117)]  # 15 tiles; neither a multiple of 32 nor of 8: tiles partly outside the image
CAMS = {"pinhole": scenes.cam_pinhole, "thin_lens": scenes.cam_dof}
CHUNKS = {32: 2, 48: 3, 64: 4, 70: 4}  # spp -> K (70: chunks of 18, the last one of 16)


def _launch(sc, W, H, spp, cam, depth, relay, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, depth, SEED, counters=cnt, sample_relay=relay, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy()[:2].copy()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "nhit", "rays and Hitpoints")):
        assert np.array_equal(x, y), "%s: %s differs between the relayed and the unrelayed launch" % (what, name)


def _both(sc, W, H, spp, cam, depth=5, k=None, relay=4, **kw):
    """The launch with the relay forced on (relay=4: up to four chunks, CHUNKS; True: the default two) and switched off:
    identical bits; the read-back says which was which.  Returns the relayed launch's results and what it relayed."""
    on = _launch(sc, W, H, spp, cam, depth, relay, **kw)
    did = sc.last_sample_relay()
    off = _launch(sc, W, H, spp, cam, depth, False, **kw)
    assert sc.last_sample_relay() == dict(tiles=0, chunks=0, parked_values=0), "sample_relay=False still relayed"
    k = (CHUNKS[spp] if relay == 4 else 2) if k is None else k
    if k > 1:
        assert did["tiles"] > 0 and did["chunks"] == k and did["parked_values"] > 0, did
    else:
        assert did == dict(tiles=0, chunks=0, parked_values=0), did
    _same(on, off, "%dx%d spp %d depth %d %r" % (W, H, spp, depth, kw))
    return on, did


def _vs_oracle(orc, objs, cam, W, H, spp, got, depth=5):
    rgb, nhit, cnt = got
    o = BackendScene(orc, objs)
    want = o.trace_grid(cam, W, H, spp, depth, SEED)
    o.close()
    assert int(cnt[0]) == want["nrays"]
    assert np.array_equal(nhit, want["nhit"])
    assert float(np.abs(rgb - to_acc32(want["acc_sum"], spp)).max()) <= 1e-6


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("lens", sorted(CAMS))
@pytest.mark.parametrize("W,H", SIZES)
def test_c2_relayed_equals_unrelayed(c2, orc, W, H, lens):
    cam = CAMS[lens]()
    for spp in sorted(CHUNKS):
        for depth in (2, 5):
            got, did = _both(c2, W, H, spp, cam, depth)
            order = c2.last_tile_order()
            assert did["tiles"] == int(order["plan"][2]), "the relayed tiles are classes 0 and 1"
            if spp == 32 and depth == 5 and (W, H) == SIZES[0]:
                _vs_oracle(orc, scenes.scene_c2(), cam, W, H, 32, got)
    _both(c2, W, H, 70, cam, 5, relay=True)  # the default: two chunks of 35
    _both(c2, W, H, 32, cam, 1, k=1)  # depth 1: no refracted ray, no glass variant, no relay
    _both(c2, W, H, 16, cam, 5, k=1)  # fewer than two chunks of 16 samples


@pytest.mark.parametrize("cam_name,cam", DEEP_SCENES[1][2], ids=[c[0] for c in DEEP_SCENES[1][2]])
def test_full_depth_trees(gpu_ready, cam_name, cam):
    """The camera inside a glass sphere (test_gpu_deep_trees' sphere scene): every tile is of class 0, more than a tenth of the
    rays hold three pending rays and reach the last level (test_deep_trees_host), so the PARK body's third stack level and its
    longest streams are in use.  What went through the area is exactly what chunk 1's samples produce, launched on their own."""
    import cgraytracing_amd as cg
    name, mk, _ = DEEP_SCENES[1]
    assert name == "inside_glass_c2"
    W, H, spp = 96, 40, 32
    with cg.Scene(mk()) as sc:
        assert "PAIR=1" in sc.kernel_variant(W, H, spp, cam, 5)
        (rgb, nhit, cnt), did = _both(sc, W, H, spp, cam)
        assert did["tiles"] == 15, "every tile looks through the sphere around the camera"
        tail = _launch(sc, W, H, 16, cam, 5, False, sample_offset=16, spp_total=spp)
        assert did["parked_values"] == int(tail[2][1]), "parked values are chunk 1's Hitpoints"
        assert int(nhit.max()) > spp, "no pixel with more than one Hitpoint a sample"


def test_a_tile_with_exactly_one_glass_pixel(c2):
    """The glass sphere's silhouette at 200x117, pinhole: the nearest-hit query over the frame's primary rays tells the pixels
    that look at the glass sphere (object 7).  Some 32x8 tile holds exactly one of them; it is relayed like the others -- one
    lane with a long stream, 255 with short ones -- and the frame keeps its bits."""
    W, H = SIZES[1]
    cam = scenes.cam_pinhole()
    assert scenes.scene_c2()[7].transparency > 0
    org, dirs, _ = c2.camera_rays(W, H, 1, cam, SEED)
    glass = (c2.trace_rays(org, dirs, want=("hit",))["hit_obj"].cpu().numpy() == 7).reshape(H, W)
    tx, ty = (W + 31) // 32, (H + 7) // 8
    per_tile = np.array([[int(glass[y * 8:(y + 1) * 8, x * 32:(x + 1) * 32].sum()) for x in range(tx)] for y in range(ty)])
    ones = [(y, x) for y in range(ty) for x in range(tx) if per_tile[y, x] == 1]
    assert ones, "no tile with exactly one glass pixel:\n%s" % per_tile
    _, did = _both(c2, W, H, 64, cam)
    order = c2.last_tile_order()
    relayed = set(int(t) for t in order["list"][:did["tiles"]])
    for y, x in ones:
        assert y * tx + x in relayed, "tile (%d, %d) with one glass pixel is not among the relayed tiles" % (x, y)


def test_striped_launch_and_progressive_passes(c2):
    import torch
    W, H = SIZES[1]
    cam = scenes.cam_dof()
    for rank in range(2):
        _both(c2, W, H, 32, cam, rows=64, stripe=(16, rank, 2))
    frames = []
    for relay in (True, False):
        out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        for k in range(2):
            _, nhit, _ = c2.trace_grid(W, H, 32, cam, 5, SEED, sample_offset=32 * k, spp_total=64, out=out, counters=cnt, accumulate=True,
                                       sample_relay=relay)
        torch.cuda.synchronize()
        assert (c2.last_sample_relay()["tiles"] > 0) == relay
        frames.append((out.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy()[:2].copy()))
    _same(frames[0], frames[1], "accumulate 2 x 32 samples")


def test_one_handle_many_launches(c2):
    """The arrival words are back at 0 after every launch, the area serves another K and another stream."""
    import torch
    W, H = SIZES[0]
    cam = scenes.cam_dof()
    want = {spp: _launch(c2, W, H, spp, cam, 5, False) for spp in (32, 64)}
    for _ in range(3):
        _same(_launch(c2, W, H, 64, cam, 5, True), want[64], "three relayed launches in a row")
    for relay in (False, True, False, True):
        _same(_launch(c2, W, H, 64, cam, 5, relay), want[64], "relay on and off alternating")
    for spp in (32, 64, 32):
        _same(_launch(c2, W, H, spp, cam, 5, 4), want[spp], "K changes between launches")
        assert c2.last_sample_relay()["chunks"] == CHUNKS[spp]
    # two launches on two streams, nothing between them: the second waits for the first's use of the area
    dev = torch.device("cuda")
    outs = []
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for st, spp in zip(streams, (64, 32)):
        cnt = torch.zeros(8, dtype=torch.int64, device=dev)
        with torch.cuda.stream(st):
            rgb, nhit, _ = c2.trace_grid(W, H, spp, cam, 5, SEED, counters=cnt, sample_relay=True, stream=st.cuda_stream)
        outs.append((spp, rgb, nhit, cnt))
    torch.cuda.synchronize()
    for spp, rgb, nhit, cnt in outs:
        _same((rgb.cpu().numpy(), nhit.cpu().numpy().view(np.uint32), cnt.cpu().numpy()[:2]), want[spp], "two streams, spp %d" % spp)


_CHILD = r"""
import sys
import numpy as np
import torch
import cgraytracing_amd as cg
import scenes
bound = int(sys.argv[1])
sc = cg.Scene(scenes.scene_c2())
cam = scenes.cam_dof()
res = []
for relay in (True, False):
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(96, 40, 32, cam, 5, 12345, counters=cnt, sample_relay=relay)
    torch.cuda.synchronize()
    res.append((rgb.cpu().numpy(), nhit.cpu().numpy(), cnt.cpu().numpy()[:2]))
    if relay:
        did = sc.last_sample_relay()
        special = int(sc.last_tile_order()["plan"][2])
for a, b in zip(*res):
    assert np.array_equal(a, b), "relayed and unrelayed launch differ"
assert special > bound, (special, bound)
assert did["tiles"] == bound and did["chunks"] == 2 and did["parked_values"] > 0, did
sc.close()
print("child ok", did)
"""


@pytest.mark.parametrize("bound", [1, 3])
def test_fewer_slots_than_tiles(gpu_ready, bound):
    """CGRT_RELAY_TILES bounds the area's capacity below the number of class-0 and class-1 tiles: the first `bound` entries are
    relayed, the others render unsplit; same bits.  The knob is read once per process, so a fresh interpreter."""
    env = dict(os.environ, CGRT_RELAY_TILES=str(bound))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.run([sys.executable, "-c", _CHILD, str(bound)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr


def test_the_gate(c2):
    """By default the relay needs 4 tiles per compute unit: 200x117 (105 tiles) goes unrelayed -- its CGRT_CNT_WAVE_ITERS is
    pinned elsewhere --, 1920x1080 (8100 tiles) is relayed and equals its unrelayed twin."""
    import torch
    cam = scenes.cam_dof()
    _launch(c2, 200, 117, 64, cam, 5, None)
    assert c2.last_sample_relay()["tiles"] == 0
    frames = []
    for relay in (None, False):
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        rgb, _, _ = c2.trace_grid(1920, 1080, 32, cam, 5, SEED, counters=cnt, nhit=False, sample_relay=relay)
        torch.cuda.synchronize()
        did = c2.last_sample_relay()
        assert (did["tiles"] > 0 and did["chunks"] == 2) if relay is None else did["tiles"] == 0, did
        frames.append((rgb, int(cnt[0].item())))
    assert torch.equal(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]
