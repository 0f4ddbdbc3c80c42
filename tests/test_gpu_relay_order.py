"""GPU: the sample relay's extent and launch order (relay_mirror / relay_order; CGRT_GRID_RELAY_MIRROR, the order field).

The mirror extent relays the class-2 tiles -- those that may see a reflecting sphere only -- as well as classes 0 and 1; the
order says where the class-2 workgroups start among the others.  Either is index arithmetic on workgroup-uniform values in
front of the same bodies, so every launch here is compared bit for bit with the unrelayed launch of the same process: rgb,
per-pixel nhit, rays (counter 0) and Hitpoints (counter 1).  The scene is C2, with sample_relay=True so that small frames relay.

The frame is 200x117: 105 tiles, neither a multiple of 32 nor of 8, and it has class-2 tiles for both cameras (asserted)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
W, H = 200, 117
CAMS = {"pinhole": scenes.cam_pinhole, "thin_lens": scenes.cam_dof}
ORDERS = ("chunks_first", "mirror_first", "interleaved")
FORMS = [(mirror, order) for mirror in (False, True) for order in ORDERS]
SPP = {32: True, 64: 4}  # samples -> sample_relay: two chunks of 16, four chunks of 16


def _launch(sc, spp, cam, depth, relay, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, depth, SEED, counters=cnt, sample_relay=relay, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy()[:2].copy()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "nhit", "rays and Hitpoints")):
        assert np.array_equal(x, y), "%s: %s differs between the relayed and the unrelayed launch" % (what, name)


def _form(sc, spp, cam, depth, relay, mirror, order, want, **kw):
    """One launch in the form (mirror, order): the unrelayed launch's bits (`want`), and the read-backs name what was asked."""
    got = _launch(sc, spp, cam, depth, relay, relay_mirror=mirror, relay_order=order, **kw)
    did, form, plan = sc.last_sample_relay(), sc.last_relay_form(), sc.last_tile_order()["plan"]
    what = "spp %d depth %d mirror %r %s %r" % (spp, depth, mirror, order, kw)
    assert form == dict(mirror=mirror, order=order), (what, form)
    assert did["tiles"] == int(plan[3] if mirror else plan[2]), (what, did, plan)
    assert did["chunks"] == (2 if relay is True else 4) and did["parked_values"] > 0, (what, did)
    _same(got, want, what)
    return got, did


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("lens", sorted(CAMS))
def test_every_form_equals_the_unrelayed_launch(c2, orc, lens):
    cam = CAMS[lens]()
    for spp, relay in sorted(SPP.items()):
        for depth in (5, 2):
            want = _launch(c2, spp, cam, depth, False)
            assert c2.last_sample_relay() == dict(tiles=0, chunks=0, parked_values=0) and c2.last_relay_form() is None
            plan = c2.last_tile_order()["plan"]
            assert int(plan[3]) - int(plan[2]) >= 2, "the frame has fewer than two class-2 tiles: %s" % plan
            parked = {}
            for mirror, order in FORMS:
                got, did = _form(c2, spp, cam, depth, relay, mirror, order, want)
                parked.setdefault(mirror, did["parked_values"])
                assert did["parked_values"] == parked[mirror], "the order changed what was parked"
            assert parked[True] > parked[False], "the class-2 tiles parked nothing"
            print("%s spp %d depth %d: plan %s, parked values %s" % (lens, spp, depth, [int(x) for x in plan], parked))
            if spp == 32 and depth == 5:  # `got`: the mirror extent, interleaved
                o = BackendScene(orc, scenes.scene_c2())
                ref = o.trace_grid(cam, W, H, spp, depth, SEED)
                o.close()
                assert int(got[2][0]) == ref["nrays"]
                assert np.array_equal(got[1], ref["nhit"])
                assert float(np.abs(got[0] - to_acc32(ref["acc_sum"], spp)).max()) <= 1e-6


def test_requests_without_the_new_arguments_keep_their_meaning(c2):
    """sample_relay=True, 2 and 4 alone relay classes 0 and 1, chunk workgroups first; below the gate the default relays nothing,
    whatever form is named."""
    cam = scenes.cam_dof()
    for relay, spp in ((True, 32), (2, 64), (4, 64)):
        _launch(c2, spp, cam, 5, relay)
        did, plan = c2.last_sample_relay(), c2.last_tile_order()["plan"]
        assert did["tiles"] == int(plan[2]) and did["chunks"] == (4 if relay == 4 else 2), (relay, did, plan)
        assert c2.last_relay_form() == dict(mirror=False, order="chunks_first")
    _launch(c2, 64, cam, 5, None, relay_mirror=True, relay_order="interleaved")  # 105 tiles: below 4 per compute unit
    assert c2.last_sample_relay()["tiles"] == 0 and c2.last_relay_form() is None
    with pytest.raises(ValueError):
        _launch(c2, 32, cam, 5, True, relay_order="sideways")


def test_striped_launch_and_progressive_passes(c2):
    import torch
    cam = scenes.cam_dof()
    for rank in range(2):
        kw = dict(rows=64, stripe=(16, rank, 2))
        want = _launch(c2, 32, cam, 5, False, **kw)
        _form(c2, 32, cam, 5, True, True, "interleaved", want, **kw)
    frames = []
    for relay in (True, False):
        out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        for k in range(2):
            _, nhit, _ = c2.trace_grid(W, H, 32, cam, 5, SEED, sample_offset=32 * k, spp_total=64, out=out, counters=cnt, accumulate=True,
                                       sample_relay=relay, relay_mirror=True, relay_order="mirror_first")
        torch.cuda.synchronize()
        assert c2.last_relay_form() == (dict(mirror=True, order="mirror_first") if relay else None)
        if relay:
            assert c2.last_sample_relay()["tiles"] == int(c2.last_tile_order()["plan"][3])
        frames.append((out.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy()[:2].copy()))
    _same(frames[0], frames[1], "accumulate 2 x 32 samples")


def test_a_mirror_sphere_without_glass_is_not_relayed(gpu_ready):
    """Without a refracting sphere the launch is no PAIR variant: it renders unrelayed, with no error, whatever is asked."""
    import cgraytracing_amd as cg
    objs = scenes.scene_c2()[:7]  # the walls, the diffuse and the mirror sphere
    assert objs[6].reflection > 0 and all(o.transparency == 0 for o in objs)
    cam = scenes.cam_dof()
    with cg.Scene(objs) as sc:
        assert "PAIR=1" not in sc.kernel_variant(W, H, 32, cam, 5)
        want = _launch(sc, 32, cam, 5, False)
        for mirror, order in FORMS:
            got = _launch(sc, 32, cam, 5, True, relay_mirror=mirror, relay_order=order)
            assert sc.last_sample_relay() == dict(tiles=0, chunks=0, parked_values=0) and sc.last_relay_form() is None
            _same(got, want, "mirror sphere only, mirror %r %s" % (mirror, order))


_CHILD = r"""
import sys
import numpy as np
import torch
import cgraytracing_amd as cg
import scenes
bound = int(sys.argv[1])
sc = cg.Scene(scenes.scene_c2())
cam = scenes.cam_dof()
def launch(relay, **kw):
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(200, 117, 32, cam, 5, 12345, counters=cnt, sample_relay=relay, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), nhit.cpu().numpy(), cnt.cpu().numpy()[:2]
want = launch(False)
plan = [int(x) for x in sc.last_tile_order()["plan"]]
assert bound < plan[3], (bound, plan)
for order in ("chunks_first", "mirror_first", "interleaved"):
    got = launch(True, relay_mirror=True, relay_order=order)
    did = sc.last_sample_relay()
    assert did["tiles"] == bound and did["chunks"] == 2 and did["parked_values"] > 0, (order, did)
    assert sc.last_relay_form() == dict(mirror=True, order=order)
    for a, b in zip(got, want):
        assert np.array_equal(a, b), "relayed and unrelayed launch differ: " + order
sc.close()
print("child ok", plan, did)
"""


@pytest.mark.parametrize("where", ["inside_class_2", "inside_classes_0_1"])
def test_the_area_ends_inside_a_class(c2, where):
    """CGRT_RELAY_TILES bounds the area's capacity: the first `bound` entries are relayed, the others -- of the same class
    too -- render unsplit; same bits in all three orders.  The knob is read once per process, so a fresh interpreter."""
    _launch(c2, 32, scenes.cam_dof(), 5, False)
    plan = [int(x) for x in c2.last_tile_order()["plan"]]
    assert plan[2] >= 2 and plan[3] - plan[2] >= 2, plan
    bound = plan[2] + (plan[3] - plan[2]) // 2 if where == "inside_class_2" else plan[2] // 2
    assert (plan[2] < bound < plan[3]) if where == "inside_class_2" else (0 < bound < plan[2])
    env = dict(os.environ, CGRT_RELAY_TILES=str(bound))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.run([sys.executable, "-c", _CHILD, str(bound)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr
