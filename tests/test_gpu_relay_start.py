"""GPU: the relay's start order by cost (relay_start="cost"; CGRT_GRID_RELAY_COST_START, cgrt_relay.h).

A probe -- the launch's own kernel over the first samples of the tiles of classes 0-2, storing nothing but each wave's
iteration count -- leaves a cost per wave tile; a small kernel ranks the relay's workgroups of classes 0-2 by tile cost x
samples, and the launch maps workgroup b through that table.  The same workgroups run the same bodies, so every launch here is
compared bit for bit with the list-start launch of the same process: rgb, per-pixel nhit and all eight counters.  The table
read back must be the host function's (cgrt_relay_start_host) on the costs read back, and is checked on its own terms too: a
permutation of the items, weights not increasing.  The scene is C2, with sample_relay=True so that small frames relay."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
CAMS = {"pinhole": scenes.cam_pinhole, "thin_lens": scenes.cam_dof}
FRAMES = ((200, 117), (96, 54))  # 105 tiles, neither a multiple of 32 nor of 8; 21 tiles


def _launch(sc, W, H, spp, cam, depth, start, seed=SEED, relay=True, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, depth, seed, counters=cnt, sample_relay=relay, relay_start=start, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "nhit", "the eight counters")):
        assert np.array_equal(x, y), "%s: %s differs between cost start and list start" % (what, name)


def _check_table(sc, W, H, spp, mirror, what, cap=None):
    """The last launch's table: the host function's on the costs read back, and a longest-first permutation of the items."""
    from cgraytracing_amd.engine import relay_start_host
    st, did, order = sc.last_relay_start(), sc.last_sample_relay(), sc.last_tile_order()
    assert st is not None, what
    plan, lst = [int(x) for x in order["plan"]], order["list"]
    k, n_split = did["chunks"], did["tiles"]
    assert k >= 2 and n_split == min(plan[3] if mirror else plan[2], n_split if cap is None else cap), (what, did, plan)
    chunk_spp = -(-spp // k)
    assert st["t"] == plan[3] + (k - 1) * n_split and st["start"].size == st["t"], (what, st["t"], plan, did)
    wtx, wty, tx = (W + 15) // 16, (H + 3) // 4, (W + 31) // 32
    assert st["wcost"].size == wtx * wty
    host = relay_start_host(k, chunk_spp, spp, n_split, mirror, order["plan"], lst, st["wcost"], W, H)
    assert np.array_equal(st["start"], host), "%s: the table is not the host function's on the costs read back" % what
    # on its own terms: the cost of a tile, the weight of an item
    wc = st["wcost"].reshape(wty, wtx).astype(np.int64)
    cls = order["cls"]
    for e in range(plan[4]):
        t = int(lst[e])
        waves = wc[2 * (t // tx):2 * (t // tx) + 2, 2 * (t % tx):2 * (t % tx) + 2]
        assert (waves.min() > 0) if e < plan[3] else (waves.max() == 0), "%s: entry %d (class %d) has costs %s" % (what, e, cls[t], waves)
    entry, chunk = st["start"] >> 2, (st["start"] & 3).astype(np.int64)
    assert entry.max(initial=0) < max(plan[3], 1) and (chunk < k).all() and (chunk[entry >= n_split] == 0).all(), what
    keys = entry.astype(np.int64) * 4 + chunk
    assert np.unique(keys).size == st["t"], "%s: an item twice" % what
    per_entry = np.bincount(entry, minlength=plan[3])[:plan[3]]
    assert (per_entry[:n_split] == k).all() and (per_entry[n_split:] == 1).all(), what
    tiles = lst[entry].astype(np.int64)
    cost = np.zeros(st["t"], np.int64)
    for dy in range(2):
        for dx in range(2):
            wy, wx = 2 * (tiles // tx) + dy, 2 * (tiles % tx) + dx
            ok = (wy < wty) & (wx < wtx)
            cost = np.maximum(cost, np.where(ok, wc[np.minimum(wy, wty - 1), np.minimum(wx, wtx - 1)], 0))
    samples = np.where(entry < n_split, np.minimum((chunk + 1) * chunk_spp, spp) - chunk * chunk_spp, spp)
    weight = cost * samples
    assert (samples > 0).all() and (np.diff(weight) <= 0).all(), "%s: weights increase along the table" % what
    ties = np.diff(weight) == 0
    assert (np.diff(keys)[ties] > 0).all(), "%s: equal weights out of (entry, chunk) order" % what
    return st


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("mirror", [False, True], ids=["glass_extent", "mirror_extent"])
@pytest.mark.parametrize("lens", sorted(CAMS))
def test_cost_start_equals_list_start(c2, lens, mirror):
    cam = CAMS[lens]()
    for W, H in FRAMES:
        for spp in (32, 40):
            for depth in (5, 2):
                what = "%s %dx%d spp %d depth %d mirror %r" % (lens, W, H, spp, depth, mirror)
                want = _launch(c2, W, H, spp, cam, depth, "list", relay_mirror=mirror)
                assert c2.last_relay_start() is None and c2.last_sample_relay()["tiles"] > 0, what
                got = _launch(c2, W, H, spp, cam, depth, "cost", relay_mirror=mirror)
                assert c2.last_relay_form() == dict(mirror=mirror, order="chunks_first"), what  # the order behind the table
                _same(got, want, what)
                st = _check_table(c2, W, H, spp, mirror, what)
                assert not st["reused"], what
                assert want[2][2] > 0 and want[2][0] > want[2][1] > 0, want[2]  # wave iterations, rays, Hitpoints
    print(lens, mirror, "t", st["t"], "largest cost", int(st["wcost"].max()))


def test_default_launch_starts_by_cost(c2):
    """1920 x 1080 relays by default, and then by cost: several batches of the ranking kernel, an area that ends inside the
    list; naming an order, or the list, gives the launch without a table -- the same bits."""
    W, H, spp, cam = 1920, 1080, 32, scenes.cam_dof()
    got = _launch(c2, W, H, spp, cam, 5, None, relay=None)
    assert c2.last_relay_form() == dict(mirror=True, order="interleaved")
    st = _check_table(c2, W, H, spp, True, "default 1920x1080")
    assert st["t"] > 1024 and not st["reused"]
    again = _launch(c2, W, H, spp, cam, 5, None, relay=None)
    assert c2.last_relay_start()["reused"] and c2.last_tile_order_reused()
    _same(again, got, "default, reused")
    want = _launch(c2, W, H, spp, cam, 5, "list", relay=None)
    assert c2.last_relay_start() is None and c2.last_relay_form() == dict(mirror=True, order="interleaved")
    _same(got, want, "default 1920x1080")
    named = _launch(c2, W, H, spp, cam, 5, None, relay=None, relay_order="interleaved")
    assert c2.last_relay_start() is None
    _same(named, want, "default 1920x1080, order named")
    with pytest.raises(ValueError):
        _launch(c2, W, H, spp, cam, 5, "longest")


def test_reuse_and_stale_tables(gpu_ready):
    """A second launch reuses costs and table; another depth, seed or sample count does not get a stale table: the table read
    back is the host function's on that launch's costs every time, and the image the list start's."""
    import cgraytracing_amd as cg
    W, H, cam = 200, 117, scenes.cam_dof()
    with cg.Scene(scenes.scene_c2()) as sc:
        def cost(spp, depth, seed, what, reused):
            got = _launch(sc, W, H, spp, cam, depth, "cost", seed=seed, relay_mirror=True)
            st = _check_table(sc, W, H, spp, True, what)
            assert st["reused"] == reused, (what, st["reused"])
            want = _launch(sc, W, H, spp, cam, depth, "list", seed=seed, relay_mirror=True)
            assert sc.last_relay_start() is None
            _same(got, want, what)
            return st
        a = cost(32, 5, SEED, "first", False)
        b = cost(32, 5, SEED, "second", True)  # (the list launch in between leaves costs and table where they are)
        assert sc.last_tile_order_reused()
        assert np.array_equal(a["start"], b["start"]) and np.array_equal(a["wcost"], b["wcost"])
        c = cost(32, 2, SEED, "other depth", False)
        assert not np.array_equal(c["wcost"], a["wcost"]), "depth 2 and depth 5 cost the same"
        d = cost(32, 2, SEED + 1, "other seed", False)
        assert not np.array_equal(d["wcost"], c["wcost"]), "another seed, the same iteration counts everywhere"
        e = cost(40, 2, SEED + 1, "other sample count", False)  # the probe's samples are the same ones: only the table is new
        assert np.array_equal(e["wcost"], d["wcost"])
        assert e["t"] == d["t"]
        f = cost(40, 2, SEED + 1, "and again", True)
        assert np.array_equal(e["start"], f["start"])
        # the other extent: fewer items, the same costs
        got = _launch(sc, W, H, 40, cam, 2, "cost", seed=SEED + 1, relay_mirror=False)
        st = _check_table(sc, W, H, 40, False, "other extent")
        assert not st["reused"] and np.array_equal(st["wcost"], e["wcost"]) and st["t"] < e["t"]
        _same(got, _launch(sc, W, H, 40, cam, 2, "list", seed=SEED + 1, relay_mirror=False), "other extent")
        # another camera: the order itself is new, and costs and table with it
        cam2 = scenes.cam_pinhole()
        got = _launch(sc, W, H, 40, cam2, 2, "cost", seed=SEED + 1, relay_mirror=False)
        st = _check_table(sc, W, H, 40, False, "other camera")
        assert not st["reused"] and not sc.last_tile_order_reused()
        _same(got, _launch(sc, W, H, 40, cam2, 2, "list", seed=SEED + 1, relay_mirror=False), "other camera")


def test_captured_stream_goes_without_a_table(gpu_ready):
    """A launch captured into a graph relays nothing and has no table; its replay renders the list start's image."""
    import torch
    import cgraytracing_amd as cg
    W, H, spp, cam = 200, 117, 32, scenes.cam_dof()
    with cg.Scene(scenes.scene_c2()) as sc:
        want = _launch(sc, W, H, spp, cam, 5, "list")
        first = _launch(sc, W, H, spp, cam, 5, "cost")  # (every buffer of the handle has its size before the capture)
        assert sc.last_relay_start() is not None
        _same(first, want, "before the capture")
        out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        nhit = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sc.trace_grid(W, H, spp, cam, 5, SEED, out=out, nhit=nhit, counters=cnt, sample_relay=True, relay_start="cost")
        assert sc.last_relay_start() is None and sc.last_relay_form() is None
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(nhit.cpu().numpy().view(np.uint32), want[1])
        assert np.array_equal(cnt.cpu().numpy()[:2], want[2][:2])  # rays and Hitpoints (the unrelayed launch iterates otherwise)
        del graph
        # from then on the handle keeps nothing between launches: a table again, built anew
        again = _launch(sc, W, H, spp, cam, 5, "cost")
        st = _check_table(sc, W, H, spp, False, "after the capture")
        assert not st["reused"]
        _same(again, want, "after the capture")


_CHILD = r"""
import sys
import numpy as np
import scenes
import cgraytracing_amd as cg
sys.path.insert(0, sys.argv[2])
import test_gpu_relay_start as T
bound = int(sys.argv[1])
sc = cg.Scene(scenes.scene_c2())
for lens in sorted(T.CAMS):
    cam = T.CAMS[lens]()
    for spp, depth in ((32, 5), (40, 2)):
        want = T._launch(sc, 200, 117, spp, cam, depth, "list", relay_mirror=True)
        plan = [int(x) for x in sc.last_tile_order()["plan"]]
        assert plan[2] < bound < plan[3], (bound, plan)
        got = T._launch(sc, 200, 117, spp, cam, depth, "cost", relay_mirror=True)
        assert sc.last_sample_relay()["tiles"] == bound
        T._same(got, want, "bounded area")
        st = T._check_table(sc, 200, 117, spp, True, "bounded area %s spp %d" % (lens, spp), cap=bound)
        assert st["t"] == plan[3] + bound
sc.close()
print("child ok", plan, st["t"])
"""


def test_the_area_ends_inside_class_2(c2):
    """CGRT_RELAY_TILES bounds the area: the entries beyond it, of class 2 too, are single items of the table with all the
    launch's samples.  The knob is read once per process, so a fresh interpreter."""
    bounds = []
    for lens in sorted(CAMS):
        _launch(c2, 200, 117, 32, CAMS[lens](), 5, "list")
        plan = [int(x) for x in c2.last_tile_order()["plan"]]
        assert plan[3] - plan[2] >= 2, plan
        bounds.append((plan[2], plan[3]))
    lo, hi = max(b[0] for b in bounds), min(b[1] for b in bounds)
    bound = (lo + hi) // 2
    assert lo < bound < hi, bounds
    env = dict(os.environ, CGRT_RELAY_TILES=str(bound))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.run([sys.executable, "-c", _CHILD, str(bound), os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=300,
                         env=env, cwd=ROOT)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr
