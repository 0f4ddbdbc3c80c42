"""GPU: the lens table of classes 0-2 (CGRT_GRID_NO_LENS_TABLE, lens_table=False; cgrt_lens_stage.h).

Under a thin lens a small kernel ahead of the frame finds the accepted lens draw of every sample of the tiles that may see a
mirror or a glass sphere and leaves it in a table on the handle; the full and the parking body of those tiles read their draws
there instead of running the rejection loop in lockstep.  The draw of (pixel, sample) is a pure function of both, so the points
are the same bits: every launch here runs with the table and with lens_table=False on one handle and is compared bit for bit --
rgb, per-pixel nhit and all eight counters -- and the read-back names what ran.  "With the table" is lens_table=True, under which
a launch that does not find its draws in the table writes them wherever it stands; left to itself (lens_table=None) a launch
writes them only beside its cost probe and otherwise goes without, which has a test of its own.  The scene is C2."""
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
BUDGET = 256 << 20
ZERO = dict(entries=0, capacity=0, reused=False)


def _launch(sc, W, H, spp, cam, table, stream=None, seed=SEED, depth=5, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, depth, seed, counters=cnt, lens_table=table, stream=stream, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "nhit", "counters")):
        assert np.array_equal(x, y), "%s: %s differs between table and per-sample lens points" % (what, name)


def _expected(sc, spp, budget=BUDGET):
    """What the read-back must say of a launch that read the table: the list's entries of classes 0-2 below the capacity."""
    order = sc.last_tile_order()
    plan = [int(x) for x in order["plan"]]
    cap = min(plan[4], budget // (spp * 256 * 8))
    assert plan[3] > 0 and cap > 0, plan
    return dict(entries=min(plan[3], cap), capacity=cap)


def _both(sc, W, H, spp, cam, tabled=True, budget=BUDGET, **kw):
    """The launch with the table and without; tabled: whether the first is expected to read one."""
    what = "%dx%d spp %d %r" % (W, H, spp, kw)
    on = _launch(sc, W, H, spp, cam, True, **kw)
    did = sc.last_lens_table()
    if tabled:
        want = _expected(sc, spp, budget)
        assert (did["entries"], did["capacity"]) == (want["entries"], want["capacity"]), (what, did, want)
    else:
        assert did == ZERO, (what, did)
    off = _launch(sc, W, H, spp, cam, False, **kw)
    assert sc.last_lens_table() == ZERO, what
    _same(on, off, what)
    return on


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("spp", [1, 5, 32, 33, 64])
def test_sample_counts_around_the_batch(c2, orc, spp):
    got = _both(c2, 96, 54, spp, scenes.cam_dof())
    if spp in (5, 33):
        o = BackendScene(orc, scenes.scene_c2())
        want = o.trace_grid(scenes.cam_dof(), 96, 54, spp, 5, SEED)
        o.close()
        assert int(got[2][0]) == want["nrays"] and np.array_equal(got[1], want["nhit"])
        assert float(np.abs(got[0] - to_acc32(want["acc_sum"], spp)).max()) <= 1e-6


@pytest.mark.parametrize("spp,relay", [(33, True), (64, True), (33, 4), (64, 4)])
def test_the_parking_body_reads_its_own_sample_range(c2, spp, relay):
    _both(c2, 96, 54, spp, scenes.cam_dof(), sample_relay=relay, relay_mirror=True)
    _launch(c2, 96, 54, spp, scenes.cam_dof(), True, sample_relay=relay, relay_mirror=True)
    r = c2.last_sample_relay()
    assert r["tiles"] > 0 and r["parked_values"] > 0 and r["chunks"] == (min(4, spp // 16) if relay == 4 else 2), r


def test_the_start_twin_and_promoted_tiles(c2):
    """relay_start="cost": the START twin of the table-reading kernel renders the frame (its cost probe is the START twin without
    a table: the counts are the same); relay_boost with the threshold at 0: promoted tiles of four chunks."""
    cam = scenes.cam_dof()
    for spp in (33, 64):
        _both(c2, 96, 54, spp, cam, sample_relay=True, relay_mirror=True, relay_start="cost")
        _launch(c2, 96, 54, spp, cam, True, sample_relay=True, relay_mirror=True, relay_start="cost")
        assert c2.last_relay_start() is not None
    old = os.environ.get("CGRT_RELAY_BOOST")
    os.environ["CGRT_RELAY_BOOST"] = "0/1"  # (read at every launch)
    try:
        _both(c2, 96, 54, 64, cam, sample_relay=True, relay_mirror=True, relay_start="cost", relay_boost=True)
        _launch(c2, 96, 54, 64, cam, True, sample_relay=True, relay_mirror=True, relay_start="cost", relay_boost=True)
        b = c2.last_relay_boost()
        assert b is not None and b["promoted"] > 0 and b["k_boost"] == 4, b
        assert c2.last_lens_table()["entries"] > 0
    finally:
        if old is None:
            os.environ.pop("CGRT_RELAY_BOOST", None)
        else:
            os.environ["CGRT_RELAY_BOOST"] = old


def test_sample_offset_partial_tiles_and_stripes(c2):
    _both(c2, 96, 54, 20, scenes.cam_dof(), sample_offset=3, spp_total=64)
    _both(c2, 96, 54, 40, scenes.cam_dof(), sample_offset=3, spp_total=64, sample_relay=True, relay_start="cost")  # (the probe's samples start at 0, the table's at 3)
    _both(c2, 200, 52, 17, scenes.cam_dof())                               # partial tiles: lanes that are not live
    _both(c2, 200, 117, 18, scenes.cam_dof(), rows=56, stripe=(8, 1, 2))   # rows beyond the image


def test_reuse(c2):
    """The table is kept with the order: the same launch again finds it written; another seed or sample offset rewrites it."""
    cam = scenes.cam_dof()
    first = _launch(c2, 128, 72, 20, cam, True, seed=777, spp_total=64)
    assert c2.last_lens_table()["entries"] > 0 and not c2.last_lens_table()["reused"]
    again = _launch(c2, 128, 72, 20, cam, True, seed=777, spp_total=64)
    assert c2.last_lens_table()["reused"] and c2.last_tile_order_reused()
    _same(again, first, "the table reused")
    _same(first, _launch(c2, 128, 72, 20, cam, False, seed=777, spp_total=64), "seed 777")
    # another seed, another sample offset: each rebuilds the table; the third repeats the second, a launch without a table between them
    for kw, reused in ((dict(seed=778), False), (dict(seed=778, sample_offset=5), False), (dict(seed=778, sample_offset=5), True)):
        got = _launch(c2, 128, 72, 20, cam, True, spp_total=64, **kw)
        did = c2.last_lens_table()
        assert did["entries"] > 0 and did["reused"] == reused, (kw, did)
        _same(got, _launch(c2, 128, 72, 20, cam, False, spp_total=64, **kw), repr(kw))
        seen = kw
    got = _launch(c2, 128, 72, 24, cam, True, spp_total=64, **seen)  # other spp: other rows
    assert not c2.last_lens_table()["reused"]
    _same(got, _launch(c2, 128, 72, 24, cam, False, spp_total=64, **seen), "spp 24")


def test_the_probe_runs_again_under_a_table_that_stands(c2):
    """Another max_depth with everything else the same: the table is reused, the costs are not -- the probe runs again, without
    the table, and the frame reads it."""
    cam = scenes.cam_dof()
    kw = dict(seed=555, sample_relay=True, relay_mirror=True, relay_start="cost")
    _launch(c2, 96, 54, 64, cam, True, **kw)
    assert c2.last_lens_table()["entries"] > 0
    got = _launch(c2, 96, 54, 64, cam, True, depth=4, **kw)
    did, start = c2.last_lens_table(), c2.last_relay_start()
    assert did["entries"] > 0 and did["reused"] and start is not None and not start["reused"], (did, start)
    _same(got, _launch(c2, 96, 54, 64, cam, False, depth=4, **kw), "depth 4 under the table of depth 5")


def test_left_to_itself_a_launch_writes_the_table_only_beside_its_cost_probe(c2):
    """lens_table=None, the default: written alone the table costs more than one frame gains, so a launch writes it where its
    cost probe runs anyway (a new seed here), reads it where it stands, and goes without -- the kernels without table code -- in
    a pass whose sample offset has moved while the costs stand, and in a launch that has no probe."""
    cam = scenes.cam_dof()
    kw = dict(seed=991, sample_relay=True, relay_mirror=True, relay_start="cost", spp_total=128)
    first = _launch(c2, 96, 54, 40, cam, None, **kw)
    did = c2.last_lens_table()
    assert did["entries"] > 0 and not did["reused"] and not c2.last_relay_start()["reused"], did
    again = _launch(c2, 96, 54, 40, cam, None, **kw)
    assert c2.last_lens_table()["reused"] and c2.last_relay_start()["reused"]
    _same(again, first, "the table reused")
    _same(first, _launch(c2, 96, 54, 40, cam, False, **kw), "written beside the probe")
    moved = _launch(c2, 96, 54, 40, cam, None, sample_offset=40, **kw)
    assert c2.last_lens_table() == ZERO and c2.last_relay_start()["reused"]
    _same(moved, _launch(c2, 96, 54, 40, cam, False, sample_offset=40, **kw), "the next pass")
    back = _launch(c2, 96, 54, 40, cam, None, **kw)  # the pass without a table left it as it was
    assert c2.last_lens_table()["reused"]
    _same(back, first, "the first pass again")
    _launch(c2, 96, 54, 5, cam, None, seed=992)  # no relay, no probe
    assert c2.last_lens_table() == ZERO


def test_no_table_without_a_lens_or_outside_the_one_launch_tile_order(c2):
    _both(c2, 96, 54, 17, scenes.cam_pinhole(), tabled=False)
    _both(c2, 96, 54, 17, scenes.cam_dof(), tabled=False, sphere_pairs=False)
    _both(c2, 96, 54, 17, scenes.cam_dof(), tabled=False, tile_order=False)
    _both(c2, 96, 54, 17, scenes.cam_dof(), tabled=False, diffuse_tiles=True)
    assert c2.last_diffuse_tiles() > 0
    _both(c2, 96, 54, 32, scenes.cam_dof(), tabled=False, split_samples=True)
    # the LDS stage's flag does not touch the table, nor the table's flag the LDS stage
    _launch(c2, 96, 54, 17, scenes.cam_dof(), True, lens_stage=False)
    assert c2.last_lens_table()["entries"] > 0 and c2.last_lens_stage() == dict(lds_tiles=0, area_tiles=0)
    _launch(c2, 96, 54, 17, scenes.cam_dof(), False)
    assert c2.last_lens_table() == ZERO and c2.last_lens_stage()["lds_tiles"] > 0 and c2.last_lens_stage()["area_tiles"] == 0


def test_two_streams_on_one_handle(c2):
    import torch
    cam = scenes.cam_dof()
    want = _launch(c2, 96, 54, 33, cam, False, seed=4242)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for st in (s1, s2):
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        st.wait_stream(torch.cuda.current_stream())
        rgb, nhit, _ = c2.trace_grid(96, 54, 33, cam, 5, 4242, counters=cnt, stream=st.cuda_stream, lens_table=True)
        outs.append((rgb, nhit, cnt))
    torch.cuda.synchronize()
    did = c2.last_lens_table()
    assert did["entries"] > 0 and did["reused"], did  # the second stream's launch waits for the first's table
    for k, (rgb, nhit, cnt) in enumerate(outs):
        _same((rgb.cpu().numpy(), nhit.cpu().numpy().view(np.uint32), cnt.cpu().numpy()), want, "stream %d" % k)


def test_captured_stream_goes_without_a_table(gpu_ready):
    """A launch captured into a graph reads no table -- the table and the handle's record of it belong to launches that run now --
    and its replay renders the same image."""
    import torch
    import cgraytracing_amd as cg
    W, H, spp, cam = 96, 54, 17, scenes.cam_dof()
    with cg.Scene(scenes.scene_c2()) as sc:
        want = _launch(sc, W, H, spp, cam, False)
        warm = _launch(sc, W, H, spp, cam, True)  # (every buffer of the handle has its size before the capture)
        assert sc.last_lens_table()["entries"] > 0
        _same(warm, want, "before the capture")
        out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        nhit = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sc.trace_grid(W, H, spp, cam, 5, SEED, out=out, nhit=nhit, counters=cnt)
        assert sc.last_lens_table() == ZERO
        graph.replay()
        torch.cuda.synchronize()
        _same((out.cpu().numpy(), nhit.cpu().numpy().view(np.uint32), cnt.cpu().numpy()), want, "the replay")
        del graph
        again = _launch(sc, W, H, spp, cam, True)  # from then on the handle keeps nothing between launches: a table, written anew
        did = sc.last_lens_table()
        assert did["entries"] > 0 and not did["reused"], did
        _same(again, want, "after the capture")


_CHILD = r"""
import sys
import scenes
import cgraytracing_amd as cg
sys.path.insert(0, sys.argv[2])
import test_gpu_lens_table as T
budget = int(sys.argv[1])
sc = cg.Scene(scenes.scene_c2())
cam = scenes.cam_dof()
T._both(sc, 96, 54, 64, cam, budget=budget)
T._launch(sc, 96, 54, 64, cam, True)
did, plan = sc.last_lens_table(), [int(x) for x in sc.last_tile_order()["plan"]]
assert did["entries"] == 2 and did["capacity"] == 2 and plan[3] > 2, (did, plan)   # two read the table, the rest run the loop
T._both(sc, 96, 54, 64, cam, budget=budget, sample_relay=True, relay_mirror=True, relay_start="cost")
T._both(sc, 96, 54, 33, cam, budget=budget)
T._launch(sc, 96, 54, 33, cam, True)
assert sc.last_lens_table()["capacity"] == 3, sc.last_lens_table()
sc.close()
print("child ok", did, plan)
"""


def test_a_budget_of_two_entries(gpu_ready):
    """CGRT_LENS_TABLE_BYTES pays for two entries at 64 samples: their workgroups read the table, the other tiles of classes 0-2
    run the loop in the same launch.  The knobs are read once per process, hence a fresh interpreter."""
    budget = 2 * 64 * 256 * 8
    env = dict(os.environ, CGRT_LENS_TABLE_BYTES=str(budget))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.run([sys.executable, "-c", _CHILD, str(budget), os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=300,
                         env=env, cwd=ROOT)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr
