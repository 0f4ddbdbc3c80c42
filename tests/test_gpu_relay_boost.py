"""GPU: four chunks for the relay's heaviest tiles (relay_boost=True; CGRT_GRID_RELAY_BOOST, cgrt_relay.h).

A launch that starts by cost renders the relayed tiles whose workgroups are long -- tile cost x samples of a chunk above
num/den of the frame's work per workgroup slot -- by k_boost workgroups instead of 2, parked in a second area.  The additions
keep the unsplit loop's order, so every launch here is compared bit for bit with the list-start launch of the same process:
rgb, per-pixel nhit and every counter but the wave iterations, which must differ from the unpromoted launch's.  The promoted
set, the boost slots, S and the table read back must be the host function's (cgrt_relay_boost_host) on the costs read back.
The threshold knob CGRT_RELAY_BOOST is read at every launch, so the tests set it in their own process.  The scene is C2, with
sample_relay=True so that small frames relay."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from test_deep_trees_host import DEEP_SCENES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
CAMS = {"pinhole": scenes.cam_pinhole, "thin_lens": scenes.cam_dof}
FRAMES = ((200, 117), (96, 54))  # 105 tiles, neither a multiple of 32 nor of 8; 21 tiles
WAVE_ITERS = 2  # CGRT_CNT_WAVE_ITERS


@contextlib.contextmanager
def knob(value, tiles=None):
    """CGRT_RELAY_BOOST (and CGRT_RELAY_BOOST_TILES) for the launches inside"""
    old = {k: os.environ.get(k) for k in ("CGRT_RELAY_BOOST", "CGRT_RELAY_BOOST_TILES")}
    try:
        for k, v in (("CGRT_RELAY_BOOST", value), ("CGRT_RELAY_BOOST_TILES", tiles)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _launch(sc, W, H, spp, cam, depth, start, boost=None, seed=SEED, relay=True, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, depth, seed, counters=cnt, sample_relay=relay, relay_start=start, relay_boost=boost, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _same(a, b, what):
    """rgb, nhit and every counter except the wave iterations"""
    assert np.array_equal(a[0], b[0]), "%s: rgb differs from the list start's" % what
    assert np.array_equal(a[1], b[1]), "%s: nhit differs from the list start's" % what
    keep = [i for i in range(8) if i != WAVE_ITERS]
    assert np.array_equal(a[2][keep], b[2][keep]), "%s: counters %s vs %s" % (what, a[2], b[2])


def _forms(spp):
    k0 = min(4, spp // 16)
    cs = -(-spp // k0)
    return -(-spp // cs), cs  # k_boost, boost chunk_spp


def _check_boost(sc, W, H, spp, mirror, what):
    """The last launch's promoted set and table: the host function's on the costs read back; returns the read-backs"""
    from cgraytracing_amd.engine import relay_boost_host
    bo, st, did, order = sc.last_relay_boost(), sc.last_relay_start(), sc.last_sample_relay(), sc.last_tile_order()
    assert bo is not None and st is not None, what
    k, n_split = did["chunks"], did["tiles"]
    kb, bcs = _forms(spp)
    assert k == 2 and bo["k_boost"] == kb > k, (what, did, bo)
    host = relay_boost_host(k, -(-spp // k), spp, n_split, mirror, order["plan"], order["list"], st["wcost"], W, H, kb, bcs, bo["boost_cap"],
                            bo["num"], bo["den"], bo["wg_slots"])
    assert bo["S"] == host["S"] and bo["promoted"] == host["promoted"], (what, bo, host)
    assert np.array_equal(bo["bslot"], host["bslot"]), "%s: the promoted set is not the host function's" % what
    assert int((bo["bslot"] != 0).sum()) == bo["promoted"] <= bo["boost_cap"], what
    slots = bo["bslot"][bo["bslot"] != 0]
    assert np.unique(slots).size == slots.size and slots.max(initial=0) <= bo["boost_cap"], "%s: a boost slot twice" % what
    assert st["t"] == int(order["plan"][3]) + (k - 1) * n_split + (kb - k) * bo["promoted"] == st["start"].size, (what, st["t"])
    assert np.array_equal(st["start"], host["start"]), "%s: the table is not the host function's on the costs read back" % what
    entry, chunk = st["start"] >> 2, st["start"] & 3
    per_entry = np.bincount(entry, minlength=int(order["plan"][3]))
    want = np.ones(int(order["plan"][3]), np.int64)
    want[:n_split] = np.where(bo["bslot"] != 0, kb, k)
    assert np.array_equal(per_entry, want), "%s: chunks per entry" % what
    assert np.unique(entry.astype(np.int64) * 4 + chunk).size == st["t"], "%s: an item twice" % what
    return bo, st, did


def _mid_threshold(bo, st, order, W, spp, n_split):
    """num/den that about half of the relayed tiles pass: the median tile cost, as the rule weighs it"""
    wtx, tx = (W + 15) // 16, (W + 31) // 32
    wc = st["wcost"].reshape(-1, wtx).astype(np.int64)
    tiles = order["list"][:n_split].astype(np.int64)
    cost = np.zeros(n_split, np.int64)
    for dy in range(2):
        for dx in range(2):
            wy, wx = 2 * (tiles // tx) + dy, 2 * (tiles % tx) + dx
            ok = (wy < wc.shape[0]) & (wx < wtx)
            cost = np.maximum(cost, np.where(ok, wc[np.minimum(wy, wc.shape[0] - 1), np.minimum(wx, wtx - 1)], 0))
    med = int(np.sort(cost)[n_split // 2])
    den, cs = 4096, -(-spp // 2)
    while den > 1 and med * cs * bo["wg_slots"] * den // bo["S"] > 4096:
        den //= 2
    num = med * cs * bo["wg_slots"] * den // bo["S"]
    assert 0 < num <= 4096, (med, bo)
    passing = int((cost * cs * bo["wg_slots"] * den > num * bo["S"]).sum())  # the rule, in integers
    if 0 < passing < n_split:
        return "%d/%d" % (num, den), None
    # (tiles of one cost -- a pinhole frame at depth 2 -- pass together: there the second area, bounded, leaves both kinds)
    return "0/1", n_split // 2


def _case(sc, W, H, spp, cam, depth, mirror, what, seed=SEED):
    """list start, promotion at 0/1, at a mid threshold and off: the same bits; returns the three read-backs of parked values"""
    want = _launch(sc, W, H, spp, cam, depth, "list", seed=seed, relay_mirror=mirror)
    assert sc.last_relay_boost() is None and sc.last_relay_start() is None, what
    order = sc.last_tile_order()
    with knob("0/1"):
        got_all = _launch(sc, W, H, spp, cam, depth, "cost", True, seed=seed, relay_mirror=mirror)
        bo, st, did_all = _check_boost(sc, W, H, spp, mirror, what + " 0/1")
    _same(got_all, want, what + " 0/1")
    assert bo["promoted"] == did_all["tiles"] > 0, (what, bo, did_all)  # (a relayed tile's probe cost is never 0)
    mid, bound = _mid_threshold(bo, st, order, W, spp, did_all["tiles"])
    with knob(mid, bound):
        got_mid = _launch(sc, W, H, spp, cam, depth, "cost", True, seed=seed, relay_mirror=mirror)
        bm, _, did_mid = _check_boost(sc, W, H, spp, mirror, what + " " + mid)
    _same(got_mid, want, what + " " + mid)
    assert 0 < bm["promoted"] < did_mid["tiles"], "%s %s (%s): promoted %d of %d" % (what, mid, bound, bm["promoted"], did_mid["tiles"])
    got_off = _launch(sc, W, H, spp, cam, depth, "cost", False, seed=seed, relay_mirror=mirror)
    assert sc.last_relay_boost() is None and sc.last_relay_start() is not None, what
    did_off = sc.last_sample_relay()
    _same(got_off, want, what + " off")
    assert np.array_equal(got_off[2], want[2]), what  # (the cost start alone: the wave iterations too)
    # A wave iterates as long as its longest lane, so shorter chunks change the count -- where a pixel's samples differ in
    # length: under the thin lens at full depth.  Every sample of a pinhole pixel traces the same rays, and at depth 2 a sample
    # is one or two rays wherever the lens point lies: a lane's iterations are its samples times a constant, the wave's largest
    # lane is the same in every chunk, and the chunks' counts add up to the same sum however the samples are cut.
    if cam.lens_radius > 0 and depth == 5:
        assert got_all[2][WAVE_ITERS] != got_off[2][WAVE_ITERS], what  # (every relayed tile promoted; a few tiles may add up alike)
    assert did_all["chunks"] == did_mid["chunks"] == did_off["chunks"] == 2 and did_all["tiles"] == did_mid["tiles"] == did_off["tiles"], what
    assert did_off["parked_values"] < did_mid["parked_values"] < did_all["parked_values"], (what, did_off, did_mid, did_all)
    return bo, bm


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("mirror", [False, True], ids=["glass_extent", "mirror_extent"])
@pytest.mark.parametrize("lens", sorted(CAMS))
def test_promoted_launch_equals_list_start(c2, lens, mirror):
    cam = CAMS[lens]()
    for W, H in FRAMES:
        for spp in (64, 70):
            for depth in (5, 2):
                what = "%s %dx%d spp %d depth %d mirror %r" % (lens, W, H, spp, depth, mirror)
                bo, bm = _case(c2, W, H, spp, cam, depth, mirror, what)
    print(lens, mirror, "promoted", bo["promoted"], "mid", bm["promoted"], "S", bo["S"])


def test_three_chunks_at_48_samples(c2):
    bo, _ = _case(c2, 200, 117, 48, scenes.cam_dof(), 5, True, "48 samples")
    assert bo["k_boost"] == 3


def test_nothing_to_promote_to_at_40_samples(c2):
    """k_boost == relay_k: the flag changes nothing, and every read-back is the launch's without it"""
    W, H, spp, cam = 200, 117, 40, scenes.cam_dof()
    want = _launch(c2, W, H, spp, cam, 5, "list", relay_mirror=True)
    plain = _launch(c2, W, H, spp, cam, 5, "cost", None, relay_mirror=True)
    reads = (c2.last_relay_start(), c2.last_sample_relay(), c2.last_relay_form(), c2.last_relay_boost())
    with knob("0/1"):
        asked = _launch(c2, W, H, spp, cam, 5, "cost", True, relay_mirror=True)
    again = (c2.last_relay_start(), c2.last_sample_relay(), c2.last_relay_form(), c2.last_relay_boost())
    assert again[3] is None and reads[3] is None
    assert again[1] == reads[1] and again[2] == reads[2]
    assert again[0]["t"] == reads[0]["t"] and np.array_equal(again[0]["start"], reads[0]["start"]) and np.array_equal(again[0]["wcost"], reads[0]["wcost"])
    for got in (plain, asked):
        _same(got, want, "40 samples")
        assert np.array_equal(got[2], want[2])


def test_reuse_and_stale_tables(gpu_ready):
    """A second launch reuses costs and table; another threshold, sample count or seed rebuilds; each launch is the list start's"""
    import cgraytracing_amd as cg
    W, H, cam = 200, 117, scenes.cam_dof()
    with cg.Scene(scenes.scene_c2()) as sc:
        def boosted(spp, seed, th, what, reused):
            with knob(th):
                got = _launch(sc, W, H, spp, cam, 5, "cost", True, seed=seed, relay_mirror=True)
                bo, st, _ = _check_boost(sc, W, H, spp, True, what)
            assert st["reused"] == reused, (what, st["reused"])
            _same(got, _launch(sc, W, H, spp, cam, 5, "list", seed=seed, relay_mirror=True), what)
            return bo, st
        a = boosted(64, SEED, "0/1", "first", False)
        b = boosted(64, SEED, "0/1", "second", True)  # (the list launch in between leaves costs and table where they are)
        assert np.array_equal(a[1]["start"], b[1]["start"]) and np.array_equal(a[0]["bslot"], b[0]["bslot"])
        mid, bound = _mid_threshold(a[0], a[1], sc.last_tile_order(), W, 64, a[0]["bslot"].size)
        assert bound is None
        c = boosted(64, SEED, mid, "other threshold", False)
        assert 0 < c[0]["promoted"] < a[0]["promoted"] and np.array_equal(c[1]["wcost"], a[1]["wcost"])
        boosted(64, SEED, mid, "and again", True)
        d = boosted(70, SEED, mid, "other sample count", False)
        assert np.array_equal(d[1]["wcost"], a[1]["wcost"])  # the probe's samples are the same ones: only the table is new
        e = boosted(70, SEED + 1, mid, "other seed", False)
        assert not np.array_equal(e[1]["wcost"], d[1]["wcost"])
        # without promotion the unpromoted table is rebuilt, not the promoted one read
        got = _launch(sc, W, H, 70, cam, 5, "cost", False, seed=SEED + 1, relay_mirror=True)
        st = sc.last_relay_start()
        assert sc.last_relay_boost() is None and not st["reused"] and st["t"] < e[1]["t"]
        _same(got, _launch(sc, W, H, 70, cam, 5, "list", seed=SEED + 1, relay_mirror=True), "promotion off")


def test_forms_in_turn_on_one_handle(gpu_ready):
    """What the handle keeps between launches -- the record of the last launch, the two keys, the zeroed extents of both areas --
    through five forms in turn on one Scene: C2 at 96 x 56 (21 tiles) and 48 samples, the smallest count with a promoted form
    (3 chunks against 2).  Every launch is the unrelayed one's bit for bit (rgb, nhit, rays, Hitpoints), and the read-backs
    report the form that launch asked for, nothing for the unrelayed one."""
    import cgraytracing_amd as cg
    W, H, spp, cam = 96, 56, 48, scenes.cam_dof()
    form = dict(mirror=False, order="chunks_first")  # what sample_relay=True has always meant
    with cg.Scene(scenes.scene_c2()) as sc:
        def reads():
            return sc.last_sample_relay(), sc.last_relay_form(), sc.last_relay_start(), sc.last_relay_boost()
        got = []
        got.append(_launch(sc, W, H, spp, cam, 5, "cost", True))  # 1: by cost, promoting
        bo, st, did = _check_boost(sc, W, H, spp, False, "1: cost, boost")
        n_split = did["tiles"]
        assert n_split > 0 and did["chunks"] == 2 and bo["k_boost"] == 3 and bo["boost_cap"] >= n_split, (did, bo)
        assert sc.last_relay_form() == form and not st["reused"]
        got.append(_launch(sc, W, H, spp, cam, 5, "cost", False))  # 2: by cost, two chunks a tile throughout
        did2, form2, st2, bo2 = reads()
        assert did2["tiles"] == n_split and did2["chunks"] == 2 and form2 == form and bo2 is None, (did2, form2, bo2)
        assert st2 is not None and not st2["reused"] and st2["t"] == int(sc.last_tile_order()["plan"][3]) + n_split, st2
        assert np.array_equal(st2["wcost"], st["wcost"])
        assert did2["parked_values"] <= did["parked_values"]
        got.append(_launch(sc, W, H, spp, cam, 5, "list"))  # 3: from the list
        did3, form3, st3, bo3 = reads()
        assert did3 == did2 and form3 == form and st3 is None and bo3 is None, (did3, form3, st3, bo3)
        with knob(None, 1):  # 4: promoting again, into an area for one tile
            got.append(_launch(sc, W, H, spp, cam, 5, "cost", True))
            bo4, st4, did4 = _check_boost(sc, W, H, spp, False, "4: cost, boost, one tile")
        assert bo4["boost_cap"] == 1 and bo4["promoted"] <= 1 and did4["tiles"] == n_split and sc.last_relay_form() == form, (bo4, did4)
        assert not st4["reused"] and np.array_equal(st4["wcost"], st["wcost"])
        want = _launch(sc, W, H, spp, cam, 5, None, None, relay=False)  # 5: no relay
        did5, form5, st5, bo5 = reads()
        assert did5 == dict(tiles=0, chunks=0, parked_values=0) and form5 is None and st5 is None and bo5 is None, (did5, form5, st5, bo5)
        for i, g in enumerate(got):
            assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "launch %d: image or nhit differs from the unrelayed launch's" % (i + 1)
            assert np.array_equal(g[2][:2], want[2][:2]), "launch %d: rays / Hitpoints %s vs %s" % (i + 1, g[2], want[2])


@pytest.mark.parametrize("cam_name,cam", DEEP_SCENES[1][2], ids=[c[0] for c in DEEP_SCENES[1][2]])
def test_full_depth_trees(gpu_ready, cam_name, cam):
    """The camera inside a glass sphere (test_gpu_deep_trees' sphere scene): every tile is of class 0 and many rays reach the
    last level, so a 16-sample chunk that ends in 16 Hitpoints a sample fills its stream's slots exactly."""
    import cgraytracing_amd as cg
    name, mk, _ = DEEP_SCENES[1]
    assert name == "inside_glass_c2"
    W, H, spp = 96, 40, 64
    with cg.Scene(mk()) as sc:
        want = _launch(sc, W, H, spp, cam, 5, "list")
        with knob("0/1"):
            got = _launch(sc, W, H, spp, cam, 5, "cost", True)
            bo, _, did = _check_boost(sc, W, H, spp, False, "inside glass " + cam_name)
        _same(got, want, "inside glass " + cam_name)
        assert bo["promoted"] == did["tiles"] == 15, (bo, did)
        tail = _launch(sc, W, H, 48, cam, 5, "list", relay=False, sample_offset=16, spp_total=spp)
        assert did["parked_values"] == int(tail[2][1]), "parked values are the Hitpoints of chunks 1-3"
        assert int(want[1].max()) > spp, "no pixel with more than one Hitpoint a sample"
        print(cam_name, "most Hitpoints of a pixel", int(want[1].max()), "of", 16 * spp)


def test_default_launch_promotes(c2):
    """1920 x 1080 at 64 samples promotes by default; the second launch reuses; the image is the list start's"""
    W, H, spp, cam = 1920, 1080, 64, scenes.cam_dof()
    got = _launch(c2, W, H, spp, cam, 5, None, None, relay=None)
    bo, st, did = _check_boost(c2, W, H, spp, True, "default 1920x1080")
    assert 0 < bo["promoted"] <= bo["boost_cap"] and not st["reused"], bo
    again = _launch(c2, W, H, spp, cam, 5, None, None, relay=None)
    assert c2.last_relay_start()["reused"] and c2.last_tile_order_reused() and c2.last_relay_boost()["promoted"] == bo["promoted"]
    assert all(np.array_equal(x, y) for x, y in zip(again, got)), "default, reused"
    want = _launch(c2, W, H, spp, cam, 5, "list", relay=None)
    assert c2.last_relay_boost() is None
    _same(got, want, "default 1920x1080")
    print("default: promoted", bo["promoted"], "of", did["tiles"], "cap", bo["boost_cap"], "t", st["t"])


_CHILD = r"""
import sys
import numpy as np
import scenes
import cgraytracing_amd as cg
sys.path.insert(0, sys.argv[2])
import test_gpu_relay_boost as T
bound = int(sys.argv[1])
sc = cg.Scene(scenes.scene_c2())
cam = scenes.cam_dof()
want = T._launch(sc, 200, 117, 64, cam, 5, "list", relay_mirror=True)
got = T._launch(sc, 200, 117, 64, cam, 5, "cost", True, relay_mirror=True)
bo, st, did = T._check_boost(sc, 200, 117, 64, True, "bounded boost area")
assert bo["boost_cap"] == bound == bo["promoted"] < did["tiles"], (bo, did)
T._same(got, want, "bounded boost area")
sc.close()
print("child ok", bo["promoted"], st["t"])
"""


def test_the_boost_area_ends_inside_the_promoted_set(c2):
    """CGRT_RELAY_BOOST_TILES bounds the second area: the heaviest candidates are promoted, the others keep two chunks.  Run in
    a fresh interpreter, the knob in its environment from the start."""
    with knob("0/1"):
        _launch(c2, 200, 117, 64, scenes.cam_dof(), 5, "cost", True, relay_mirror=True)
        promoted = c2.last_relay_boost()["promoted"]
    assert promoted >= 4
    bound = promoted // 2
    env = dict(os.environ, CGRT_RELAY_BOOST="0/1", CGRT_RELAY_BOOST_TILES=str(bound))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.run([sys.executable, "-c", _CHILD, str(bound), os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=300,
                         env=env, cwd=ROOT)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr
