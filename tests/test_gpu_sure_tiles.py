"""GPU: the sure tiles of the terminal-diffuse body (CGRT_GRID_NO_SURE_TILES, sure_tiles=False).

Where every primary ray of a 16x4 wave tile of a class-3 tile provably hits one and the same sphere first (sure_first_kernel,
cgrt_sure_first.h), the wave adds that sphere's colour once per sample instead of running the sample loop.  Nothing may change: every
launch here is rendered with the shortcut and without it in one process and compared bit for bit -- rgb, per-pixel nhit and every
counter.  The bytes themselves are read back (Scene.last_sure_tiles) and compared with the CPU oracle's first hits."""
import numpy as np
import pytest

import scenes
from backends import BackendScene

pytestmark = pytest.mark.gpu

SEED = 12345
NONE = 255


def _launch(sc, W, H, spp, cam, sure, out=None, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, 5, SEED, counters=cnt, sure_tiles=sure, out=out, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _class3_wave_tiles(order, W, rows):
    """Indices of the wave tiles that lie in tiles of class 3."""
    tiles_x, wtx, wty = (W + 31) // 32, (W + 15) // 16, (rows + 3) // 4
    wy, wx = np.divmod(np.arange(wtx * wty), wtx)
    return np.nonzero(order["cls"][(wy // 2) * tiles_x + wx // 2] == 3)[0]


def _both(sc, W, H, spp, cam, expect_sure=True, **kw):
    """The launch with the shortcut and without: identical bits.  Returns the first launch's results, its bytes and its order."""
    on = _launch(sc, W, H, spp, cam, True, **kw)
    sure, order = sc.last_sure_tiles(), sc.last_tile_order()
    off = _launch(sc, W, H, spp, cam, False, **kw)
    assert sc.last_sure_tiles() is None, "sure_tiles=False still wrote sure tiles"
    for a, b, what in zip(on, off, ("rgb", "nhit", "counters")):
        assert np.array_equal(a, b), "%dx%d spp %d %r: %s differs between the shortcut and the sample loop" % (W, H, spp, kw, what)
    rows = kw.get("rows") or H
    if expect_sure:
        assert sure is not None and len(sure) == ((W + 15) // 16) * ((rows + 3) // 4)
        c3 = _class3_wave_tiles(order, W, rows)
        assert np.count_nonzero(sure[c3] != NONE) > 0, "no class-3 wave tile is sure: the shortcut was not used"
        assert np.all(np.delete(sure, c3) == NONE), "a wave tile of a tile of classes 0-2 is sure"
    else:
        assert sure is None or np.all(sure == NONE)
    return on, sure, order


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("diffuse_tiles", [False, True])
@pytest.mark.parametrize("W,H,spp,lens", [(192, 108, 4, True), (192, 108, 4, False), (200, 52, 3, True), (192, 108, 1, True)])
def test_c2_shortcut_equals_sample_loop(c2, W, H, spp, lens, diffuse_tiles):
    cam = scenes.cam_dof() if lens else scenes.cam_pinhole()
    _, sure, order = _both(c2, W, H, spp, cam, diffuse_tiles=diffuse_tiles)
    winners = set(int(x) for x in sure[sure != NONE])
    assert winners and winners <= {0, 1, 2, 3, 4, 5}, "C2's winners are its walls and its diffuse sphere: %r" % winners


@pytest.mark.parametrize("diffuse_tiles", [False, True])
def test_stripe_and_band(c2, diffuse_tiles):
    _both(c2, 200, 117, 4, scenes.cam_dof(), rows=56, stripe=(8, 1, 2), diffuse_tiles=diffuse_tiles)
    _both(c2, 192, 108, 4, scenes.cam_dof(), rows=40, row_offset=24, diffuse_tiles=diffuse_tiles)


def test_two_accumulating_passes(c2):
    """Samples 0..2 and then 3..6 added into the same fp32 frame: the second pass's additions start from the first's pixels."""
    import torch
    W, H, cam = 192, 108, scenes.cam_dof()
    frames = []
    for sure in (True, False):
        out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        a = _launch(c2, W, H, 3, cam, sure, out=out, sample_offset=0, spp_total=7, accumulate=True)
        if sure:
            assert np.count_nonzero(c2.last_sure_tiles() != NONE) > 0
        b = _launch(c2, W, H, 4, cam, sure, out=out, sample_offset=3, spp_total=7, accumulate=True)
        frames.append((a, b))
    for p in range(2):
        for a, b, what in zip(frames[0][p], frames[1][p], ("rgb", "nhit", "counters")):
            assert np.array_equal(a, b), "pass %d: %s differs" % (p, what)


def test_with_the_relay_in_the_same_launch(c2):
    """The relay forced on a small frame: relayed glass tiles and sure wall tiles in one launch."""
    _both(c2, 192, 108, 32, scenes.cam_dof(), sample_relay=True)
    _launch(c2, 192, 108, 32, scenes.cam_dof(), True, sample_relay=True)
    assert c2.last_sample_relay()["tiles"] > 0 and np.count_nonzero(c2.last_sure_tiles() != NONE) > 0


def test_many_spheres(gpu_ready):
    import cgraytracing_amd as cg
    with cg.Scene(scenes.many_spheres(32, 11)) as sc:
        _both(sc, 192, 108, 4, scenes.cam_dof())
        _both(sc, 192, 108, 4, scenes.cam_pinhole())


def test_room_without_its_back_wall(gpu_ready):
    """Rays can miss: a tile with such a ray is never sure, and the frames agree."""
    import cgraytracing_amd as cg
    objs = scenes.scene_c2()
    del objs[3]
    with cg.Scene(objs) as sc:
        on, sure, _ = _both(sc, 192, 108, 4, scenes.cam_dof())
        nhit = on[1]
        wy, wx = np.divmod(np.nonzero(sure != NONE)[0], (192 + 15) // 16)
        assert np.count_nonzero(nhit < 4) > 0, "no ray of this frame misses"
        for y, x in zip(wy, wx):
            assert np.all(nhit[4 * y:4 * y + 4, 16 * x:16 * x + 16] == 4), "a ray of sure wave tile (%d, %d) hit nothing" % (x, y)


def test_none_without_the_knob_or_the_masks(c2):
    cam = scenes.cam_dof()
    _launch(c2, 192, 108, 2, cam, True)
    assert c2.last_sure_tiles() is not None
    _launch(c2, 192, 108, 2, cam, False)
    assert c2.last_sure_tiles() is None and c2.last_sphere_masks() is not None
    _launch(c2, 192, 108, 2, cam, True, sphere_masks=False)
    assert c2.last_sure_tiles() is None and c2.last_sphere_masks() is None
    _launch(c2, 192, 108, 2, cam, True, tile_order=False)
    assert c2.last_sure_tiles() is None


def test_oracle_rays_of_sure_tiles_hit_the_winner_first(c2, orc):
    """C2 at 192x108, thin lens: the oracle's Hitpoints of a sure wave tile -- one per ray, at the ray's first hit, for a class-3
    tile's rays end there -- all lie on the tile's winner, and no ray of it goes without one."""
    W, H, spp, cam = 192, 108, 4, scenes.cam_dof()
    _launch(c2, W, H, spp, cam, True)
    sure = c2.last_sure_tiles()
    objs = scenes.scene_c2()
    o = BackendScene(orc, objs)
    want = o.trace_grid(cam, W, H, spp, 5, SEED, capture=True)
    o.close()
    row, w = np.divmod(want["hp_pix"], W)
    wt = (row // 4) * ((W + 15) // 16) + w // 16
    win = sure[wt]
    on_sure = win != NONE
    assert on_sure.sum() == np.count_nonzero(sure != NONE) * 64 * spp, "a ray of a sure wave tile left no Hitpoint, or more than one"
    assert on_sure.sum() > 10000
    pos = want["hp"][on_sure, 3:6]
    centre = np.array([objs[i].center for i in win[on_sure]])
    radius = np.array([objs[i].radius for i in win[on_sure]])
    resid = np.abs(np.linalg.norm(pos - centre, axis=1) - radius)
    assert resid.max() < 1e-6, "a ray of a sure wave tile hit another sphere first (%.3g off the winner)" % resid.max()


def test_benchmark_frame_share(c2):
    """The benchmark's frame, one sample: of the wave tiles of class-3 tiles at least 80 % are sure on the device's own bytes --
    the floor tests/native/sure_first.cpp sets for the same function on the CPU."""
    W, H = 1920, 1080
    _launch(c2, W, H, 1, scenes.cam_dof(), True)
    sure, order = c2.last_sure_tiles(), c2.last_tile_order()
    c3 = _class3_wave_tiles(order, W, H)
    assert len(c3) > 20000
    share = np.count_nonzero(sure[c3] != NONE) / len(c3)
    print("class-3 wave tiles %d, sure %d, share %.4f" % (len(c3), np.count_nonzero(sure[c3] != NONE), share))
    assert np.all(np.delete(sure, c3) == NONE)
    assert share >= 0.80
