"""GPU: the terminal-diffuse launch for a sphere-only scene's class-3 tiles (CGRT_GRID_DIFFUSE_TILES, diffuse_tiles=True).

An image-order launch over a sphere-only scene in tile order can hand the tiles none of whose primary rays can reach a reflecting
or refracting sphere (class 3 of tile_order_kernel) to a second launch beside the main one: a kernel variant in which every ray
ends at its first hit.  Both variants compute a pixel with the same operations in the same order, so every launch here is
rendered with the path on and with it off in one process and compared bit for bit -- rgb, per-pixel nhit and all counters --
and with the CPU oracle at the bar of test_trace_grid_matches_oracle.  How many tiles the second launch took is read back
(Scene.last_diffuse_tiles) and compared with the tile order's own class boundaries (Scene.last_tile_order)."""
import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32
from cgraytracing_amd.scene import Camera, Sphere

pytestmark = pytest.mark.gpu

SEED = 12345
DIFFUSE = 128  # CGRT_GRID_DIFFUSE_TILES
SIZES = [(96, 40), (200, 72)]  # 3 x 5 tiles; 7 x 9 tiles with a part column (200 is no multiple of 32)
CAMS = {"pinhole": scenes.cam_pinhole, "thin_lens": scenes.cam_dof}


def _launch(sc, W, H, spp, cam, depth, diffuse_tiles, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, depth, SEED, counters=cnt, diffuse_tiles=diffuse_tiles, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _same(on, off, what):
    for a, b, name in zip(on, off, ("rgb", "nhit", "counters")):
        assert np.array_equal(a, b), "%s: %s differs between the diffuse-tile launch and the single launch" % (what, name)


def _both(sc, W, H, spp, cam, depth=5, **kw):
    """The launch with the path on and off: identical bits.  Returns (results, tile order, tiles of the diffuse launch)."""
    on = _launch(sc, W, H, spp, cam, depth, True, **kw)
    taken, order = sc.last_diffuse_tiles(), sc.last_tile_order()
    off = _launch(sc, W, H, spp, cam, depth, False, **kw)
    assert sc.last_diffuse_tiles() == 0, "diffuse_tiles=False still issued the second launch"
    _same(on, off, "%dx%d spp %d depth %d %r" % (W, H, spp, depth, kw))
    return on, order, taken


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("lens", sorted(CAMS))
@pytest.mark.parametrize("W,H", SIZES)
def test_c2_on_equals_off(c2, W, H, lens):
    cam = CAMS[lens]()
    name = c2.diffuse_variant(W, H, 8, cam, 5, flags=DIFFUSE)
    assert "DIFF=1" in name and ("DOF=%d" % (lens == "thin_lens")) in name
    assert c2.diffuse_variant(W, H, 8, cam, 5) == ""  # the path is opt-in
    for spp in (1, 8):
        for depth in (1, 2, 5):
            _, order, taken = _both(c2, W, H, spp, cam, depth)
            n = int(order["plan"][4])
            assert n == ((W + 31) // 32) * ((H + 7) // 8)
            assert 0 < taken < n and taken == n - int(order["plan"][3]), "the second launch takes exactly class 3"


def test_c2_sample_offset(c2):
    for W, H in SIZES:
        _both(c2, W, H, 8, scenes.cam_dof(), sample_offset=24, spp_total=64)


def test_c2_accumulate_over_two_calls(c2):
    import torch
    cam = scenes.cam_dof()
    for W, H in SIZES:
        frames = []
        for diffuse_tiles in (True, False):
            out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
            for k in range(2):
                _, nhit, _ = c2.trace_grid(W, H, 4, cam, 5, SEED, sample_offset=4 * k, spp_total=8, out=out, counters=cnt,
                                           accumulate=True, diffuse_tiles=diffuse_tiles)
            torch.cuda.synchronize()
            assert (c2.last_diffuse_tiles() > 0) == diffuse_tiles
            frames.append((out.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()))
        _same(frames[0], frames[1], "accumulate %dx%d" % (W, H))


def test_c2_two_share_stripes_of_8_rows(c2):
    for W, H in SIZES:
        rows = ((H + 15) // 16) * 8  # each share's local rows: its 8-row stripes, the last may reach beyond the image
        for rank in range(2):
            _, order, taken = _both(c2, W, H, 8, scenes.cam_dof(), rows=rows, stripe=(8, rank, 2))
            assert taken == int(order["plan"][4]) - int(order["plan"][3])


def test_lens_so_large_that_no_tile_is_class_3(c2):
    """lens_radius 100: the glass sphere's bound (7 at 38 units from the camera) grows by 100 x 0.4 and holds the camera, so every
    tile is doubtful -- the host sees that without the device's answer and issues no second launch."""
    cam = Camera(lens_radius=100.0)
    W, H = 96, 40
    assert c2.diffuse_variant(W, H, 8, cam, 5, flags=DIFFUSE) == ""
    _, order, taken = _both(c2, W, H, 8, cam)
    assert taken == 0
    assert order["plan"][3] == order["plan"][4] == 15


def test_special_spheres_behind_the_camera(gpu_ready):
    """Pinhole (behind a thin lens a sphere is doubtful for every tile): no primary ray can reach them, every tile is class 3 and
    every workgroup of the main launch leaves at once."""
    import cgraytracing_amd as cg
    objs = scenes.scene_c2()
    objs[6] = Sphere((10.0, -13.0, -50), 7, (1.0, 1.0, 1.0), 0.8, 0.0)
    objs[7] = Sphere((-8.0, -13.0, -45), 7, (1.0, 1.0, 1.0), 0.8, 0.5)
    sc = cg.Scene(objs)
    try:
        for W, H in SIZES:
            _, order, taken = _both(sc, W, H, 8, scenes.cam_pinhole())
            assert order["plan"][3] == 0 and taken == int(order["plan"][4]) == ((W + 31) // 32) * ((H + 7) // 8)
    finally:
        sc.close()


def test_c1_takes_the_old_path(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c1())
    try:
        assert sc.diffuse_variant(96, 40, 8, scenes.cam_dof(), 5, flags=DIFFUSE) == ""
        _, order, taken = _both(sc, 96, 40, 8, scenes.cam_dof())
        assert order is None and taken == 0, "a diffuse-only scene took an extra launch"
    finally:
        sc.close()


def test_seventeen_special_spheres_take_the_old_path(gpu_ready):
    import cgraytracing_amd as cg
    objs = scenes.wall_spheres() + [Sphere((-16.0 + 2.0 * i, -10.0 + (i % 3), 30 + i), 1.5, (1.0, 1.0, 1.0), 0.8, 0.5 * (i % 2))
                                    for i in range(17)]
    sc = cg.Scene(objs)
    try:
        assert sc.diffuse_variant(96, 40, 8, scenes.cam_dof(), 5, flags=DIFFUSE) == ""
        _, order, taken = _both(sc, 96, 40, 8, scenes.cam_dof())
        assert order is None and taken == 0
    finally:
        sc.close()


def test_class_3_tiles_on_every_side_of_a_special_tile(gpu_ready):
    """A small glass sphere on the focus plane at the image's centre (pixel (48, 20) of 96x40: the corner of four wave tiles).  The
    classification looks at cones around 16x4 wave tiles, 1.5 x their half-angle wide, so at this image size only a bound this
    small leaves a class-3 tile above and below: the middle column's rows 1-3 are class 0/1, every tile round them class 3."""
    import cgraytracing_amd as cg
    objs = scenes.wall_spheres() + [Sphere((0.0, 0.0, 20), 0.25, (1.0, 1.0, 1.0), 0.8, 0.5)]
    sc = cg.Scene(objs)
    try:
        for cam in (scenes.cam_dof(), scenes.cam_pinhole()):
            _, order, taken = _both(sc, 96, 40, 8, cam)
            cls = order["cls"].reshape(5, 3)
            special = cls < 3
            assert special.any() and taken == int((~special).sum())
            sides = {"left": (0, -1), "right": (0, 1), "above": (-1, 0), "below": (1, 0)}
            for name, (dy, dx) in sides.items():
                found = any(special[y, x] and 0 <= y + dy < 5 and 0 <= x + dx < 3 and not special[y + dy, x + dx]
                            for y in range(5) for x in range(3))
                assert found, "no class-3 tile borders a special tile on the %s: %r" % (name, cls)
    finally:
        sc.close()


def test_thin_lens_96x40_matches_oracle(c2, orc):
    W, H, spp = 96, 40, 8
    cam, objs = scenes.cam_dof(), scenes.scene_c2()
    rgb, nhit, cnt = _launch(c2, W, H, spp, cam, 5, True)
    assert c2.last_diffuse_tiles() > 0
    o = BackendScene(orc, objs)
    want = o.trace_grid(cam, W, H, spp, 5, seed=SEED)
    o.close()
    assert int(cnt[0]) == want["nrays"], "ray count"
    assert int(cnt[1]) == int(want["nhit"].sum()), "hitpoint count"
    assert np.array_equal(nhit, want["nhit"]), "per-pixel hitpoint counts"
    ref32 = to_acc32(want["acc_sum"], spp)
    diff = np.abs(rgb.astype(np.float64) - ref32.astype(np.float64))
    exact = float((rgb == ref32).mean())
    print("diffuse tiles vs oracle: Linf=%.3e exact=%.6f" % (diff.max(), exact))
    assert diff.max() <= 1e-6 and exact > 0.999


def test_hitpoint_capture_never_takes_the_diffuse_body(c2):
    """trace_grid_hitpoints has no switch of its own: its launch is the general HPS variant whatever the grid call did before."""
    W, H, spp, cam = 96, 40, 2, scenes.cam_dof()
    assert "HPS=1" in c2.kernel_variant(W, H, spp, cam, hitpoints=True)
    caps = []
    for diffuse_tiles in (True, False):
        _launch(c2, W, H, spp, cam, 5, diffuse_tiles)
        hp = c2.trace_grid_hitpoints(W, H, spp, cam, 5, SEED)
        key = np.lexsort((hp["seq"], hp["smp"], hp["pix"])) if "seq" in hp else np.lexsort((hp["smp"], hp["pix"]))
        caps.append((hp["count"], hp["hp"][key], hp["pix"][key], hp["smp"][key]))
    assert caps[0][0] == caps[1][0]
    for a, b in zip(caps[0][1:], caps[1][1:]):
        assert np.array_equal(a, b)
