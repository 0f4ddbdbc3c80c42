"""GPU: the pair form of the sphere loop and the class-3 tiles' diffuse body inside the one launch (CGRT_GRID_NO_SPHERE_PAIRS,
sphere_pairs=False).

The image-order launch of a sphere-only scene with a refracting sphere that the tile order serves tests its spheres two at a
time (sphere_len_pair: two independent instruction chains, the same operations per sphere), and in tile order its class-3
workgroups run the terminal-diffuse body inside the same kernel.  Neither changes an operation that reaches a result, so every
launch here is rendered with the switch on and off in one process and compared bit for bit -- rgb, per-pixel nhit and all
counters, the wave iterations (CGRT_CNT_WAVE_ITERS) among them -- and each scene once with the CPU oracle in the way
tests/test_gpu_tile_order.py does."""
import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32
from cgraytracing_amd.scene import Camera, Sphere

pytestmark = pytest.mark.gpu

SEED = 12345
NO_PAIRS = 256  # CGRT_GRID_NO_SPHERE_PAIRS
SIZES = [(200, 117), (96, 40)]  # neither a multiple of 32 nor of 8; 3 x 5 tiles
CAMS = {"pinhole": scenes.cam_pinhole, "thin_lens": scenes.cam_dof}


def _launch(sc, W, H, spp, cam, depth, pairs, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, depth, SEED, counters=cnt, sphere_pairs=pairs, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "nhit", "counters")):
        assert np.array_equal(x, y), "%s: %s differs between the pair form and the single form" % (what, name)


def _both(sc, W, H, spp, cam, depth=5, pair_expected=True, **kw):
    """The launch with the switch on and off: identical bits, and the variant names tell them apart.  Returns the default
    launch's results, its tile order and the tiles its in-kernel diffuse body took."""
    rows, stripe = kw.get("rows"), kw.get("stripe")
    v_on = sc.kernel_variant(W, H, spp, cam, depth, rows=rows, stripe=stripe)
    v_off = sc.kernel_variant(W, H, spp, cam, depth, rows=rows, stripe=stripe, flags=NO_PAIRS)
    assert ("PAIR=1" in v_on) == pair_expected and "PAIR" not in v_off, (v_on, v_off)
    on = _launch(sc, W, H, spp, cam, depth, True, **kw)
    taken, order = sc.last_inkernel_diffuse_tiles(), sc.last_tile_order()
    assert sc.last_diffuse_tiles() == 0, "the default launch issued a second launch"
    off = _launch(sc, W, H, spp, cam, depth, False, **kw)
    assert sc.last_inkernel_diffuse_tiles() == 0 and sc.last_diffuse_tiles() == 0, "sphere_pairs=False still ran the diffuse body"
    _same(on, off, "%dx%d spp %d depth %d %r" % (W, H, spp, depth, kw))
    return on, order, taken


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
def test_c2_pairs_equal_singles(c2, orc, W, H, lens):
    cam = CAMS[lens]()
    for spp in (1, 8):
        for depth in (1, 2, 5):
            # depth 1: no refracted ray exists, the launch takes the variant without pending rays and the switch changes nothing
            got, order, taken = _both(c2, W, H, spp, cam, depth, pair_expected=depth > 1)
            n = int(order["plan"][4])
            assert n == ((W + 31) // 32) * ((H + 7) // 8)
            assert taken == (n - int(order["plan"][3]) if depth > 1 else 0), "the diffuse body takes exactly class 3"
            assert depth == 1 or 0 < taken < n
    _vs_oracle(orc, scenes.scene_c2(), cam, W, H, 8, got)


def test_c2_default_switch_off_and_two_launches_agree(c2):
    """The one-launch form (default), the full body for every tile (switch off) and the two-launch form (diffuse_tiles=True,
    whose main launch is the pair variant too) give the same bits; each read-back answers for its own form only."""
    for W, H in SIZES:
        for cam in (scenes.cam_dof(), scenes.cam_pinhole()):
            on, order, taken = _both(c2, W, H, 8, cam)
            n3 = int(order["plan"][4]) - int(order["plan"][3])
            assert taken == n3 > 0
            two = _launch(c2, W, H, 8, cam, 5, True, diffuse_tiles=True)
            assert c2.last_diffuse_tiles() == n3 and c2.last_inkernel_diffuse_tiles() == 0
            _same(on, two, "two launches %dx%d" % (W, H))
            row_major = _launch(c2, W, H, 8, cam, 5, True, tile_order=False)  # the pair loop without the tile order: full body
            assert c2.last_inkernel_diffuse_tiles() == 0 and c2.last_tile_order() is None
            _same(on, row_major, "row-major %dx%d" % (W, H))


def test_lens_so_large_that_no_tile_is_class_3(c2):
    """Every tile is doubtful (the host sees it): the launch is the pair variant, no workgroup takes the diffuse body."""
    _, order, taken = _both(c2, 96, 40, 8, Camera(lens_radius=100.0))
    assert taken == 0 and order["plan"][3] == order["plan"][4] == 15


def _small(i, refl, transp):
    return Sphere((-14.0 + 3.5 * (i % 9), -12.0 + 5.0 * (i // 9) + (i % 3), 24 + 2 * (i % 5)), 1.5, (1.0, 0.9 - 0.05 * (i % 7), 0.8), refl, transp)


def _objects(n):
    """n objects: a glass sphere, a mirror sphere, C2's walls, small diffuse spheres -- the first n of that list."""
    objs = [Sphere((-8.0, -13.0, 25), 7, (1.0, 1.0, 1.0), 0.8, 0.5), Sphere((10.0, -13.0, 30), 7, (1.0, 1.0, 1.0), 0.8, 0.0)]
    objs += scenes.wall_spheres() + [_small(i, 0.0, 0.0) for i in range(4)]
    return objs[:n]


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9])
def test_object_counts(gpu_ready, orc, n):
    """A list of one (the odd tail alone), one pair, a pair and the tail, four pairs, four pairs and the tail."""
    import cgraytracing_amd as cg
    objs, cam = _objects(n), scenes.cam_dof()
    with cg.Scene(objs) as sc:
        for W, H in SIZES:
            got, order, _ = _both(sc, W, H, 8, cam)
            assert order is not None
    _vs_oracle(orc, objs, cam, W, H, 8, got)


@pytest.mark.parametrize("special", [16, 17])
def test_special_sphere_counts(gpu_ready, orc, special):
    """16 reflecting / refracting spheres: the tile order's limit, 21 objects (ten pairs and the tail).  17: the tile order does
    not serve the scene, the launch is the one-sphere-at-a-time variant and its name says so."""
    import cgraytracing_amd as cg
    objs = scenes.wall_spheres() + [_small(i, 0.8, 0.5 * (i % 2)) for i in range(special)]
    cam, (W, H) = scenes.cam_dof(), SIZES[1]
    with cg.Scene(objs) as sc:
        got, order, taken = _both(sc, W, H, 8, cam, pair_expected=special == 16)
        assert (order is not None) == (special == 16) and (special == 16 or taken == 0)
        _both(sc, SIZES[0][0], SIZES[0][1], 2, cam, pair_expected=special == 16)
    _vs_oracle(orc, objs, cam, W, H, 8, got)


@pytest.mark.parametrize("first", [6, 5])
def test_ties_go_to_the_earlier_sphere(gpu_ready, orc, first):
    """Two identical spheres, red then blue, at indices (6, 7) -- one pair -- and at (5, 6) -- the second of one pair and the
    first of the next: every ray that hits them hits both at the same distance, the earlier one wins (main.cpp:57), no pixel
    shows blue, and the pixel whose centre ray (pinhole, 96x40: pixel (48, 20) looks along +z) meets them is pure red."""
    import cgraytracing_amd as cg
    red, blue = Sphere((0.0, 0.0, 30), 3, (1.0, 0.0, 0.0), 0.0, 0.0), Sphere((0.0, 0.0, 30), 3, (0.0, 0.0, 1.0), 0.0, 0.0)
    glass, mirror = Sphere((-8.0, -13.0, 25), 7, (1.0, 1.0, 1.0), 0.8, 0.5), Sphere((10.0, -13.0, 30), 7, (1.0, 1.0, 1.0), 0.8, 0.0)
    objs = scenes.wall_spheres() + ([glass, red, blue, mirror] if first == 6 else [red, blue, glass, mirror])
    assert objs[first] is red and objs[first + 1] is blue
    with cg.Scene(objs) as sc:
        for cam in (scenes.cam_pinhole(), scenes.cam_dof()):
            got, _, _ = _both(sc, 96, 40, 1, cam)
            _vs_oracle(orc, objs, cam, 96, 40, 1, got)
        rgb = _both(sc, 96, 40, 1, scenes.cam_pinhole())[0][0]
    assert tuple(rgb[20, 48]) == (1.0, 0.0, 0.0), rgb[20, 48]
    only_red = [o for o in objs if o is not blue]
    with cg.Scene(only_red) as sc:
        want = _launch(sc, 96, 40, 1, scenes.cam_pinhole(), 5, True)[0]
    assert np.array_equal(rgb, want), "the frame differs from the one without the blue twin"


def test_camera_inside_a_glass_sphere_and_a_tangent_centre_ray(gpu_ready, orc):
    """The camera (0, 0, -10) inside a glass sphere: every primary ray has t0 < 0 and takes t1.  Pinhole, 96x40: pixel (48, 20)
    looks along +z exactly, and the sphere of radius 2 centred at (2, 0, 20) touches that ray -- l2 = 904, tca^2 = 900,
    d2 = r2 = 4 exactly, so r2 - d2 == 0 and the wave takes the library root for that sphere."""
    import cgraytracing_amd as cg
    inside = scenes.wall_spheres() + [Sphere((0.5, 0.5, -9.0), 3, (1.0, 1.0, 1.0), 0.8, 0.5), Sphere((10.0, -13.0, 30), 7, (1.0, 1.0, 1.0), 0.8, 0.0)]
    tangent = scenes.wall_spheres() + [Sphere((2.0, 0.0, 20), 2, (0.2, 0.9, 0.3), 0.0, 0.0), Sphere((-8.0, -13.0, 25), 7, (1.0, 1.0, 1.0), 0.8, 0.5),
                                       Sphere((-2.0, 0.0, 26), 2, (0.9, 0.2, 0.3), 0.0, 0.0)]
    for objs in (inside, tangent):
        with cg.Scene(objs) as sc:
            for cam in (scenes.cam_pinhole(), scenes.cam_dof()):
                got, _, _ = _both(sc, 96, 40, 4, cam)
                _vs_oracle(orc, objs, cam, 96, 40, 4, got)


def test_striped_launch_and_progressive_passes(c2):
    import torch
    W, H = SIZES[0]
    cam = scenes.cam_dof()
    for rank in range(2):
        _both(c2, W, H, 8, cam, rows=64, stripe=(16, rank, 2))
    frames = []
    for pairs in (True, False):
        out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        for k in range(4):
            _, nhit, _ = c2.trace_grid(W, H, 2, cam, 5, SEED, sample_offset=2 * k, spp_total=8, out=out, counters=cnt, accumulate=True,
                                       sphere_pairs=pairs)
        torch.cuda.synchronize()
        assert (c2.last_inkernel_diffuse_tiles() > 0) == pairs
        frames.append((out.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()))
    _same(frames[0], frames[1], "accumulate 4 x 2 samples")
