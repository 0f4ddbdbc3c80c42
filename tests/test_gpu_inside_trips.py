"""GPU: the inside trips of the pair kernels' sphere loop (CGRT_GRID_NO_INSIDE_TRIPS, inside_trips=False).

An iteration in which every lane's ray starts inside the scene's refracting sphere tests only the spheres of that sphere's mask
(cgrt_inside_sphere.h), one by one, instead of all of them two at a time.  Nothing may change: every launch here is rendered with
the guarded loop and with the pair loop alone in one process and compared bit for bit -- rgb, per-pixel nhit and all eight
counters, CGRT_CNT_WAVE_ITERS among them.  The loop itself is run on chosen rays through Scene.inside_probe, and the trait is read
back (Scene.inside_spheres) and compared with the header's rule recomputed here."""
import math

import numpy as np
import pytest

import scenes
from cgraytracing_amd import Camera, Sphere

pytestmark = pytest.mark.gpu

SEED = 12345
W, H = 192, 108
GLASS, MIRROR = 7, 6
K_EPS = 1e-4


def _rin2(r):
    r_in = r * (1 - 1e-9) - 1e-6
    return r_in * r_in


def _launch(sc, cam, inside, spp=8, depth=5, w=W, h=H, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(w, h, spp, cam, depth, SEED, counters=cnt, inside_trips=inside, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _both(sc, cam, **kw):
    on = _launch(sc, cam, True, **kw)
    off = _launch(sc, cam, False, **kw)
    for a, b, what in zip(on, off, ("rgb", "nhit", "counters")):
        assert np.array_equal(a, b), "%r: %s differs between the guarded loop and the pair loop\n%r\n%r" % (kw, what, a if what == "counters" else "", b if what == "counters" else "")
    assert on[2][0] > 0 and np.count_nonzero(on[0]) > 0
    return on


def _scene(objs):
    import cgraytracing_amd as cg
    return cg.Scene(objs)


def _c2_with(glass=None, extra=(), insert=None, mirror_transp=None):
    objs = scenes.scene_c2()
    if glass is not None:
        objs[GLASS] = Sphere(glass, 7, (1.0, 1.0, 1.0), 0.8, 0.5)
    if mirror_transp is not None:
        objs[MIRROR] = Sphere((10.0, -13.0, 30), 7, (1.0, 1.0, 1.0), 0.8, mirror_transp)
    objs = objs + list(extra)
    if insert is not None:
        objs.insert(insert[0], insert[1])
    return objs


Y_TOUCH = -10020 + math.sqrt(10007.0 * 10007.0 - 64 - 625)  # the glass sphere's centre when it touches the floor sphere

# name -> (objects, the trait Scene.inside_spheres() must report: [(index, mask)] )
SCENES = {
    "c2": (lambda: scenes.scene_c2(), [(GLASS, 1 << GLASS)]),
    "touching_floor": (lambda: _c2_with(glass=(-8.0, Y_TOUCH, 25)), [(GLASS, (1 << GLASS) | 1)]),
    "overlapping_floor": (lambda: _c2_with(glass=(-8.0, Y_TOUCH - 0.5, 25)), [(GLASS, (1 << GLASS) | 1)]),
    "overlapping_mirror": (lambda: _c2_with(glass=(0.0, -13.0, 28)), [(GLASS, (1 << GLASS) | (1 << MIRROR))]),
    "diffuse_inside_glass": (lambda: _c2_with(extra=[Sphere((-5.0, -13.0, 25), 2, (0.9, 0.2, 0.2), 0.0, 0.0)]), [(GLASS, (1 << GLASS) | (1 << 8))]),
    "glass_inside_glass": (lambda: _c2_with(insert=(5, Sphere((-8.0, -12.0, 25), 12, (1.0, 1.0, 1.0), 0.8, 0.5))), []),
    "two_glass": (lambda: _c2_with(mirror_transp=0.5), []),
    "one_glass_too_many": (lambda: _c2_with(extra=[Sphere((-12.0, 5.0, 30.0), 1.0, (1.0, 1.0, 1.0), 0.8, 0.5)]), []),
}


@pytest.fixture(scope="module")
def c2(gpu_ready):
    sc = _scene(scenes.scene_c2())
    yield sc
    sc.close()


def test_trait_read_back(c2):
    """C2: the glass sphere, alone in its mask, r_in as the header takes it; a mesh scene has no trait."""
    assert c2.inside_spheres() == [dict(index=GLASS, mask=1 << GLASS, rin2=_rin2(7.0))]
    assert "PAIR=1" in c2.kernel_variant(W, H, 8, scenes.cam_dof(), 5)
    sc = _scene(scenes.scene_pyramid())
    try:
        assert sc.inside_spheres() == []
    finally:
        sc.close()


@pytest.mark.parametrize("lens", [True, False])
@pytest.mark.parametrize("kw", [dict(), dict(depth=2), dict(lens_table=True), dict(rows=56, stripe=(8, 1, 2)),
                                dict(spp=32, sample_relay=True, relay_start="cost"),
                                dict(spp=32, sample_relay=True, relay_start="cost", lens_table=True)],
                         ids=["plain", "depth2", "ltab", "stripe", "relay_cost", "relay_cost_ltab"])
def test_c2_guarded_loop_equals_pair_loop(c2, lens, kw):
    cam = scenes.cam_dof() if lens else scenes.cam_pinhole()
    _both(c2, cam, **kw)
    if "sample_relay" in kw:
        assert c2.last_sample_relay()["tiles"] > 0, "the relay did not run: no parking body"
        assert c2.last_relay_start() is not None, "no start table: no START twin"
    if lens and kw.get("lens_table"):
        assert c2.last_lens_table()["entries"] > 0, "no lens table: no LTAB twin"


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_that_change_the_mask(gpu_ready, name):
    build, want = SCENES[name]
    sc = _scene(build())
    try:
        got = sc.inside_spheres()
        assert [(t["index"], t["mask"]) for t in got] == want, got
        _both(sc, scenes.cam_dof())
        _both(sc, scenes.cam_pinhole())
    finally:
        sc.close()


def test_camera_inside_the_glass_sphere(c2):
    """A pinhole camera at the glass sphere's centre and one kEps inside its shell: the primary rays are inside rays."""
    _both(c2, Camera(cam=(-8.0, -13.0, 25.0)))
    _both(c2, Camera(cam=(-8.0, -13.0, 25.0 - 7 + K_EPS)))
    _both(c2, Camera(cam=(-8.0, -13.0, 25.0), lens_radius=1.5, focus_plane=40.0))


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _probe_rays(objs, rng, n_waves):
    """Waves of 64 rays whose origins all lie inside the glass sphere -- on the shell r - kEps, on the shell at r_in, at the centre,
    anywhere inside -- in random directions, aimed at every other sphere's nearest point, tangential, along the centre lines."""
    c, r = np.asarray(objs[GLASS].center, np.float64), objs[GLASS].radius
    n = 64 * n_waves
    u = _unit(rng.standard_normal((n, 3)))
    kind = rng.integers(0, 4, n)
    rad = np.where(kind == 0, r - K_EPS, np.where(kind == 1, math.sqrt(_rin2(r)) * (1 - 1e-12), np.where(kind == 2, 0.0, r * 0.999 * rng.random(n) ** (1 / 3))))
    o = c + u * rad[:, None]
    d = _unit(rng.standard_normal((n, 3)))
    others = np.asarray([s.center for i, s in enumerate(objs) if i != GLASS], np.float64)
    pick = others[rng.integers(0, len(others), n)]
    how = rng.integers(0, 4, n)
    aimed = _unit(pick - o)
    line = _unit(pick - c) * np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
    t = rng.standard_normal((n, 3))
    tang = _unit(t - u * np.sum(t * u, axis=1, keepdims=True))
    d = np.where((how == 1)[:, None], aimed, np.where((how == 2)[:, None], line, np.where((how == 3)[:, None], tang, d)))
    return np.concatenate([o, d], axis=1)


@pytest.mark.parametrize("name", ["c2", "touching_floor", "diffuse_inside_glass"])
def test_probe_guarded_loop_bit_for_bit(gpu_ready, name):
    """About 1e5 rays: waves all of whose rays start inside the glass sphere take the one-by-one loop and end on the pair loop's
    (t, id) to the bit; waves with one ray from outside, and whole waves of camera rays, take the pair loop."""
    objs = SCENES[name][0]()
    rng = np.random.default_rng(7)
    rays = _probe_rays(objs, rng, 1600)
    n_in = len(rays)
    mixed = _probe_rays(objs, rng, 64)
    mixed[::64, :3] = (0.0, 0.0, -10.0)  # lane 0 of every such wave starts at the camera
    outside = np.concatenate([np.tile((0.0, 0.0, -10.0), (64 * 16, 1)), _unit(rng.standard_normal((64 * 16, 3)) + (0, 0, 3.0))], axis=1)
    rays = np.concatenate([rays, mixed, outside])
    sc = _scene(objs)
    try:
        out = sc.inside_probe(rays)
    finally:
        sc.close()
    assert np.array_equal(out[:, 0].view(np.uint64), out[:, 2].view(np.uint64)), "t differs"
    assert np.array_equal(out[:, 1], out[:, 3]), "id differs"
    assert np.all(out[:n_in, 4] == 1.0), "a wave of inside rays took the pair loop"
    assert np.all(out[n_in:, 4] == 0.0), "a wave with a ray from outside took the one-by-one loop"
    assert np.all(out[:n_in, 1] >= 0) and np.all(out[:n_in, 0] < 14.0 + 1e-3), "an inside ray does not leave within 2 r"
    ids = set(int(i) for i in out[:n_in, 1])
    mask = SCENES[name][1][0][1]
    assert ids <= {i for i in range(32) if mask >> i & 1}, "a first hit outside the mask: %r" % ids
    assert GLASS in ids
