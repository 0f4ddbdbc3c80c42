"""CPU: the scenes of test_gpu_deep_trees.py reach the states they are there for, shown from the oracle alone.

The eye kernels keep a lane's waiting refracted rays (main.cpp:157) on a stack of three levels; the third is used only when the
primary ray, its reflected child and that child's reflected child all split.  The oracle says per primary ray how deep its tree
went (orc_trace_trees, oracle/cgrt_testapi.h): `max_pending`, the largest number of refracted children with depth_left >= 2
that waited at once (3 = the third level), and `path_mask`, which path labels were traced (labels >= 16 are the rays of the
last level).  With the camera INSIDE a glass sphere every primary ray meets glass from within at the same angle of incidence
at every bounce, so the reflected chain splits at every level: every ray holds three pending rays and then a leaf sibling.

DEEP_SCENES is the list both files use.  The shares asserted here are conditions on the scenes, not measurements of the code
under test: if a scene is changed until it no longer fills the stack, this file fails and the GPU file cannot pass vacuously.
The measured shares are printed and recorded in DESIGN.md (section 13)."""
import numpy as np
import pytest

import scenes
from backends import BackendScene
from cgraytracing_amd.scene import Camera, Sphere, TriangleMesh

W, H, SEED = 64, 48, 12345
KLDS = 768  # kLdsObjsMax (test_gpu_object_counts.KLDS): the eye pass and the ray list spill beyond it


def glass_around_camera():
    """The default camera (0, 0, -10) lies 4.6 units from the centre of this sphere of radius 9: inside, off centre"""
    return Sphere((2.0, 1.0, -6.0), 9, (1.0, 1.0, 1.0), 0.8, 0.5)


def inside_glass():
    return scenes.planes() + [glass_around_camera()]


def inside_glass_c2():
    return scenes.scene_c2() + [glass_around_camera()]


def glass_cluster():
    """3 x 3 glass spheres of radius 5, 0.3 apart, centred on the axis at z = 28: rays that enter a gap are reflected from
    sphere to sphere.  Seen through a narrow field (half_width 3) so that the block fills the frame."""
    step = 2 * 5.0 + 0.3
    return scenes.planes() + [Sphere(((i - 1) * step, (j - 1) * step, 28.0), 5, (1.0, 1.0, 1.0), 0.8, 0.5)
                              for j in range(3) for i in range(3)]


def inside_glass_mesh():
    """A closed glass mesh of 224 triangles around the camera, radius 9 +- 7.5 %: a reference tree of 63 nodes, which every
    workgroup keeps in LDS (<= kNodeCache = 256)"""
    tris = scenes.procedural_mesh(16, 8, (0.0, 0.0, -10.0), 9.0)
    return scenes.planes() + [TriangleMesh.from_triangles(tris, (1.0, 1.0, 1.0), 0.8, 0.5)]


def inside_glass_spill():
    """KLDS + 1 objects, the sphere around the camera last: it is read from beyond the LDS list on every ray"""
    objs = scenes.many_spheres(KLDS, 31, head=scenes.planes()) + [glass_around_camera()]
    assert len(objs) == KLDS + 1
    return objs


def inside_glass_vase():
    return inside_glass() + [scenes.vase_bezier()]


def _cams(**kw):
    return (("pinhole", Camera(**kw)), ("thin_lens", Camera(lens_radius=1.5, **kw)))


DEEP_SCENES = [
    # name, scene factory, ((camera name, camera), ...)
    ("inside_glass", inside_glass, _cams()),
    ("inside_glass_c2", inside_glass_c2, _cams()),
    ("glass_cluster", glass_cluster, _cams(half_width=3.0)),
    ("inside_glass_mesh", inside_glass_mesh, _cams()),
    ("inside_glass_spill", inside_glass_spill, _cams()),
    ("inside_glass_vase", inside_glass_vase, _cams()),
]
DEEP_IDS = [c[0] for c in DEEP_SCENES]

_TREES = {}


def trees(orc, name, mk, cam_name, cam, spp=1, depth=5, seed=SEED):
    """The oracle's eye pass with the tree shapes, computed once per (scene, camera, spp, depth, seed) and shared."""
    key = (name, cam_name, spp, depth, seed)
    if key not in _TREES:
        o = BackendScene(orc, mk())
        _TREES[key] = o.trace_trees(cam, W, H, spp, depth, seed)
        o.close()
    return _TREES[key]


def shares(r):
    """(share of rays with max_pending == 3, share with a path label >= 16, Hitpoints per ray: min, max)"""
    return (float((r["max_pending"] == 3).mean()), float(((r["path_mask"] >> 16) != 0).mean()),
            int(r["ray_nhit"].min()), int(r["ray_nhit"].max()))


def test_inside_glass_fills_the_stack_on_every_ray(orc):
    name, mk, cams = DEEP_SCENES[0]
    for cam_name, cam in cams:
        r = trees(orc, name, mk, cam_name, cam)
        print("%s %s: max_pending == 3: %.4f, label >= 16: %.4f, Hitpoints per ray %d..%d" % ((name, cam_name) + shares(r)))
        assert (r["max_pending"] == 3).all()
        assert (r["ray_nhit"] == 4).all()
        # the reflected chain 1, 2, 4, 8, 16 and the refracted child of each of its members
        assert (r["path_mask"] == sum(1 << p for p in (1, 2, 3, 4, 5, 8, 9, 16, 17))).all()
    # what each depth gives: the chain stops one level earlier, the rays that leave the sphere end on a wall
    for depth, pend, nhit in ((1, 0, 0), (2, 0, 1), (3, 1, 2), (4, 2, 3), (5, 3, 4)):
        r = trees(orc, name, mk, "pinhole", cams[0][1], depth=depth)
        print("%s depth %d: max_pending %s, Hitpoints per ray %s" % (name, depth, np.unique(r["max_pending"]), np.unique(r["ray_nhit"])))
        assert (r["max_pending"] == pend).all() and (r["ray_nhit"] == nhit).all()


@pytest.mark.parametrize("name,mk,cams", DEEP_SCENES[1:], ids=DEEP_IDS[1:])
def test_every_scene_reaches_the_third_level(orc, name, mk, cams):
    for cam_name, cam in cams:
        third, last, lo, hi = shares(trees(orc, name, mk, cam_name, cam))
        print("%s %s: max_pending == 3: %.4f, label >= 16: %.4f, Hitpoints per ray %d..%d" % (name, cam_name, third, last, lo, hi))
        assert third >= 0.10, "fewer than 10 % of the rays hold three pending rays"
        assert last >= 0.10, "fewer than 10 % of the rays trace a ray of the last level (path label >= 16)"


@pytest.mark.parametrize("name,mk,cams", DEEP_SCENES, ids=DEEP_IDS)
def test_counter_changes_nothing_and_agrees_with_the_labels(orc, name, mk, cams):
    """orc_trace_trees is orc_trace_grid observed: the same accumulator, counts and rays.  The two observations are tied to
    each other: three refracted children can wait at once only as the children 3, 5 and 9 of the chain 1, 2, 4, so
    max_pending == 3 exactly when those three labels were traced; and a ray's Hitpoints sum to its pixel's."""
    cam_name, cam = cams[1]
    spp = 2
    r = trees(orc, name, mk, cam_name, cam, spp=spp)
    o = BackendScene(orc, mk())
    want = o.trace_grid(cam, W, H, spp, 5, SEED)
    o.close()
    assert r["nrays"] == want["nrays"] and np.array_equal(r["nhit"], want["nhit"]) and np.array_equal(r["acc_sum"], want["acc_sum"])
    assert np.array_equal(r["ray_nhit"].reshape(spp, H, W).sum(axis=0), want["nhit"])
    m = r["path_mask"]
    assert (m & 2 == 2).all() and (m & 1 == 0).all()  # label 1 always, label 0 never
    chain = sum(1 << p for p in (3, 5, 9))
    assert np.array_equal(r["max_pending"] == 3, (m & chain) == chain)
    assert np.array_equal(r["max_pending"] == 0, (m & (1 << 3 | 1 << 5 | 1 << 7 | 1 << 9 | 1 << 11 | 1 << 13 | 1 << 15)) == 0)
    # every traced ray but the primary has its parent traced
    for p in range(2, 32):
        assert not ((m >> p & 1) & ~(m >> (p // 2) & 1)).any(), p
    assert int(np.array([bin(int(x)).count("1") for x in m]).sum()) == r["nrays"]


def test_shares_of_the_parity_cases(orc):
    """The same counter over test_gpu_parity.CASES at their own sizes, and the 1 000-sphere scene of the object-count tests:
    how much of the pending-ray stack the suite exercised before this file (the table of DESIGN.md section 13).  Only the
    glass bunny (2 rays of 65 536) and the sphere crowd (33 of 12 288) reach the third level at all."""
    from test_gpu_parity import CASES
    rows = list(CASES)
    rows.append(("many_spheres_1000", lambda: scenes.many_spheres(1000, 11), scenes.cam_dof, 96, 64, 2, 5))
    print()
    for name, mk, cam, w, h, spp, depth in rows:
        o = BackendScene(orc, mk())
        r = o.trace_trees(cam(), w, h, spp, depth, SEED)
        o.close()
        p, m = r["max_pending"], r["path_mask"]
        print("%-26s %4dx%-4d spp %d depth %d: rays %7d, max_pending 1 / 2 / 3: %.5f / %.5f / %.5f (%d rays), label >= 16: %.5f, "
              "Hitpoints per ray <= %d" % (name, w, h, spp, depth, len(p), (p == 1).mean(), (p == 2).mean(), (p == 3).mean(),
                                           int((p == 3).sum()), ((m >> 16) != 0).mean(), r["ray_nhit"].max()))
        assert (m & 2 == 2).all() and p.max() <= 3
        if name in ("c1_spheres_depth1", "pyramid_diffuse", "dragon_diffuse"):
            assert p.max() == 0
