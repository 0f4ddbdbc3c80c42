"""GPU: the bounds the device holds for a committed opaque mesh -- bounding sphere (ObjRec::a, s0), TreeRec::bmax and the cover
spheres -- read back by cgrt_scene_mesh_bounds_host (Scene.mesh_bounds) after a commit, a refit and a rebuild, and held to numpy.

Frames see these values only through early-outs and tile classes: a sphere that is too large changes no pixel and one that is
too small may not either, so they are compared here directly, BIT FOR BIT.  numpy uses the kernels' own operations (min / max,
0.5 * (lo + hi), dx*dx + dy*dy + dz*dz left to right, sqrt, + 1e-3, (1 + 1e-9), tree_bmax's factors); each of them is exactly
rounded and the library is compiled without contraction, so equality is the expectation and the assertion.

A cover sphere belongs to a contiguous range [g n / G, (g + 1) n / G) of the hierarchy's triangle order: bvh_order for a
device-built tree (its k is the construction index), refit_plan's src for a host-built one (k is the leaf-order index there).  A
host-built mesh's spheres come from median splits at the commit and from those ranges only once it has been refitted, which is
what is checked for build="host"."""
import numpy as np
import pytest

from test_gpu_refit import MESH, PAD, _deform, _objs, _refit, _soup_of
from test_gpu_rebuild import DEV, _rebuild

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 5, 63, 64, 127, 128, 129, 300, 16500]


def _cover_groups(n):
    """devbuild::cover_groups: halve while a half keeps 64 triangles, six times at the most."""
    depth = 0
    while depth < 6 and (n >> (depth + 1)) >= 64:
        depth += 1
    return 1 << depth


GROUPS = {n: _cover_groups(n) for n in SIZES}
assert [GROUPS[n] for n in (127, 128, 300, 16500)] == [1, 2, 4, 64]  # (64 is the most there is: from 8 192 triangles on)


def _d2(P, c):
    d = P - c
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def _sphere(P):
    """(centre of the box of points P, largest squared distance from it)"""
    c = 0.5 * (P.min(0) + P.max(0))
    return c, _d2(P, c).max()


def _numpy_bounds(tris, order, G):
    V = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    n = len(V)
    P = V.reshape(-1, 3)
    c, r2 = _sphere(P)
    r = np.sqrt(r2) + 1e-3
    m = max(np.abs(P.min(0)).max(), np.abs(P.max(0)).max())
    bmax = np.float32((m + 2 * PAD) * (1 + 1e-6)) * (np.float32(1.0) + np.float32(1e-6))
    cover = np.zeros((G, 4))
    for g in range(G):
        cg, g2 = _sphere(V[order[g * n // G:(g + 1) * n // G]].reshape(-1, 3))
        cover[g, :3], cover[g, 3] = cg, np.sqrt(g2) + 1e-3
    return dict(centre=c, s0=r * r * (1 + 1e-9), bmax=bmax, cover=cover)


def _same(got, want, what):
    for k in ("centre", "cover"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), "%s: %s\n%r\n%r" % (what, k, got[k], want[k])
    assert np.float64(got["s0"]).tobytes() == np.float64(want["s0"]).tobytes(), "%s: s0 %r %r" % (what, got["s0"], want["s0"])
    assert got["bmax"].dtype == np.float32 and got["bmax"].tobytes() == np.float32(want["bmax"]).tobytes(), "%s: bmax %r %r" % (what, got["bmax"], want["bmax"])


def _contains(b, tris, order):
    """Check 5: every vertex inside the bounding sphere and inside its range's cover sphere."""
    V = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    n, G = len(V), len(b["cover"])
    assert (_d2(V.reshape(-1, 3), b["centre"]) <= b["s0"]).all()
    for g in range(G):
        P = V[order[g * n // G:(g + 1) * n // G]].reshape(-1, 3)
        assert len(P) and (np.sqrt(_d2(P, b["cover"][g, :3])) <= b["cover"][g, 3]).all(), g


def _order(sc):
    return sc.bvh_order(0)[1].copy()


@pytest.mark.parametrize("n", SIZES)
def test_identity_updates_leave_the_bounds_bit_equal(gpu_ready, n):
    """Checks 1, 3, 5: commit, identity refit and identity rebuild of a device-built mesh give the same bounds, numpy's."""
    import cgraytracing_amd as cg
    tris = _soup_of(n)
    sc = cg.Scene(_objs(tris), build=DEV)
    order = _order(sc)
    b0 = sc.mesh_bounds(MESH)
    assert len(b0["cover"]) == GROUPS[n]
    _same(b0, _numpy_bounds(tris, order, GROUPS[n]), "commit vs numpy")
    _contains(b0, tris, order)
    keep = _refit(sc, tris)
    _same(sc.mesh_bounds(MESH), b0, "identity refit vs commit")
    _rebuild(sc, tris)
    assert np.array_equal(_order(sc), order)
    _same(sc.mesh_bounds(MESH), b0, "identity rebuild vs commit")
    sc.close()
    del keep


@pytest.mark.parametrize("n", SIZES)
def test_moved_vertices_device_build(gpu_ready, n):
    """Checks 2, 3, 5: after a refit to moved vertices the bounds are numpy's over the OLD order's ranges, and the bounding sphere
    and bmax, which depend on no order, are the fresh commit's; after a rebuild everything is the fresh commit's."""
    import cgraytracing_amd as cg
    tris = _soup_of(n)
    moved = _deform(tris, 70 + n)
    fresh = cg.Scene(_objs(moved), build=DEV)
    want, fresh_order = fresh.mesh_bounds(MESH), _order(fresh)
    fresh.close()
    _same(want, _numpy_bounds(moved, fresh_order, GROUPS[n]), "fresh commit vs numpy")
    sc = cg.Scene(_objs(tris), build=DEV)
    order = _order(sc)
    keep = _refit(sc, moved)
    got = sc.mesh_bounds(MESH)
    _same(got, _numpy_bounds(moved, order, GROUPS[n]), "refit vs numpy")
    _same(dict(got, cover=want["cover"]), want, "refit vs fresh commit (bounding sphere, bmax)")
    _contains(got, moved, order)
    _rebuild(sc, moved)
    assert np.array_equal(_order(sc), fresh_order)
    got = sc.mesh_bounds(MESH)
    _same(got, want, "rebuild vs fresh commit")
    _contains(got, moved, fresh_order)
    sc.close()
    del keep


@pytest.mark.parametrize("n", SIZES)
def test_refitted_host_build(gpu_ready, n):
    """Checks 4, 5: a host-built mesh keeps the sphere count of its commit; a refit gives numpy's spheres over the ranges of its
    triangle order."""
    import cgraytracing_amd as cg
    tris = _soup_of(n)
    moved = _deform(tris, 70 + n)
    sc = cg.Scene(_objs(tris), build="host")
    G = len(sc.mesh_bounds(MESH)["cover"])
    assert 1 <= G <= 64
    order = sc.refit_plan(0)[3].copy()
    for pose in (tris, moved):
        keep = _refit(sc, pose)
        got = sc.mesh_bounds(MESH)
        _same(got, _numpy_bounds(pose, order, G), "host build, refit vs numpy")
        _contains(got, pose, order)
        del keep
    sc.close()


def test_refusals_and_sizing(gpu_ready):
    import ctypes as C
    import cgraytracing_amd as cg
    import scenes
    from cgraytracing_amd._capi import CgrtError
    tris = _soup_of(300)
    sc = cg.Scene([scenes.Sphere((5, -12, 30), 5, (1, 1, 1), 0.8, 0.0), scenes.TriangleMesh.from_triangles(tris, (1, 1, 1), 0.8, 0.5),
                   scenes.TriangleMesh.from_triangles(tris, (1, 1, 1))], build=DEV)
    for obj, word in ((0, "bounds: the object is a sphere"), (1, "bounds: the mesh is transparent"), (3, "bounds: no such object")):
        with pytest.raises(CgrtError) as e:
            sc.mesh_bounds(obj)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
    n = C.c_int32()
    room = np.zeros(16)
    assert sc._L.cgrt_scene_mesh_bounds_host(sc._h, 2, None, None, None, None, 0, C.byref(n)) == 0 and n.value == 4
    assert sc._L.cgrt_scene_mesh_bounds_host(sc._h, 2, None, None, None, room.ctypes.data, 3, C.byref(n)) == -1
    assert (room == 0).all()
    sc.close()
