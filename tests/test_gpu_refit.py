"""GPU: cgrt_scene_refit_mesh (include/cgrt.h, "refit"; cgraytracing_amd/csrc/cgrt_refit.hpp) -- new vertices for a committed
opaque mesh, by kernels -- against a scene FRESHLY COMMITTED with the same vertices in the same build mode, and against the CPU
oracle.

Parity class (the header's): every ray with a unique nearest hit gets the fresh scene's hit bit for bit, because boxes are
supersets and the triangle test is the same code (test_gpu_devbuild.py::test_device_mesh_fuzz asserts the same of the two
builds).  Random soups have no exact ties, so their frames are asserted array_equal; the dragon and the bunny share edges and
are held to test_gpu_devbuild._compare's bars: L-inf < 1e-4 on all pixels, at most max(4, npx/500) pixels not bit-equal, hit and
ray counts equal."""
import os
import subprocess

import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, SEED = 96, 80, 2, 99
MESH = 5  # the mesh's position in planes() + [mesh]
SIZES = [1, 2, 4, 5, 17, 333, 2000]
BUILDS = ["host", "device"]
NONE = -2 ** 31
PAD = 1.001e-4  # kBoxPad


def _soup(rng, n, spread=6.0, size=1.5):
    c = rng.uniform(-spread, spread, (n, 1, 3)) + np.array([0.0, -8.0, 30.0])
    return (c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 9)


def _soup_of(n):
    return _soup(np.random.default_rng(7000 + n), n)


def _objs(tris, refl=0.0, transp=0.0):
    return scenes.planes() + [scenes.TriangleMesh.from_triangles(tris, (0.6, 0.7, 0.9), refl, transp)]


def _deform(tris, seed, jitter=0.05, centre=(0.0, -8.0, 30.0)):
    """A rotation about the vertical axis through `centre`, a non-uniform scale and a jitter per vertex."""
    rng = np.random.default_rng(seed)
    p = np.asarray(tris, np.float64).reshape(-1, 3) - np.asarray(centre)
    a = 0.6
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    p = (p @ rot.T) * np.array([1.2, 0.7, 0.9]) + rng.uniform(-jitter, jitter, p.shape)
    return np.ascontiguousarray((p + np.asarray(centre)).reshape(-1, 9))


def _deform_shared(tris, centre):
    """The same for a mesh with shared vertices: the displacement is a function of the vertex, so shared edges stay shared
    (and rays through them still tie)."""
    p = np.asarray(tris, np.float64).reshape(-1, 3) - np.asarray(centre)
    a = 0.5
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    p = (p @ rot.T) * np.array([1.1, 0.8, 0.95])
    p = p + 0.05 * np.sin(3.0 * p[:, [1, 2, 0]])
    return np.ascontiguousarray((p + np.asarray(centre)).reshape(-1, 9))


def _refit(sc, tris, obj=MESH):
    """Through the tensor path; returns the tensor, which the caller keeps until the next synchronising call."""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(tris, np.float64).reshape(-1, 9), device="cuda:0")
    sc.refit_mesh(obj, t)
    return t


def _frame(sc, cam=None, w=W, h=H, spp=SPP):
    return sc.trace_grid_host(w, h, spp, cam or scenes.cam_dof(), 5, SEED)


def _fresh(objs, build, cam=None, w=W, h=H, spp=SPP):
    import cgraytracing_amd as cg
    sc = cg.Scene(objs, build=build)
    out = _frame(sc, cam, w, h, spp)
    sc.close()
    return out


def _assert_same(got, want):
    assert got["nrays"] == want["nrays"] and got["nhp"] == want["nhp"]
    assert np.array_equal(got["nhit"], want["nhit"])
    assert np.array_equal(got["rgb"], want["rgb"])


def _assert_oracle(got, want, spp=SPP):
    assert got["nrays"] == want["nrays"], "ray count vs oracle"
    assert np.array_equal(got["nhit"], want["nhit"])
    e = np.abs(got["rgb"].astype(np.float64) - to_acc32(want["acc_sum"], spp).astype(np.float64)).max()
    print("vs oracle: Linf=%.3e" % e)
    assert e < 1e-4


def _check_structure(sc, t, tris):
    """After a refit: every leaf's box contains its triangles grown by kBoxPad (and is tight), every inner slot's box is the
    union of its node's boxes, every triangle lies in one leaf."""
    box, ref, need = sc.wide_dump(t)
    _, _, _, src = sc.refit_plan(t)
    P = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    covered = np.zeros(len(P), np.int32)
    for i in range(len(ref)):
        for k in range(4):
            r = int(ref[i, k])
            if r == NONE:
                continue
            if r >= 0:
                first, cnt = r >> 4, r & 15
                ids = src[first:first + cnt]
                covered[ids] += 1
                lo, hi = P[ids].min((0, 1)), P[ids].max((0, 1))
                b = box[i, k].astype(np.float64)
                assert (b[:3] <= lo - PAD).all() and (b[3:] >= hi + PAD).all()
                assert (b[:3] >= lo - 1.1e-4 - 1e-6 * np.abs(lo)).all() and (b[3:] <= hi + 1.1e-4 + 1e-6 * np.abs(hi)).all()
            else:
                c = ~r
                ck = [q for q in range(4) if ref[c, q] != NONE]
                assert (box[c, ck, :3].min(0) == box[i, k, :3]).all() and (box[c, ck, 3:].max(0) == box[i, k, 3:]).all()
    assert (covered == 1).all()


# ---------------------------------------------------------------- 1. identity
def _identity(build, tris, objs, w=W, h=H, spp=SPP):
    import cgraytracing_amd as cg
    sc = cg.Scene(objs, build=build)
    before = _frame(sc, None, w, h, spp)
    box0, ref0, need0 = sc.wide_dump(0)
    order0 = sc.bvh_order(0)[1].copy()
    keep = _refit(sc, tris, len(objs) - 1)
    after = _frame(sc, None, w, h, spp)
    box1, ref1, need1 = sc.wide_dump(0)
    assert box0.tobytes() == box1.tobytes() and ref0.tobytes() == ref1.tobytes() and need0 == need1
    assert np.array_equal(order0, sc.bvh_order(0)[1])
    _assert_same(after, before)
    inf = sc.refit_info(len(objs) - 1)
    assert inf["refits"] == 1 and inf["plan_built"] == 1 and inf["geometry_gen"] == 1 and inf["ntris"] == len(tris) and inf["nwide"] == len(ref0)
    # the reference's tree describes nothing any more: empty, as for a device-built tree
    nodes, leaf, bbox, _ = sc.tree_dump(0)
    assert len(nodes) == 0 and len(leaf) == 0 and len(bbox) == 0
    sc.close()
    del keep


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("build", BUILDS)
def test_identity_refit_changes_nothing(gpu_ready, build, n):
    tris = _soup_of(n)
    _identity(build, tris, _objs(tris, refl=0.8 if n % 2 else 0.0))


@pytest.mark.parametrize("build", BUILDS)
def test_identity_refit_dragon(gpu_ready, build):
    _identity(build, scenes.dragon_tris(), scenes.scene_dragon(), 128, 128, 1)


# ---------------------------------------------------------------- 2. deformation
_ORACLE = {}


def _oracle(orc, key, objs, cam, w=W, h=H, spp=SPP):
    """The oracle's frame of a pose, computed once and shared by the build modes."""
    if key not in _ORACLE:
        o = BackendScene(orc, objs)
        _ORACLE[key] = o.trace_grid(cam, w, h, spp, 5, seed=SEED)
        o.close()
    return _ORACLE[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("build", BUILDS)
def test_deformed_soup_equals_fresh_scene_and_oracle(gpu_ready, orc, build, n):
    import cgraytracing_amd as cg
    tris = _soup_of(n)
    moved = _deform(tris, 10 + n)
    refl = 0.8 if n % 2 else 0.0
    cam = scenes.cam_dof() if n % 3 else scenes.cam_pinhole()
    sc = cg.Scene(_objs(tris, refl), build=build)
    keep = _refit(sc, moved)
    got = _frame(sc, cam)
    _check_structure(sc, 0, moved)
    sc.close()
    del keep
    _assert_same(got, _fresh(_objs(moved, refl), build, cam))
    _assert_oracle(got, _oracle(orc, ("soup", n), _objs(moved, refl), cam))


# ---------------------------------------------------------------- 3. meshes with shared edges
def _compare_tolerant(name, got, fresh, want, spp):
    assert got["nrays"] == fresh["nrays"] and got["nhp"] == fresh["nhp"] and np.array_equal(got["nhit"], fresh["nhit"])
    diff = np.abs(got["rgb"].astype(np.float64) - fresh["rgb"].astype(np.float64))
    npx = diff.shape[0] * diff.shape[1]
    n_bits = int((got["rgb"] != fresh["rgb"]).any(axis=2).sum())
    print("%s: refitted vs fresh: Linf=%.3e, %d of %d pixels not bit-equal" % (name, diff.max(), n_bits, npx))
    assert diff.max() < 1e-4
    assert n_bits <= max(4, npx // 500)
    _assert_oracle(got, want, spp)


SHARED = [("dragon", scenes.dragon_tris, lambda t: scenes.planes() + [scenes.TriangleMesh.from_triangles(t, (0.25, 0.25, 0.5), 0.0, 0.0, 1)],
           (-5.0, -12.0, 30.0)),
          ("bunny", scenes.bunny_tris, lambda t: scenes.planes(scenes.chessboard_texture(False)) + [scenes.TriangleMesh.from_triangles(t, (1.0, 1.0, 1.0))],
           (0.0, -10.0, 35.0))]


@pytest.mark.parametrize("name,mk,scene,centre", SHARED, ids=[c[0] for c in SHARED])
@pytest.mark.parametrize("build", BUILDS)
def test_deformed_dragon_and_bunny(gpu_ready, orc, build, name, mk, scene, centre):
    import cgraytracing_amd as cg
    tris = mk()
    moved = _deform_shared(tris, centre)
    cam, w, h, spp = scenes.cam_dof(), 128, 128, 1
    sc = cg.Scene(scene(tris), build=build)
    keep = _refit(sc, moved)
    got = _frame(sc, cam, w, h, spp)
    sc.close()
    del keep
    _compare_tolerant("%s/%s" % (name, build), got, _fresh(scene(moved), build, cam, w, h, spp),
                      _oracle(orc, (name,), scene(moved), cam, w, h, spp), spp)


# ---------------------------------------------------------------- 4. bounds follow the mesh
@pytest.mark.parametrize("build", BUILDS)
def test_bounding_and_cover_spheres_follow_the_mesh(gpu_ready, build):
    """From the left third of the frame to the right third, and shrunk: a stale bounding sphere would cut the mesh out, stale
    cover spheres would send its tiles to the light kernel."""
    import cgraytracing_amd as cg
    rng = np.random.default_rng(21)
    left = _soup(rng, 600, spread=3.0, size=1.0) + np.tile([-9.0, 0.0, 0.0], 3)
    p = left.reshape(-1, 3) - np.array([-9.0, -8.0, 30.0])
    right = np.ascontiguousarray((p * 0.5 + np.array([9.0, -6.0, 28.0])).reshape(-1, 9))
    sc = cg.Scene(_objs(left), build=build)
    before = _frame(sc)
    keep = _refit(sc, right)
    got = _frame(sc)
    sc.close()
    del keep
    want = _fresh(_objs(right), build)
    _assert_same(got, want)
    assert not np.array_equal(before["rgb"], got["rgb"])


@pytest.mark.parametrize("build", BUILDS)
def test_error_bound_follows_a_mesh_moved_far_out(gpu_ready, build):
    """Coordinates about 50 times larger (TreeRec::bmax, the fp32 box test's error term, must follow): equal to the fresh scene.
    No claim that a stale bound always shows."""
    import cgraytracing_amd as cg
    near = _soup(np.random.default_rng(22), 400)
    far = np.ascontiguousarray(near * 50.0)
    objs = lambda t: [scenes.Plane((0.0, -1000.0, 0.0), (0, 1, 0), (0.3, 0.3, 0.3)), scenes.TriangleMesh.from_triangles(t, (0.6, 0.7, 0.9))]
    sc = cg.Scene(objs(near), build=build)
    keep = _refit(sc, far, 1)
    got = _frame(sc, scenes.cam_pinhole())
    sc.close()
    del keep
    _assert_same(got, _fresh(objs(far), build, scenes.cam_pinhole()))
    assert got["nhp"] > 0


# ---------------------------------------------------------------- 5. two refits back to back
@pytest.mark.parametrize("build", BUILDS)
def test_two_refits_enqueued_back_to_back(gpu_ready, build):
    """No synchronisation between them (the plan exists from a first refit): the arrival counters are cleared on the stream."""
    import cgraytracing_amd as cg
    tris = _soup_of(2000)
    one, two = _deform(tris, 31), _deform(_deform(tris, 32), 33)
    sc = cg.Scene(_objs(tris), build=build)
    k0 = _refit(sc, tris)
    k1 = _refit(sc, one)
    k2 = _refit(sc, two)
    got = _frame(sc)
    assert sc.refit_info(MESH)["refits"] == 3
    _check_structure(sc, 0, two)
    sc.close()
    del k0, k1, k2
    _assert_same(got, _fresh(_objs(two), build))


# ---------------------------------------------------------------- 6. other readers
@pytest.mark.parametrize("build", BUILDS)
def test_ray_queries_and_photon_pass_see_the_moved_mesh(gpu_ready, build):
    import cgraytracing_amd as cg
    import torch
    tris = _soup_of(333)
    moved = _deform(tris, 41)
    sc = cg.Scene(_objs(tris, 0.8), build=build)
    # (the hit-attribute table is built BEFORE the refit here, and after the commit in the fresh scene: construction indices)
    org, dirs, keys = sc.camera_rays(64, 48, 1, scenes.cam_pinhole(), SEED)
    h0 = sc.trace_rays(org, dirs, keys, want=("hit",))
    sc.hit_attributes(org, dirs, h0["hit_obj"], h0["hit_t"], want=("prim",))
    keep = _refit(sc, moved)
    fresh = cg.Scene(_objs(moved, 0.8), build=build)
    res = []
    for s in (sc, fresh):
        hit = s.trace_rays(org, dirs, keys, want=("hit",))
        att = s.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=("prim", "uv"))
        tmax = torch.full((org.shape[0],), 35.0, dtype=torch.float64, device=org.device)
        occ = s.occluded(org, dirs, tmax)
        torch.cuda.synchronize()
        ppm = s.ppm_render(64, 48, 1, scenes.cam_pinhole(), 5, SEED, nphotons=20000)
        res.append(dict(hit_obj=hit["hit_obj"].cpu().numpy(), hit_t=hit["hit_t"].cpu().numpy(), prim=att["prim"].cpu().numpy(),
                        uv=att["uv"].cpu().numpy(), occ=occ["occluded"].cpu().numpy(), ppm=ppm))
    sc.close()
    fresh.close()
    del keep
    a, b = res
    assert (a["hit_obj"] == MESH).sum() > 50
    for k in ("hit_obj", "hit_t", "prim", "uv", "occ"):
        assert np.array_equal(a[k], b[k]), k
    assert a["ppm"]["count"] == b["ppm"]["count"] and a["ppm"]["n_events"] == b["ppm"]["n_events"]
    assert np.array_equal(a["ppm"]["image"], b["ppm"]["image"])


# ---------------------------------------------------------------- 7. refusals
def _refused(sc, obj, tris, word):
    from cgraytracing_amd._capi import CgrtError
    with pytest.raises(CgrtError) as e:
        sc.refit_mesh_host(obj, tris)
    assert e.value.code == -1 and word in str(e.value), str(e.value)
    with pytest.raises(CgrtError) as e:
        _refit(sc, tris, obj)
    assert e.value.code == -1 and word in str(e.value), str(e.value)


def test_refusals(gpu_ready, monkeypatch):
    import cgraytracing_amd as cg
    tris = _soup_of(17)
    objs = [scenes.Sphere((5, -12, 30), 5, (1, 1, 1), 0.8, 0.0), scenes.Plane((0.0, -20, 0), (0, 1, 0), (0.15, 0.15, 0.15)),
            scenes.vase_bezier(), scenes.TriangleMesh.from_triangles(tris, (1, 1, 1), 0.8, 0.5), scenes.TriangleMesh.from_triangles(tris, (1, 1, 1))]
    sc = cg.Scene(objs)
    _refused(sc, 0, tris, "sphere")
    _refused(sc, 1, tris, "plane")
    _refused(sc, 2, tris, "Bezier")
    _refused(sc, 3, tris, "transparent")
    _refused(sc, 4, tris[:16], "ntri")
    _refused(sc, 5, tris, "no such object")
    _refused(sc, -1, tris, "no such object")
    assert sc.refit_info(4)["refits"] == 0 and sc.refit_info(4)["geometry_gen"] == 0
    sc.refit_mesh_host(4, tris)  # (and the one that is allowed)
    assert sc.refit_info(4)["refits"] == 1
    sc.close()
    floor = cg.Scene(scenes.planes(scenes.stone_small_texture(True)))
    _refused(floor, 0, tris, "bump floor")
    floor.close()
    empty = cg.Scene([scenes.TriangleMesh.from_triangles(np.zeros((0, 9)), (1, 1, 1))])
    empty.refit_mesh_host(0, np.zeros((0, 9)))  # accepted, nothing done
    assert empty.refit_info(0)["geometry_gen"] == 0
    empty.close()
    monkeypatch.setenv("CGRT_TREE", "ref")
    ref = cg.Scene(_objs(tris))
    _refused(ref, MESH, tris, "4-wide")
    ref.close()


# ---------------------------------------------------------------- 8. sessions
def test_sessions_created_before_a_refit_refuse_to_trace(gpu_ready):
    import cgraytracing_amd as cg
    from cgraytracing_amd._capi import CgrtError
    tris = _soup_of(333)
    moved = _deform(tris, 51)
    cam = scenes.cam_pinhole()
    sc = cg.Scene(_objs(tris))
    ppm = sc.ppm_session(64, 48, 1, cam, 5, SEED, nphotons=5000, lookahead=False)
    sppm = sc.sppm_session(64, 48, 1, cam)
    sppm.add_passes(1, 5000)
    img0, simg0 = ppm.image(), sppm.image()
    sc.refit_mesh_host(MESH, moved)
    with pytest.raises(CgrtError) as e:
        ppm.add_photons(1000)
    assert e.value.code == -1 and "refitted after this session" in str(e.value)
    with pytest.raises(CgrtError) as e:
        sppm.add_passes(1, 1000)
    assert e.value.code == -1 and "refitted after this session" in str(e.value)
    assert np.array_equal(ppm.image(), img0) and np.array_equal(sppm.image(), simg0)
    assert ppm.info()["photons_done"] == 5000 and sppm.info()["passes"] == 1
    ppm.close()
    sppm.close()
    # sessions created after the refit work, and see the moved mesh
    after = sc.ppm_session(64, 48, 1, cam, 5, SEED, nphotons=5000, lookahead=False)
    after.add_photons(1000)
    s2 = sc.sppm_session(64, 48, 1, cam)
    s2.add_passes(1, 5000)
    got, sgot = after.image(), s2.image()
    after.close()
    s2.close()
    sc.close()
    fresh = cg.Scene(_objs(moved))
    want = fresh.ppm_render(64, 48, 1, cam, 5, SEED, nphotons=6000)
    fs = fresh.sppm_session(64, 48, 1, cam)
    fs.add_passes(1, 5000)
    swant = fs.image()
    fs.close()
    fresh.close()
    assert np.array_equal(got, want["image"]) and np.array_equal(sgot, swant)


# ---------------------------------------------------------------- 9. tensor path = host path
@pytest.mark.parametrize("build", BUILDS)
def test_tensor_path_and_host_path_give_the_same_frame(gpu_ready, build):
    import cgraytracing_amd as cg
    import torch
    tris = _soup_of(333)
    moved = _deform(tris, 61)
    a = cg.Scene(_objs(tris), build=build)
    t = torch.as_tensor(moved.reshape(-1, 3, 3), device="cuda:0")  # (the [n,3,3] form)
    a.refit_mesh(MESH, t)
    fa = _frame(a)
    with pytest.raises(ValueError):
        a.refit_mesh(MESH, t.to(torch.float32))
    with pytest.raises(ValueError):
        a.refit_mesh(MESH, t.cpu())
    a.close()
    b = cg.Scene(_objs(tris), build=build)
    b.refit_mesh_host(MESH, moved)
    fb = _frame(b)
    # the host entry refreshed the mirrors: the triangles tree_dump returns are the new ones
    assert np.array_equal(b.tree_dump(0)[3], moved)
    b.close()
    _assert_same(fa, fb)


# ---------------------------------------------------------------- 10. the C++ host layer
def test_cpp_host_wrapper_refits_between_frames(gpu_ready):
    """examples/refit_host.cpp over include/cgrt_host.hpp's DeformingScene: three poses of a soup, each refitted frame equal to
    the frame of a scene freshly committed on the same vertices (the program compares the floats itself)."""
    exe = os.path.join(ROOT, "cgraytracing_amd", "cgrt_refit_host")
    assert os.path.exists(exe), "build it with make -C cgraytracing_amd/csrc all"
    out = subprocess.run([exe, "--tris", "500", "--frames", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok: 3 frames equal (500 triangles" in out.stdout, out.stdout
