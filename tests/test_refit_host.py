"""CPU: the host side of cgrt_scene_refit_mesh (include/cgrt.h, "refit") -- the symbols and their binding, the refusals that come
before any device call, and the refit plan (cgraytracing_amd/csrc/cgrt_refit_plan.h) of host-built hierarchies against
cgrt_scene_wide_dump / cgrt_scene_bvh_order.  No device is touched: every scene here is uncommitted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -2 ** 31


def _soup(rng, n, spread=6.0, size=1.5):
    c = rng.uniform(-spread, spread, (n, 1, 3)) + np.array([0.0, -8.0, 30.0])
    return (c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 9)


def _mesh(tris, transp=0.0):
    return scenes.TriangleMesh.from_triangles(tris, (0.6, 0.7, 0.9), 0.0, transp)


def test_symbols_are_exported_and_bound():
    from cgraytracing_amd import _capi
    import cgraytracing_amd as cg
    L = _capi.lib()
    assert L.cgrt_version() == 112
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ("cgrt_scene_refit_mesh", "cgrt_scene_refit_mesh_host", "cgrt_scene_refit_info", "cgrt_scene_refit_plan_host"):
        assert hasattr(raw, name) and name in _capi.SIGNATURES
    assert C.sizeof(_capi.RefitInfo) == 40  # int64, 3 x int32 (+ 4 bytes of padding), double, uint64
    for name in ("refit_mesh", "refit_mesh_host", "refit_info", "refit_plan"):
        assert callable(getattr(cg.Scene, name))


def test_argument_errors_come_before_any_device_call():
    """A null scene and an uncommitted one are refused by both entries with CGRT_ERR_INVALID and a message that says which;
    this machine has no device to touch."""
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()
    t = np.zeros((1, 9))
    for call in (lambda h: L.cgrt_scene_refit_mesh(h, 0, t.ctypes.data, 1, None), lambda h: L.cgrt_scene_refit_mesh_host(h, 0, t.ctypes.data, 1)):
        assert call(None) == -1 and b"null scene" in L.cgrt_last_error()
    sc = cg.Scene([_mesh(_soup(np.random.default_rng(0), 5))], commit=False)
    for call in (lambda: sc.refit_mesh_host(0, np.zeros((5, 9))), lambda: _capi.check(L.cgrt_scene_refit_mesh(sc._h, 0, t.ctypes.data, 5, None))):
        with pytest.raises(_capi.CgrtError) as e:
            call()
        assert e.value.code == -1 and "not committed" in str(e.value)
    with pytest.raises(ValueError):
        sc.refit_mesh_host(0, np.zeros((5, 8)))
    inf = sc.refit_info(0)
    assert inf["refits"] == 0 and inf["plan_built"] == 0 and inf["ntris"] == 5 and inf["nwide"] >= 1 and inf["geometry_gen"] == 0
    assert L.cgrt_scene_refit_info(sc._h, 1, C.byref(_capi.RefitInfo())) == -1
    assert L.cgrt_scene_refit_info(None, 0, C.byref(_capi.RefitInfo())) == -1
    assert L.cgrt_scene_refit_plan_host(None, 0, None, None, None, None, None, None) == -1
    assert L.cgrt_scene_refit_plan_host(sc._h, 1, None, None, None, None, None, None) == -1
    sc.close()


def _check_plan(sc, t, tris):
    box, ref, _ = sc.wide_dump(t)
    tri_level, order = sc.bvh_order(t)
    _, leaf_ids, _, tri9 = sc.tree_dump(t)
    parent, slot, arrivals, src = sc.refit_plan(t)
    n = len(tris)
    assert tri_level and len(ref) >= 1 and len(parent) == len(slot) == len(arrivals) == len(ref) and len(src) == n
    assert parent[0] == -1
    # every non-root node has exactly one parent, and the slot that names it
    referenced = np.zeros(len(ref), np.int32)
    inner = np.zeros(len(ref), np.int32)
    for i in range(len(ref)):
        for k in range(4):
            r = int(ref[i, k])
            if r < 0 and r != NONE:
                referenced[~r] += 1
                inner[i] += 1
    assert referenced[0] == 0 and (referenced[1:] == 1).all()
    for i in range(1, len(ref)):
        assert ref[parent[i], slot[i]] == ~i
    assert np.array_equal(arrivals, inner + 1)
    assert sorted(src.tolist()) == list(range(n))
    # the triangle at each position of the hierarchy's order is the one src names
    assert np.array_equal(leaf_ids[order], src)
    assert np.array_equal(tri9[src], np.asarray(tris, np.float64).reshape(-1, 9)[src])


PLAN_CASES = [("pyramid", lambda: scenes.pyramid_tris()), ("bunny", scenes.bunny_tris)] + \
             [("soup%d" % n, (lambda n=n: _soup(np.random.default_rng(40 + n), n))) for n in (1, 2, 4, 5, 17, 333)]


@pytest.mark.parametrize("name,mk", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_plan_of_host_built_scene_matches_wide_dump(name, mk):
    import cgraytracing_amd as cg
    tris = mk()
    sc = cg.Scene(scenes.planes() + [_mesh(tris)], commit=False, build="host")
    _check_plan(sc, 0, tris)
    sc.close()


def test_plan_of_a_tree_without_the_wide_form_is_empty():
    """A transparent mesh keeps the reference's leaves: no triangle-level hierarchy, no plan."""
    import cgraytracing_amd as cg
    sc = cg.Scene([_mesh(_soup(np.random.default_rng(3), 50), transp=0.5)], commit=False, build="host")
    parent, slot, arrivals, src = sc.refit_plan(0)
    assert len(parent) == len(slot) == len(arrivals) == len(src) == 0
    sc.close()


def test_plan_builder_under_sanitizers(tmp_path):
    """cgrt_refit_plan.h over cgrt_build.cpp's hierarchies (soups of 1 to 5000 triangles, two meshes in one scene) and its
    refusals of corrupted trees, as a stand-alone program under ASan + UBSan (tests/native/refit_plan.cpp)."""
    exe = str(tmp_path / "refit_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "refit_plan.cpp"),
                           os.path.join(csrc, "cgrt_build.cpp"), "-pthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
