"""CPU: the host side of cgrt_scene_rebuild_mesh and cgrt_scene_mesh_cost (include/cgrt.h, "rebuild") -- the symbols and their
binding, and the refusals that come before any device call.  No device is touched: every scene here is uncommitted."""
import ctypes as C

import numpy as np
import pytest

import scenes

SYMBOLS = ("cgrt_scene_rebuild_mesh", "cgrt_scene_rebuild_mesh_host", "cgrt_scene_rebuild_info", "cgrt_scene_mesh_cost",
           "cgrt_scene_mesh_cost_host")


def _soup(rng, n, spread=6.0, size=1.5):
    c = rng.uniform(-spread, spread, (n, 1, 3)) + np.array([0.0, -8.0, 30.0])
    return (c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 9)


def _mesh(tris):
    return scenes.TriangleMesh.from_triangles(tris, (0.6, 0.7, 0.9), 0.0, 0.0)


def test_symbols_are_exported_and_bound():
    """The five functions and the two structs of the issue's seven names."""
    from cgraytracing_amd import _capi
    import cgraytracing_amd as cg
    L = _capi.lib()
    assert L.cgrt_version() == 112
    raw = C.CDLL(_capi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name) and name in _capi.SIGNATURES, name
    assert C.sizeof(_capi.RebuildInfo) == 48  # int64, 6 x int32, double, int64
    assert C.sizeof(_capi.TreeCost) == 24
    assert C.sizeof(_capi.RefitInfo) == 40
    for name in ("rebuild_mesh", "rebuild_mesh_host", "rebuild_info", "mesh_cost"):
        assert callable(getattr(cg.Scene, name))


def test_argument_errors_come_before_any_device_call():
    """A null scene and an uncommitted one are refused by every entry with CGRT_ERR_INVALID and a message that says which;
    this machine has no device to touch."""
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()
    t = np.zeros((5, 9))
    cost = _capi.TreeCost()
    room = np.zeros(3)
    entries = (lambda h: L.cgrt_scene_rebuild_mesh(h, 0, t.ctypes.data, 5, None),
               lambda h: L.cgrt_scene_rebuild_mesh_host(h, 0, t.ctypes.data, 5),
               lambda h: L.cgrt_scene_mesh_cost(h, 0, room.ctypes.data, None),
               lambda h: L.cgrt_scene_mesh_cost_host(h, 0, C.byref(cost)))
    for call in entries:
        assert call(None) == -1 and b"null scene" in L.cgrt_last_error()
    assert L.cgrt_scene_rebuild_info(None, 0, C.byref(_capi.RebuildInfo())) == -1 and b"null" in L.cgrt_last_error()
    sc = cg.Scene([_mesh(_soup(np.random.default_rng(0), 5))], commit=False, build="device")
    for call in entries:
        assert call(sc._h) == -1 and b"not committed" in L.cgrt_last_error()
    for call in (lambda: sc.rebuild_mesh_host(0, t), lambda: sc.mesh_cost(0)):
        with pytest.raises(_capi.CgrtError) as e:
            call()
        assert e.value.code == -1 and "not committed" in str(e.value)
    with pytest.raises(ValueError):
        sc.rebuild_mesh_host(0, np.zeros((5, 8)))
    inf = sc.rebuild_info(0)
    assert inf["rebuilds"] == 0 and inf["scratch_bytes"] == 0 and inf["levels"] == 0 and inf["readbacks"] == 0
    assert L.cgrt_scene_rebuild_info(sc._h, 1, C.byref(_capi.RebuildInfo())) == -1
    assert sc.refit_info(0)["geometry_gen"] == 0
    sc.close()
