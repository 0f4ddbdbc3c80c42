"""CPU: the occlusion-query entry points (cgrt_occlusion_rays, _host, _variant) are exported and bound, cgrt_occlusion has
the header's layout, and every argument error is returned before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import scenes

NAMES = ("cgrt_occlusion_rays", "cgrt_occlusion_rays_host", "cgrt_occlusion_rays_variant")
INVALID, LIMIT = -1, -5


def test_symbols_exported_and_bound():
    from cgraytracing_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), "libcgrt.so does not export %s" % name
        assert name in _capi.SIGNATURES, name
    assert C.sizeof(_capi.Occlusion) == 16
    assert _capi.RAYS_SKIP_TRANSPARENT == 8


def _args(n, occluded=True, tmax=False):
    from cgraytracing_amd import _capi
    m = max(1, min(n, 4))
    keep = [np.zeros((m, 3)), np.tile([0.0, 0.0, 1.0], (m, 1)), np.ones(m), np.zeros(m, np.uint8)]
    r = _capi.Rays(n, keep[0].ctypes.data, keep[1].ctypes.data, None, 0, 1, 1, 0)
    o = _capi.Occlusion(keep[2].ctypes.data if tmax else None, keep[3].ctypes.data if occluded else None)
    return r, o, keep


@pytest.mark.parametrize("entry", ["device", "host"])
def test_argument_errors_without_a_device(entry):
    """Null scene, uncommitted scene, null occluded, n < 0 and n > 2^36 are refused by both forms before anything is launched
    or allocated; n == 0 is valid and does nothing."""
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()

    def call(h, r, o):
        if entry == "device":
            return L.cgrt_occlusion_rays(h, C.byref(r) if r is not None else None, C.byref(o) if o is not None else None, None, None)
        return L.cgrt_occlusion_rays_host(h, C.byref(r) if r is not None else None, C.byref(o) if o is not None else None, None)

    s = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        r, o, keep = _args(4)
        assert call(None, r, o) == INVALID and b"null" in L.cgrt_last_error()
        assert call(s._h, None, o) == INVALID
        assert call(s._h, r, None) == INVALID
        assert call(s._h, r, o) == INVALID and b"not committed" in L.cgrt_last_error()
        r, o, keep = _args(4, occluded=False)
        assert call(s._h, r, o) == INVALID and b"occluded" in L.cgrt_last_error()
        r, o, keep = _args(-1)
        assert call(s._h, r, o) == INVALID and b"negative" in L.cgrt_last_error()
        r, o, keep = _args((1 << 36) + 1)
        assert call(s._h, r, o) == LIMIT and b"2^36" in L.cgrt_last_error()
        r, o, keep = _args(0)
        assert call(s._h, r, o) == _capi.CGRT_OK
        assert keep[3][0] == 0
        # the variant's name needs a committed scene too
        buf = C.create_string_buffer(160)
        assert L.cgrt_occlusion_rays_variant(s._h, C.byref(r), buf, len(buf)) == INVALID
        assert L.cgrt_occlusion_rays_variant(None, C.byref(r), buf, len(buf)) == INVALID
    finally:
        s.close()


def test_python_forms_refuse_an_uncommitted_scene():
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    s = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        with pytest.raises(_capi.CgrtError) as e:
            s.occluded_host(np.zeros((3, 3)), np.tile([0.0, 0.0, 1.0], (3, 1)), tmax=np.ones(3))
        assert e.value.code == INVALID
        with pytest.raises(ValueError):
            s.occluded_host(np.zeros((3, 3)), np.tile([0.0, 0.0, 1.0], (3, 1)), tmax=np.ones(2))
        none = s.occluded_host(np.zeros((0, 3)), np.zeros((0, 3)))
        assert none["occluded"].shape == (0,) and none["nrays"] == 0
    finally:
        s.close()
