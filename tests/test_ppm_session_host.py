"""CPU: the resumable photon-mapping ABI (cgrt_ppm_session_*) refuses bad arguments before it touches a device, its info
struct has the header's layout, and an uncommitted scene cannot start a session."""
import ctypes as C

import pytest

import scenes


def test_session_info_layout():
    from cgraytracing_amd import _capi
    # int64, 4 x uint64, int64, 5 doubles (include/cgrt.h cgrt_ppm_session_info)
    assert C.sizeof(_capi.PpmSessionInfo) == 88
    assert [f for f, _ in _capi.PpmSessionInfo._fields_] == [
        "photons_done", "hp_count", "n_events", "n_pairs", "n_batch_halvings", "device_bytes", "ms_eye", "ms_table",
        "ms_photons", "ms_last_add", "ms_last_image"]
    assert _capi.PPM_SESSION_NO_LOOKAHEAD == 1


def test_null_and_out_of_range_arguments_are_invalid():
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()
    info = _capi.PpmSessionInfo()
    cnt = C.c_uint64(0)
    assert L.cgrt_ppm_session_add_photons(None, 1) == -1
    assert L.cgrt_ppm_session_add_photons(None, -1) == -1
    assert L.cgrt_ppm_session_image(None, None, None) == -1
    assert L.cgrt_ppm_session_image_device(None, None, None, None) == -1
    assert L.cgrt_ppm_session_hitpoints(None, None, 0, C.byref(cnt)) == -1
    assert L.cgrt_ppm_session_get_info(None, C.byref(info)) == -1
    L.cgrt_ppm_session_destroy(None)  # ignored
    h = C.c_void_p()
    assert L.cgrt_ppm_session_create(None, None, None, None, 0, C.byref(h)) == -1 and not h.value
    s = cg.Scene(scenes.scene_c1(), commit=False)
    cc, g = s._structs(None, 16, 16, 16, 1, 5, 1, 0, None, 0, None, 0)
    ph = _capi.Photons((C.c_double * 3)(0, 19.999, 20), 2.0, 700.0, 0.7, 0, 1000001, 0, 777, 0.0, 0)
    assert L.cgrt_ppm_session_create(s._h, C.byref(cc), C.byref(g), C.byref(ph), 0, None) == -1  # no out pointer
    assert L.cgrt_ppm_session_create(s._h, C.byref(cc), C.byref(g), None, 0, C.byref(h)) == -1
    assert L.cgrt_ppm_session_create(s._h, C.byref(cc), C.byref(g), C.byref(ph), 0, C.byref(h)) == -1
    assert b"not committed" in L.cgrt_last_error() and not h.value
    assert L.cgrt_ppm_session_create(s._h, C.byref(cc), C.byref(g), C.byref(ph), 4, C.byref(h)) == -1  # unknown flag
    s.close()


def test_uncommitted_scene_session_raises():
    import cgraytracing_amd as cg
    from cgraytracing_amd._capi import CgrtError
    s = cg.Scene(scenes.scene_c2(), commit=False)
    with pytest.raises(CgrtError) as e:
        s.ppm_session(48, 36, nphotons=1000)
    assert e.value.code == -1
    for kw in (dict(nphotons=-1), dict(hashsize=0), dict(batch=-1), dict(pair_cap=-5), dict(initial_radius=-1.0)):
        with pytest.raises(CgrtError) as e:
            s.ppm_session(48, 36, **kw)
        assert e.value.code == -1, kw
    s.close()
