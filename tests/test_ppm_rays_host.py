"""CPU: photon mapping of caller-supplied rays (cgrt_ppm_session_create_rays, cgrt_trace_rays_hitpoints) refuses bad arguments
before it touches a device, cgrt_ray_pixels has the header's layout in Python and in C99, and an uncommitted scene cannot
start a ray session."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ray_pixels_layout():
    from cgraytracing_amd import _capi
    # 4 x int32, one pointer (include/cgrt.h cgrt_ray_pixels)
    assert C.sizeof(_capi.RayPixels) == 24
    assert [f for f, _ in _capi.RayPixels._fields_] == ["width", "rows", "spp", "pad_", "pixel"]
    assert _capi.RayPixels.pixel.offset == 16
    assert _capi.RAYS_HITPOINTS == 4
    for name in ("cgrt_ppm_session_create_rays", "cgrt_trace_rays_hitpoints"):
        assert name in _capi.SIGNATURES and getattr(_capi.lib(), name) is not None
    assert _capi.lib().cgrt_version() == 112


def test_ray_pixels_layout_in_c99(tmp_path):
    """The same sizeof / offsetof as compile-time asserts of a strict C99 translation unit, linked against libcgrt.so."""
    from cgraytracing_amd import _capi
    src = os.path.join(ROOT, "tests", "native", "abi_ray_pixels_c99.c")
    obj = str(tmp_path / "abi_ray_pixels.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", obj])
    so = str(tmp_path / "libabi_ray_pixels.so")
    subprocess.check_call(["gcc", "-shared", "-o", so, obj, "-L", os.path.dirname(_capi.LIB_PATH), "-lcgrt",
                           "-Wl,-rpath," + os.path.dirname(_capi.LIB_PATH)])
    assert C.CDLL(so).cgrt_abi_ray_pixels_smoke() == 0


def test_null_and_out_of_range_arguments_are_invalid():
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()
    org = np.zeros((4, 3), np.float64)
    dirs = np.tile([0.0, 0.0, 1.0], (4, 1))
    s = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        def rays(n=4, o=org.ctypes.data, d=dirs.ctypes.data, depth=5):
            return _capi.Rays(n, o, d, None, 0, 12345, depth, 0)

        def photons(**kw):
            f = dict(nphotons=0, hashsize=1000001, batch=0, initial_radius=0.0, pair_cap=0)
            f.update(kw)
            return _capi.Photons((C.c_double * 3)(0, 19.999, 20), 2.0, 700.0, 0.7, f["nphotons"], f["hashsize"], f["batch"], 777,
                                 f["initial_radius"], f["pair_cap"])

        def create(scene=s._h, r=rays(), px=_capi.RayPixels(2, 2, 1, 0, None), ph=photons(), flags=0, out=True):
            h = C.c_void_p()
            rc = L.cgrt_ppm_session_create_rays(scene, C.byref(r) if r is not None else None, C.byref(px) if px is not None else None,
                                                C.byref(ph) if ph is not None else None, flags, C.byref(h) if out else None)
            assert not h.value
            return rc, L.cgrt_last_error().decode()

        cases = [("no out pointer", dict(out=False), "null"), ("null scene", dict(scene=None), "null"),
                 ("null rays", dict(r=None), "null"), ("null pixels", dict(px=None), "null"), ("null photons", dict(ph=None), "null"),
                 ("n < 0", dict(r=rays(n=-1)), "negative"), ("null org3", dict(r=rays(o=None)), "org3"),
                 ("null dir3", dict(r=rays(d=None)), "dir3"), ("max_depth 0", dict(r=rays(depth=0)), "max_depth"),
                 ("max_depth 6", dict(r=rays(depth=6)), "max_depth"),
                 ("width 0", dict(px=_capi.RayPixels(0, 2, 1, 0, None)), "width"), ("rows -1", dict(px=_capi.RayPixels(2, -1, 1, 0, None)), "rows"),
                 ("spp 0", dict(px=_capi.RayPixels(2, 2, 0, 0, None)), "spp"), ("hashsize 0", dict(ph=photons(hashsize=0)), "photon"),
                 ("nphotons < 0", dict(ph=photons(nphotons=-1)), "photon"), ("unknown flag", dict(flags=4), "flags"),
                 ("uncommitted scene", {}, "not committed")]
        for what, kw, word in cases:
            rc, msg = create(**kw)
            assert rc == -1, what  # CGRT_ERR_INVALID
            assert word in msg, (what, msg)
        cnt = C.c_uint64(7)
        rec = np.zeros((64, 10), np.float64)

        def capture(scene=s._h, r=rays(), hp=rec.ctypes.data, cap=64, count=True):
            rc = L.cgrt_trace_rays_hitpoints(scene, C.byref(r) if r is not None else None, hp, cap, C.byref(cnt) if count else None)
            return rc, L.cgrt_last_error().decode()

        for what, kw, word in [("null scene", dict(scene=None), "null"), ("null rays", dict(r=None), "null"),
                               ("n < 0", dict(r=rays(n=-1)), "negative"), ("null org3", dict(r=rays(o=None)), "org3"),
                               ("max_depth 0", dict(r=rays(depth=0)), "max_depth"), ("max_depth 6", dict(r=rays(depth=6)), "max_depth"),
                               ("uncommitted scene", {}, "not committed")]:
            rc, msg = capture(**kw)
            assert rc == -1, what
            assert word in msg, (what, msg)
        # the capture's kernel name is refused the same way
        buf = C.create_string_buffer(160)
        r = _capi.Rays(1, None, None, None, 0, 0, 5, _capi.RAYS_HITPOINTS)
        assert L.cgrt_trace_rays_variant(s._h, C.byref(r), None, buf, len(buf)) == -1 and b"not committed" in L.cgrt_last_error()
        r = _capi.Rays(1, None, None, None, 0, 0, 5, 0)
        assert L.cgrt_trace_rays_variant(s._h, C.byref(r), None, buf, len(buf)) == -1  # without the flag `out` is needed
    finally:
        s.close()


def test_uncommitted_scene_ray_session_raises():
    import cgraytracing_amd as cg
    from cgraytracing_amd._capi import CgrtError
    s = cg.Scene(scenes.scene_c2(), commit=False)
    try:
        with pytest.raises(CgrtError) as e:
            s.ppm_session_rays(None, None, width=48, rows=36, nphotons=1000)
        assert e.value.code == -1 and "not committed" in str(e.value)
        with pytest.raises(CgrtError) as e:
            s.trace_rays_hitpoints(None, None)
        assert e.value.code == -1 and "not committed" in str(e.value)
    finally:
        s.close()
