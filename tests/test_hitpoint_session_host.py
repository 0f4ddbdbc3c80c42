"""CPU: photon mapping of caller-supplied Hitpoint records (cgrt_ppm_session_create_hitpoints) refuses bad arguments before it
touches a device, cgrt_hitpoints has the header's layout in Python and in C99, and an uncommitted scene cannot start a
hitpoint session."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, LIMIT = -1, -5


def test_hitpoints_layout():
    from cgraytracing_amd import _capi
    H = _capi.Hitpoints
    assert C.sizeof(H) == 72
    assert [f for f, _ in H._fields_] == ["n", "hp9", "ray", "path", "pixel", "width", "rows", "spp", "max_depth", "reserved"]
    assert [getattr(H, f).offset for f, _ in H._fields_] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56]
    assert C.sizeof(C.c_void_p) == 8 and H.reserved.size == 16
    assert "cgrt_ppm_session_create_hitpoints" in _capi.SIGNATURES
    assert getattr(_capi.lib(), "cgrt_ppm_session_create_hitpoints") is not None
    assert _capi.lib().cgrt_version() == 112


def test_hitpoints_layout_in_c99(tmp_path):
    """The same sizeof / offsetof as compile-time asserts of a strict C99 translation unit, linked against libcgrt.so."""
    from cgraytracing_amd import _capi
    src = os.path.join(ROOT, "tests", "native", "abi_hitpoints_c99.c")
    obj = str(tmp_path / "abi_hitpoints.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", obj])
    so = str(tmp_path / "libabi_hitpoints.so")
    subprocess.check_call(["gcc", "-shared", "-o", so, obj, "-L", os.path.dirname(_capi.LIB_PATH), "-lcgrt",
                           "-Wl,-rpath," + os.path.dirname(_capi.LIB_PATH)])
    assert C.CDLL(so).cgrt_abi_hitpoints_smoke() == 0


def test_every_refusal_comes_before_a_device_is_touched():
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()
    hp9 = np.zeros((4, 9), np.float64)  # a host array: nothing may read it
    s = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        def records(n=4, hp=hp9.ctypes.data, width=2, rows=2, spp=1, depth=5):
            return _capi.Hitpoints(n, hp, None, None, None, width, rows, spp, depth)

        def photons(**kw):
            f = dict(nphotons=0, hashsize=1000001, batch=0, initial_radius=0.0, pair_cap=0)
            f.update(kw)
            return _capi.Photons((C.c_double * 3)(0, 19.999, 20), 2.0, 700.0, 0.7, f["nphotons"], f["hashsize"], f["batch"], 777,
                                 f["initial_radius"], f["pair_cap"])

        def create(scene=s._h, hps=records(), ph=photons(), flags=0, out=True):
            h = C.c_void_p(0xDEAD0)  # a failure leaves NULL behind
            rc = L.cgrt_ppm_session_create_hitpoints(scene, C.byref(hps) if hps is not None else None,
                                                     C.byref(ph) if ph is not None else None, flags, C.byref(h) if out else None)
            assert not out or h.value is None
            return rc, L.cgrt_last_error().decode()

        cases = [("no out pointer", dict(out=False), INVALID, "null"), ("null scene", dict(scene=None), INVALID, "null"),
                 ("null hitpoints", dict(hps=None), INVALID, "null"), ("null photons", dict(ph=None), INVALID, "null"),
                 ("n < 0", dict(hps=records(n=-1)), INVALID, "negative"), ("n > 0, null hp9", dict(hps=records(hp=None)), INVALID, "hp9"),
                 ("width 0", dict(hps=records(width=0)), INVALID, "width"), ("rows -1", dict(hps=records(rows=-1)), INVALID, "rows"),
                 ("spp 0", dict(hps=records(spp=0)), INVALID, "spp"), ("max_depth 0", dict(hps=records(depth=0)), INVALID, "max_depth"),
                 ("max_depth 6", dict(hps=records(depth=6)), INVALID, "max_depth"),
                 ("unknown flag", dict(flags=4), INVALID, "flags"), ("hashsize 0", dict(ph=photons(hashsize=0)), INVALID, "photon"),
                 ("nphotons < 0", dict(ph=photons(nphotons=-1)), INVALID, "photon"),
                 ("pair_cap < 0", dict(ph=photons(pair_cap=-1)), INVALID, "photon"),
                 ("npix = 2^31", dict(hps=records(width=65536, rows=32768)), LIMIT, "texels"),
                 ("n = 2^31", dict(hps=records(n=1 << 31)), LIMIT, "records"),
                 ("uncommitted scene", {}, INVALID, "not committed"),
                 ("uncommitted scene, n = 0", dict(hps=records(n=0, hp=None)), INVALID, "not committed"),
                 ("largest valid sizes, uncommitted", dict(hps=records(n=(1 << 31) - 1, width=65536, rows=32767)), INVALID, "not committed")]
        for what, kw, code, word in cases:
            rc, msg = create(**kw)
            assert rc == code, (what, rc, msg)
            assert word in msg, (what, msg)
    finally:
        s.close()


def test_uncommitted_scene_hitpoint_session_raises():
    import cgraytracing_amd as cg
    from cgraytracing_amd._capi import CgrtError
    s = cg.Scene(scenes.scene_c2(), commit=False)
    try:
        with pytest.raises(CgrtError) as e:
            s.ppm_session_hitpoints(None, width=48, rows=36, nphotons=1000)
        assert e.value.code == INVALID and "not committed" in str(e.value)
    finally:
        s.close()
