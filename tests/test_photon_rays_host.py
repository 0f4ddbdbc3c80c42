"""Caller-supplied photons, the part that needs no GPU: the ABI of cgrt_ppm_session_add_photon_rays / cgrt_photon_emit /
cgrt_photon_ray_events, and the host form of the built-in emitter (cgrt_photon_emit_host) against a numpy restatement of the
photon's keyed stream (cgrt_rng.hpp's header comment) and of main.cpp:240-246."""
import ctypes as C
import os
import subprocess

import numpy as np

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777
LIGHT, JITTER, POWER = (0.0, 19.999, 20.0), 2.0, 700.0
G = np.uint64(0x9E3779B97F4A7C15)
PHOT = np.uint64(0x70686F74)  # 'phot'


def _fin64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _photon_keys(seed, index):
    """stream_key(seed, index, 0, 'phot'): k_pix = fin(fin(seed+G) + index + G), k_smp = fin(k_pix + 0 + G), key = fin(k_smp + purpose + G)"""
    k_pix = _fin64(_fin64(np.uint64(seed) + G) + index.astype(np.uint64) + G)
    return _fin64(_fin64(k_pix + np.uint64(0) + G) + PHOT + G)


def _u01(keys, n):
    """draw n of the streams: z = fin(key + (n/2 + 1) G), the upper 31 bits for an even n, bits 2..32 for an odd one, / RAND_MAX"""
    z = _fin64(keys + np.uint64(n // 2 + 1) * G)
    r = (z >> np.uint64(2)) & np.uint64(0x7FFFFFFF) if n & 1 else z >> np.uint64(33)
    return r.astype(np.float64) / 2147483647.0


def restated_emitter(seed, first, count, light=LIGHT, jitter=JITTER, power=POWER, attempts=64):
    """main.cpp:240-246 on the photons' streams, in numpy: (org, dirs, flux, keys, draws)"""
    with np.errstate(over="ignore"):
        keys = _photon_keys(seed, first + np.arange(count))
        a = _u01(keys, 0) * (2 * jitter) - jitter
        b = _u01(keys, 1) * (2 * jitter) - jitter
        org = np.stack([light[0] + a, np.full(count, light[1] + 0.0), light[2] + b], axis=1)
        dirs = np.zeros((count, 3))
        draws = np.zeros(count, np.uint32)
        for j in range(attempts):  # sampling.h:11-20: reject outside the unit ball, then normalise (vec3.h:36-44)
            x, y, z = (_u01(keys, 2 + 3 * j + c) * 2.0 - 1 for c in range(3))
            s2 = x * x + y * y + z * z
            take = (draws == 0) & (s2 <= 1)
            r = 1 / np.sqrt(s2[take])
            dirs[take] = np.stack([x[take] * r, y[take] * r, z[take] * r], axis=1)
            draws[take] = 2 + 3 * (j + 1)
    assert (draws > 0).all()
    flux = np.full((count, 3), power * (3.14159265358979 * 4))
    return org, dirs, flux, keys, draws


def test_symbols_and_struct_layout():
    from cgraytracing_amd import _capi
    assert C.sizeof(_capi.PhotonRays) == 48
    assert [f for f, _ in _capi.PhotonRays._fields_] == ["n", "org3", "dir3", "flux3", "keys", "draws"]
    for name in ("cgrt_ppm_session_add_photon_rays", "cgrt_photon_emit", "cgrt_photon_emit_host", "cgrt_photon_ray_events"):
        assert name in _capi.SIGNATURES and getattr(_capi.lib(), name) is not None
    import cgraytracing_amd as cg
    assert callable(cg.emit_photons_host)
    for name in ("emit_photons", "photon_ray_events"):
        assert callable(getattr(cg.Scene, name))
    from cgraytracing_amd.engine import PpmSession
    assert callable(PpmSession.add_photon_rays)


def test_photon_rays_layout_in_c99(tmp_path):
    """sizeof / offsetof as compile-time asserts of a strict C99 translation unit, linked against libcgrt.so and run."""
    from cgraytracing_amd import _capi
    src = os.path.join(ROOT, "tests", "native", "abi_photon_rays_c99.c")
    obj = str(tmp_path / "abi_photon_rays.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", obj])
    so = str(tmp_path / "libabi_photon_rays.so")
    subprocess.check_call(["gcc", "-shared", "-o", so, obj, "-L", os.path.dirname(_capi.LIB_PATH), "-lcgrt",
                           "-Wl,-rpath," + os.path.dirname(_capi.LIB_PATH)])
    assert C.CDLL(so).cgrt_abi_photon_rays_smoke() == 0


def test_emit_host_properties():
    import cgraytracing_amd as cg
    n = 5000
    org, dirs, flux, keys, draws = cg.emit_photons_host(1234, n, SEED, LIGHT, JITTER, POWER)
    a, b = org[:, 0] - LIGHT[0], org[:, 2] - LIGHT[2]
    assert np.array_equal(org[:, 1], np.full(n, LIGHT[1]))
    assert (np.abs(a) <= JITTER).all() and (np.abs(b) <= JITTER).all() and a.std() > 0.5 and b.std() > 0.5
    x = dirs.astype(np.longdouble)
    assert float(np.abs(np.sqrt((x * x).sum(axis=1)) - 1).max()) <= 2 * 2.0 ** -52  # 2 ulp of 1
    assert np.array_equal(flux, np.full((n, 3), POWER * (3.14159265358979 * 4)))
    assert (draws >= 5).all() and ((draws.astype(np.int64) - 2) % 3 == 0).all()
    assert len(np.unique(draws)) > 1, "the stream position behind the rejection loop differs per photon"
    assert len(np.unique(keys)) == n
    # a range asked for whole or in two pieces
    p1, p2 = cg.emit_photons_host(1234, 1777, SEED), cg.emit_photons_host(1234 + 1777, n - 1777, SEED)
    for whole, x1, x2 in zip((org, dirs, flux, keys, draws), p1, p2):
        assert np.array_equal(whole, np.concatenate([x1, x2]))
    # other emitter fields move the photons as main.cpp:240-246 says
    o2, d2, f2, k2, n2 = cg.emit_photons_host(1234, n, SEED, light=(3.0, 10.0, 25.0), jitter=0.5, power=10.0)
    assert np.array_equal(d2, dirs) and np.array_equal(k2, keys) and np.array_equal(n2, draws)
    assert (np.abs(o2[:, 0] - 3.0) <= 0.5).all() and np.array_equal(f2, np.full((n, 3), 10.0 * (3.14159265358979 * 4)))
    # pointers may be NULL; nothing asked for is fine
    from cgraytracing_amd import _capi
    ph = _capi.Photons((C.c_double * 3)(*LIGHT), JITTER, POWER, 0.7, 0, 1000001, 0, SEED, 0.0, 0)
    assert _capi.lib().cgrt_photon_emit_host(C.byref(ph), 0, 10, None, None, None, None, None) == 0
    assert _capi.lib().cgrt_photon_emit_host(C.byref(ph), 0, 0, None, None, None, None, None) == 0


def test_emit_host_equals_numpy_restatement():
    import cgraytracing_amd as cg
    for first in (0, 123456789):
        got = cg.emit_photons_host(first, 1000, SEED)
        want = restated_emitter(SEED, first, 1000)
        for name, g, w in zip(("org", "dirs", "flux", "keys", "draws"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (first, name)


def test_argument_errors():
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()
    INVALID, LIMIT = -1, -5
    buf = np.zeros((4, 3))
    pr = lambda n: _capi.PhotonRays(n, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None)
    # the struct is looked at before the session (a session needs a GPU; these refusals do not)
    assert L.cgrt_ppm_session_add_photon_rays(None, None) == INVALID and L.cgrt_last_error()
    assert L.cgrt_ppm_session_add_photon_rays(None, C.byref(pr(-1))) == INVALID
    assert L.cgrt_ppm_session_add_photon_rays(None, C.byref(pr((1 << 36) + 1))) == LIMIT
    assert L.cgrt_ppm_session_add_photon_rays(None, C.byref(pr(4))) == INVALID  # no session
    assert L.cgrt_ppm_session_add_photon_rays(None, C.byref(_capi.PhotonRays(4, buf.ctypes.data, None, buf.ctypes.data, None, None))) == INVALID
    ev, va = np.zeros((32, 9)), np.zeros(32, np.uint8)
    sc = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        call = lambda p: L.cgrt_photon_ray_events(sc._h, p, SEED, 0, 5, ev.ctypes.data, va.ctypes.data)
        assert call(None) == INVALID
        assert call(C.byref(pr(-1))) == INVALID
        assert call(C.byref(pr((1 << 36) + 1))) == LIMIT
        assert call(C.byref(pr(4))) == INVALID  # the scene is not committed
    finally:
        sc.close()
    ph = _capi.Photons((C.c_double * 3)(*LIGHT), JITTER, POWER, 0.7, 0, 1000001, 0, SEED, 0.0, 0)
    for fn, tail in ((L.cgrt_photon_emit_host, ()), (L.cgrt_photon_emit, (None,))):
        assert fn(None, 0, 1, None, None, None, None, None, *tail) == INVALID
        assert fn(C.byref(ph), 0, -1, None, None, None, None, None, *tail) == INVALID
        assert fn(C.byref(ph), -1, 1, None, None, None, None, None, *tail) == INVALID
        assert fn(C.byref(ph), 0, (1 << 36) + 1, None, None, None, None, None, *tail) == LIMIT
