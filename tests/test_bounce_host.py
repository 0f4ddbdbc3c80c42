"""CPU: the bounce-query entry points (cgrt_bounce_rays, _host, _variant) are exported and bound, cgrt_bounce has the header's
layout, and every argument error is returned before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenes

NAMES = ("cgrt_bounce_rays", "cgrt_bounce_rays_host", "cgrt_bounce_rays_variant")
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_bound():
    from cgraytracing_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), "libcgrt.so does not export %s" % name
        assert name in _capi.SIGNATURES, name
    assert C.sizeof(_capi.Bounce) == 120
    # the binding's fields are the header's, in its order
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgrt.h")).read(), flags=re.S)
    body = re.search(r"typedef struct cgrt_bounce \{(.*?)\} cgrt_bounce;", hdr, flags=re.S).group(1)
    fields = [f for decl in body.split(";") for f in re.findall(r"\*\s*([a-z_0-9]+)", decl)]
    assert fields == [f[0] for f in _capi.Bounce._fields_], fields
    # ... and the step codes
    steps = {k: int(v) for k, v in re.findall(r"\bCGRT_(STEP_[A-Z]+)\s*=\s*(\d+)", hdr)}
    assert steps == dict(STEP_NONE=0, STEP_HITPOINT=1, STEP_REFLECT=2, STEP_SPLIT=3)
    assert {k: getattr(_capi, k) for k in steps} == steps


def _args(n, outputs=True):
    from cgraytracing_amd import _capi
    m = max(1, min(n, 4))
    keep = [np.zeros((m, 3)), np.tile([0.0, 0.0, 1.0], (m, 1)), np.full(m, 7, np.uint8), np.full((2 * m, 3), 7.0)]
    r = _capi.Rays(n, keep[0].ctypes.data, keep[1].ctypes.data, None, 0, 1, 1, 0)
    b = _capi.Bounce()
    if outputs:
        b.step, b.child_dir3 = keep[2].ctypes.data, keep[3].ctypes.data
    return r, b, keep


@pytest.mark.parametrize("entry", ["device", "host"])
def test_argument_errors_without_a_device(entry):
    """Null scene, null rays, null cgrt_bounce, uncommitted scene, n < 0 and n > 2^36 are refused by both forms before anything
    is launched or allocated; n == 0 is valid and does nothing, and so is a call that asks for no output (on an uncommitted
    scene the refusal comes first)."""
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    L = _capi.lib()

    def call(h, r, b):
        if entry == "device":
            return L.cgrt_bounce_rays(h, C.byref(r) if r is not None else None, C.byref(b) if b is not None else None, None, None)
        return L.cgrt_bounce_rays_host(h, C.byref(r) if r is not None else None, C.byref(b) if b is not None else None, None)

    s = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        r, b, keep = _args(4)
        assert call(None, r, b) == INVALID and b"null" in L.cgrt_last_error()
        assert call(s._h, None, b) == INVALID and b"null" in L.cgrt_last_error()
        assert call(s._h, r, None) == INVALID and b"null" in L.cgrt_last_error()
        assert call(s._h, r, b) == INVALID and b"not committed" in L.cgrt_last_error()
        r, b, keep = _args(4, outputs=False)
        assert call(s._h, r, b) == INVALID and b"not committed" in L.cgrt_last_error()
        r, b, keep = _args(-1)
        assert call(s._h, r, b) == INVALID and b"negative" in L.cgrt_last_error()
        r, b, keep = _args((1 << 36) + 1)
        assert call(s._h, r, b) == LIMIT and b"2^36" in L.cgrt_last_error()
        r, b, keep = _args(0)
        assert call(s._h, r, b) == _capi.CGRT_OK
        assert keep[2][0] == 7 and keep[3][0, 0] == 7.0  # nothing written
        # the variant's name needs a committed scene too
        buf = C.create_string_buffer(160)
        assert L.cgrt_bounce_rays_variant(s._h, C.byref(r), buf, len(buf)) == INVALID
        assert L.cgrt_bounce_rays_variant(None, C.byref(r), buf, len(buf)) == INVALID
    finally:
        s.close()


def test_python_forms_refuse_an_uncommitted_scene():
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    s = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        o, d = np.zeros((3, 3)), np.tile([0.0, 0.0, 1.0], (3, 1))
        with pytest.raises(_capi.CgrtError) as e:
            s.bounce_host(o, d, adj=np.ones((3, 3)), path=np.ones(3, np.uint32))
        assert e.value.code == INVALID
        for kw in (dict(adj=np.ones((2, 3))), dict(path=np.ones(2, np.uint32)), dict(keys=np.ones(4, np.uint64)), dict(want=("colour",)),
                   dict(want=())):
            with pytest.raises(ValueError):
                s.bounce_host(o, d, **kw)
        none = s.bounce_host(np.zeros((0, 3)), np.zeros((0, 3)))
        assert none["step"].shape == (0,) and none["child_dir"].shape == (0, 3) and none["nrays"] == 0
        assert sorted(s.bounce_host(np.zeros((0, 3)), np.zeros((0, 3)), want=("step", "children"))) == sorted(
            ["step", "child_org", "child_dir", "child_adj", "child_path", "child_keys", "counters", "nrays", "nhp"])
    finally:
        s.close()
