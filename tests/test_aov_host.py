"""CPU: the grid AOV pass (cgrt_trace_grid_aov) as far as it goes without a device -- its symbols and struct, its refusals, the
Python binding's argument faults (the fake device tensors of test_py_binding_host.py) and its launch plan under ASan + UBSan
(tests/native/aov_plan.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import scenes
import cgraytracing_amd as cg
from cgraytracing_amd import _capi, aov, refit
from cgraytracing_amd._capi import CgrtError
from test_py_binding_host import dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cgrt_trace_grid_aov", "cgrt_trace_grid_aov_host", "cgrt_trace_grid_aov_variant")
INVALID = -1
W, H = 45, 19


def test_symbols_struct_and_version():
    lib = C.CDLL(_capi.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgrt.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert C.sizeof(_capi.GridAov) == 40 and [f for f, _ in _capi.GridAov._fields_] == ["albedo3", "normal3", "depth", "hits", "obj_id"]
    assert re.search(r"typedef struct cgrt_grid_aov \{[^}]*\} cgrt_grid_aov;", hdr)
    assert _capi.lib().cgrt_version() == 112 and "#define CGRT_VERSION 112" in hdr
    # the package's Scene is the AOV one, on top of the refit one; engine's own surface is left alone
    assert cg.Scene is aov.Scene and issubclass(aov.Scene, refit.Scene)
    assert not hasattr(cg.engine.Scene, "trace_grid_aov")


def _grid(**kw):
    g = dict(width=W, height=H, rows=H, row_offset=0, stripe_rows=0, stripe_rank=0, stripe_nranks=1, spp=3, sample_offset=0, spp_total=3,
             max_depth=5, flags=0, seed=12345)
    g.update(kw)
    return _capi.Grid(*[g[f] for f, _ in _capi.Grid._fields_])


def _camera(**kw):
    c = dict(cam=(0.0, 0.0, -10.0), half_width=10.0, focus_plane=20.0, lens_radius=1.5)
    c.update(kw)
    return _capi.Camera((C.c_double * 3)(*c["cam"]), c["half_width"], c["focus_plane"], c["lens_radius"])


def _calls(L, h, cam, grid, out):
    """the three entry points on (scene, cam, grid, out): name -> return code, message"""
    buf = C.create_string_buffer(160)
    cam_p, grid_p, out_p = (C.byref(x) if x is not None else None for x in (cam, grid, out))
    res = {}
    for name, call in (("device", lambda: L.cgrt_trace_grid_aov(h, cam_p, grid_p, out_p, None, None)),
                       ("host", lambda: L.cgrt_trace_grid_aov_host(h, cam_p, grid_p, out_p, None)),
                       ("variant", lambda: L.cgrt_trace_grid_aov_variant(h, cam_p, grid_p, buf, len(buf)))):
        rc = call()
        res[name] = (rc, L.cgrt_last_error().decode())
    return res


BAD_GRIDS = [dict(width=0), dict(height=0), dict(rows=0), dict(width=-3), dict(spp=0), dict(spp_total=0), dict(sample_offset=-1),
             dict(stripe_nranks=2, stripe_rows=0), dict(stripe_nranks=2, stripe_rows=12), dict(stripe_nranks=3, stripe_rows=8, stripe_rank=3),
             dict(stripe_nranks=3, stripe_rows=8, stripe_rank=-1), dict(row_offset=-1)]


def test_refusals_before_any_device():
    """On an uncommitted scene (no device was ever named): a null scene, cam, grid or out, every grid field cgrt_trace_grid
    refuses, a negative lens, CGRT_GRID_POSED with a pose that is not orthonormal, and the uncommitted scene itself are
    CGRT_ERR_INVALID with a message from all three entry points; max_depth is not looked at."""
    L = _capi.lib()
    arr = np.zeros(8)
    out = _capi.GridAov(arr.ctypes.data, None, None, None, None)
    with cg.Scene(scenes.scene_c1(), commit=False) as sc:
        h = sc._h
        for args in ((None, _camera(), _grid(), out), (h, None, _grid(), out), (h, _camera(), None, out)):
            for name, (rc, msg) in _calls(L, *args).items():
                assert rc == INVALID and "null" in msg, (name, rc, msg)
        for name, (rc, msg) in _calls(L, h, _camera(), _grid(), None).items():
            if name != "variant":  # (which has no `out`)
                assert rc == INVALID and "null" in msg, (name, rc, msg)
        name_buf = C.create_string_buffer(160)
        assert L.cgrt_trace_grid_aov_variant(h, C.byref(_camera()), C.byref(_grid()), None, 160) == INVALID
        assert L.cgrt_trace_grid_aov_variant(h, C.byref(_camera()), C.byref(_grid()), name_buf, 0) == INVALID
        # the scene itself, whatever max_depth says and whatever is asked for
        for g in (_grid(), _grid(max_depth=0), _grid(max_depth=99)):
            for o in (out, _capi.GridAov()):
                for name, (rc, msg) in _calls(L, h, _camera(), g, o).items():
                    assert rc == INVALID and msg.endswith("scene not committed"), (name, rc, msg)
        # cgrt_trace_grid's own answer to each bad field is this call's answer
        posed = _capi.PosedCamera(_camera(), (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 0, 0), (C.c_double * 3)(0, 1, 0), (C.c_double * 3)(0, 0.6, 0.9))
        cases = [(_camera(), _grid(**kw)) for kw in BAD_GRIDS] + [(_camera(lens_radius=-1.0), _grid()), (_camera(lens_radius=float("nan")), _grid()),
                                                                  (posed.base, _grid(flags=_capi.GRID_POSED))]
        for cam, g in cases:
            want_rc = L.cgrt_trace_grid(h, C.byref(cam), C.byref(g), arr.ctypes.data, None, None, None)
            want_msg = L.cgrt_last_error().decode()
            assert want_rc == INVALID and want_msg
            for name, (rc, msg) in _calls(L, h, cam, g, out).items():
                assert (rc, msg) == (want_rc, want_msg), (name, rc, msg, want_msg)
    assert (arr == 0).all()


def test_python_argument_faults():
    """trace_grid_aov on an uncommitted scene with fake device tensors: a wrong dtype, shape or device in out[...] and an unknown
    name in `want` raise ValueError naming the argument; a call whose Python checks all pass reaches the library, which refuses
    the scene."""
    spec = dict(albedo=(torch.float32, (H, W, 3)), normal=(torch.float32, (H, W, 3)), depth=(torch.float32, (H, W)),
                hits=(torch.int32, (H, W)), obj_id=(torch.int32, (H, W)))
    good = lambda: {k: dev(s, dt) for k, (dt, s) in spec.items()}
    cnt = lambda: dev((8,), torch.int64)
    with cg.Scene(scenes.scene_c1(), commit=False) as sc:
        call = lambda **kw: sc.trace_grid_aov(W, H, 3, **dict(dict(out=good(), counters=cnt(), stream=0), **kw))
        with pytest.raises(CgrtError, match="scene not committed"):
            call()
        with pytest.raises(CgrtError, match="scene not committed"):
            call(want=("depth",), out=dict(depth=dev((H, W), torch.float32)), accumulate=True)
        for name, (dt, shape) in spec.items():
            wrong = torch.float64 if dt == torch.float32 else torch.int64
            for fault, t in (("dtype", dev(shape, wrong)), ("shape", dev(shape + (2,), dt)), ("rows", dev((shape[0] + 1,) + shape[1:], dt)),
                             ("transposed", dev((shape[1], shape[0]) + shape[2:], dt)), ("cpu", torch.zeros(shape, dtype=dt)),
                             ("ndarray", np.zeros(shape, np.float32)), ("strided", dev((2 * shape[0],) + shape[1:], dt)[::2])):
                with pytest.raises(ValueError, match=re.escape("trace_grid_aov: out[%r] must be a contiguous" % name)):
                    call(out=dict(good(), **{name: t}))
        # a striped share's buffers have the share's rows
        with pytest.raises(ValueError, match=re.escape("out['depth']")):
            call(rows=16, stripe=(8, 2, 3), want=("depth",), out=dict(depth=dev((H, W), torch.float32)))
        for want in ((), ("nope",), ("albedo", "nope"), ("color",)):
            with pytest.raises(ValueError, match="trace_grid_aov: want"):
                call(want=want)
            with pytest.raises(ValueError, match="trace_grid_aov_host: want"):
                sc.trace_grid_aov_host(W, H, 3, want=want)
        with pytest.raises(ValueError, match="trace_grid_aov: counters"):
            call(counters=dev((8,), torch.int32))
        with pytest.raises(CgrtError, match="scene not committed"):
            sc.trace_grid_aov_host(W, H, 3)
        with pytest.raises(CgrtError, match="scene not committed"):
            sc.aov_variant(W, H)


def test_aov_plan_over_every_trait_combination(tmp_path):
    """aov_choice over every scene class of rays_plan.cpp's sweep: every choice is a row of CGRT_AOV_VARIANTS, every row is
    chosen, each equals rays_plan's nearest-hit row for the same traits with its resident objects and LDS, the rows' layouts
    fit a workgroup's LDS at a full object list (600 objects for the general row), the workgroups are the eye pass's tiles,
    the names of six fixed scenes are the literal strings; sizeof(cgrt_grid_aov) is 40."""
    exe = str(tmp_path / "aov_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    native = os.path.join(ROOT, "tests", "native")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-I", native, os.path.join(native, "aov_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
    m = re.search(r"traits checked: (\d+)", out.stdout)
    assert m and int(m.group(1)) >= 5 * 2 * 16, out.stdout
