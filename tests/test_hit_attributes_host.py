"""Hit attributes of caller-supplied rays, the part that needs no GPU: the ABI of cgrt_ray_hit_attributes and what both forms
and the Python wrappers refuse before any device is touched (tests/test_rays_host.py is the model)."""
import ctypes as C

import numpy as np
import pytest

import scenes
from cgraytracing_amd import _capi

INVALID, LIMIT = -1, -5  # CGRT_ERR_INVALID, CGRT_ERR_LIMIT (include/cgrt.h)


def test_abi():
    L = _capi.lib()
    for name in ("cgrt_ray_hit_attributes", "cgrt_ray_hit_attributes_host"):
        assert getattr(L, name) is not None and name in _capi.SIGNATURES
        assert getattr(L, name).argtypes == _capi.SIGNATURES[name][1]
    assert C.sizeof(_capi.HitAttributes) == 32
    assert [f for f, _ in _capi.HitAttributes._fields_] == ["prim", "uv2", "color3", "material2"]
    assert L.cgrt_version() == 112  # new declarations only


def test_refused_without_a_device():
    import cgraytracing_amd as cg

    L = _capi.lib()
    n = 4
    org = np.zeros((n, 3), np.float64)
    dirs = np.tile([0.0, 0.0, 1.0], (n, 1))
    obj = np.full(n, -1, np.int32)
    t = np.zeros(n, np.float64)
    prim = np.full(n, 7, np.int32)
    sc = cg.Scene(scenes.scene_pyramid(), commit=False)
    try:
        def call(device_form, n=n, o=org.ctypes.data, d=dirs.ctypes.data, scene=sc._h, rays=True, out=True,
                 hit_obj=obj.ctypes.data, hit_t=t.ctypes.data):
            r = _capi.Rays(n, o, d, None, 0, 0, 1, 0)
            res = _capi.HitAttributes(prim.ctypes.data, None, None, None)
            args = [scene, C.byref(r) if rays else None, hit_obj, hit_t, C.byref(res) if out else None]
            if device_form:
                rc = L.cgrt_ray_hit_attributes(*args, None)
            else:
                rc = L.cgrt_ray_hit_attributes_host(*args)
            return rc, L.cgrt_last_error().decode()

        for device_form in (False, True):
            for what, kw, word in [("uncommitted scene", {}, "committed"), ("n < 0", dict(n=-1), "negative"),
                                   ("null org3", dict(o=None), "org3"), ("null dir3", dict(d=None), "dir3"),
                                   ("null scene", dict(scene=None), "null"), ("null rays", dict(rays=False), "null"),
                                   ("null out", dict(out=False), "null"), ("null hit_obj", dict(hit_obj=None), "null"),
                                   ("null hit_t", dict(hit_t=None), "null")]:
                rc, msg = call(device_form, **kw)
                assert rc == INVALID, (what, device_form, rc)
                assert msg and word in msg, (what, device_form, msg)
            rc, msg = call(device_form, n=(1 << 36) + 1)
            assert rc == LIMIT and "2^36" in msg, (device_form, rc, msg)
            rc, _ = call(device_form, n=1 << 36)  # the limit itself is no LIMIT error (the scene is uncommitted: INVALID)
            assert rc == INVALID
            rc, _ = call(device_form, n=0)
            assert rc == _capi.CGRT_OK, device_form
        assert (prim == 7).all()  # nothing was written
    finally:
        sc.close()


def test_host_wrapper_raises_value_error():
    import cgraytracing_amd as cg

    n = 5
    org, dirs = np.zeros((n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1))
    obj, t = np.full(n, -1, np.int32), np.zeros(n)
    sc = cg.Scene(scenes.scene_pyramid(), commit=False)
    try:
        for what, args, kw in [
            ("org shape", (np.zeros((n, 2)), dirs, obj, t), {}),
            ("lengths differ", (org, dirs[:3], obj, t), {}),
            ("hit_obj dtype", (org, dirs, obj.astype(np.int64), t), {}),
            ("hit_obj shape", (org, dirs, obj[:3], t), {}),
            ("hit_t dtype", (org, dirs, obj, t.astype(np.float32)), {}),
            ("hit_t shape", (org, dirs, obj, t.reshape(n, 1)), {}),
            ("unknown want", (org, dirs, obj, t), dict(want=("prim", "normal"))),
            ("empty want", (org, dirs, obj, t), dict(want=())),
        ]:
            with pytest.raises(ValueError):
                sc.hit_attributes_host(*args, **kw)
                pytest.fail(what)
        # no rays: the arrays asked for, empty, and nothing else
        res = sc.hit_attributes_host(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0), want=("prim", "uv"))
        assert sorted(res) == ["prim", "uv"] and res["prim"].shape == (0,) and res["uv"].shape == (0, 2)
        assert res["prim"].dtype == np.int32 and res["uv"].dtype == np.float64
    finally:
        sc.close()


def test_torch_wrapper_raises_value_error():
    """Tensors on the CPU stand for the wrong device: the checks run before anything reaches the library."""
    import torch
    import cgraytracing_amd as cg

    n = 5
    org, dirs = torch.zeros((n, 3), dtype=torch.float64), torch.zeros((n, 3), dtype=torch.float64)
    obj, t = torch.full((n,), -1, dtype=torch.int32), torch.zeros(n, dtype=torch.float64)
    sc = cg.Scene(scenes.scene_pyramid(), commit=False)
    try:
        for what, args, kw in [
            ("device", (org, dirs, obj, t), {}),
            ("org dtype", (org.float(), dirs, obj, t), {}),
            ("org shape", (org[:, :2].contiguous(), dirs, obj, t), {}),
            ("numpy", (org.numpy(), dirs, obj, t), {}),
            ("want", (org, dirs, obj, t), dict(want=("hit",))),
        ]:
            with pytest.raises(ValueError):
                sc.hit_attributes(*args, **kw)
                pytest.fail(what)
    finally:
        sc.close()
