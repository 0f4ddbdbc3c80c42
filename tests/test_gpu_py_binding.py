"""GPU: the three faces of every ray query of the Python binding -- the torch form with fresh results, the torch form writing
into preallocated `out` and `counters`, and the numpy `_host` form -- give the same numbers in the dtypes and shapes the
docstrings promise, at 64 rays and at none; and the two session classes' image getters agree and close as documented.  Written
against the binding as its callers see it: it passes unchanged on the commit before the checks moved into _buffers.py."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W = H = 8
# result -> (torch dtype, numpy dtype of the _host form, shape with n rays; m = the Hitpoints returned): the docstrings, literally
TRACE_RAYS = {"acc": ("float64", "float64", "n,3"), "nhit": ("int32", "uint32", "n"), "hit_obj": ("int32", "int32", "n"),
              "hit_t": ("float64", "float64", "n"), "hit_normal": ("float64", "float64", "n,3"), "counters": ("int64", "uint64", "8")}
HIT_ATTRIBUTES = {"prim": ("int32", "int32", "n"), "uv": ("float64", "float64", "n,2"), "color": ("float64", "float64", "n,3"),
                  "material": ("float64", "float64", "n,2")}
OCCLUDED = {"occluded": ("uint8", "uint8", "n"), "counters": ("int64", "uint64", "8")}
BOUNCE = {"step": ("uint8", "uint8", "n"), "hit_obj": ("int32", "int32", "n"), "hit_t": ("float64", "float64", "n"),
          "pos": ("float64", "float64", "n,3"), "normal": ("float64", "float64", "n,3"), "value": ("float64", "float64", "n,3"),
          "child_org": ("float64", "float64", "2n,3"), "child_dir": ("float64", "float64", "2n,3"), "child_adj": ("float64", "float64", "2n,3"),
          "child_path": ("int32", "uint32", "2n"), "child_keys": ("int64", "uint64", "2n"), "counters": ("int64", "uint64", "8")}
WAVEFRONT = {"acc": ("float64", "float64", "n,3"), "nhit": ("int32", "uint32", "n"), "hp9": ("float64", "float64", "m,9"),
             "hp_ray": ("int64", "int64", "m"), "hp_path": ("int32", "uint32", "m"), "counters": ("int64", "uint64", "8")}
WAVEFRONT_INTS = ("hp_count", "slices", "halvings", "levels")
HOST_INTS = {"trace_rays": ("nrays", "nhp"), "hit_attributes": (), "occluded": ("nrays",), "bounce": ("nrays", "nhp"), "wavefront": ("nrays", "nhp")}


def _shape(s, n, m):
    rows = {"n": n, "2n": 2 * n, "m": m}
    return tuple(rows[d] if d in rows else int(d) for d in s.split(","))


def _check(name, table, dev_res, pre_res, host_res, pre_out, pre_cnt, base, n):
    """The three results of one query against `table` and against each other."""
    import torch
    ints = (WAVEFRONT_INTS if name == "wavefront" else ()) + (("rays_per_level",) if name == "wavefront" else ())
    assert set(dev_res) == set(pre_res) == set(table) | set(ints), (name, sorted(dev_res))
    assert set(host_res) == set(table) | set(ints) | set(HOST_INTS[name]), (name, sorted(host_res))
    m = dev_res.get("hp_count", 0)
    for k, (tdt, ndt, shape) in table.items():
        d, p, h = dev_res[k], pre_res[k], host_res[k]
        want = _shape(shape, n, m)
        assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == getattr(torch, tdt) and tuple(d.shape) == want, (name, k, d.dtype, d.shape)
        assert p.dtype == d.dtype and p.shape == d.shape, (name, k)
        assert isinstance(h, np.ndarray) and h.dtype == np.dtype(ndt) and h.shape == want, (name, k, h.dtype, h.shape)
        dn, pn = d.cpu().numpy().view(ndt), p.cpu().numpy().view(ndt)  # the documented signed / unsigned pairs as one type
        if k == "counters":
            assert np.array_equal(pn, dn + np.uint64(base)), (name, "counters are added to", pn, dn)
            assert p is pre_cnt or pre_cnt is None
        else:
            assert np.array_equal(pn, dn), (name, k)
            if k.startswith("hp"):  # the first m rows of the caller's hp_cap rows
                assert m == 0 or p.data_ptr() == pre_out[k].data_ptr(), (name, k)
            elif k in pre_out:
                assert p is pre_out[k], (name, k)
        assert np.array_equal(h, dn), (name, k)
    for k in ints:
        assert dev_res[k] == pre_res[k] == host_res[k], (name, k)
    for k in HOST_INTS[name]:
        assert host_res[k] == int(host_res["counters"][{"nrays": 0, "nhp": 1}[k]])


@pytest.fixture(scope="module")
def scene(gpu_ready):
    import cgraytracing_amd as cg
    with cg.Scene(scenes.scene_c1()) as sc:
        yield sc


@pytest.mark.parametrize("n", [64, 0])
def test_torch_preallocated_and_host_forms_agree(scene, n):
    import torch
    sc = scene
    dev = torch.device("cuda", sc.device)
    org, dirs, keys = (t[:n] for t in sc.camera_rays(W, H, spp=1))
    assert org.shape == (n, 3) and org.is_contiguous()
    o, d, k = org.cpu().numpy(), dirs.cpu().numpy(), keys.cpu().numpy().view(np.uint64)
    BASE = 1000

    def pre(table, m=0):
        out = {name: torch.full(_shape(shape, n, m), 7, dtype=getattr(torch, tdt), device=dev) for name, (tdt, _, shape) in table.items() if name != "counters"}
        return out, torch.full((8,), BASE, dtype=torch.int64, device=dev)

    out, cnt = pre(TRACE_RAYS)
    fresh = sc.trace_rays(org, dirs, keys)
    _check("trace_rays", TRACE_RAYS, fresh, sc.trace_rays(org, dirs, keys, out=out, counters=cnt), sc.trace_rays_host(o, d, k), out, cnt, BASE, n)
    if n:
        assert int(fresh["counters"][0]) >= n and (fresh["hit_obj"] >= 0).all()

    hit_obj, hit_t = fresh["hit_obj"], fresh["hit_t"]
    out, _ = pre(HIT_ATTRIBUTES)
    _check("hit_attributes", HIT_ATTRIBUTES, sc.hit_attributes(org, dirs, hit_obj, hit_t), sc.hit_attributes(org, dirs, hit_obj, hit_t, out=out),
           sc.hit_attributes_host(o, d, hit_obj.cpu().numpy(), hit_t.cpu().numpy()), out, None, 0, n)

    tmax = hit_t * torch.where(torch.arange(n, device=dev) % 2 == 0, 2.0, 0.5).to(torch.float64)
    out, _ = pre(OCCLUDED)
    occ = sc.occluded(org, dirs, tmax, keys)
    as_tensor = sc.occluded(org, dirs, tmax, keys, out=out["occluded"])
    _check("occluded", OCCLUDED, occ, sc.occluded(org, dirs, tmax, keys, out=out), sc.occluded_host(o, d, tmax.cpu().numpy(), k), out, None, 0, n)
    assert as_tensor["occluded"] is out["occluded"]
    if n:
        assert occ["occluded"].cpu().tolist() == [1, 0] * (n // 2)

    out, cnt = pre(BOUNCE)
    _check("bounce", BOUNCE, sc.bounce(org, dirs, keys=keys), sc.bounce(org, dirs, keys=keys, out=out, counters=cnt), sc.bounce_host(o, d, keys=k),
           out, cnt, BASE, n)

    want = ("acc", "nhit", "hp")
    fresh = sc.wavefront(org, dirs, keys, want=want)
    out, cnt = pre(WAVEFRONT, 4 * n)
    _check("wavefront", WAVEFRONT, fresh, sc.wavefront(org, dirs, keys, want=want, out=out, counters=cnt), sc.wavefront_host(o, d, k, want=want),
           out, cnt, BASE, n)
    assert fresh["hp_count"] == (n if n else 0) and fresh["levels"] == (1 if n else 0)  # C1 is diffuse: one Hitpoint a ray


def test_hitpoint_getters_with_less_room_than_records(gpu_ready):
    """cgrt_ppm_session_hitpoints / cgrt_sppm_session_last_hitpoints given room for fewer records than the table holds: the first
    `cap` rows of the full dump, nothing written behind them, and the full count.  32 x 24, spp 2, four batches a call."""
    import ctypes as C
    import cgraytracing_amd as cg
    from cgraytracing_amd._capi import check
    with cg.Scene(scenes.scene_c2()) as sc:
        ppm = sc.ppm_session(32, 24, 2, scenes.cam_dof(), nphotons=3000, batch=800)
        sppm = sc.sppm_session(32, 24, 2, scenes.cam_dof(), initial_radius=2.0, batch=800).add_passes(1, 3000)
        for ses in (ppm, sppm):
            full = ses._hitpoint_dump()
            n = len(full)
            assert n == ses.info()["hp_count"] > 2 * 32 * 24 and full[:, 11:14].any()
            for cap in (0, 1, n // 2 + 1, n - 1, n + 5):
                part = np.full((cap + 2, 16), 7.0)
                count = C.c_uint64(0)
                check(ses._fn(ses._HITPOINTS)(ses._h, part.ctypes.data if cap else None, cap, C.byref(count)))
                m = min(cap, n)
                assert count.value == n, cap
                assert np.array_equal(part[:m].view(np.uint64), full[:m].view(np.uint64)) and (part[m:] == 7.0).all(), cap


def test_sessions_share_their_image_getters_and_their_end(gpu_ready):
    import torch
    import cgraytracing_amd as cg
    from cgraytracing_amd import _capi
    sc = cg.Scene(scenes.scene_c1())
    dev = torch.device("cuda", sc.device)
    ppm = sc.ppm_session(16, 16, spp=1, nphotons=2000)
    sppm = sc.sppm_session(16, 16, spp=1).add_passes(1, 2000)
    for ses, info in ((ppm, _capi.PpmSessionInfo), (sppm, _capi.SppmSessionInfo)):
        assert list(ses.info()) == [f for f, _ in info._fields_]
        assert ses.photons_done == ses.info()["photons_done"] == 2000
        img, rgb8 = ses.image(), ses.rgb8()
        assert img.dtype == np.float64 and img.shape == (16, 16, 3) and rgb8.dtype == np.uint8 and rgb8.shape == (16, 16, 3)
        assert img.max() > 0 and rgb8.max() > 0
        rgb = torch.full((16, 16, 3), 7, dtype=torch.uint8, device=dev)
        out = torch.empty((16, 16, 3), dtype=torch.float64, device=dev)
        assert ses.image_tensor(out=out, rgb8_out=rgb) is out
        fresh = ses.image_tensor()
        torch.cuda.synchronize(dev)
        assert np.array_equal(out.cpu().numpy(), img) and np.array_equal(fresh.cpu().numpy(), img)
        assert np.array_equal(rgb.cpu().numpy(), rgb8)
    assert sppm.passes == 1 and len(ppm.hitpoints()) == ppm.info()["hp_count"] and sppm.last_hitpoints().shape[1] == 16
    ppm.close()
    ppm.close()  # twice is harmless
    assert ppm._h is None and sppm._h is not None
    sc.close()  # closes the sessions it still has
    assert sppm._h is None and sc._h is None
    sppm.close()
    sc.close()
