"""Caller-supplied rays, the part that needs no GPU: the ABI of cgrt_trace_rays / cgrt_camera_rays and the host form of the
camera's primary rays (cgrt_camera_rays_host) against the oracle's lens sampler and a numpy restatement of set_pixel."""
import ctypes as C

import numpy as np
import pytest

import scenes
from backends import Backend, have_ref, lens_samples
from cgraytracing_amd import _capi
from cgraytracing_amd.scene import Camera

SEED = 12345
CAMERAS = [
    ("dof", lambda: scenes.cam_dof()),
    ("off_axis_a", lambda: Camera(cam=(3.0, 2.0, -14.0), lens_radius=1.5)),
    ("off_axis_b", lambda: Camera(cam=(-4.5, 1.25, -8.0), focus_plane=17.0, lens_radius=0.7)),
]
SIZES = [(64, 48), (67, 45), (96, 54)]
SPP = 8  # samples 0..7


def _cam_id(c):
    return c[0]


def test_abi_and_errors():
    import cgraytracing_amd as cg

    L = _capi.lib()
    for name in ("cgrt_trace_rays", "cgrt_trace_rays_host", "cgrt_trace_rays_variant", "cgrt_camera_rays", "cgrt_camera_rays_host"):
        assert getattr(L, name) is not None
    assert L.cgrt_version() == 112
    org = np.zeros((4, 3), np.float64)
    dirs = np.tile([0.0, 0.0, 1.0], (4, 1))
    acc = np.zeros((4, 3), np.float64)
    cnt = np.zeros(8, np.uint64)
    sc = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        def call(n=4, o=org.ctypes.data, d=dirs.ctypes.data, depth=5, scene=sc._h, rays=True, out=True):
            r = _capi.Rays(n, o, d, None, 0, SEED, depth, 0)
            res = _capi.RayResults(acc.ctypes.data, None, None, None, None)
            rc = L.cgrt_trace_rays_host(scene, C.byref(r) if rays else None, C.byref(res) if out else None, cnt.ctypes.data)
            return rc, L.cgrt_last_error().decode()

        for what, kw, word in [("uncommitted scene", {}, "committed"), ("n < 0", dict(n=-1), "negative"),
                               ("null org3", dict(o=None), "org3"), ("null dir3", dict(d=None), "dir3"),
                               ("max_depth 0", dict(depth=0), "max_depth"), ("max_depth 6", dict(depth=6), "max_depth"),
                               ("null scene", dict(scene=None), "null"), ("null rays", dict(rays=False), "null"),
                               ("null out", dict(out=False), "null")]:
            rc, msg = call(**kw)
            assert rc == _capi.CGRT_OK - 1, what  # CGRT_ERR_INVALID
            assert msg and word in msg, (what, msg)
        # the device form refuses the same way, before it touches a device
        r = _capi.Rays(-1, org.ctypes.data, dirs.ctypes.data, None, 0, SEED, 5, 0)
        res = _capi.RayResults(acc.ctypes.data, None, None, None, None)
        assert L.cgrt_trace_rays(sc._h, C.byref(r), C.byref(res), None, None) == -1 and L.cgrt_last_error()
    finally:
        sc.close()
    # camera rays: bad grids
    cc = _capi.Camera((C.c_double * 3)(0, 0, -10), 10.0, 20.0, 0.0)
    for g in (_capi.Grid(0, 8, 8, 0, 0, 0, 1, 1, 0, 1, 5, 0, SEED), _capi.Grid(8, 8, 8, 0, 0, 0, 1, 0, 0, 1, 5, 0, SEED),
              _capi.Grid(8, 8, 8, 0, 4, 0, 2, 1, 0, 1, 5, 0, SEED), _capi.Grid(8, 8, 8, -1, 0, 0, 1, 1, 0, 1, 5, 0, SEED)):
        assert L.cgrt_camera_rays_host(C.byref(cc), C.byref(g), None, None, None) == -1 and L.cgrt_last_error()
    assert L.cgrt_camera_rays_host(None, None, None, None, None) == -1


def _pixels(W, H, spp):
    """(pixel, sample, w, h) of every ray of a full-frame camera_rays call, in ray order."""
    k, h, w = np.meshgrid(np.arange(spp), np.arange(H), np.arange(W), indexing="ij")
    return (h * W + w).reshape(-1).astype(np.int64), k.reshape(-1).astype(np.int32), w.reshape(-1), h.reshape(-1)


def _norm_err(d):
    """| ||d|| - 1 | measured in extended precision, so that the measurement adds nothing to the figure."""
    x = d.astype(np.longdouble)
    return np.abs(np.sqrt((x * x).sum(axis=1)) - 1).astype(np.float64)


def _pinhole_dirs(cam, W, H, w, h):
    """normalized((px, py, 0) - cam) with the expressions of set_pixel (main.cpp:188-189,198; vec3.h:36-44), operation by
    operation in IEEE double."""
    px = (2.0 * (w.astype(np.float64) / W) - 1) * cam.half_width
    py = (2.0 * (h.astype(np.float64) / H) - 1) * cam.half_width * H / W
    x, y, z = px - cam.cam[0], py - cam.cam[1], np.full_like(px, 0.0) - cam.cam[2]
    r = 1 / np.sqrt(x * x + y * y + z * z)
    return np.stack([x * r, y * r, z * r], axis=1)


@pytest.mark.parametrize("cam_case", CAMERAS, ids=_cam_id)
@pytest.mark.parametrize("W,H", SIZES)
def test_camera_rays_host_vs_oracle_sampler(orc, cam_case, W, H):
    """Thin lens: the origin is cam + uniform_sampling_circle(lens_radius) of the (pixel, sample)'s lens stream -- the oracle's
    sampler and, where it has been built, the reference's own -- bit for bit, written as org == cam + sample (the same IEEE
    addition; org - cam == sample holds only where the subtraction is exact, which the default camera's x = y = 0 make it:
    asserted there too).  Pinhole: org == cam and dir == the numpy restatement, bit for bit.  Every direction has unit length to
    4 * 2^-53."""
    from cgraytracing_amd.engine import camera_rays_host

    cam = cam_case[1]()
    org, dirs, keys = camera_rays_host(W, H, SPP, cam, SEED)
    pix, smp, w, h = _pixels(W, H, SPP)
    assert org.shape == (SPP * H * W, 3) and dirs.shape == org.shape and keys.shape == (SPP * H * W,)
    camv = np.asarray(cam.cam, np.float64)
    backends = [orc] + ([Backend("ref")] if have_ref() else [])
    for be in backends:
        ls = lens_samples(be, SEED, pix, smp, cam.lens_radius)
        assert np.array_equal(ls[:, 2], np.zeros(len(ls)))
        assert np.array_equal(org, camv[None, :] + ls), be.prefix
        if cam.cam[0] == 0 and cam.cam[1] == 0:
            assert np.array_equal(org - camv[None, :], ls), be.prefix
    # the direction goes from the lens point to the pixel's point on the focus plane (main.cpp:203-206)
    pd = _pinhole_dirs(cam, W, H, w, h)
    pof = pd * ((cam.focus_plane - cam.cam[2]) / pd[:, 2])[:, None] + camv[None, :]
    v = pof - org
    r = 1 / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    assert np.array_equal(dirs, v * r[:, None])
    assert _norm_err(dirs).max() <= 4 * 2.0 ** -53

    pin = Camera(cam=cam.cam, half_width=cam.half_width, focus_plane=cam.focus_plane, lens_radius=0.0)
    porg, pdirs, pkeys = camera_rays_host(W, H, SPP, pin, SEED)
    assert np.array_equal(porg, np.tile(camv, (len(porg), 1)))
    assert np.array_equal(pdirs, pd)
    assert _norm_err(pdirs).max() <= 4 * 2.0 ** -53
    assert np.array_equal(pkeys, keys)  # the key belongs to (pixel, sample), not to the lens


@pytest.mark.parametrize("cam_case", CAMERAS[:2], ids=_cam_id)
def test_camera_rays_rows_stripes_and_keys(cam_case):
    """Row ranges, sample ranges and block-cyclic stripes select rays of the full frame: local row -> global row as cgrt_grid
    documents, rows beyond `height` get dir == 0; keys are equal for equal (pixel, sample), distinct otherwise, and do not
    depend on how the frame is cut."""
    from cgraytracing_amd.engine import camera_rays_host

    cam = cam_case[1]()
    W, H = 67, 45
    full = [a.reshape(SPP, H, W, -1) for a in camera_rays_host(W, H, SPP, cam, SEED)]
    assert len(np.unique(full[2])) == SPP * H * W, "keys of distinct (pixel, sample) collide"
    # a band of rows, a range of samples
    part = [a.reshape(3, 13, W, -1) for a in camera_rays_host(W, H, 3, cam, SEED, rows=13, row_offset=20, sample_offset=4)]
    for f, p in zip(full, part):
        assert np.array_equal(p, f[4:7, 20:33])
    # another seed: other keys everywhere
    assert not np.any(camera_rays_host(W, H, 1, cam, SEED + 1)[2] == full[2][0].reshape(-1))
    # stripes of 8 rows dealt to 3 ranks: each rank's local rows cover ceil(6 stripes / 3) * 8 = 16 rows
    S, nranks = 8, 3
    seen = np.zeros(H, bool)
    for rank in range(nranks):
        rows = 16
        st = [a.reshape(SPP, rows, W, -1) for a in camera_rays_host(W, H, SPP, cam, SEED, rows=rows, stripe=(S, rank, nranks))]
        for j in range(rows):
            h = ((j // S) * nranks + rank) * S + j % S
            if h < H:
                seen[h] = True
                for f, p in zip(full, st):
                    assert np.array_equal(p[:, j], f[:, h]), (rank, j, h)
            else:
                assert np.array_equal(st[1][:, j], np.zeros((SPP, W, 3))), (rank, j, h)
                assert np.array_equal(st[0][:, j], np.tile(np.asarray(cam.cam, np.float64), (SPP, W, 1)))
    assert seen.all()
