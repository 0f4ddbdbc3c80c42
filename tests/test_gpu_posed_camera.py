"""GPU: the posed camera (CGRT_GRID_POSED) in the grid kernels.  The chain to the reference: a posed launch of one sample equals
trace_rays over the posed camera_rays ray for ray, and trace_rays is pinned to the oracle per ray by test_gpu_rays.py; the
identity pose is the built-in camera bit for bit; several samples in one launch are the sequential fp64 fold of the captured
Hitpoint records; scheduling, ignored flags, the handle's caches, stripes, split samples and the PPM / SPPM sessions keep their
contracts under a pose.

Views: the identity frame, a 90 degree turn about y (a basis of exact unit axes, the eye inside the room looking along +x) and
the look-at view of examples/lookat_grid.py.  A case's own camera is the camera in its frame; under the look-at view a thin-lens
case keeps a lens (radius 0.5, sharp at distance 30)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from cgraytracing_amd import _capi
from cgraytracing_amd.scene import Camera
from test_gpu_parity import BEZ_SCENE_BAR
from test_gpu_rays import CASES, _bezier_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
TURNED = ((-8.0, 0.0, 20.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))  # forward +x, right = up x forward = -z
EYE, TARGET, FOV = (17.0, 8.0, 2.0), (-2.0, -13.0, 30.0), 70.0
RAYS, HITPOINTS = _capi.CNT_RAYS, _capi.CNT_HITPOINTS


def posed(cam, view):
    """The case's camera `cam` under a view: "identity" / "turned" keep it as the camera of the frame; "lookat" is cgrt_look_at's."""
    if view == "lookat":
        return Camera.look_at(EYE, TARGET, (0.0, 1.0, 0.0), FOV, focus_distance=30.0, lens_radius=0.5 if cam.lens_radius > 0 else 0.0)
    return Camera(cam.cam, cam.half_width, cam.focus_plane, cam.lens_radius, pose=IDENTITY if view == "identity" else TURNED)


def grid(sc, cam, W, H, spp, depth, seed=SEED, **kw):
    """trace_grid as numpy: (rgb float32, nhit uint32, counters)"""
    import torch
    rgb, nhit, cnt = sc.trace_grid(W, H, spp, cam, depth, seed, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), nhit.cpu().numpy().view(np.uint32), cnt.cpu().numpy()


def rays(sc, cam, W, H, spp, depth, seed=SEED, **kw):
    """trace_rays over camera_rays of the same grid as numpy: (acc float64 [spp, rows, W, 3], nhit uint32 [spp, rows, W], counters)"""
    import torch
    org, dirs, keys = sc.camera_rays(W, H, spp, cam, seed, **kw)
    res = sc.trace_rays(org, dirs, keys, max_depth=depth, seed=seed, want=("acc", "nhit"))
    torch.cuda.synchronize()
    rows = org.shape[0] // (spp * W)
    return (res["acc"].cpu().numpy().reshape(spp, rows, W, 3), res["nhit"].cpu().numpy().view(np.uint32).reshape(spp, rows, W),
            res["counters"].cpu().numpy())


def _case(name):
    return next(c for c in CASES if c[0] == name)


@pytest.mark.parametrize("view", ["identity", "turned", "lookat"])
def test_device_camera_rays_equal_host(gpu_ready, view):
    """cgrt_camera_rays on the device equals cgrt_camera_rays_host bit for bit: lens and pinhole, a full odd-sized frame, a
    striped share with padding rows, a band of rows with a sample range."""
    import cgraytracing_amd as cg
    from cgraytracing_amd.engine import camera_rays_host

    with cg.Scene(scenes.scene_c1()) as sc:
        for base in (scenes.cam_dof(), scenes.cam_pinhole(), Camera(cam=(-4.5, 1.25, -8.0), focus_plane=17.0, lens_radius=0.7)):
            cam = posed(base, view)
            for kw in (dict(), dict(rows=16, stripe=(8, 2, 3)), dict(rows=13, row_offset=20, sample_offset=4)):
                want = camera_rays_host(67, 45, 3, cam, SEED, **kw)
                got = [t.cpu().numpy() for t in sc.camera_rays(67, 45, 3, cam, SEED, **kw)]
                assert all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want)), (view, kw)
                assert np.any(want[1] != 0)


IDENTITY_CASES = [
    # deep enough (64 samples, the relay and the lens table asked for) that the unposed side relays and reads its lens table
    ("c2_lens_160x90_spp64", scenes.scene_c2, scenes.cam_dof, 160, 90, 64, dict(sample_relay=True, lens_table=True)),
    ("c3_bunny_glass_64x64_spp4", lambda: scenes.scene_c3(True), scenes.cam_dof, 64, 64, 4, {}),
    ("dragon_128x128_spp4", scenes.scene_dragon, scenes.cam_pinhole, 128, 128, 4, {}),
]


@pytest.mark.parametrize("name,mk,cam,W,H,spp,kw", IDENTITY_CASES, ids=[c[0] for c in IDENTITY_CASES])
def test_identity_pose_is_the_builtin_camera(gpu_ready, name, mk, cam, W, H, spp, kw):
    """trace_grid with the identity pose against the launch without the flag: image, hit counts, rays and Hitpoints equal
    (CGRT_CNT_WAVE_ITERS may differ: the unposed launch relays)."""
    import cgraytracing_amd as cg

    with cg.Scene(mk()) as sc:
        a = grid(sc, cam(), W, H, spp, 5, **kw)
        relay = sc.last_sample_relay() if name.startswith("c2") else None
        plain_name = sc.kernel_variant(W, H, spp, cam(), 5)
        b = grid(sc, posed(cam(), "identity"), W, H, spp, 5, **kw)
        posed_name = sc.kernel_variant(W, H, spp, posed(cam(), "identity"), 5)
    print(name, plain_name, "->", posed_name, "rays", a[2][RAYS], "relay", relay)
    assert "POSE" not in plain_name and posed_name.endswith(",POSE=1>")
    if relay is not None:
        assert relay["tiles"] > 0, "the unposed side was meant to relay"
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2][RAYS] == b[2][RAYS] > 0 and a[2][HITPOINTS] == b[2][HITPOINTS] > 0


ONE_RAY_CASES = [(n, W, H) for n, W, H in [("c1_spheres_depth1", 128, 128), ("c2_glass_dof", 96, 54), ("pyramid_glass", 96, 96),
                                           ("c3_bunny_glass_chess", 64, 64), ("dragon_diffuse", 128, 128), ("glass_bump_floor", 96, 72),
                                           ("plain_planes_depth1", 64, 48)]]


@pytest.mark.parametrize("name,W,H", ONE_RAY_CASES, ids=[c[0] for c in ONE_RAY_CASES])
def test_one_sample_is_one_ray(gpu_ready, name, W, H):
    """For the turned view and the look-at view and each sample k in 0..3: trace_grid at spp 1, sample_offset k, spp_total 1
    equals float32 of trace_rays' acc over camera_rays of the same grid, pixel for pixel; nhit and the two counters too.  The
    scene classes of test_gpu_rays.CASES, where trace_rays itself is pinned to the oracle ray for ray."""
    import cgraytracing_amd as cg

    _, mk, cam, _, _, _, depth = _case(name)
    with cg.Scene(mk()) as sc:
        for view in ("turned", "lookat"):
            pc = posed(cam(), view)
            variant = sc.kernel_variant(W, H, 1, pc, depth)
            assert variant.endswith(",POSE=1>"), variant
            seen = 0
            for k in range(4):
                rgb, nhit, cnt = grid(sc, pc, W, H, 1, depth, sample_offset=k, spp_total=1)
                acc, rnhit, rcnt = rays(sc, pc, W, H, 1, depth, sample_offset=k)
                bad = np.nonzero((rgb != acc[0].astype(np.float32)).any(axis=2))
                assert len(bad[0]) == 0, (name, view, k, variant, len(bad[0]), list(zip(*bad))[:5])
                assert np.array_equal(nhit, rnhit[0]), (name, view, k)
                assert cnt[RAYS] == rcnt[RAYS] and cnt[HITPOINTS] == rcnt[HITPOINTS], (name, view, k)
                seen += int(nhit.sum())
            print(name, view, variant, "Hitpoints", seen)
            assert seen > 0 and float(np.abs(rgb).max()) > 0, "the view sees nothing"


@pytest.mark.parametrize("glass", [False, True], ids=["mirror_vase", "glass_vase"])
def test_one_sample_is_one_ray_bezier(gpu_ready, glass):
    """Bezier scenes (96 x 72): the same comparison under the bar test_gpu_rays.test_bezier_scene_rays_vs_oracle applies to this
    scene class -- share of pixels within 1e-4, relative ray-count gap -- since a Newton outcome is allowed to flip there."""
    import cgraytracing_amd as cg

    W, H = 96, 72
    with cg.Scene(_bezier_scene(glass)) as sc:
        for view in ("turned", "lookat"):
            pc = posed(scenes.cam_dof(), view)
            variant = sc.kernel_variant(W, H, 1, pc, 5)
            assert "BEZ=1,DOF=1,GLASS=%d" % glass in variant and variant.endswith("NT=64,POSE=1>"), variant
            for k in range(4):
                rgb, nhit, cnt = grid(sc, pc, W, H, 1, 5, seed=7, sample_offset=k, spp_total=1)
                acc, rnhit, rcnt = rays(sc, pc, W, H, 1, 5, seed=7, sample_offset=k)
                err = np.abs(rgb.astype(np.float64) - acc[0].astype(np.float32)).max(axis=2)
                frac = float((err < 1e-4).mean())
                gap = abs(int(cnt[RAYS]) - int(rcnt[RAYS])) / max(1, int(rcnt[RAYS]))
                print("%s %s k=%d: within 1e-4 %.6f, bit-equal %.6f, rays %d vs %d" % (variant, view, k, frac, float((err == 0).mean()), cnt[RAYS], rcnt[RAYS]))
                assert frac >= BEZ_SCENE_BAR[0] and gap <= BEZ_SCENE_BAR[1], (view, k, frac, gap)


def _fold(hp, pix, smp, seq, npix, spp_total):
    """The grid kernel's store: per pixel the fp64 sum of its records' f, sample by sample, emission order inside a sample, one
    addition after the other from 0, times 1.0 / spp_total, rounded to fp32."""
    order = np.lexsort([seq, smp, pix])
    f, p = hp[order, 0:3], pix[order]
    first = np.r_[0, np.nonzero(np.diff(p))[0] + 1]
    rank = np.arange(len(p)) - np.repeat(first, np.diff(np.r_[first, len(p)]))
    acc = np.zeros((npix, 3))
    for r in range(int(rank.max()) + 1 if len(rank) else 0):  # every pixel gets at most one addition per round, in its order
        sel = rank == r
        acc[p[sel]] += f[sel]
    return (acc * (1.0 / spp_total)).astype(np.float32)


HITPOINT_CASES = [("c2_glass_dof", 96, 54, 4), ("pyramid_glass", 96, 96, 2), ("dragon_diffuse", 128, 128, 4)]


@pytest.mark.parametrize("name,W,H,spp", HITPOINT_CASES, ids=[c[0] for c in HITPOINT_CASES])
def test_many_samples_in_one_launch(gpu_ready, name, W, H, spp):
    """trace_grid_hitpoints posed against trace_rays_hitpoints over the posed camera_rays: the labels coincide by construction
    (sample * pixels + pixel, position in the ray tree), and the record sets, sorted by label, are equal in all 10 doubles.  The
    posed launch's image at that spp then equals the sequential fp64 fold of those records per pixel."""
    import cgraytracing_amd as cg

    _, mk, cam, _, _, _, depth = _case(name)
    with cg.Scene(mk()) as sc:
        pc = posed(cam(), "lookat")
        g = sc.trace_grid_hitpoints(W, H, spp, pc, depth, SEED)
        org, dirs, keys = sc.camera_rays(W, H, spp, pc, SEED)
        r = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=depth, seed=SEED)
        rgb, nhit, cnt = grid(sc, pc, W, H, spp, depth)
        assert "HPS=1" in sc.kernel_variant(W, H, spp, pc, depth, hitpoints=True) and sc.kernel_variant(W, H, spp, pc, depth, hitpoints=True).endswith("POSE=1>")
    npix = W * H
    glab = ((g["smp"] * npix + g["pix"]) << 4) | g["seq"]
    rlab = (r["ray"] << 4) | r["seq"]
    assert g["count"] == r["count"] == len(glab) == len(rlab) > npix // 4
    go, ro = np.argsort(glab, kind="stable"), np.argsort(rlab, kind="stable")
    assert np.array_equal(glab[go], rlab[ro]) and len(np.unique(glab)) == len(glab)
    assert np.array_equal(g["hp"][go], r["hp"][ro]), "records (f, pos, normal)"
    assert cnt[HITPOINTS] == g["count"] and int(nhit.sum()) == g["count"]
    want = _fold(g["hp"], g["pix"], g["smp"], g["seq"], npix, spp).reshape(H, W, 3)
    assert np.array_equal(rgb, want)
    assert np.array_equal(nhit.reshape(-1), np.bincount(g["pix"], minlength=npix).astype(np.uint32))


SCHED_CASES = [("dragon", scenes.scene_dragon, scenes.cam_pinhole, 128, 128), ("c3_bunny_glass", lambda: scenes.scene_c3(True), scenes.cam_dof, 64, 64)]


@pytest.mark.parametrize("name,mk,cam,W,H", SCHED_CASES, ids=[c[0] for c in SCHED_CASES])
def test_scheduling_does_not_change_the_image(gpu_ready, name, mk, cam, W, H):
    """Posed at spp 8: the default (cost-scheduled) launch against CGRT_GRID_NO_REORDER -- image, hit counts, rays and Hitpoints
    equal.  A posed scheduled launch has no light-tile split and no primary walk: every tile by the full variant.  And
    CGRT_GRID_STATS has no posed kernel: refused as unsupported, nothing launched."""
    import cgraytracing_amd as cg

    with cg.Scene(mk()) as sc:
        for view in ("turned", "lookat"):
            pc = posed(cam(), view)
            sched_name = sc.kernel_variant(W, H, 8, pc, 5)
            image_name = sc.kernel_variant(W, H, 8, pc, 5, flags=_capi.GRID_NO_REORDER)
            assert sched_name.startswith("trace_grid_sched_kernel<") and sched_name.endswith(",POSE=1>"), sched_name
            assert image_name.startswith("trace_grid_kernel<") and image_name.endswith(",POSE=1>"), image_name
            a = grid(sc, pc, W, H, 8, 5)
            b = grid(sc, pc, W, H, 8, 5, reorder=False)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, view)
            assert a[2][RAYS] == b[2][RAYS] > 0 and a[2][HITPOINTS] == b[2][HITPOINTS] > 0
            # ... and the scheduled launch is the per-sample ray trace, sample by sample
            acc, rnhit, rcnt = rays(sc, pc, W, H, 8, 5)
            assert np.array_equal(a[1], rnhit.sum(axis=0).astype(np.uint32)) and a[2][RAYS] == rcnt[RAYS]
        with pytest.raises(_capi.CgrtError) as e:
            sc.trace_grid(W, H, 8, pc, 5, SEED, stats=True)
        assert e.value.code == -4, e.value  # CGRT_ERR_UNSUPPORTED


def test_ignored_flags_and_split_samples(gpu_ready):
    """C2 posed with CGRT_GRID_SAMPLE_RELAY | _LENS_TABLE | _DIFFUSE_TILES: the same image as without them, and the readers say
    that nothing was taken.  CGRT_GRID_SPLIT_SAMPLES is supported under a pose: the identity pose gives the chunks' sums of the
    unposed split launch in image order, bit for bit."""
    import cgraytracing_amd as cg

    W, H, spp = 160, 90, 64
    with cg.Scene(scenes.scene_c2()) as sc:
        pc = posed(scenes.cam_dof(), "lookat")
        a = grid(sc, pc, W, H, spp, 5)
        b = grid(sc, pc, W, H, spp, 5, sample_relay=True, lens_table=True, diffuse_tiles=True)
        assert sc.last_sample_relay()["tiles"] == 0 and sc.last_lens_table()["entries"] == 0 and sc.last_diffuse_tiles() == 0
        assert sc.last_inkernel_diffuse_tiles() == 0 and sc.last_tile_order() is None and sc.last_lens_stage()["lds_tiles"] == 0
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert float(a[0].max()) > 0
        # force_reorder is not followed either: the same kernel, the same counters
        c = grid(sc, pc, W, H, spp, 5, force_reorder=True)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[2], c[2])
        s0 = grid(sc, scenes.cam_dof(), W, H, spp, 5, split_samples=True, tile_order=False)
        s1 = grid(sc, posed(scenes.cam_dof(), "identity"), W, H, spp, 5, split_samples=True)
        assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1]) and s0[2][RAYS] == s1[2][RAYS]
        s2 = grid(sc, pc, W, H, spp, 5, split_samples=True)
        assert np.array_equal(s2[1], a[1]) and s2[2][RAYS] == a[2][RAYS]
        assert float(np.abs(s2[0].astype(np.float64) - a[0]).max()) <= 1e-6  # (the chunk sums' order differs in the last fp64 bit)


def test_the_handles_caches(gpu_ready):
    """The built-in camera, then a posed launch whose base has the same six numbers, then the built-in camera again: the first and
    the third are equal and the third reused the first's tile order; the posed image is the posed image of a fresh scene."""
    import cgraytracing_amd as cg

    W, H, spp = 160, 90, 32
    cam, pc = scenes.cam_dof(), posed(scenes.cam_dof(), "turned")
    with cg.Scene(scenes.scene_c2()) as sc:
        first = grid(sc, cam, W, H, spp, 5, sample_relay=True, lens_table=True)
        assert sc.last_tile_order() is not None and not sc.last_tile_order_reused()
        mid = grid(sc, pc, W, H, spp, 5, sample_relay=True, lens_table=True)
        assert sc.last_tile_order() is None and not sc.last_tile_order_reused()
        third = grid(sc, cam, W, H, spp, 5, sample_relay=True, lens_table=True)
        assert sc.last_tile_order_reused(), "the posed launch dropped or overwrote the cached tile order"
        assert sc.last_lens_table()["reused"], "the posed launch dropped the cached lens table"
    with cg.Scene(scenes.scene_c2()) as fresh:
        alone = grid(fresh, pc, W, H, spp, 5)
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1]) and first[2][RAYS] == third[2][RAYS]
    assert np.array_equal(mid[0], alone[0]) and np.array_equal(mid[1], alone[1]) and np.array_equal(mid[2], alone[2])
    assert not np.array_equal(mid[0], first[0])


def test_stripes(gpu_ready):
    """The look-at view as two striped shares (stripe_rows 8, 2 ranks, a height that is no multiple of 16), row by row the full
    frame."""
    import cgraytracing_amd as cg
    from cgraytracing_amd import dist as cdist

    W, H, spp, S, n = 96, 54, 4, 8, 2
    pc = posed(scenes.cam_dof(), "lookat")
    rows_local = cdist.local_rows(H, S, 0, n)
    with cg.Scene(scenes.scene_c2()) as sc:
        full = grid(sc, pc, W, H, spp, 5)
        seen, total_rays = 0, 0
        for r in range(n):
            share = grid(sc, pc, W, H, spp, 5, rows=rows_local, stripe=(S, r, n))
            total_rays += int(share[2][RAYS])
            for j in range(rows_local):
                h = cdist.global_row(j, S, r, n)
                if h < H:
                    assert np.array_equal(share[0][j], full[0][h]) and np.array_equal(share[1][j], full[1][h]), (r, j, h)
                    seen += 1
                else:
                    assert not share[0][j].any() and not share[1][j].any(), (r, j, h)
    assert seen == H and total_rays == int(full[2][RAYS])


def test_ppm_session(gpu_ready):
    """ppm_session(posed camera) against ppm_session_rays over the posed camera_rays with the grid's pixel map: image and hp16
    bit for bit -- the comparison test_gpu_ppm_rays makes for the built-in camera, at its sizes (32 x 24, spp 2, 20000 photons
    fed in chunks that straddle the batches)."""
    import cgraytracing_amd as cg
    from test_gpu_ppm_rays import _ray_to_ps
    from test_gpu_ppm_session import _feed

    W, H, spp, nph = 32, 24, 2, 20000
    pc = posed(scenes.cam_dof(), "lookat")
    with cg.Scene(scenes.scene_c2()) as sc:
        org, dirs, keys = sc.camera_rays(W, H, spp, pc, SEED)
        with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=spp, batch=3000) as ses:
            _feed(ses, nph)
            img, rgb8, hp, inf = ses.image(), ses.rgb8(), ses.hitpoints(), ses.info()
        with sc.ppm_session(W, H, spp, pc, 5, SEED, batch=3000) as ses:
            _feed(ses, nph)
            gimg, grgb8, ghp, ginf = ses.image(), ses.rgb8(), ses.hitpoints(), ses.info()
        one = sc.ppm_render(W, H, spp, pc, 5, SEED, nphotons=nph, batch=3000)
    hp = _ray_to_ps(hp, W * H, spp)
    assert len(hp) > W * H and float(img.max()) > 0
    assert np.array_equal(img, gimg) and np.array_equal(rgb8, grgb8)
    assert np.array_equal(hp, ghp), "table order"
    assert inf["n_events"] == ginf["n_events"] and inf["hp_count"] == ginf["hp_count"] == len(hp)
    assert np.array_equal(one["image"], gimg), "cgrt_ppm_render under the pose"


def test_sppm_grid_pass_is_ray_pass(gpu_ready):
    """An SPPM session of two posed grid passes against two pass_rays passes over the posed camera_rays, texel for texel, as
    test_gpu_sppm.test_grid_pass_is_ray_pass does for the built-in camera."""
    import cgraytracing_amd as cg
    from test_gpu_sppm import H, KW, NPH, SPP, W, _same

    pc = posed(scenes.cam_dof(), "lookat")
    with cg.Scene(scenes.scene_c2()) as sc, sc.sppm_session(W, H, SPP, pc, **KW) as g, sc.sppm_session(W, H, SPP, pc, **KW) as r:
        for k in range(2):
            g.add_passes(1, NPH)
            org, dirs, keys = sc.camera_rays(W, H, SPP, pc, SEED, sample_offset=k * SPP)
            r.add_pass_rays(org, dirs, NPH, keys=keys, pixel=None)
            assert _same(r.pixels(), g.pixels()), k
        assert _same(r.image(), g.image()) and np.array_equal(r.rgb8(), g.rgb8())
        assert (g.pixels()[:, 6] > 0).sum() > W * H // 2, "the view sees too little for the comparison to mean anything"


def test_example_lookat_grid(gpu_ready, tmp_path):
    """examples/lookat_grid.py at a small size writes a PNG whose pixels are the session's rgb8(), and its eye pass is posed."""
    import zlib
    out = str(tmp_path / "lookat_grid.png")
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import lookat_grid; "
            "e, i, r = lookat_grid.main(%r, W=64, H=36, spp=4, photons=2000); np.save(%r, r, allow_pickle=False); assert e.shape == (36, 64, 3) and e.max() > 0"
            % (os.path.join(ROOT, "examples"), out, str(tmp_path / "rgb8.npy")))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "POSE=1" in p.stdout, p.stdout
    rgb8 = np.load(str(tmp_path / "rgb8.npy"))
    png = open(out, "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(png):
        n, kind = int.from_bytes(png[pos:pos + 4], "big"), png[pos + 4:pos + 8]
        if kind == b"IHDR":
            size = (int.from_bytes(png[pos + 8:pos + 12], "big"), int.from_bytes(png[pos + 12:pos + 16], "big"))
        if kind == b"IDAT":
            idat += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    assert size == (64, 36)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(36, 1 + 64 * 3)
    assert (raw[:, 0] == 0).all()
    assert rgb8.shape == (36, 64, 3) and rgb8.max() > 0
    assert np.array_equal(raw[:, 1:].reshape(36, 64, 3), rgb8)
