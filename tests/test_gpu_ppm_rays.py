"""GPU: photon mapping of caller-supplied rays (cgrt_ppm_session_create_rays, cgrt_trace_rays_hitpoints).  A session on the
camera's own rays is the grid session bit for bit (and through it the compiled reference's golden vectors); the pixel map, the
order contract and the capture kernel are checked against trace_rays, which test_gpu_rays.py pins to the oracle per ray; and a
look-at camera's session is checked end to end against a numpy replay of the reference's photon loop over the oracle's hits."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from backends import BackendScene
from test_gpu_ppm_session import CHUNKS, _canon, _feed
from test_gpu_rays import RANDOM_SCENES, _bezier_scene, oracle_depth1, oracle_nearest, random_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_golden  # noqa: E402

PI_REF = 3.14159265358979  # main.cpp:26
EPS = 1e-4


def _ray_to_ps(hp, npix, spp):
    """hp16[0] of a ray session on camera rays (ray = sample * npix + texel) as a grid session's pixel * spp + sample"""
    out = hp.copy()
    ray = hp[:, 0].astype(np.int64)
    out[:, 0] = (ray % npix) * spp + ray // npix
    return out


def _dev(sc):
    import torch
    return torch.device("cuda", sc.device)


@pytest.mark.parametrize("case", make_golden.photon_cases(), ids=[c[0] for c in make_golden.photon_cases()])
def test_camera_ray_session_matches_reference_golden_and_grid_session(gpu_ready, orc, case):
    import cgraytracing_amd as cg
    name, mk, cam, W, H, spp, nph = case
    g = np.load(os.path.join(GOLD, "ppm_%s.npz" % name))
    with cg.Scene(mk()) as sc:
        org, dirs, keys = sc.camera_rays(W, H, spp, cam(), 12345)
        with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=spp, batch=3000) as ses:
            _feed(ses, nph)
            img, rgb8, hp, inf = ses.image(), ses.rgb8(), ses.hitpoints(), ses.info()
        with sc.ppm_session(W, H, spp, cam(), 5, 12345, batch=3000) as ses:
            _feed(ses, nph)
            gimg, grgb8, ghp, ginf = ses.image(), ses.rgb8(), ses.hitpoints(), ses.info()
    hp = _ray_to_ps(hp, W * H, spp)
    got = _canon(hp, spp)
    assert got.shape == g["hp"].shape
    assert np.array_equal(got, g["hp"]), "hitpoints (geometry, flux, r2, n)"
    assert np.array_equal(img, g["image"]), "gathered image"
    assert np.array_equal(img, gimg) and np.array_equal(rgb8, grgb8)
    assert np.array_equal(hp, ghp), "table order"
    assert inf["n_events"] == ginf["n_events"] and inf["hp_count"] == ginf["hp_count"] == len(hp)
    assert inf["photons_done"] == nph


def test_pixel_map(gpu_ready):
    import cgraytracing_amd as cg
    import torch
    name, mk, cam, W, H, spp, nph = next(c for c in make_golden.photon_cases() if c[0] == "c2_dof_32x24")
    g = np.load(os.path.join(GOLD, "ppm_%s.npz" % name))
    npix = W * H
    rng = np.random.default_rng(17)
    perm = rng.permutation(npix)
    with cg.Scene(mk()) as sc:
        dev = _dev(sc)
        org, dirs, keys = sc.camera_rays(W, H, spp, cam(), 12345)
        texel = np.tile(np.arange(npix), spp)  # of ray i

        def run(o, d, k, pixel):
            with sc.ppm_session_rays(o, d, k, width=W, rows=H, spp=spp, pixel=torch.from_numpy(pixel).to(dev), batch=3000) as ses:
                _feed(ses, nph)
                return ses.image(), ses.info()["hp_count"]

        # texel p's rays gather into perm[p]
        img, _ = run(org, dirs, keys, perm[texel])
        assert np.array_equal(img.reshape(-1, 3)[perm], g["image"].reshape(-1, 3))
        # the ray array reordered: texels shuffled, each texel's rays in their relative (sample) order
        order = np.concatenate([np.arange(spp) * npix + p for p in rng.permutation(npix)])
        t_order = torch.from_numpy(order).to(dev)
        img, _ = run(org[t_order].contiguous(), dirs[t_order].contiguous(), keys[t_order].contiguous(), texel[order])
        assert np.array_equal(img, g["image"])
        # every third texel's rays belong to no texel
        drop = (texel % 3) == 0
        pixel = np.where(drop, -1, texel)
        img, count = run(org, dirs, keys, pixel)
        nhit = sc.trace_rays(org, dirs, keys, want=("nhit",))["nhit"].cpu().numpy()
        flat, want = img.reshape(-1, 3), g["image"].reshape(-1, 3)
        gone = (np.arange(npix) % 3) == 0
        assert (flat[gone] == 0).all() and np.array_equal(flat[~gone], want[~gone])
        assert count == int(nhit[~drop].sum()) and 0 < count < int(nhit.sum())


def _check_capture(sc, org, dirs, keys, depth, tag):
    """trace_rays_hitpoints against trace_rays on the same rays; returns the number of Hitpoints"""
    full = {k: v.cpu().numpy() for k, v in sc.trace_rays(org, dirs, keys, max_depth=depth).items()}
    cap = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=depth)
    n = org.shape[0]
    nhit = full["nhit"].view(np.uint32).astype(np.int64)
    assert cap["count"] == len(cap["hp"]) == int(nhit.sum()), tag
    assert np.array_equal(np.bincount(cap["ray"], minlength=n), nhit), tag
    order = np.lexsort([cap["seq"], cap["ray"]])
    ray, seq, hp = cap["ray"][order], cap["seq"][order], cap["hp"][order]
    start = np.concatenate([[0], np.cumsum(nhit)[:-1]])
    assert np.array_equal(seq, np.arange(len(ray)) - start[ray]), tag  # emission positions 0 .. nhit-1 of every ray
    acc = np.zeros((n, 3))
    for k in range(int(nhit.max()) if len(nhit) else 0):  # fp64 sums in emission order
        sel = seq == k
        acc[ray[sel]] += hp[sel, 0:3]
    assert np.array_equal(acc, full["acc"]), tag
    nrm = hp[:, 6:9].astype(np.longdouble)
    assert float(np.abs(np.sqrt((nrm * nrm).sum(axis=1)) - 1).max(initial=0.0)) <= 1e-12, tag
    o, d = org.cpu().numpy(), dirs.cpu().numpy()
    own = (seq == 0) & (nhit[ray] == 1) & (full["hit_obj"][ray] >= 0)
    diffuse = np.array([ob.reflection < EPS and ob.transparency < EPS for ob in sc_objs(sc)])
    own &= diffuse[np.maximum(full["hit_obj"][ray], 0)]
    assert own.any(), tag
    r = ray[own]
    assert np.array_equal(hp[own, 3:6], o[r] + d[r] * full["hit_t"][r][:, None]), tag
    # every pos lies on its ray's tree: a first Hitpoint of a ray whose own hit is not diffuse lies behind that hit
    return int(nhit.sum())


_OBJS = {}


def sc_objs(sc):
    return _OBJS[id(sc)]


@pytest.mark.parametrize("name,mk,walls", RANDOM_SCENES, ids=[c[0] for c in RANDOM_SCENES])
def test_capture_equals_ray_kernel_random_rays(gpu_ready, name, mk, walls):
    import cgraytracing_amd as cg
    import torch
    objs = mk()
    org, dirs, _ = random_rays(walls, 2024)
    with cg.Scene(objs) as sc:
        _OBJS[id(sc)] = objs
        dev = _dev(sc)
        to, td = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
        total = _check_capture(sc, to, td, None, 5, name)
        small = sc.trace_rays_hitpoints(to, td, None, max_depth=5, cap=100)
        assert small["count"] == total and len(small["hp"]) == 100
        print(name, sc.capture_variant(5), total, "Hitpoints")


@pytest.mark.parametrize("glass", [False, True], ids=["mirror_vase", "glass_vase"])
def test_capture_equals_ray_kernel_bezier(gpu_ready, glass):
    import cgraytracing_amd as cg
    objs = _bezier_scene(glass)
    with cg.Scene(objs) as sc:
        _OBJS[id(sc)] = objs
        org, dirs, keys = sc.camera_rays(64, 64, 2, scenes.cam_dof(), 7)
        _check_capture(sc, org, dirs, keys, 5, glass)
        assert "BEZ=1,GLASS=%d" % glass in sc.capture_variant(5) and "NT=64" in sc.capture_variant(5)


# ---- a look-at camera against the oracle, end to end --------------------------------------------------------------
LOOKAT = dict(eye=(14.0, 6.0, -8.0), target=(0.0, -5.0, 25.0), W=80, H=60, fov_deg=70.0)
LOOKAT_PHOTONS = 100000
LOOKAT_SCENES = [("c1", scenes.scene_c1), ("stone_bump_floor", lambda: scenes.planes(scenes.stone_small_texture(True)))]


def lookat_rays_np(eye, target, W, H, fov_deg):
    """One ray through the centre of every texel of a pinhole camera at eye looking at target (up = +y); row 0 = bottom."""
    eye, target, up = np.array(eye), np.array(target), np.array([0.0, 1.0, 0.0])
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    upv = np.cross(fwd, right)
    t = math.tan(math.radians(fov_deg) / 2)
    x = ((np.arange(W) + 0.5) / W * 2 - 1)[None, :, None]
    y = ((np.arange(H) + 0.5) / H * 2 - 1)[:, None, None]
    d = fwd + x * (t * right) + y * (t * H / W * upv)
    d = (d / np.sqrt((d * d).sum(axis=2))[:, :, None]).reshape(-1, 3)
    return np.ascontiguousarray(np.tile(eye, (W * H, 1))), np.ascontiguousarray(d)


def _ref_hash(ix, iy, iz, hashsize):  # hash.h:35-37, wrapping 32-bit products
    m = 0xFFFFFFFF
    return ((((ix & m) * 73856093) & m) ^ (((iy & m) * 19349663) & m) ^ (((iz & m) * 83492791) & m)) % hashsize


def _ref_coord(p, cl):  # hash.h:38-42
    return (int(math.floor((p[0] - (-35.0)) / cl)), int(math.floor((p[1] - (-35.0)) / cl)), int(math.floor((p[2] - (-15.0)) / cl)))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def lookat_expected(orc, objs, org, dirs, nphotons, hashsize=1000001, alpha=0.7):
    """From the oracle alone: the depth-1 Hitpoints of the rays (main.cpp:52-100), the table in the order contract (bucket,
    texel = ray), the replay of main.cpp:103-125 over the oracle's photon events in photon order, and the gathered image of
    main.cpp:252-258 (one ray per texel).  Returns (table [n,16] as hitpoints(), image [npix,3])."""
    o, obj, t, nrm = oracle_nearest(orc, objs, org, dirs)
    acc, nhit = oracle_depth1(o, objs, org, dirs, obj, t)
    events = o.photon_events(0, nphotons, depth=1)
    o.close()
    rays = np.nonzero(nhit)[0]
    P = org + dirs * t[:, None]
    flip = (nrm[:, 0] * dirs[:, 0] + nrm[:, 1] * dirs[:, 1] + nrm[:, 2] * dirs[:, 2]) > 0  # main.cpp:73-76
    n = np.where(flip[:, None], -nrm, nrm)
    r0 = 200.0 / 768
    cl = 70.0 / math.ceil(70.0 / r0)  # hash.h:25-26
    bucket = np.array([_ref_hash(*_ref_coord(P[i], cl), hashsize) for i in rays], np.int64)
    order = np.lexsort([rays, bucket])  # (bucket, texel); one ray per texel, one Hitpoint per ray
    rays, bucket = rays[order], bucket[order]
    hps = [dict(f=[float(v) for v in acc[i]], pos=[float(v) for v in P[i]], n=[float(v) for v in n[i]], flux=[0.0, 0.0, 0.0],
                r2=r0 * r0, cnt=0) for i in rays]
    buckets = {}
    for k, b in enumerate(bucket):
        buckets.setdefault(int(b), []).append(hps[k])
    for ev in events:
        Pe, ne, fe = [float(v) for v in ev[1:4]], [float(v) for v in ev[4:7]], [float(v) for v in ev[7:10]]
        ix, iy, iz = _ref_coord(Pe, cl)
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    for h in buckets.get(_ref_hash(ix - 1 + dx, iy - 1 + dy, iz - 1 + dz, hashsize), ()):
                        dd = [h["pos"][0] - Pe[0], h["pos"][1] - Pe[1], h["pos"][2] - Pe[2]]
                        if _dot(h["n"], ne) > EPS and _dot(dd, dd) <= h["r2"]:  # main.cpp:116
                            g = (h["cnt"] * alpha + alpha) / (h["cnt"] * alpha + 1.0)  # main.cpp:119
                            h["r2"] *= g
                            h["cnt"] += 1
                            h["flux"] = [(h["flux"][c] + (h["f"][c] * fe[c]) * (1.0 / PI_REF)) * g for c in range(3)]  # main.cpp:122
    table = np.zeros((len(hps), 16))
    image = np.zeros((len(org), 3))
    norm = float(nphotons) * 1
    for k, h in enumerate(hps):
        table[k] = [rays[k], 0] + h["f"] + h["pos"] + h["n"] + h["flux"] + [h["r2"], h["cnt"]]
        s = 1.0 / (PI_REF * h["r2"] * norm)  # main.cpp:256
        image[rays[k]] = [0.0 + h["flux"][c] * s for c in range(3)]
    return table, image


@pytest.mark.parametrize("name,mk", LOOKAT_SCENES, ids=[c[0] for c in LOOKAT_SCENES])
def test_lookat_camera_session_against_oracle_replay(gpu_ready, orc, name, mk):
    import cgraytracing_amd as cg
    import torch
    objs = mk()
    W, H = LOOKAT["W"], LOOKAT["H"]
    org, dirs = lookat_rays_np(**LOOKAT)
    table, image = lookat_expected(orc, objs, org, dirs, LOOKAT_PHOTONS)
    # the oracle's numbers alone say that the case is not vacuous
    assert len(table) >= 0.6 * W * H, "fewer than 60 % of the texels have a Hitpoint"
    assert (table[:, 15] > 0).sum() >= 0.5 * len(table), "fewer than half of the Hitpoints received a photon"
    with cg.Scene(objs) as sc:
        dev = _dev(sc)
        with sc.ppm_session_rays(torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev), width=W, rows=H, spp=1,
                                 max_depth=1, batch=30000) as ses:
            ses.add_photons(LOOKAT_PHOTONS)
            hp, img = ses.hitpoints(), ses.image()
    print(name, len(table), "Hitpoints,", int((table[:, 15] > 0).sum()), "with photons")
    assert hp.shape == table.shape
    assert np.array_equal(hp[:, :2], table[:, :2]), "ray index / emission index in table order"
    assert np.array_equal(hp[:, 2:11], table[:, 2:11]), "f, pos, normal"
    assert np.array_equal(hp[:, 11:16], table[:, 11:16]), "flux, r2, n"
    assert np.array_equal(img.reshape(-1, 3), image)


def test_schedule_independence(gpu_ready):
    import cgraytracing_amd as cg
    import torch
    name, mk, cam, W, H, spp, nph = next(c for c in make_golden.photon_cases() if c[0] == "c2_dof_32x24")
    npix = W * H
    with cg.Scene(mk()) as sc:
        dev = _dev(sc)
        org, dirs, keys = sc.camera_rays(W, H, spp, cam(), 12345)
        runs = []
        for _ in range(2):
            with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=spp, nphotons=nph) as ses:
                runs.append((ses.hitpoints(), ses.image()))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        texel = np.tile(np.arange(npix), spp)
        total = np.zeros_like(runs[0][1])
        for third in range(3):
            pixel = np.where(texel % 3 == third, texel, -1)
            with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=spp, pixel=torch.from_numpy(pixel).to(dev),
                                     nphotons=nph) as ses:
                part = ses.image()
            mine = (np.arange(npix) % 3 == third).reshape(H, W)
            assert (part[~mine] == 0).all()
            total[mine] = part[mine]
        assert np.array_equal(total, runs[0][1])


def test_edge_cases(gpu_ready, orc):
    import cgraytracing_amd as cg
    import torch
    from cgraytracing_amd._capi import CgrtError
    W, H = 16, 12
    with cg.Scene(scenes.scene_c2()) as sc:
        dev = _dev(sc)
        none = torch.zeros((0, 3), dtype=torch.float64, device=dev)
        with sc.ppm_session_rays(none, none, width=W, rows=H) as ses:  # no rays
            assert ses.info()["hp_count"] == 0
            ses.add_photons(1)
            assert (ses.image() == 0).all()
        cap = sc.trace_rays_hitpoints(none, none)
        assert cap["count"] == 0 and len(cap["hp"]) == 0
        # every ray misses: from behind the camera within 2 degrees of -z (test_gpu_rays.random_rays' group built to miss)
        o, d, miss = random_rays("spheres", 2024)
        o, d = torch.from_numpy(o[miss][:W * H].copy()).to(dev), torch.from_numpy(d[miss][:W * H].copy()).to(dev)
        with sc.ppm_session_rays(o, d, width=W, rows=H, nphotons=100) as ses:
            assert ses.info()["hp_count"] == 0 and (ses.image() == 0).all()
        org, dirs, keys = sc.camera_rays(W, H, 1, scenes.cam_pinhole(), 12345)
        with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H) as ses:
            with pytest.raises(CgrtError) as e:  # no photon yet
                ses.image()
            assert e.value.code == -1
            ses.add_photons(5000)
            img = ses.image()
            assert img.max() > 0 and np.array_equal(ses.rgb8(), orc.tonemap(img))


# (label, scene, max_depth): between them every instantiation of capture_rays_kernel
CAPTURE_LAUNCHES = [
    ("bezier_mirror", lambda: _bezier_scene(False), 5), ("bezier_glass", lambda: _bezier_scene(True), 5),
    ("dragon_depth1", scenes.scene_dragon, 1), ("c3_glass_bunny", lambda: scenes.scene_c3(True), 5),
    ("c2_depth1", scenes.scene_c2, 1), ("c2", scenes.scene_c2, 5),
    ("planes_sphere_depth1", lambda: scenes.planes() + [scenes.Sphere((5, -12, 30), 5, (1, 1, 1), 0.8, 0.5)], 1),
    ("planes_glass_sphere", lambda: scenes.planes() + [scenes.Sphere((5, -12, 30), 5, (1, 1, 1), 0.8, 0.5)], 5),
    ("spheres_1000_depth1", lambda: scenes.many_spheres(1000, 11), 1), ("spheres_1000", lambda: scenes.many_spheres(1000, 11), 5),
    ("room_800", lambda: scenes.room_with_objects(800, 5), 5),
]


def _capture_table():
    """The flag tuples (TREES, BEZ, GLASS, SPH, SPILL, NT) of the capture kernels: one per full-trace entry of CGRT_RAY_VARIANTS
    without STATS, read from cgrt_variants.h itself."""
    import variants
    out = variants.capture_variants()
    assert len(out) >= 11
    return set(out)


def test_every_capture_instantiation_is_launched(gpu_ready):
    """Every instantiation of capture_rays_kernel is launched on a small set of camera rays and produces trace_rays' Hitpoint count
    and sums; nothing outside the table is asked for.  room_800 (more objects than LDS holds, the SPILL capture of the general
    body) also runs as a session against the grid session."""
    import cgraytracing_amd as cg
    seen = {}
    for label, mk, depth in CAPTURE_LAUNCHES:
        objs = mk()
        with cg.Scene(objs) as sc:
            org, dirs, keys = sc.camera_rays(16, 8, 1, scenes.cam_dof(), 3)
            full = sc.trace_rays(org, dirs, keys, max_depth=depth)
            cap = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=depth)
            nhit = full["nhit"].cpu().numpy().view(np.uint32).astype(np.int64)
            assert cap["count"] == int(nhit.sum()) and np.array_equal(np.bincount(cap["ray"], minlength=128), nhit), label
            order = np.lexsort([cap["seq"], cap["ray"]])
            acc = np.zeros((128, 3))
            for r, f in zip(cap["ray"][order], cap["hp"][order, 0:3]):
                acc[r] += f
            assert np.array_equal(acc, full["acc"].cpu().numpy()), label
            v = sc.capture_variant(depth)
            assert v.startswith("capture_rays_kernel<")
            seen.setdefault(tuple(int(p.split("=")[1]) for p in v[v.index("<") + 1:-1].split(",")), label)
            if label == "room_800":
                W, H, nph = 24, 16, 3000
                cam = scenes.cam_pinhole()
                org, dirs, keys = sc.camera_rays(W, H, 1, cam, 12345)
                with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, nphotons=nph) as ses:
                    img, hp = ses.image(), ses.hitpoints()
                with sc.ppm_session(W, H, 1, cam, 5, 12345, nphotons=nph) as ses:
                    gimg, ghp = ses.image(), ses.hitpoints()
                assert "SPILL=1" in v and len(hp) > 0
                assert np.array_equal(img, gimg) and np.array_equal(_ray_to_ps(hp, W * H, 1), ghp)
    table = _capture_table()
    print("\n".join("%s  <- %s" % (v, seen.get(v)) for v in sorted(table)))
    assert set(seen) == table, dict(never_launched=sorted(table - set(seen)), not_in_table=sorted(set(seen) - table))


def test_example_lookat_ppm(gpu_ready, tmp_path):
    """examples/lookat_ppm.py writes a PNG whose pixels are the session's rgb8()."""
    import zlib
    out = str(tmp_path / "lookat_ppm.png")
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import lookat_ppm; "
            "np.save(%r, lookat_ppm.main(%r, W=64, H=36, spp=1, steps=2, photons_per_step=2000), allow_pickle=False)"
            % (os.path.join(ROOT, "examples"), str(tmp_path / "rgb8.npy"), out))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
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
    assert (raw[:, 0] == 0).all()  # filter type None on every scanline
    assert rgb8.shape == (36, 64, 3) and rgb8.max() > 0
    assert np.array_equal(raw[:, 1:].reshape(36, 64, 3), rgb8)
