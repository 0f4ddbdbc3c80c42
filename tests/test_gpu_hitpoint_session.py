"""GPU: photon mapping of caller-supplied Hitpoint records (cgrt_ppm_session_create_hitpoints).  A session on the records that
the wavefront trace returns at depth 5 is the ray session on the same rays bit for bit (and through the golden vectors the
compiled reference's); the order contract, the defaults, the per-record texels and the dropped records are checked against that
session; and eye depths past 5 and rays with more than 16 Hitpoints are checked end to end against a numpy replay of the
reference's photon loop over the oracle's photon hits, whose table is built with Python's own comparison of the paths' bit
strings."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from backends import BackendScene
from ppm_design import _bits, replay_expected
from test_gpu_ppm_rays import LOOKAT_PHOTONS, _ray_to_ps
from test_gpu_ppm_session import _canon, _feed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_golden  # noqa: E402

CASES = {c[0]: c for c in make_golden.photon_cases()}
ORDER_CASE = "c2_dof_32x24"
DEEP_W, DEEP_H, DEEP_EYE = 24, 18, 12  # test 8's rays and eye depth
DEEP_PHOTONS = LOOKAT_PHOTONS         # at least half of test 8's Hitpoints receive a photon (asserted there)
MANY_DEPTH = 24                       # test 9's eye depth


def _dev(sc):
    import torch
    return torch.device("cuda", sc.device)


def _t(sc, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(sc))


def _path_i32(path):
    """uint32 paths as the int32 tensor's bit pattern"""
    return np.ascontiguousarray(path, np.uint32).view(np.int32)


def _session(sc, hp9, ray, path, pixel, W, H, spp, nph, feed=True, **kw):
    """A hitpoint session on numpy records, fed nph photons in chunks; (image, rgb8, hitpoints, info)"""
    args = [_t(sc, hp9)] + [None if a is None else _t(sc, a) for a in (ray, None if path is None else _path_i32(path), pixel)]
    with sc.ppm_session_hitpoints(*args, width=W, rows=H, spp=spp, batch=3000, **kw) as ses:
        if feed:
            _feed(ses, nph)
        else:
            ses.add_photons(nph)
        return ses.image(), ses.rgb8(), ses.hitpoints(), ses.info()


_BASE = {}


def _base(name):
    """Per golden case, computed once: the depth-5 wavefront records of the camera rays (numpy), the hitpoint session on them
    and the ray session on the same rays."""
    if name in _BASE:
        return _BASE[name]
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = CASES[name]
    with cg.Scene(mk()) as sc:
        org, dirs, keys = sc.camera_rays(W, H, spp, cam(), 12345)
        wf = sc.wavefront(org, dirs, keys, max_depth=5, want=("hp",), hp_cap=16 * org.shape[0])
        assert wf["hp_count"] == wf["hp9"].shape[0]
        with sc.ppm_session_hitpoints(wf["hp9"], wf["hp_ray"], wf["hp_path"], width=W, rows=H, spp=spp, batch=3000) as ses:
            _feed(ses, nph)
            img, rgb8, hp, inf = ses.image(), ses.rgb8(), ses.hitpoints(), ses.info()
        with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=spp, batch=3000) as ses:
            _feed(ses, nph)
            rimg, rrgb8, rhp, rinf = ses.image(), ses.rgb8(), ses.hitpoints(), ses.info()
        rec = dict(hp9=wf["hp9"].cpu().numpy(), ray=wf["hp_ray"].cpu().numpy(), path=wf["hp_path"].cpu().numpy().view(np.uint32))
    _BASE[name] = dict(rec=rec, img=img, rgb8=rgb8, hp=hp, inf=inf, rimg=rimg, rrgb8=rrgb8, rhp=rhp, rinf=rinf)
    return _BASE[name]


# ---- 1. golden parity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_wavefront_records_session_matches_golden_and_ray_session(gpu_ready, name):
    _, mk, cam, W, H, spp, nph = CASES[name]
    g = np.load(os.path.join(GOLD, "ppm_%s.npz" % name))
    b = _base(name)
    assert np.array_equal(b["img"], g["image"]), "gathered image against the compiled reference"
    got = _canon(_ray_to_ps(b["hp"], W * H, spp), spp)
    assert got.shape == g["hp"].shape
    assert np.array_equal(got, g["hp"]), "hitpoints (geometry, flux, r2, n) against the compiled reference"
    assert b["hp"].shape == b["rhp"].shape and np.array_equal(b["hp"], b["rhp"]), "all 16 columns in table order"
    assert np.array_equal(b["rgb8"], b["rrgb8"]) and np.array_equal(b["img"], b["rimg"])
    assert b["inf"]["n_events"] == b["rinf"]["n_events"] and b["inf"]["hp_count"] == b["rinf"]["hp_count"] == len(b["hp"])
    assert b["inf"]["photons_done"] == nph and b["inf"]["ms_eye"] == 0


# ---- 2. input order ------------------------------------------------------------------------------------------------
def test_input_order_does_not_matter(gpu_ready):
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = CASES[ORDER_CASE]
    b = _base(ORDER_CASE)
    r = b["rec"]
    perm = np.random.default_rng(29).permutation(len(r["ray"]))
    with cg.Scene(mk()) as sc:
        img, rgb8, hp, inf = _session(sc, r["hp9"][perm], r["ray"][perm], r["path"][perm], None, W, H, spp, nph)
    assert np.array_equal(img, b["img"]) and np.array_equal(hp, b["hp"]) and np.array_equal(rgb8, b["rgb8"])
    assert inf["n_events"] == b["inf"]["n_events"]


# ---- 3. defaults -----------------------------------------------------------------------------------------------------
def test_defaults_ray_is_the_index_path_is_the_root(gpu_ready):
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = CASES[ORDER_CASE]
    g = np.load(os.path.join(GOLD, "ppm_%s.npz" % ORDER_CASE))
    b = _base(ORDER_CASE)
    r = b["rec"]
    npix = W * H
    with cg.Scene(mk()) as sc:
        img, _, hp, inf = _session(sc, r["hp9"], None, None, r["ray"] % npix, W, H, spp, nph)
    assert np.array_equal(img, g["image"])
    # the wavefront's records stand by ray, then emission order: record index = start of the ray's run + rank
    nrec = np.bincount(r["ray"], minlength=spp * npix)
    start = np.concatenate([[0], np.cumsum(nrec)[:-1]])
    assert np.array_equal(hp[:, 0], start[b["hp"][:, 0].astype(np.int64)] + b["hp"][:, 1]), "hp16[0] is the record index"
    assert np.array_equal(r["hp9"][hp[:, 0].astype(np.int64)], hp[:, 2:11])
    assert (hp[:, 1] == 0).all()
    assert np.array_equal(hp[:, 2:], b["hp"][:, 2:]), "same table order, same state"
    assert inf["hp_count"] == len(r["ray"])


# ---- 4. per-record texels --------------------------------------------------------------------------------------------
def test_per_record_texels(gpu_ready):
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = CASES[ORDER_CASE]
    g = np.load(os.path.join(GOLD, "ppm_%s.npz" % ORDER_CASE))
    r = _base(ORDER_CASE)["rec"]
    npix = W * H
    texel = r["ray"] % npix
    perm = np.random.default_rng(17).permutation(npix)
    with cg.Scene(mk()) as sc:
        img, _, _, inf = _session(sc, r["hp9"], r["ray"], r["path"], perm[texel], W, H, spp, nph)
        assert np.array_equal(img.reshape(-1, 3)[perm], g["image"].reshape(-1, 3))
        assert inf["hp_count"] == len(texel)
        drop = (texel % 3) == 0
        img, _, hp, inf = _session(sc, r["hp9"], r["ray"], r["path"], np.where(drop, -1, texel), W, H, spp, nph)
    flat, want = img.reshape(-1, 3), g["image"].reshape(-1, 3)
    gone = (np.arange(npix) % 3) == 0
    assert (flat[gone] == 0).all() and np.array_equal(flat[~gone], want[~gone])
    kept = int((~drop).sum())
    assert inf["hp_count"] == kept == len(hp) and 0 < kept < len(texel)
    assert ((hp[:, 0].astype(np.int64) % npix) % 3 != 0).all()


# ---- 5. dropped records ----------------------------------------------------------------------------------------------
def test_dropped_records_show_nowhere(gpu_ready):
    import cgraytracing_amd as cg
    import torch
    _, mk, cam, W, H, spp, nph = CASES[ORDER_CASE]
    b = _base(ORDER_CASE)
    r = b["rec"]
    npix = W * H
    n = len(r["ray"])
    k = 40  # copies per kind, taken from all over the records
    src = np.linspace(0, n - 1, k).astype(np.int64)
    hp9 = np.concatenate([r["hp9"]] + [r["hp9"][src]] * 6)
    ray = np.concatenate([r["ray"]] + [r["ray"][src]] * 6)
    path = np.concatenate([r["path"]] + [r["path"][src]] * 6)
    pixel = ray % npix
    at = lambda j: slice(n + j * k, n + (j + 1) * k)
    path[at(0)] = 0
    path[at(1)] = 1 << 31
    pixel[at(2)] = npix
    ray[at(3)] = -1
    hp9[n + 4 * k + np.arange(k), 3 + (np.arange(k) % 3)] = np.nan  # one coordinate of pos, each of the three in turn
    hp9[n + 5 * k + np.arange(k), 3 + (np.arange(k) % 3)] = np.where(np.arange(k) % 2, np.inf, -np.inf)
    shuffle = np.random.default_rng(31).permutation(len(ray))  # the bad records among the good ones
    with cg.Scene(mk()) as sc:
        img, rgb8, hp, inf = _session(sc, hp9[shuffle], ray[shuffle], path[shuffle], pixel[shuffle], W, H, spp, nph)
        assert inf["hp_count"] == b["inf"]["hp_count"] == n
        assert np.array_equal(img, b["img"]) and np.array_equal(hp, b["hp"]) and np.array_equal(rgb8, b["rgb8"])
        assert inf["n_events"] == b["inf"]["n_events"]
        # only dropped records: no Hitpoint, a zero image
        img, _, hp, inf = _session(sc, hp9[n:], ray[n:], path[n:], pixel[n:], W, H, spp, 100, feed=False)
        assert inf["hp_count"] == 0 and len(hp) == 0 and (img == 0).all()
        # no record at all
        with sc.ppm_session_hitpoints(torch.zeros((0, 9), dtype=torch.float64, device=_dev(sc)), width=W, rows=H) as ses:
            assert ses.info()["hp_count"] == 0
            ses.add_photons(1)
            assert (ses.image() == 0).all() and len(ses.hitpoints()) == 0


# ---- 6. values are used as given -------------------------------------------------------------------------------------
def test_values_are_used_as_given(gpu_ready):
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = CASES[ORDER_CASE]
    b = _base(ORDER_CASE)
    r = b["rec"]
    hp9 = r["hp9"].copy()
    hp9[:, 0:3] *= 0.5
    with cg.Scene(mk()) as sc:
        img, _, hp, _ = _session(sc, hp9, r["ray"], r["path"], None, W, H, spp, nph)
    # a power of two commutes with every operation of main.cpp:119-122,256
    assert np.array_equal(img, 0.5 * b["img"]) and b["img"].max() > 0
    assert np.array_equal(hp[:, 2:5], 0.5 * b["hp"][:, 2:5]) and np.array_equal(hp[:, 11:14], 0.5 * b["hp"][:, 11:14])
    assert np.array_equal(hp[:, 14:16], b["hp"][:, 14:16]) and np.array_equal(hp[:, 0:2], b["hp"][:, 0:2])
    assert np.array_equal(hp[:, 5:11], b["hp"][:, 5:11])


# ---- 7. mixed photon sources ---------------------------------------------------------------------------------------
def test_mixed_photon_sources(gpu_ready):
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = CASES[ORDER_CASE]
    b = _base(ORDER_CASE)
    r = b["rec"]
    half = nph // 2
    with cg.Scene(mk()) as sc:
        with sc.ppm_session_hitpoints(_t(sc, r["hp9"]), _t(sc, r["ray"]), _t(sc, _path_i32(r["path"])), width=W, rows=H, spp=spp,
                                      batch=3000) as ses:
            ses.add_photons(half)
            ses.add_photon_rays(*sc.emit_photons(half, nph - half))
            assert ses.photons_done == nph
            img, hp = ses.image(), ses.hitpoints()
    assert np.array_equal(img, b["img"]) and np.array_equal(hp, b["hp"])


# ---- the replay (main.cpp:103-125 and 252-258 over arbitrary records) is tests/ppm_design.py's replay_expected ----------------
_EVENTS = {}


def _c2_events(orc, nph):
    if nph not in _EVENTS:
        o = BackendScene(orc, scenes.scene_c2())
        _EVENTS[nph] = o.photon_events(0, nph, depth=5)
        o.close()
    return _EVENTS[nph]


_DEEP = {}


def _deep(orc):
    """Test 8's session, computed once: C2, a pinhole camera's 24x18 rays, the depth-12 wavefront's records, DEEP_PHOTONS photons
    at depth 5; and its replay."""
    if _DEEP:
        return _DEEP
    import cgraytracing_amd as cg
    W, H = DEEP_W, DEEP_H
    with cg.Scene(scenes.scene_c2()) as sc:
        org, dirs, keys = sc.camera_rays(W, H, 1, scenes.cam_pinhole(), 12345)
        n5 = sc.wavefront(org, dirs, keys, max_depth=5, want=())["hp_count"]
        wf = sc.wavefront(org, dirs, keys, max_depth=DEEP_EYE, want=("hp",), hp_cap=64 * W * H)
        assert wf["hp_count"] == wf["hp9"].shape[0]
        rec = dict(hp9=wf["hp9"].cpu().numpy(), ray=wf["hp_ray"].cpu().numpy(), path=wf["hp_path"].cpu().numpy().view(np.uint32))
        with sc.ppm_session_hitpoints(wf["hp9"], wf["hp_ray"], wf["hp_path"], width=W, rows=H, spp=1, max_depth=5, batch=30000) as ses:
            ses.add_photons(DEEP_PHOTONS)
            img, hp, inf = ses.image(), ses.hitpoints(), ses.info()
    table, image, _ = replay_expected(rec["ray"], rec["path"], rec["hp9"], rec["ray"] % (W * H), _c2_events(orc, DEEP_PHOTONS), W * H, 1,
                                      DEEP_PHOTONS)
    _DEEP.update(rec=rec, n5=n5, img=img, hp=hp, inf=inf, table=table, image=image)
    return _DEEP


# ---- 8. deeper than 5 ------------------------------------------------------------------------------------------------
def test_eye_depth_12_against_replay(gpu_ready, orc):
    d = _deep(orc)
    table, image = d["table"], d["image"]
    # the records and the replay alone say that the case is not vacuous
    assert len(table) > d["n5"] > 0, "depth 12 yields no more Hitpoints than depth 5"
    assert (table[:, 15] > 0).sum() >= 0.5 * len(table), "fewer than half of the Hitpoints received a photon"
    print(len(table), "Hitpoints at depth 12,", d["n5"], "at depth 5,", int((table[:, 15] > 0).sum()), "with photons,",
          int(table[:, 1].max()) + 1, "at most on one ray")
    hp = d["hp"]
    assert hp.shape == table.shape and d["inf"]["hp_count"] == len(table)
    assert np.array_equal(hp[:, :2], table[:, :2]), "ray / rank in table order"
    assert np.array_equal(hp[:, 2:11], table[:, 2:11]), "value, pos, normal"
    assert np.array_equal(hp[:, 11:16], table[:, 11:16]), "flux, r2, n"
    assert np.array_equal(d["img"].reshape(-1, 3), image)


# ---- 9. more than 16 Hitpoints on one ray ----------------------------------------------------------------------------
def test_more_than_16_hitpoints_on_one_ray(gpu_ready, orc):
    """Eye depth used: MANY_DEPTH = 24 (C2's glass sphere; a chain inside the sphere adds about one Hitpoint per level)."""
    import cgraytracing_amd as cg
    W, H = 8, 6  # the texels the rays gather into: ray i into texel i % 48
    cam = scenes.cam_pinhole()
    with cg.Scene(scenes.scene_c2()) as sc:
        org, dirs, keys = sc.camera_rays(64, 48, 1, cam, 12345)
        o, dn = org.cpu().numpy(), dirs.cpu().numpy()
        # the rays whose line passes within 0.8 radii of the glass sphere's centre (main.cpp:290: centre (-8, -13, 25), radius 7)
        oc = np.array([-8.0, -13.0, 25.0]) - o
        along = (oc * dn).sum(axis=1)
        dist2 = (oc * oc).sum(axis=1) - along * along
        through = np.nonzero((along > 0) & (dist2 < (0.8 * 7.0) ** 2))[0]
        assert len(through) >= 36
        pick = _t(sc, through[np.linspace(0, len(through) - 1, 36).astype(np.int64)])
        org, dirs, keys = org[pick].contiguous(), dirs[pick].contiguous(), keys[pick].contiguous()
        wf = sc.wavefront(org, dirs, keys, max_depth=MANY_DEPTH, min_adj=0.0, want=("hp", "nhit"), hp_cap=36 * 256)
        assert wf["hp_count"] == wf["hp9"].shape[0]
        nhit = wf["nhit"].cpu().numpy().view(np.uint32).astype(np.int64)
        assert nhit.max() > 16, "no ray with more than 16 Hitpoints at depth %d: %r" % (MANY_DEPTH, nhit)
        rec = dict(hp9=wf["hp9"].cpu().numpy(), ray=wf["hp_ray"].cpu().numpy(), path=wf["hp_path"].cpu().numpy().view(np.uint32))
        # records in a shuffled order: the rank comes from the paths, not from the input
        sh = np.random.default_rng(37).permutation(len(rec["ray"]))
        with sc.ppm_session_hitpoints(_t(sc, rec["hp9"][sh]), _t(sc, rec["ray"][sh]), _t(sc, _path_i32(rec["path"][sh])), width=W, rows=H,
                                      spp=1, max_depth=5, batch=30000) as ses:
            ses.add_photons(DEEP_PHOTONS)
            img, hp = ses.image(), ses.hitpoints()
    print("depth", MANY_DEPTH, "nhit", nhit.tolist())
    big = int(np.argmax(nhit))
    mine = hp[hp[:, 0] == big]
    assert len(mine) == nhit[big] and sorted(mine[:, 1].tolist()) == list(range(nhit[big]))
    # the ray's records in the wavefront's own (emission) order carry the ranks 0 .. nhit-1
    for k, i in enumerate(np.nonzero(rec["ray"] == big)[0]):
        row = mine[mine[:, 1] == k]
        assert len(row) == 1 and np.array_equal(row[0, 2:11], rec["hp9"][i])
    assert [_bits(p) for p in rec["path"][rec["ray"] == big]] == sorted(_bits(p) for p in rec["path"][rec["ray"] == big])
    table, image, _ = replay_expected(rec["ray"][sh], rec["path"][sh], rec["hp9"][sh], rec["ray"][sh] % (W * H),
                                      _c2_events(orc, DEEP_PHOTONS), W * H, 1, DEEP_PHOTONS)
    assert hp.shape == table.shape and np.array_equal(hp, table)
    assert np.array_equal(img.reshape(-1, 3), image) and (table[:, 15] > 0).any()


# ---- 10. ppm_session_wavefront and the example -------------------------------------------------------------------------
def test_ppm_session_wavefront(gpu_ready, orc):
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, nph = CASES[ORDER_CASE]
    b = _base(ORDER_CASE)
    npix = W * H
    with cg.Scene(mk()) as sc:
        org, dirs, keys = sc.camera_rays(W, H, spp, cam(), 12345)
        ses, wf = sc.ppm_session_wavefront(org, dirs, keys, width=W, rows=H, spp=spp, eye_depth=5, batch=3000)
        with ses:
            _feed(ses, nph)
            assert np.array_equal(ses.image(), b["rimg"]) and np.array_equal(ses.hitpoints(), b["rhp"])
            assert np.array_equal(ses.rgb8(), b["rrgb8"]) and ses.info()["n_events"] == b["rinf"]["n_events"]
        assert wf["hp_count"] == len(b["rhp"]) == wf["hp9"].shape[0]
        # a per-ray pixel map reaches the records
        perm = np.random.default_rng(17).permutation(npix)
        ses, _ = sc.ppm_session_wavefront(org, dirs, keys, width=W, rows=H, spp=spp, eye_depth=5, batch=3000, nphotons=nph,
                                          pixel=_t(sc, perm[np.tile(np.arange(npix), spp)]))
        with ses:
            assert np.array_equal(ses.image().reshape(-1, 3)[perm], b["rimg"].reshape(-1, 3))
    d = _deep(orc)
    with cg.Scene(scenes.scene_c2()) as sc:
        org, dirs, keys = sc.camera_rays(DEEP_W, DEEP_H, 1, scenes.cam_pinhole(), 12345)
        ses, wf = sc.ppm_session_wavefront(org, dirs, keys, width=DEEP_W, rows=DEEP_H, eye_depth=DEEP_EYE, batch=30000,
                                           nphotons=DEEP_PHOTONS)
        with ses:
            assert np.array_equal(ses.image(), d["img"]) and np.array_equal(ses.hitpoints(), d["hp"])
        assert wf["levels"] > 5


def test_example_deep_glass_ppm(gpu_ready, tmp_path):
    """examples/deep_glass_ppm.py at a tiny size: three PNGs, the depth-5 image equal to the ray session's, more Hitpoints at 12."""
    prefix = str(tmp_path / "dgp")
    code = ("import sys, json; sys.path.insert(0, %r); import deep_glass_ppm; "
            "print('INFO ' + json.dumps(deep_glass_ppm.main(%r, W=48, H=27, spp=1, photons=3000, check=True)))"
            % (os.path.join(ROOT, "examples"), prefix))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    import json
    info = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("INFO ")][0][5:])
    assert info["5"]["equals_ray_session"] is True and info["12"]["hitpoints"] > info["5"]["hitpoints"] > 0
    for tag in ("depth5", "depth12", "diff"):
        png = open("%s_%s.png" % (prefix, tag), "rb").read()
        assert png[:8] == b"\x89PNG\r\n\x1a\n" and int.from_bytes(png[16:20], "big") == 48 and int.from_bytes(png[20:24], "big") == 27
