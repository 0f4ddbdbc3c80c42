"""GPU: caller-supplied photons (cgrt_ppm_session_add_photon_rays, cgrt_photon_emit, cgrt_photon_ray_events).

1. The built-in emitter's photons, made by emit_photons and fed through add_photon_rays, give the session that add_photons gives,
   bit for bit -- and through it the compiled reference's golden vectors -- on every photon_trace_kernel<BEZ, SPILL, RAYS = 1>.
2. The events of caller-made photons against photon_events (emitted photons) and against the oracle's nearest hits (a spot light).
3. A spot light end to end against a numpy replay of main.cpp:103-125 over events derived from the oracle alone.
4. The contract: flux scales linearly, dead photons count and change nothing else, the default stream, n = 0, argument checks.
5. examples/spot_light_ppm.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from test_gpu_object_counts import KLDS, _scene as _many_objects
from test_gpu_ppm_rays import EPS, LOOKAT, LOOKAT_SCENES, PI_REF, _dot, _ref_coord, _ref_hash, lookat_rays_np
from test_gpu_ppm_session import CHUNKS
from test_gpu_rays import oracle_depth1, oracle_nearest
from test_photon_rays_host import _photon_keys

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_golden  # noqa: E402

PHOTON_SEED = 777
BATCH = 3000  # several batches per call, so the overlap path (batch k+1 traced under batch k's replay) runs


def _dev(sc):
    import torch
    return torch.device("cuda", sc.device)


def _t(sc, a):
    """numpy -> tensor on the scene's device; uint64 / uint32 as the int64 / int32 bit patterns the API takes"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(_dev(sc))


def _feed_rays(ses, tensors, first, total, chunks=CHUNKS):
    """tensors = the photons [first, total) as (org, dirs, flux, keys, draws); fed in the chunk pattern, then the rest"""
    off = 0
    sizes = [c for c in chunks]
    for c in sizes + [None]:
        n = total - first - off if c is None or off + c > total - first else c
        if n <= 0:
            break
        ses.add_photon_rays(*[None if t is None else t[off:off + n] for t in tensors])
        off += n
    assert off == total - first and ses.photons_done == total


def _state(ses):
    inf = ses.info()
    return dict(image=ses.image(), rgb8=ses.rgb8(), hp=ses.hitpoints(), n_events=inf["n_events"], n_pairs=inf["n_pairs"],
                photons_done=inf["photons_done"])


def _same(a, b, tag, pairs=True):
    for k in ("image", "rgb8", "hp"):
        assert np.array_equal(a[k], b[k]), (tag, k)
    for k in ("n_events", "photons_done") + (("n_pairs",) if pairs else ()):
        assert a[k] == b[k], (tag, k, a[k], b[k])


# ---- 1. the built-in emitter through the new door ----------------------------------------------------------------------
def _big(kind, nph):
    """more objects than the LDS list holds (the SPILL instantiations): the room and spheres, without / with the Bezier vase"""
    return ("room_%s_%d" % (kind, KLDS + 1), lambda: _many_objects(kind, KLDS + 1), scenes.cam_pinhole, 24, 16, 1, nph)


OLD_DOOR_CASES = ([c + (True,) for c in make_golden.photon_cases() + make_golden.photon_cases_bezier()] +
                  [_big("A", 7001) + (False,), _big("E", 3501) + (False,)])


@pytest.mark.parametrize("case", OLD_DOOR_CASES, ids=[c[0] for c in OLD_DOOR_CASES])
def test_emitted_photons_through_add_photon_rays_equal_add_photons(gpu_ready, case):
    import cgraytracing_amd as cg
    name, mk, cam, W, H, spp, nph, golden = case
    kw = dict(camera=cam(), max_depth=5, seed=12345, photon_seed=PHOTON_SEED, batch=BATCH)
    with cg.Scene(mk()) as sc:
        st = sc.stats()
        if not golden:
            assert st["n_objects"] > KLDS and (st["n_beziers"] > 0) == ("_E_" in name)  # SPILL, and BEZ where the vase is
        with sc.ppm_session(W, H, spp, **kw) as ses:
            ses.add_photons(nph)
            a = _state(ses)
        em = sc.emit_photons(0, nph, PHOTON_SEED)
        host = cg.emit_photons_host(0, nph, PHOTON_SEED)
        for name_, d, h in zip(("org", "dirs", "flux", "keys", "draws"), em, host):
            assert np.array_equal(d.cpu().numpy().view(h.dtype), h), ("emit_photons on the device vs host", name_)
        with sc.ppm_session(W, H, spp, **kw) as ses:
            _feed_rays(ses, em, 0, nph)
            b = _state(ses)
        with sc.ppm_session(W, H, spp, **kw) as ses:  # the old door in the same calls as b: the same batches
            for c_ in CHUNKS:
                if ses.photons_done + c_ < nph:
                    ses.add_photons(c_)
            ses.add_photons(nph - ses.photons_done)
            a_chunked = _state(ses)
        k = 4000 if nph > 4000 else 1000  # add_photons leaves a batch traced ahead, which the ray call drops
        with sc.ppm_session(W, H, spp, **kw) as ses:
            ses.add_photons(k)
            ses.add_photon_rays(*[t[k:] for t in em])
            c = _state(ses)
        with sc.ppm_session(W, H, spp, **kw) as ses:  # and the other way round
            ses.add_photon_rays(*[t[:k] for t in em])
            ses.add_photons(nph - k)
            d = _state(ses)
        with sc.ppm_session(W, H, spp, **kw) as ses:  # the old door in the calls of c and d
            ses.add_photons(k)
            ses.add_photons(nph - k)
            a_two = _state(ses)
    assert a["n_events"] > 0 and a["n_pairs"] > 0 and a["hp"][:, 15].max() > 0
    # n_pairs counts the candidates that pass the radius each Hitpoint had when their BATCH began (cgrt_ppm_session.hpp, step 2), so
    # unlike everything else it depends on where the batches begin, through either door: 1961 against 1966 on c2_48x36 between
    # one call and the chunked calls.  It is compared where the batches are the same -- the old door fed in the same calls -- and
    # everything else also against the single add_photons call.
    _same(a, b, "chunked add_photon_rays against one add_photons", pairs=False)
    _same(a_chunked, b, "chunked add_photon_rays against chunked add_photons")
    _same(a_two, c, "add_photons then add_photon_rays")
    _same(a_two, d, "add_photon_rays then add_photons")
    _same(a, a_two, "two calls against one", pairs=False)
    if golden:
        g = np.load(os.path.join(GOLD, "ppm_%s.npz" % name))
        assert np.array_equal(b["image"], g["image"]), "golden image of the compiled reference"


# ---- the test's own photons: a spot light -------------------------------------------------------------------------------
# The apex stands near the room's far left corner and the count is what the two conditions of test 3 need (checked on the CPU
# with the oracle: 2542 / 2541 of the 4800 Hitpoints receive a photon; at 30 011 photons only 2248 / 2276 do); n is not a
# multiple of 256
SPOT = dict(apex=(-8.0, 19.5, 32.0), half_angle_deg=40.0, n=50021, seed=31)


def spot_photons(apex, half_angle_deg, n, seed):
    """n photons from `apex` in random unit directions (numpy) inside the cone of the half-angle about -y; a flux that differs
    per channel and per photon"""
    rng = np.random.default_rng(seed)
    cos_t = rng.uniform(math.cos(math.radians(half_angle_deg)), 1.0, n)
    phi = rng.uniform(0, 2 * math.pi, n)
    sin_t = np.sqrt(1 - cos_t * cos_t)
    d = np.stack([sin_t * np.cos(phi), -cos_t, sin_t * np.sin(phi)], axis=1)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    org = np.ascontiguousarray(np.tile(np.asarray(apex, np.float64), (n, 1)))
    flux = np.ascontiguousarray(rng.uniform(0.5, 1.5, (n, 1)) * np.array([9000.0, 6000.0, 2500.0]))
    return org, np.ascontiguousarray(d), flux


def oracle_photon_events(orc, objs, org, dirs, flux):
    """What trace(flag=false) does with a photon's first segment (main.cpp:52-76,101-125), from the oracle's per-object
    intersect() alone: (valid [n], events [n,9] = P, normal turned against the ray, the photon's flux)."""
    o, obj, t, nrm = oracle_nearest(orc, objs, org, dirs)
    o.close()
    diffuse = np.array([ob.reflection < EPS and ob.transparency < EPS for ob in objs])
    valid = (obj >= 0) & diffuse[np.maximum(obj, 0)]
    P = org + dirs * t[:, None]
    flip = (nrm[:, 0] * dirs[:, 0] + nrm[:, 1] * dirs[:, 1] + nrm[:, 2] * dirs[:, 2]) > 0
    n = np.where(flip[:, None], -nrm, nrm)
    return valid, np.concatenate([P, n, flux], axis=1)


def spot_expected(orc, objs, org, dirs, events, nphotons, hashsize=1000001, alpha=0.7):
    """test_gpu_ppm_rays.lookat_expected fed with given events [m,9] in photon order: the depth-1 Hitpoints of the eye rays from
    the oracle, the table in the order contract, the replay of main.cpp:103-125 and the gather of main.cpp:252-258 over
    `nphotons` photons.  Returns (table [n,16], image [npix,3])."""
    o, obj, t, nrm = oracle_nearest(orc, objs, org, dirs)
    acc, nhit = oracle_depth1(o, objs, org, dirs, obj, t)
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
        Pe, ne, fe = [float(v) for v in ev[0:3]], [float(v) for v in ev[3:6]], [float(v) for v in ev[6:9]]
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


_SPOT_CACHE = {}


def _spot_case(orc, name, mk):
    """The oracle's side of tests 2 and 3 for one scene, computed once"""
    if name not in _SPOT_CACHE:
        objs = mk()
        org, dirs, flux = spot_photons(**SPOT)
        valid, ev = oracle_photon_events(orc, objs, org, dirs, flux)
        _SPOT_CACHE[name] = dict(objs=objs, org=org, dirs=dirs, flux=flux, valid=valid, events=ev)
    return _SPOT_CACHE[name]


# ---- 2. events -----------------------------------------------------------------------------------------------------------
EVENT_SCENES = [("c2", scenes.scene_c2), ("vase_hidden", make_golden.photon_cases_bezier()[0][1]),
                ("room_A_%d" % (KLDS + 1), lambda: _many_objects("A", KLDS + 1))]


@pytest.mark.parametrize("name,mk", EVENT_SCENES, ids=[c[0] for c in EVENT_SCENES])
def test_events_of_emitted_photons_equal_photon_events(gpu_ready, name, mk):
    import cgraytracing_amd as cg
    first, count = 1000, 4097
    org, dirs, flux, keys, draws = cg.emit_photons_host(first, count, PHOTON_SEED)
    with cg.Scene(mk()) as sc:
        want = sc.photon_events(first, count, 5, PHOTON_SEED)
        got = sc.photon_ray_events(org, dirs, flux, keys, draws, max_depth=5, photon_seed=PHOTON_SEED, first_index=first)
        # the stream position is part of the photon: without it the bounces repeat the emitter's draws
        other = sc.photon_ray_events(org, dirs, flux, None, None, max_depth=5, photon_seed=PHOTON_SEED, first_index=first)
    assert len(want) > count and got.shape == want.shape
    assert np.array_equal(got, want)
    assert other.shape[1] == want.shape[1] and not np.array_equal(other, want)


@pytest.mark.parametrize("name,mk", LOOKAT_SCENES, ids=[c[0] for c in LOOKAT_SCENES])
def test_spot_photon_first_segment_against_oracle(gpu_ready, orc, name, mk):
    import cgraytracing_amd as cg
    c = _spot_case(orc, name, mk)
    assert not np.allclose(SPOT["apex"], (0.0, 19.999, 20.0)) and 0.3 * len(c["valid"]) < c["valid"].sum()
    with cg.Scene(c["objs"]) as sc:
        chunks = [sc.photon_ray_events(c["org"][a:a + 20011], c["dirs"][a:a + 20011], c["flux"][a:a + 20011], max_depth=1,
                                       first_index=a) for a in range(0, len(c["org"]), 20011)]
    got = np.concatenate(chunks)
    idx = np.nonzero(c["valid"])[0]
    assert np.array_equal(got[:, 0].astype(np.int64), idx), "valid exactly where the oracle's nearest object is diffuse"
    assert np.array_equal(got[:, 1:4], c["events"][idx, 0:3]), "P = org + dir * t"
    assert np.array_equal(got[:, 4:7], c["events"][idx, 3:6]), "normal turned against the ray"
    assert np.array_equal(got[:, 7:10], c["flux"][idx]), "the given flux"
    assert (np.einsum("ij,ij->i", got[:, 4:7], c["dirs"][idx]) <= 0).all()


# ---- 3. a spot light end to end ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mk", LOOKAT_SCENES, ids=[c[0] for c in LOOKAT_SCENES])
def test_spot_light_session_against_oracle_replay(gpu_ready, orc, name, mk):
    import cgraytracing_amd as cg
    c = _spot_case(orc, name, mk)
    W, H = LOOKAT["W"], LOOKAT["H"]
    org, dirs = lookat_rays_np(**LOOKAT)
    n = len(c["org"])
    table, image = spot_expected(orc, c["objs"], org, dirs, c["events"][c["valid"]], n)
    # the oracle's numbers alone say that the case is not vacuous
    assert len(table) >= 0.6 * W * H, "fewer than 60 % of the texels have a Hitpoint"
    assert (table[:, 15] > 0).sum() >= 0.5 * len(table), "fewer than half of the Hitpoints received a photon"
    with cg.Scene(c["objs"]) as sc:
        with sc.ppm_session_rays(_t(sc, org), _t(sc, dirs), width=W, rows=H, spp=1, max_depth=1, batch=BATCH) as ses:
            ses.add_photon_rays(_t(sc, c["org"]), _t(sc, c["dirs"]), _t(sc, c["flux"]))
            hp, img, inf = ses.hitpoints(), ses.image(), ses.info()
    print(name, len(table), "Hitpoints,", int((table[:, 15] > 0).sum()), "with photons,", int(c["valid"].sum()), "events")
    assert inf["photons_done"] == n and inf["n_events"] == int(c["valid"].sum())
    assert hp.shape == table.shape
    assert np.array_equal(hp[:, :11], table[:, :11]), "ray index, emission index, f, pos, normal in table order"
    assert np.array_equal(hp[:, 11:16], table[:, 11:16]), "flux, r2, n"
    assert np.array_equal(img.reshape(-1, 3), image)


# ---- 4. contract properties ---------------------------------------------------------------------------------------------
def _gather_np(hp, W, H, spp, photons_done):
    """main.cpp:252-258 as ppm_gather_kernel sums it: per pixel, over its Hitpoints in table order, flux * (1 / (PI r2 N spp))"""
    img = np.zeros((W * H, 3))
    s = 1.0 / (PI_REF * hp[:, 14] * (float(photons_done) * spp))
    np.add.at(img, hp[:, 0].astype(np.int64) // spp, hp[:, 11:14] * s[:, None])  # unbuffered: added in table order
    return img.reshape(H, W, 3)


def test_contract_properties(gpu_ready):
    import torch
    import cgraytracing_amd as cg
    _, mk, cam, W, H, spp, _ = next(c for c in make_golden.photon_cases() if c[0] == "c2_dof_32x24")
    n = 7001
    org, dirs, flux = spot_photons((3.0, 17.0, 24.0), 40.0, n, 5)
    kw = dict(camera=cam(), max_depth=5, seed=12345, photon_seed=PHOTON_SEED, batch=BATCH)
    with cg.Scene(mk()) as sc:
        dev = _dev(sc)
        to, td, tf = _t(sc, org), _t(sc, dirs), _t(sc, flux)

        def run(*photons, chunk=None):
            with sc.ppm_session(W, H, spp, **kw) as ses:
                if chunk:
                    _feed_rays(ses, photons, 0, photons[0].shape[0])
                else:
                    ses.add_photon_rays(*photons)
                return _state(ses)

        base = run(to, td, tf)
        assert base["n_events"] > n and base["hp"][:, 15].max() > 0 and base["photons_done"] == n
        assert np.array_equal(base["image"], _gather_np(base["hp"], W, H, spp, n))
        _same(base, run(to, td, tf, None, None, chunk=True), "chunks", pairs=False)  # (other batches: other candidate pairs)
        # keys / draws omitted = the stream (photon_seed, photon index) from its start
        keys = _photon_keys(PHOTON_SEED, np.arange(n))
        _same(base, run(to, td, tf, _t(sc, keys), torch.zeros(n, dtype=torch.int32, device=dev)), "default stream")
        assert not np.array_equal(base["hp"], run(to, td, tf, _t(sc, keys[::-1].copy()), None)["hp"])  # (the keys are read)
        # twice the flux: twice every Hitpoint's flux, exactly; radii, counts and events as they were
        dbl = run(to, td, tf * 2)
        assert np.array_equal(dbl["hp"][:, 11:14], base["hp"][:, 11:14] * 2)
        assert np.array_equal(dbl["hp"][:, 14:16], base["hp"][:, 14:16]) and np.array_equal(dbl["hp"][:, :11], base["hp"][:, :11])
        assert dbl["n_events"] == base["n_events"] and dbl["n_pairs"] == base["n_pairs"]
        # dead photons (dir = 0) between the others, streams given explicitly: counted, and nothing else
        rng = np.random.default_rng(9)
        m = n + 1500
        live = np.sort(rng.choice(m, n, replace=False))
        o2, d2, f2 = np.full((m, 3), 7.0), np.zeros((m, 3)), np.full((m, 3), 1e6)
        k2, n2 = rng.integers(0, 2 ** 63, m, dtype=np.uint64), np.full(m, 4, np.uint32)
        o2[live], d2[live], f2[live], k2[live], n2[live] = org, dirs, flux, keys, 0
        dead = run(_t(sc, o2), _t(sc, d2), _t(sc, f2), _t(sc, k2), _t(sc, n2), chunk=True)
        assert dead["photons_done"] == m and dead["n_events"] == base["n_events"]
        assert np.array_equal(dead["hp"], base["hp"]), "flux, r2 and n of every Hitpoint"
        assert np.array_equal(dead["image"], _gather_np(base["hp"], W, H, spp, m)) and not np.array_equal(dead["image"], base["image"])
        # n = 0 does nothing; tensors are checked in Python before any launch
        with sc.ppm_session(W, H, spp, **kw) as ses:
            ses.add_photon_rays(to[:0], td[:0], tf[:0])
            assert ses.photons_done == 0
            ses.add_photon_rays(to[:10], td[:10], tf[:10])
            ses.add_photon_rays(to[:0], td[:0], tf[:0], None, None)
            assert ses.photons_done == 10
            for bad in ((to.cpu(), td, tf), (to, td.float(), tf), (to, td, tf[:-1]), (to, td[:, :2], tf), (to, td, tf.t().contiguous().t()),
                        (org, td, tf), (to, td, tf, _t(sc, keys).int()), (to, td, tf, None, torch.zeros(n, dtype=torch.int64, device=dev)),
                        (to, td, tf, _t(sc, keys).cpu())):
                with pytest.raises(ValueError):
                    ses.add_photon_rays(*bad)
            assert ses.photons_done == 10


# ---- 5. the example -------------------------------------------------------------------------------------------------------
def test_example_spot_light_ppm(gpu_ready, tmp_path):
    """examples/spot_light_ppm.py at a small size: it writes a PNG, and the floor is brighter under the cone than beside it."""
    from PIL import Image
    import cgraytracing_amd as cg
    out = str(tmp_path / "spot_light_ppm.png")
    W, H = 64, 36
    code = ("import sys; sys.path.insert(0, %r); import spot_light_ppm; spot_light_ppm.main(%r, W=%d, H=%d, spp=1, photons=60000)"
            % (os.path.join(ROOT, "examples"), out, W, H))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    rgb = np.asarray(Image.open(out).convert("RGB")).astype(np.float64)
    assert rgb.shape == (H, W, 3) and rgb.max() > 0
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import spot_light_ppm as ex
    with cg.Scene(scenes.scene_c2()) as sc:
        org, dirs = ex.eye_rays(W, H, 1, _dev(sc))
        hit = sc.trace_rays(org, dirs, want=("hit",))
        obj, t = hit["hit_obj"].cpu().numpy(), hit["hit_t"].cpu().numpy()
        P = org.cpu().numpy() + dirs.cpu().numpy() * t[:, None]
    v = P - np.asarray(ex.SPOT["pos"])
    cos_a = -v[:, 1] / np.sqrt((v * v).sum(axis=1))
    floor = obj == 0  # the floor is C2's first wall sphere
    inside = floor & (cos_a >= math.cos(math.radians(ex.SPOT["half_angle_deg"] - 3)))
    outside = floor & (cos_a < math.cos(math.radians(ex.SPOT["half_angle_deg"] + 3)))
    lum = rgb[::-1].reshape(-1, 3).sum(axis=1)  # the PNG's top row is the image's last
    assert inside.sum() > 50 and outside.sum() > 50, (int(inside.sum()), int(outside.sum()))
    print("floor texels under the cone %d (mean %.1f), beside it %d (mean %.1f)" % (inside.sum(), lum[inside].mean(), outside.sum(),
                                                                                  lum[outside].mean()))
    assert lum[inside].mean() > lum[outside].mean()
