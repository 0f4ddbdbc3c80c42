"""Caller-supplied rays on the GPU (cgrt_trace_rays, cgrt_camera_rays) against the CPU oracle.

The camera's own rays, traced as a ray list, must give the oracle's eye pass per ray in fp64, bit for bit: the ray kernel adds a
ray tree's Hitpoint values in the lane, in the reference's emission order.  Rays no camera makes are checked against the
oracle's per-object intersect() composed as main.cpp:52-62 composes it, and against getSurfaceColor at depth 1."""

import numpy as np
import pytest

import scenes
from backends import BackendScene
from cgraytracing_amd import _capi
from cgraytracing_amd.scene import Camera
from test_rays_host import CAMERAS, SIZES, SPP
from test_rays_host import SEED as CAM_SEED
from test_gpu_parity import BEZ_SCENE_BAR

pytestmark = pytest.mark.gpu


def _bump_sphere_scene():
    return scenes.planes(scenes.stone_small_texture(True)) + [scenes.Sphere((5, -12, 30), 5, (1, 1, 1), 0.8, 0.5)]


def _cam_off_axis():
    return Camera(cam=(3.0, 2.0, -14.0), lens_radius=1.5)


CASES = [
    # name, scene factory, camera, W, H, spp, depth: one per kernel variant (sizes as test_gpu_parity.CASES or smaller)
    ("c1_spheres_depth1", scenes.scene_c1, scenes.cam_pinhole, 128, 128, 1, 1),
    ("c2_glass_pinhole", scenes.scene_c2, scenes.cam_pinhole, 192, 108, 1, 5),
    ("c2_glass_dof", scenes.scene_c2, scenes.cam_dof, 160, 90, 4, 5),
    ("c2_depth3", scenes.scene_c2, scenes.cam_dof, 96, 54, 4, 3),
    ("pyramid_diffuse", lambda: scenes.scene_pyramid(False), scenes.cam_pinhole, 96, 96, 1, 5),
    ("pyramid_glass", lambda: scenes.scene_pyramid(True), scenes.cam_dof, 96, 96, 2, 5),
    ("c3_bunny_glass_chess", lambda: scenes.scene_c3(True), scenes.cam_dof, 96, 96, 2, 5),
    ("dragon_diffuse", scenes.scene_dragon, scenes.cam_pinhole, 128, 128, 1, 5),
    ("textured_walls", scenes.scene_textured_walls, scenes.cam_dof, 160, 120, 2, 5),
    ("glass_bump_floor", scenes.scene_glass_bump_floor, scenes.cam_dof, 96, 72, 2, 5),
    ("bump_floor_glass_sphere", _bump_sphere_scene, scenes.cam_dof, 96, 72, 2, 5),
    ("plain_planes_depth1", scenes.planes, scenes.cam_pinhole, 64, 48, 1, 1),
    # nothing may rest on the default camera's symmetry
    ("c2_off_axis", scenes.scene_c2, _cam_off_axis, 96, 54, 2, 5),
    ("c3_off_axis", lambda: scenes.scene_c3(True), _cam_off_axis, 64, 64, 1, 5),
]


def oracle_per_ray(orc, objs, cam, W, H, spp, depth, seed):
    """The oracle's eye pass one sample at a time: at spp 1 its acc_sum IS the ray's fp64 sum and its nhit the ray's count.
    Returns (acc [spp*H*W, 3], nhit [spp*H*W], rays) in cgrt_camera_rays' ray order."""
    o = BackendScene(orc, objs)
    acc, nhit, nrays = [], [], 0
    for k in range(spp):
        r = o.trace_grid(cam, W, H, 1, depth, seed=seed, sample0=k)
        acc.append(r["acc_sum"].reshape(-1, 3))
        nhit.append(r["nhit"].reshape(-1))
        nrays += r["nrays"]
    o.close()
    return np.concatenate(acc), np.concatenate(nhit), nrays


def trace_camera(sc, cam, W, H, spp, depth, seed, **kw):
    import torch
    org, dirs, keys = sc.camera_rays(W, H, spp, cam, seed)
    res = sc.trace_rays(org, dirs, keys, max_depth=depth, seed=seed, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if "nhit" in out:
        out["nhit"] = out["nhit"].view(np.uint32)
    return out, (org, dirs, keys)


@pytest.mark.parametrize("cam_case", CAMERAS, ids=lambda c: c[0])
def test_device_camera_rays_equal_host(gpu_ready, cam_case):
    import cgraytracing_amd as cg
    from cgraytracing_amd.engine import camera_rays_host

    with cg.Scene(scenes.scene_c1()) as sc:
        for lens in (True, False):
            cam = cam_case[1]()
            if not lens:
                cam.lens_radius = 0.0
            for W, H in SIZES:
                want = camera_rays_host(W, H, SPP, cam, CAM_SEED)
                got = [t.cpu().numpy() for t in sc.camera_rays(W, H, SPP, cam, CAM_SEED)]
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (W, H, lens)
                assert np.array_equal(got[2].view(np.uint64), want[2]), (W, H, lens)
            # a striped share with padding rows, a row band with a sample range
            for kw in (dict(rows=16, stripe=(8, 2, 3)), dict(rows=13, row_offset=20, sample_offset=4)):
                want = camera_rays_host(67, 45, 3, cam, CAM_SEED, **kw)
                got = [t.cpu().numpy() for t in sc.camera_rays(67, 45, 3, cam, CAM_SEED, **kw)]
                assert all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want)), kw


@pytest.mark.parametrize("name,mk,cam,W,H,spp,depth", CASES, ids=[c[0] for c in CASES])
def test_camera_rays_traced_equal_oracle_eye_pass(gpu_ready, orc, name, mk, cam, W, H, spp, depth):
    import cgraytracing_amd as cg

    objs, camera = mk(), cam()
    acc, nhit, nrays = oracle_per_ray(orc, objs, camera, W, H, spp, depth, 12345)
    with cg.Scene(objs) as sc:
        variant = sc.rays_variant(depth)
        got, _ = trace_camera(sc, camera, W, H, spp, depth, 12345)
    bad = np.nonzero((got["acc"] != acc).any(axis=1))[0]
    print("%s: %s, %d rays, %d Hitpoints, rays differing in fp64: %d %s" %
          (name, variant, nrays, int(nhit.sum()), len(bad), [(int(i), (got["acc"][i] - acc[i]).tolist()) for i in bad[:5]]))
    assert np.array_equal(got["nhit"], nhit)
    assert np.array_equal(got["acc"], acc)
    assert int(got["counters"][_capi.CNT_RAYS]) == nrays
    assert int(got["counters"][_capi.CNT_HITPOINTS]) == int(nhit.sum())


def _bezier_scene(glass):
    """C5-shaped: planes with the stone bump floor + the vase, mirror-like (refl 0.5) or glass (refl 0.8, transp 0.5)"""
    return scenes.planes(scenes.stone_small_texture(True)) + [scenes.vase_bezier(0.8, 0.5) if glass else scenes.vase_bezier()]


@pytest.mark.parametrize("glass", [False, True], ids=["mirror_vase", "glass_vase"])
def test_bezier_scene_rays_vs_oracle(gpu_ready, orc, glass):
    """C5-shaped scenes (bump floor + Bezier vase; the glass vase drives the pending-ray levels of the one-wave workgroups) as a
    ray list with the camera's keys, so that the Newton draws are the grid's: the bars of test_gpu_parity.BEZ_SCENE_BAR in their
    form -- share of rays within 1e-4 of the oracle, relative ray-count gap -- and the rays that miss, by index.  The nearest-hit
    query draws from the same keyed streams as the full trace's first walk: its answers are the full trace's, bit for bit."""
    import cgraytracing_amd as cg
    objs = _bezier_scene(glass)
    W, H, spp = (64, 64, 2) if glass else (96, 96, 2)
    acc, nhit, nrays = oracle_per_ray(orc, objs, scenes.cam_dof(), W, H, spp, 5, 7)
    with cg.Scene(objs) as sc:
        variant, qvariant = sc.rays_variant(5), sc.rays_variant(5, want=("hit",))
        got, (org, dirs, keys) = trace_camera(sc, scenes.cam_dof(), W, H, spp, 5, 7)
        query = {k: v.cpu().numpy() for k, v in sc.trace_rays(org, dirs, keys, want=("hit",)).items()}
    err = np.abs(got["acc"] - acc).max(axis=1)
    bad = np.nonzero(err >= 1e-4)[0]
    frac = 1.0 - len(bad) / len(err)
    gap = abs(int(got["counters"][_capi.CNT_RAYS]) - nrays) / max(1, nrays)
    print("%s: %d of %d rays miss 1e-4 (within: %.6f), Linf=%.3e, bit-equal %.6f, rays %d vs %d; missing (ray, err): %s" %
          (variant, len(bad), len(err), frac, err.max(), float((got["acc"] == acc).all(axis=1).mean()),
           int(got["counters"][_capi.CNT_RAYS]), nrays, [(int(i), float(err[i])) for i in bad[:12]]))
    assert "BEZ=1,GLASS=%d" % glass in variant and "NT=64" in variant
    assert "BEZ=1,GLASS=0" in qvariant and "FIRST=1,NT=64" in qvariant
    assert frac >= BEZ_SCENE_BAR[0] and gap <= BEZ_SCENE_BAR[1]
    vase = len(objs) - 1
    assert (got["hit_obj"] == vase).sum() > 50, "no primary ray reaches the vase"
    for k in ("hit_obj", "hit_t", "hit_normal"):
        assert np.array_equal(query[k], got[k]), k
    assert int(query["counters"][_capi.CNT_RAYS]) == len(org)


STATS_CASES = [("dragon", scenes.scene_dragon, scenes.cam_pinhole, 128, 128), ("c3_glass_bunny", lambda: scenes.scene_c3(True), scenes.cam_dof, 96, 96)]


@pytest.mark.parametrize("name,mk,cam,W,H", STATS_CASES, ids=[c[0] for c in STATS_CASES])
def test_stats_counters(gpu_ready, name, mk, cam, W, H):
    """CGRT_RAYS_STATS: the STATS variants (full trace with and without pending rays, nearest-hit query) give the results of the
    plain ones bit for bit, and the node / triangle test counters are the eye pass's with CGRT_GRID_STATS on the same rays
    (one sample per pixel) -- a lane counts the tests of its own walks, so they do not depend on the schedule either."""
    import cgraytracing_amd as cg
    import torch
    NODE, TRI = _capi.CNT_NODE_TESTS, _capi.CNT_TRI_TESTS
    with cg.Scene(mk()) as sc:
        camera = cam()
        org, dirs, keys = sc.camera_rays(W, H, 1, camera, 12345)
        plain = sc.trace_rays(org, dirs, keys)
        st = sc.trace_rays(org, dirs, keys, stats=True)
        q = sc.trace_rays(org, dirs, keys, want=("hit",), stats=True)
        perm = torch.from_numpy(np.random.default_rng(2).permutation(org.shape[0])).to(org.device)
        shuf = sc.trace_rays(org[perm].contiguous(), dirs[perm].contiguous(), keys[perm].contiguous(), stats=True)
        _, _, gcnt = sc.trace_grid(W, H, 1, camera, 5, 12345, stats=True)
        torch.cuda.synchronize()
        variants = sc.rays_variant(5, stats=True), sc.rays_variant(5, want=("hit",), stats=True)
    assert all("STATS=1" in v for v in variants), variants
    c_plain, c_st, c_q, c_shuf, c_grid = (x.cpu().numpy() for x in (plain["counters"], st["counters"], q["counters"], shuf["counters"], gcnt))
    print(name, variants, "node / tri tests: rays", c_st[NODE], c_st[TRI], "grid", c_grid[NODE], c_grid[TRI], "query", c_q[NODE], c_q[TRI])
    for k in ("acc", "nhit", "hit_obj", "hit_t", "hit_normal"):
        assert np.array_equal(st[k].cpu().numpy(), plain[k].cpu().numpy()), k
    for k in ("hit_obj", "hit_t", "hit_normal"):
        assert np.array_equal(q[k].cpu().numpy(), plain[k].cpu().numpy()), k
    assert c_plain[NODE] == 0 and c_plain[TRI] == 0
    assert np.array_equal(c_st[:2], c_plain[:2]) and np.array_equal(c_st[:2], c_grid[:2])
    assert c_st[NODE] > 0 and c_st[TRI] > 0 and c_st[NODE] == c_grid[NODE] and c_st[TRI] == c_grid[TRI]
    assert c_shuf[NODE] == c_st[NODE] and c_shuf[TRI] == c_st[TRI]
    assert 0 < c_q[NODE] <= c_st[NODE] and 0 < c_q[TRI] <= c_st[TRI]


def _table_variants():
    """The flag tuples (TREES, BEZ, GLASS, SPH, STATS, SPILL, FIRST, NT) of CGRT_RAY_VARIANTS, read from cgrt_variants.h itself."""
    import variants
    out = variants.ray_variants()
    assert len(out) >= 20
    return set(out)


def test_every_table_entry_is_launched(gpu_ready, monkeypatch):
    """Every instantiation in CGRT_RAY_VARIANTS (the list is read from the source) is launched here on a small grid of camera rays
    -- by the scenes, depths and flags that the tests of this file trace against the oracle -- and nothing outside the table
    is ever asked for; a nearest-hit query and a full trace of the same rays agree on the hits."""
    import cgraytracing_amd as cg
    import torch
    launches = [(c[0], c[1], c[6], False, None) for c in CASES]
    launches += [(n, mk, 5, True, None) for n, mk, _, _, _ in STATS_CASES]
    launches += [("bezier_mirror", lambda: _bezier_scene(False), 5, False, None), ("bezier_glass", lambda: _bezier_scene(True), 5, False, None),
                 ("spheres_1000", lambda: scenes.many_spheres(1000, 11), 5, False, None),
                 ("spheres_1000_depth1", lambda: scenes.many_spheres(1000, 11), 1, False, None),
                 ("room_800", lambda: scenes.room_with_objects(800, 5), 5, False, None)]
    seen = {}
    for label, mk, depth, stats, lds_objs in launches:
        with cg.Scene(mk()) as sc:
            org, dirs, keys = sc.camera_rays(16, 8, 1, scenes.cam_dof(), 3)
            full = sc.trace_rays(org, dirs, keys, max_depth=depth, stats=stats)
            query = sc.trace_rays(org, dirs, keys, max_depth=depth, want=("hit",), stats=stats)
            torch.cuda.synchronize()
            for res, want in ((full, ("acc", "nhit", "hit")), (query, ("hit",))):
                v = sc.rays_variant(depth, want=want, stats=stats)
                seen.setdefault(tuple(int(p.split("=")[1]) for p in v[v.index("<") + 1:-1].split(",")), label)
                assert int(res["counters"][_capi.CNT_RAYS].item()) >= 128
            for k in ("hit_obj", "hit_t", "hit_normal"):
                assert torch.equal(full[k], query[k]), (label, k)
    table = _table_variants()
    print("\n".join("%s  <- %s" % (v, seen.get(v)) for v in sorted(table)))
    assert set(seen) == table, dict(never_launched=sorted(table - set(seen)), not_in_table=sorted(set(seen) - table))


# ---- rays no camera makes ------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = np.array([-19.0, -19.0, -9.0]), np.array([19.0, 19.0, 39.0])
RANDOM_SCENES = [
    ("c2", scenes.scene_c2, "spheres"),
    ("c3_glass_bunny", lambda: scenes.scene_c3(True), "planes"),
    ("dragon", scenes.scene_dragon, "planes"),
    ("stone_bump", _bump_sphere_scene, "planes"),
]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def random_rays(walls, seed):
    """50 000 rays from the room's interior box in uniform directions, 2 000 axis-parallel ones, 2 000 that start on a wall, and
    2 000 built to miss everything (sphere walls: from behind the camera within 2 degrees of -z -- the wall spheres curve away
    from such a ray faster than it spreads; plane walls: exactly -z from in front of every object -- the room has no wall there).
    Returns (org, dirs, slice of the last group)."""
    rng = np.random.default_rng(seed)
    org = [rng.uniform(BOX_LO, BOX_HI, (50000, 3))]
    dirs = [_unit(rng, 50000)]
    org.append(rng.uniform(BOX_LO, BOX_HI, (2000, 3)))
    ax = np.zeros((2000, 3))
    ax[np.arange(2000), rng.integers(0, 3, 2000)] = rng.choice([-1.0, 1.0], 2000)
    dirs.append(ax)
    on = rng.uniform(BOX_LO, BOX_HI, (2000, 3))
    k, side = rng.integers(0, 2, 2000), rng.choice([-1.0, 1.0], 2000)  # the walls x = +-20 and y = +-20
    if walls == "planes":
        on[np.arange(2000), k] = 20.0 * side
    else:  # the point of the wall sphere (centre +-10020 on axis k, radius 10000) nearest to the box point
        c = np.zeros((2000, 3))
        c[np.arange(2000), k] = 10020.0 * side
        v = on - c
        on = c + v * (10000.0 / np.sqrt((v * v).sum(axis=1)))[:, None]
    org.append(on)
    dirs.append(_unit(rng, 2000))
    if walls == "planes":
        org.append(rng.uniform([-19.0, -15.0, -9.0], [19.0, 19.0, 5.0], (2000, 3)))
        dirs.append(np.tile([0.0, 0.0, -1.0], (2000, 1)))
    else:
        org.append(rng.uniform([-10.0, -10.0, -60.0], [10.0, 10.0, -20.0], (2000, 3)))
        th, ph = np.radians(rng.uniform(0, 2.0, 2000)), rng.uniform(0, 2 * np.pi, 2000)
        dirs.append(np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], axis=1))
    org, dirs = np.ascontiguousarray(np.concatenate(org)), np.ascontiguousarray(np.concatenate(dirs))
    return org, dirs, slice(54000, 56000)


def oracle_nearest(orc, objs, org, dirs):
    """main.cpp:52-62 over the oracle's per-object intersect(): nearest = INF; an object wins with len < nearest, so the first of
    equals keeps the hit.  Returns (hit_obj, hit_t, hit_normal) with -1 / 0 / 0 for a miss."""
    o = BackendScene(orc, objs)
    n = len(org)
    nearest = np.full(n, 1e10)
    obj = np.full(n, -1, np.int32)
    nrm = np.zeros((n, 3))
    for i in range(len(objs)):
        hit, ln, nv = o.intersect_batch(i, org, dirs)
        win = (hit != 0) & (ln < nearest)
        nearest[win] = ln[win]
        obj[win] = i
        nrm[win] = nv[win]
    t = np.where(obj >= 0, nearest, 0.0)
    return o, obj, t, nrm


def oracle_depth1(o, objs, org, dirs, obj, t):
    """trace() at MAX_DEPTH 1: a diffuse winner (refl < 1e-4 and transp < 1e-4) stores Hitpoint{getSurfaceColor(P) * (1,1,1)} at
    P = org + dir * t (main.cpp:68,85-100); a mirror or glass winner spawns children that fail the depth test (main.cpp:46)."""
    acc = np.zeros((len(org), 3))
    nhit = np.zeros(len(org), np.uint32)
    P = org + dirs * t[:, None]
    for i, ob in enumerate(objs):
        sel = np.nonzero(obj == i)[0]
        if len(sel) and ob.reflection < 1e-4 and ob.transparency < 1e-4:
            acc[sel] = o.surface_color_batch(i, P[sel])
            nhit[sel] = 1
    return acc, nhit


_RANDOM_CACHE = {}


def _random_case(orc, name, mk, walls):
    """(objs, org, dirs, oracle's hit_obj / hit_t / hit_normal / depth-1 acc / nhit, the GPU's three result dicts as numpy)"""
    import cgraytracing_amd as cg
    import torch

    if name in _RANDOM_CACHE:
        if isinstance(_RANDOM_CACHE[name], BaseException):  # nothing that failed is run again
            pytest.fail("the GPU step of this scene failed in an earlier test: %r" % (_RANDOM_CACHE[name],))
        return _RANDOM_CACHE[name]
    try:
        return _random_case_run(name, orc, mk, walls)
    except BaseException as e:
        _RANDOM_CACHE[name] = e
        raise


def _random_case_run(name, orc, mk, walls):
    import cgraytracing_amd as cg
    import torch

    objs = mk()
    org, dirs, miss_group = random_rays(walls, 2024)
    o, obj, t, nrm = oracle_nearest(orc, objs, org, dirs)
    acc, nhit = oracle_depth1(o, objs, org, dirs, obj, t)
    o.close()
    assert (obj[miss_group] == -1).all(), "the group built to miss hits something (oracle)"
    with cg.Scene(objs) as sc:
        dev = torch.device("cuda", sc.device)
        to, td = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
        query = sc.trace_rays(to, td, want=("hit",))
        full1 = sc.trace_rays(to, td, max_depth=1)
        full5 = sc.trace_rays(to, td, max_depth=5, want=("nhit", "hit"))
        torch.cuda.synchronize()
        print(sc.rays_variant(1, want=("hit",)), sc.rays_variant(1), sc.rays_variant(5))
    got = [{k: v.cpu().numpy() for k, v in r.items()} for r in (query, full1, full5)]
    _RANDOM_CACHE[name] = (objs, org, dirs, obj, t, nrm, acc, nhit, got)
    return _RANDOM_CACHE[name]


@pytest.mark.parametrize("name,mk,walls", RANDOM_SCENES, ids=[c[0] for c in RANDOM_SCENES])
def test_random_rays_nearest_hit_and_depth1_shading(gpu_ready, orc, name, mk, walls):
    """56 000 rays no camera makes: hit_obj and hit_t equal the oracle's composition of intersect() (main.cpp:52-62), as a
    nearest-hit query and as part of a full trace; at max_depth 1 acc is getSurfaceColor(P) of a diffuse winner, else 0."""
    objs, org, dirs, obj, t, nrm, acc, nhit, (query, full1, full5) = _random_case(orc, name, mk, walls)
    spec = (obj >= 0) & (nhit == 0)
    shares = dict(diffuse=float((nhit == 1).mean()), specular=float(spec.mean()), miss=float((obj < 0).mean()))
    print("%s: %s" % (name, shares))
    if name == "c2":
        assert min(shares.values()) >= 0.01, shares  # each of the three outcomes is really tested
    for what, res in (("query", query), ("depth 1", full1), ("depth 5", full5)):
        bad = np.nonzero(res["hit_obj"] != obj)[0]
        assert len(bad) == 0, (what, bad[:10], res["hit_obj"][bad[:10]], obj[bad[:10]])
        assert np.array_equal(res["hit_t"], t), what
        assert (res["hit_t"][obj < 0] == 0).all() and (res["hit_normal"][obj < 0] == 0).all()
    assert "acc" not in query and "nhit" not in query
    assert int(query["counters"][_capi.CNT_RAYS]) == len(org) and int(query["counters"][_capi.CNT_HITPOINTS]) == 0
    assert np.array_equal(full1["nhit"].view(np.uint32), nhit)
    assert np.array_equal(full1["acc"], acc)
    assert int(full1["counters"][_capi.CNT_RAYS]) == len(org)
    assert int(full1["counters"][_capi.CNT_HITPOINTS]) == int(nhit.sum())


@pytest.mark.parametrize("name,mk,walls", RANDOM_SCENES, ids=[c[0] for c in RANDOM_SCENES])
def test_random_rays_hit_normal(gpu_ready, orc, name, mk, walls):
    """hit_normal equals the normal the oracle's intersect() returned, bit for bit, on every hit.

    The reference orients a mesh normal by the parity of its improvement counter (objects.h:107,321-327).  The scene walk of an
    opaque mesh prunes by distance and does not know that count; ray_normal_sign_kernel recounts it without pruning when
    hit_normal is asked for.  Prints, per scene and call, how many normals differ and how many of those are exact negations."""
    objs, org, dirs, obj, t, nrm, acc, nhit, got = _random_case(orc, name, mk, walls)
    ok = True
    for what, res in zip(("query", "depth 1", "depth 5"), got):
        diff = (res["hit_normal"] != nrm).any(axis=1)
        neg = diff & (res["hit_normal"] == -nrm).all(axis=1)
        kinds = sorted({objs[i].kind for i in np.unique(obj[diff])})
        print("%s %s: hits %d, normals that differ %d, of them exact negations %d, owners %s" %
              (name, what, int((obj >= 0).sum()), int(diff.sum()), int(neg.sum()), kinds))
        ok = ok and not diff.any()
    assert ok
    if name == "dragon":
        # the C ABI with hit_normal3 alone: the recount keeps the winners in the handle's scratch
        import ctypes as C
        import cgraytracing_amd as cg
        n = 6000
        o, d, only = np.ascontiguousarray(org[:n]), np.ascontiguousarray(dirs[:n]), np.zeros((n, 3))
        with cg.Scene(objs) as sc:
            r = _capi.Rays(n, o.ctypes.data, d.ctypes.data, None, 0, 1, 5, 0)
            res = _capi.RayResults(None, None, None, None, only.ctypes.data)
            _capi.check(sc._L.cgrt_trace_rays_host(sc._h, C.byref(r), C.byref(res), None))
            fast = sc.trace_rays_host(o, d, want=("hit",), sign_pass=False)["hit_normal"]
        assert (obj[:n] == len(objs) - 1).sum() > 100 and np.array_equal(only, nrm[:n])
        # CGRT_RAYS_NO_SIGN_PASS: the same vectors, some with the other sign, and only on the mesh
        flipped = (fast != nrm[:n]).any(axis=1)
        assert flipped.any() and np.array_equal(np.abs(fast), np.abs(nrm[:n])) and (obj[:n][flipped] == len(objs) - 1).all()


def test_schedule_independence(gpu_ready):
    """A ray's results depend on the ray alone: a random permutation of c2_glass_dof's rays (keys permuted alike) gives the
    permuted results, three calls of uneven size give the same, and so does a second run -- acc bit for bit."""
    import cgraytracing_amd as cg
    import torch

    name, mk, cam, W, H, spp, depth = next(c for c in CASES if c[0] == "c2_glass_dof")
    with cg.Scene(mk()) as sc:
        base, (org, dirs, keys) = trace_camera(sc, cam(), W, H, spp, depth, 12345)
        again = sc.trace_rays(org, dirs, keys, max_depth=depth)
        n = org.shape[0]
        perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(org.device)
        shuf = sc.trace_rays(org[perm].contiguous(), dirs[perm].contiguous(), keys[perm].contiguous(), max_depth=depth)
        cuts = [0, 777, 777 + 64 * 31 + 1, n]
        parts = [sc.trace_rays(org[a:b].contiguous(), dirs[a:b].contiguous(), keys[a:b].contiguous(), max_depth=depth)
                 for a, b in zip(cuts[:-1], cuts[1:])]
        # without keys: the default key is a function of first_index + i, so a split call continues the whole call's keys
        nokeys = sc.trace_rays(org, dirs, None, max_depth=depth, seed=3)
        nokeys_parts = [sc.trace_rays(org[a:b].contiguous(), dirs[a:b].contiguous(), None, max_depth=depth, seed=3, first_index=a)
                        for a, b in zip(cuts[:-1], cuts[1:])]
        torch.cuda.synchronize()
        perm = perm.cpu().numpy()
        for k in ("acc", "nhit", "hit_obj", "hit_t", "hit_normal"):
            want = base[k].view(np.int32) if k == "nhit" else base[k]
            assert np.array_equal(again[k].cpu().numpy(), want), ("second run", k)
            assert np.array_equal(shuf[k].cpu().numpy(), want[perm]), ("permuted", k)
            assert np.array_equal(np.concatenate([p[k].cpu().numpy() for p in parts]), want), ("split", k)
            assert np.array_equal(np.concatenate([p[k].cpu().numpy() for p in nokeys_parts]), nokeys[k].cpu().numpy()), ("split, no keys", k)
        for res in (again, shuf, nokeys):
            assert np.array_equal(res["counters"].cpu().numpy()[:2], base["counters"][:2])
        assert np.array_equal(sum(p["counters"].cpu().numpy()[:2] for p in parts), base["counters"][:2])


def test_more_objects_than_lds_holds(gpu_ready, orc, monkeypatch):
    """The scenes of test_gpu_fullsize.test_a_thousand_objects as ray lists: 1 000 spheres (768 in LDS, the rest through the
    scalar cache) and the 40-object scene of every kind with 7 objects resident (the general loop's staging record), exact; and
    object counts on either side of the LDS limit.
    CGRT_ERR_LIMIT for a launch whose LDS does not fit is not asserted: no scene reaches it -- the general variant lowers its
    resident count until it fits, the sphere variant's and the others' worst case (kLdsObjsMax objects) is a static_assert of
    cgrt_variants.h, and the ray launches take no LDS padding knob -- so launch_checked's refusal stays a guard without a case."""
    import cgraytracing_amd as cg
    cam = scenes.cam_dof()

    def check(objs, W, H, spp, seed, expect, depth=5):
        acc, nhit, nrays = oracle_per_ray(orc, objs, cam, W, H, spp, depth, seed)
        with cg.Scene(objs) as sc:
            variant = sc.rays_variant(depth)
            got, (org, dirs, keys) = trace_camera(sc, cam, W, H, spp, depth, seed)
            q = sc.trace_rays(org, dirs, keys, want=("hit",))
            first = {k: v.cpu().numpy() for k, v in q.items()}
            print(len(objs), variant, sc.rays_variant(depth, want=("hit",)))
        assert expect in variant, variant
        assert np.array_equal(got["nhit"], nhit) and np.array_equal(got["acc"], acc)
        assert int(got["counters"][_capi.CNT_RAYS]) == nrays
        for k in ("hit_obj", "hit_t", "hit_normal"):
            assert np.array_equal(first[k], got[k]), k  # the query's variant sees the same nearest hits

    check(scenes.many_spheres(1000, 11), 96, 64, 2, 9, "GLASS=1,SPH=1,STATS=0,SPILL=1")
    check(scenes.many_spheres(1000, 11), 96, 64, 1, 9, "GLASS=0,SPH=1,STATS=0,SPILL=1", depth=1)
    for n in (767, 768, 769):
        check(scenes.many_spheres(n, 21), 48, 32, 1, 9, "SPILL=%d" % (n > 768))
    objs = scenes.planes(scenes.stone_small_texture(True)) + scenes.many_spheres(38, 3)[5:]
    objs.insert(9, scenes.TriangleMesh.from_triangles(scenes.pyramid_tris(0.6, (-6.0, -13.0, 36.0)), (0.6, 0.7, 0.9), 0.0, 0.0))
    objs.append(scenes.TriangleMesh.from_triangles(scenes.bunny_tris() * 0.5 + np.tile([6.0, -6.0, 12.0], 3), (1.0, 1.0, 1.0), 0.8, 0.5))
    assert len(objs) == 40
    check(objs, 96, 72, 1, 4, "SPILL=0")
    monkeypatch.setenv("CGRT_LDS_OBJS", "7")
    check(objs, 96, 72, 1, 4, "TREES=1,BEZ=1,GLASS=1,SPH=0,STATS=0,SPILL=1")
    monkeypatch.delenv("CGRT_LDS_OBJS")
    # a room of planes and spheres beyond the list: the general loop with its resident count lowered to what fits
    check(scenes.room_with_objects(800, 5), 48, 32, 1, 4, "TREES=1,BEZ=1,GLASS=1,SPH=0,STATS=0,SPILL=1")


def test_tensors_and_streams(gpu_ready, orc):
    import cgraytracing_amd as cg
    import torch

    objs, cam = scenes.scene_c2(), scenes.cam_dof()
    W, H = 13, 5  # 65 rays: one block of 64 and one ray
    acc, nhit, nrays = oracle_per_ray(orc, objs, cam, W, H, 1, 5, 12345)
    with cg.Scene(objs) as sc:
        dev = torch.device("cuda", sc.device)
        org, dirs, keys = sc.camera_rays(W, H, 1, cam, 12345)
        assert org.shape == (65, 3)
        # a stream of our own, preallocated outputs filled with a pattern that no result has
        stream = torch.cuda.Stream(dev)
        out = dict(acc=torch.full((65, 3), -7.0, dtype=torch.float64, device=dev), nhit=torch.full((65,), -7, dtype=torch.int32, device=dev),
                   hit_obj=torch.full((65,), -7, dtype=torch.int32, device=dev), hit_t=torch.full((65,), -7.0, dtype=torch.float64, device=dev),
                   hit_normal=torch.full((65, 3), -7.0, dtype=torch.float64, device=dev))
        cnt = torch.zeros(8, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            res = sc.trace_rays(org, dirs, keys, out=out, counters=cnt)
            res2 = sc.trace_rays(org, dirs, keys, out=out, counters=cnt)  # counters are added to
        stream.synchronize()
        assert all(res[k] is out[k] for k in out) and res["counters"] is cnt
        assert np.array_equal(out["acc"].cpu().numpy(), acc) and np.array_equal(out["nhit"].cpu().numpy().view(np.uint32), nhit)
        assert (out["hit_obj"].cpu().numpy() >= 0).all() and (out["hit_t"].cpu().numpy() > 0).all()
        assert int(cnt[_capi.CNT_RAYS].item()) == 2 * nrays and res2["counters"] is cnt
        # one ray
        one = sc.trace_rays(org[64:65].contiguous(), dirs[64:65].contiguous(), keys[64:65].contiguous())
        assert np.array_equal(one["acc"].cpu().numpy(), acc[64:65]) and int(one["nhit"].item()) == int(nhit[64])
        # none
        e = torch.empty((0, 3), dtype=torch.float64, device=dev)
        none = sc.trace_rays(e, e)
        assert none["acc"].shape == (0, 3) and none["nhit"].shape == (0,) and none["hit_obj"].shape == (0,) and none["hit_t"].shape == (0,)
        assert int(none["counters"].sum().item()) == 0
        # the numpy form gives the same answers
        host = sc.trace_rays_host(org.cpu().numpy(), dirs.cpu().numpy(), keys.cpu().numpy().view(np.uint64))
        assert np.array_equal(host["acc"], acc) and np.array_equal(host["nhit"], nhit) and host["nrays"] == nrays
        # refused before any launch
        cnt.zero_()
        bad = [(org.float(), dirs, keys), (org, dirs.cpu(), keys), (org[:, :2].contiguous(), dirs, keys), (org, dirs[:64].contiguous(), keys),
               (org.t().contiguous().t(), dirs, keys), (org, dirs, keys.int()), (org, dirs, keys[:64].contiguous())]
        for o3, d3, k3 in bad:
            with pytest.raises(ValueError):
                sc.trace_rays(o3, d3, k3, counters=cnt)
        with pytest.raises(ValueError):
            sc.trace_rays(org, dirs, keys, out=dict(acc=out["acc"].float()), counters=cnt)
        with pytest.raises(ValueError):
            sc.trace_rays(org, dirs, keys, want=("colour",), counters=cnt)
        with pytest.raises(_capi.CgrtError):
            sc.trace_rays(org, dirs, keys, max_depth=6, counters=cnt)
        torch.cuda.synchronize()
        assert int(cnt.sum().item()) == 0
