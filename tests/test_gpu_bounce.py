"""Bounce queries on the GPU (cgrt_bounce_rays): one scene walk per ray, then exactly the step trace() takes at the hit.

The yardstick is the library's own full trace: a depth loop in torch over Scene.bounce -- the child slots fed back level by
level -- must visit the ray tree of cgrt_trace_rays and produce its Hitpoints bit for bit: the records of
cgrt_trace_rays_hitpoints by label, nhit, acc3 as the fp64 sum in emission order, and the two counters.  The single steps are
checked against the nearest-hit query, the objects' materials and trace()'s formulas evaluated in numpy."""
import os

import numpy as np
import pytest

import scenes
from cgraytracing_amd import _capi
from cgraytracing_amd.scene import Camera
from test_gpu_occlusion import _subset
from test_gpu_rays import _bezier_scene

pytestmark = pytest.mark.gpu

NONE, HITPOINT, REFLECT, SPLIT = _capi.STEP_NONE, _capi.STEP_HITPOINT, _capi.STEP_REFLECT, _capi.STEP_SPLIT
ARRAYS = ("step", "hit_obj", "hit_t", "pos", "normal", "value", "child_org", "child_dir", "child_adj", "child_path", "child_keys")
_SEEN = {}  # bounce_rays_kernel variants launched by the tests of this file -> the scene that did (read by the last test)


def _note(sc, label, stats=False):
    v = sc.bounce_variant(stats=stats)
    assert v.startswith("bounce_rays_kernel<"), v
    _SEEN.setdefault(tuple(int(p.split("=")[1]) for p in v[v.index("<") + 1:-1].split(",")), label)
    return v


def emission_order(root, path):
    """The order in which trace() emits the Hitpoints (root, path): by root, then depth first with the reflected subtree before
    the refracted one -- the paths compared as bit strings behind their leading 1 (reflected 0, refracted 1), a prefix ahead
    of its extensions.  Hitpoints are leaves of the ray tree, so no path of a root is a prefix of another and the left-aligned
    bit strings order them.  Returns (order, seq): the permutation and each sorted Hitpoint's position within its root."""
    path = path.astype(np.int64)
    assert (path >= 1).all() and (path < (1 << 31)).all()
    ln = np.zeros(len(path), np.int64)  # bits behind the leading 1
    for b in range(1, 32):
        ln += (path >> b) > 0
    aligned = (path - (np.int64(1) << ln)) << (32 - ln)
    order = np.lexsort((aligned, root))
    r, a = root[order], aligned[order]
    assert not ((r[1:] == r[:-1]) & (a[1:] == a[:-1])).any(), "two Hitpoints of a root at one place of the tree"
    new = np.r_[True, r[1:] != r[:-1]] if len(r) else np.zeros(0, bool)
    starts = np.nonzero(new)[0]
    seq = np.arange(len(r)) - np.repeat(starts, np.diff(np.r_[starts, len(r)]))
    return order, seq


def wavefront(sc, org, dirs, keys, depth, compact=True):
    """trace() as a wavefront: Scene.bounce level by level for `depth` levels, the child slots fed back as the next level's
    rays -- as they are (absent children are dir = 0 rays), or compacted with torch.nonzero -- and each ray's root index carried
    along.  Returns the Hitpoints in emission order (root, seq, path, value, pos, normal as numpy), the sums of CGRT_CNT_RAYS and
    _HITPOINTS over the levels and the first level's step array."""
    import torch
    n = org.shape[0]
    root = torch.arange(n, device=org.device)
    adj = path = None
    recs, nrays, nhp, first_step, per_level = [], 0, 0, None, []
    for level in range(1, depth + 1):
        res = sc.bounce(org, dirs, adj, path, keys)
        if first_step is None:
            first_step = res["step"].cpu().numpy()
        cnt = res["counters"].cpu().numpy()
        nrays += int(cnt[_capi.CNT_RAYS])
        nhp += int(cnt[_capi.CNT_HITPOINTS])
        per_level.append(int(cnt[_capi.CNT_RAYS]))
        hp = torch.nonzero(res["step"] == HITPOINT).flatten()
        assert int(cnt[_capi.CNT_HITPOINTS]) == hp.numel()
        p = path if path is not None else torch.ones(org.shape[0], dtype=torch.int32, device=org.device)
        recs.append([t[hp].cpu().numpy() for t in (root, p, res["value"], res["pos"], res["normal"])])
        if level == depth:
            break
        org, dirs, adj, path, keys = (res[k] for k in ("child_org", "child_dir", "child_adj", "child_path", "child_keys"))
        root = torch.cat([root, root])
        if compact:
            keep = torch.nonzero(path != 0).flatten()
            assert torch.equal(keep, torch.nonzero((dirs != 0).any(dim=1)).flatten())  # path 0 and dir = 0 mark the same slots
            org, dirs, adj, path, keys, root = (t[keep].contiguous() for t in (org, dirs, adj, path, keys, root))
        if org.shape[0] == 0:
            break
    root, path, value, pos, normal = (np.concatenate([r[i] for r in recs]) for i in range(5))
    order, seq = emission_order(root, path)
    return dict(root=root[order], seq=seq, path=path[order].astype(np.int64), value=value[order], pos=pos[order], normal=normal[order],
                nrays=nrays, nhp=nhp, first_step=first_step, per_level=per_level)


def summed(wf, n):
    """Per root: the Hitpoint count, and the fp64 sum of the values in emission order starting from 0, as the kernels add them"""
    nhit = np.bincount(wf["root"], minlength=n).astype(np.uint32)
    acc = np.zeros((n, 3))
    for k in range(int(wf["seq"].max()) + 1 if len(wf["seq"]) else 0):
        sel = wf["seq"] == k
        acc[wf["root"][sel]] += wf["value"][sel]  # (each root at most once per k)
    return nhit, acc


def check_against_full_trace(sc, org, dirs, keys, depth, label, need=(HITPOINT, SPLIT)):
    """The comparison of test 1; returns the compacted loop's result"""
    import torch
    n = org.shape[0]
    full = sc.trace_rays(org, dirs, keys, max_depth=depth)
    cap = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=depth)
    wf = wavefront(sc, org, dirs, keys, depth, compact=True)
    wide = wavefront(sc, org, dirs, keys, depth, compact=False)
    torch.cuda.synchronize()
    # condition, not measurement: the first level holds enough rays of each step the scene is here for
    share = {s: int((wf["first_step"] == s).sum()) for s in (NONE, HITPOINT, REFLECT, SPLIT)}
    print("%s depth %d: %s, %d rays, first level %s, rays per level %s, Hitpoints %d" %
          (label, depth, sc.bounce_variant(), n, share, wf["per_level"], len(wf["root"])))
    for s in need:
        assert share[s] >= 64, (label, share)
    # the compacted and the uncompacted loop agree exactly
    for k in ("root", "seq", "path", "value", "pos", "normal", "first_step"):
        assert np.array_equal(wf[k], wide[k]), (label, k)
    assert (wf["nrays"], wf["nhp"]) == (wide["nrays"], wide["nhp"])
    # the capture's records, by label (ray << 4) | position
    assert cap["count"] == len(cap["ray"]) == len(wf["root"]), (label, cap["count"], len(wf["root"]))
    o = np.lexsort((cap["seq"], cap["ray"]))
    assert np.array_equal((cap["ray"][o] << 4) | cap["seq"][o], (wf["root"] << 4) | wf["seq"])
    assert np.array_equal(cap["hp"][o], np.concatenate([wf["value"], wf["pos"], wf["normal"]], axis=1))
    # nhit, acc3 and the counters of the full trace
    nhit, acc = summed(wf, n)
    assert np.array_equal(nhit, full["nhit"].cpu().numpy().view(np.uint32))
    assert np.array_equal(acc, full["acc"].cpu().numpy())
    cnt = full["counters"].cpu().numpy()
    assert wf["nrays"] == int(cnt[_capi.CNT_RAYS]) and wf["nhp"] == int(cnt[_capi.CNT_HITPOINTS]) == len(wf["root"])
    return wf


# ---- 1. bit identity with the full trace ----------------------------------------------------------------------------------
# Frames: the smallest at which the CPU oracle's nearest hit (test_gpu_rays.oracle_nearest over camera_rays_host's rays) finds at
# least 64 rays on each kind of surface the scene is here for -- c2 96x54 spp 2: 9241 diffuse / 494 mirror / 633 glass; glass
# pyramid 96x96: 92 glass (48x48: 26); glass bunny 72x72: 103 (48x48: 43); glass vase 72x72: 78 (32x32: 18).  The glass bump floor
# at 48x36: the reference camera sees the floor at 53 degrees from its normal or more, and the displacement triangles' normals
# point down, along the ray (into = false, nnt = 1.33): all 260 floor hits are total internal reflections, at any frame size.  A
# camera with three times the half width looks down steeply enough: 1393 diffuse, 264 split (96 of them entering), 71 reflected.
# The tests assert the counts on the GPU's own first level.
def _cam_wide():
    return Camera(half_width=30.0, lens_radius=1.5)


FULL_CASES = [
    # name, scene, camera, W, H, spp, depths, steps the first level must hold
    ("c2", scenes.scene_c2, scenes.cam_dof, 96, 54, 2, (5, 3), (HITPOINT, REFLECT, SPLIT)),
    ("pyramid_glass", lambda: scenes.scene_pyramid(True), scenes.cam_dof, 96, 96, 1, (5,), (HITPOINT, SPLIT)),
    ("c3_glass_bunny", lambda: scenes.scene_c3(True), scenes.cam_dof, 72, 72, 1, (5,), (HITPOINT, SPLIT)),
    ("glass_bump_floor", scenes.scene_glass_bump_floor, _cam_wide, 48, 36, 1, (5,), (HITPOINT, REFLECT, SPLIT)),
    ("bezier_glass", lambda: _bezier_scene(True), scenes.cam_dof, 72, 72, 1, (5,), (HITPOINT, SPLIT)),
]


@pytest.mark.parametrize("name,mk,cam,W,H,spp,depths,need", FULL_CASES, ids=[c[0] for c in FULL_CASES])
def test_wavefront_equals_full_trace(gpu_ready, name, mk, cam, W, H, spp, depths, need):
    """A depth loop over Scene.bounce is cgrt_trace_rays: the Hitpoints {f, pos, normal} of every ray tree equal the records of
    cgrt_trace_rays_hitpoints by label, their count per root is nhit, their fp64 sum in emission order is acc3, and the rays and
    Hitpoints counted over the levels are the full trace's -- spheres (thin lens, spp 2, depths 5 and 3), a glass mesh, a glass
    mesh over a chessboard, a glass bump floor and a glass Bezier vase (its Newton draws keyed by the ray's key and path)."""
    import cgraytracing_amd as cg
    with cg.Scene(mk()) as sc:
        _note(sc, name)
        org, dirs, keys = sc.camera_rays(W, H, spp, cam(), 12345)
        for depth in depths:
            check_against_full_trace(sc, org, dirs, keys, depth, name, need)


# ---- 2. steps one by one ------------------------------------------------------------------------------------------------------
def default_keys(seed, first_index, n):
    """sample_key(pixel_key(seed, first_index + i), 0) of cgrt_rng.hpp in numpy (uint64 arithmetic wraps)"""
    G = np.uint64(0x9E3779B97F4A7C15)

    def fin(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    with np.errstate(over="ignore"):
        i = np.uint64(first_index) + np.arange(n, dtype=np.uint64)
        k_pix = fin(fin(np.full(n, seed, np.uint64) + G) + i + G)
        return fin(k_pix + np.uint64(0) + G)


def _dev(sc, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", sc.device))


def _bounce(sc, org, dirs, adj=None, path=None, keys=None, **kw):
    """Scene.bounce on numpy arrays -> dict of numpy arrays (child_path as uint32, child_keys as uint64)"""
    import torch
    res = sc.bounce(_dev(sc, org), _dev(sc, dirs), _dev(sc, adj), _dev(sc, None if path is None else path.view(np.int32)),
                    _dev(sc, None if keys is None else keys.view(np.int64)), **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if "child_path" in out:
        out["child_path"] = out["child_path"].view(np.uint32)
    if "child_keys" in out:
        out["child_keys"] = out["child_keys"].view(np.uint64)
    return out


def test_steps_one_by_one(gpu_ready):
    """The 7 768 rays of test_gpu_occlusion._subset on c2 (random rays, axis-parallel ones, rays that start on a wall, rays
    built to miss; 121 blocks of 64 and 24 rays), some of them made non-rays: every array against the nearest-hit query, the
    objects' materials and main.cpp:64-157 evaluated in numpy from the query's hit."""
    import cgraytracing_amd as cg
    objs = scenes.scene_c2()
    org, dirs = _subset("spheres")
    n = len(org)
    assert n == 7768 and n % 64 != 0
    rng = np.random.default_rng(11)
    dirs = dirs.copy()
    dead = np.zeros(n, bool)
    dead[::97] = True
    dirs[dead] = 0.0
    adj = rng.uniform(0.05, 1.0, (n, 3))
    path = rng.integers(1, 1 << 31, n).astype(np.uint32)
    path[5::101] = 0
    path[7::103] = rng.integers(1 << 31, 1 << 32, len(path[7::103])).astype(np.uint32)
    bad_path = (path == 0) | (path >= (1 << 31))
    untraced = dead | bad_path
    keys = rng.integers(0, 1 << 63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    with cg.Scene(objs) as sc:
        _note(sc, "c2")
        q = {k: v.cpu().numpy() for k, v in sc.trace_rays(_dev(sc, org), _dev(sc, dirs), want=("hit",)).items()}
        got = _bounce(sc, org, dirs, adj, path, keys)
        plain = _bounce(sc, org, dirs)
        ones = _bounce(sc, org, dirs, np.ones((n, 3)), np.ones(n, np.uint32))
        nokeys = _bounce(sc, org, dirs, adj, path, None, seed=99, first_index=1000)
        cuts = [0, 1, 64, n]
        parts = [_bounce(sc, org[a:b], dirs[a:b], adj[a:b], path[a:b], None, seed=99, first_index=1000 + a) for a, b in zip(cuts[:-1], cuts[1:])]
        # only the arrays asked for are written
        import torch
        dev = torch.device("cuda", sc.device)
        like = sc.bounce(_dev(sc, org[:0]), _dev(sc, dirs[:0]))
        sent = {k: torch.full((v.shape[0] + (2 * n if k.startswith("child_") else n),) + tuple(v.shape[1:]), 77, dtype=v.dtype, device=dev)
                for k, v in like.items() if k != "counters"}
        only = sc.bounce(_dev(sc, org), _dev(sc, dirs), _dev(sc, adj), _dev(sc, path.view(np.int32)), _dev(sc, keys.view(np.int64)),
                         want=("step",), out=sent)
        torch.cuda.synchronize()
        assert sorted(only) == ["counters", "step"] and only["step"] is sent["step"]
        assert np.array_equal(sent["step"].cpu().numpy(), got["step"])
        for k, t in sent.items():
            if k != "step":
                assert bool((t == 77).all()), k

    step, obj, t = got["step"], got["hit_obj"], got["hit_t"]
    hit = (q["hit_obj"] >= 0) & ~untraced
    # hit_obj / hit_t: the query's, and -1 / 0 for a ray that is not traced
    assert np.array_equal(obj, np.where(untraced, -1, q["hit_obj"])) and np.array_equal(t, np.where(untraced, 0.0, q["hit_t"]))
    # trace()'s step in numpy, from the query's hit
    refl = np.array([ob.reflection for ob in objs])[np.maximum(obj, 0)]
    transp = np.array([ob.transparency for ob in objs])[np.maximum(obj, 0)]
    col = np.array([ob.surfaceColor for ob in objs], float)[np.maximum(obj, 0)]
    d = dirs
    nrm = q["hit_normal"].copy()
    dn = nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1] + nrm[:, 2] * d[:, 2]
    into = ~(dn > 0)
    nrm[~into] = -nrm[~into]
    ddn = d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1] + d[:, 2] * nrm[:, 2]
    nnt = np.where(into, 1.0 / 1.33, 1.33 / 1.0)
    cos2t = 1 - nnt * nnt * (1 - ddn * ddn)
    diffuse = hit & (refl < 1e-4) & (transp < 1e-4)
    mirror = hit & ~diffuse & (transp < 1e-4)
    glass = hit & ~diffuse & ~mirror
    tir = glass & (cos2t < 0)
    want_step = np.select([diffuse, mirror | tir, glass], [HITPOINT, REFLECT, SPLIT], NONE).astype(np.uint8)
    counts = {s: int((want_step == s).sum()) for s in (NONE, HITPOINT, REFLECT, SPLIT)}
    print("steps:", counts, "TIR:", int(tir.sum()), "misses:", int((~untraced & (q["hit_obj"] < 0)).sum()), "not traced:", int(untraced.sum()))
    assert min(counts.values()) >= 64 and (~untraced & (q["hit_obj"] < 0)).sum() >= 64 and dead.sum() >= 64
    assert np.array_equal(step, want_step)
    assert int(got["counters"][_capi.CNT_RAYS]) == int((~untraced).sum()) and int(got["counters"][_capi.CNT_HITPOINTS]) == counts[HITPOINT]
    assert int(got["counters"][_capi.CNT_NODE_TESTS]) == 0 and int(got["counters"][_capi.CNT_TRI_TESTS]) == 0
    # pos, normal, value: main.cpp:68,73-76,88 (the products and sums in trace()'s order; c2 has no texture)
    h3 = hit[:, None]
    assert np.array_equal(got["pos"], np.where(h3, org + d * t[:, None], 0.0))
    assert np.array_equal(got["normal"], np.where(h3, nrm, 0.0))
    assert np.array_equal(got["value"], np.where(diffuse[:, None], col * adj, 0.0))
    # NONE: zeros everywhere
    none = step == NONE
    for k in ("pos", "normal", "value"):
        assert not got[k][none].any(), k
    for k in ("child_org", "child_dir", "child_adj", "child_path", "child_keys"):
        assert not got[k][:n][none].any() and not got[k][n:][none].any(), k
    # the children: present exactly where the step says so; 2p / 2p+1; the parent's key; mirror and TIR throughput
    has_r, has_t = step >= REFLECT, step == SPLIT
    assert np.array_equal((got["child_dir"][:n] != 0).any(axis=1), has_r) and np.array_equal((got["child_dir"][n:] != 0).any(axis=1), has_t)
    assert np.array_equal(got["child_path"][:n], np.where(has_r, path * np.uint32(2), 0).astype(np.uint32))
    assert np.array_equal(got["child_path"][n:], np.where(has_t, path * np.uint32(2) + np.uint32(1), 0).astype(np.uint32))
    assert np.array_equal(got["child_keys"][:n], np.where(has_r, keys, np.uint64(0)))
    assert np.array_equal(got["child_keys"][n:], np.where(has_t, keys, np.uint64(0)))
    for k in ("child_org", "child_adj"):
        assert not got[k][:n][~has_r].any() and not got[k][n:][~has_t].any(), k
    assert np.array_equal(got["child_adj"][:n][mirror], (col * adj)[mirror] * refl[mirror][:, None])
    assert tir.sum() >= 1 and np.array_equal(got["child_adj"][:n][tir], adj[tir])
    eps = 1e-4
    assert np.array_equal(got["child_org"][:n][has_r], (got["pos"] + nrm * eps)[has_r])
    assert np.array_equal(got["child_org"][n:][has_t], (got["pos"] - nrm * eps)[has_t])
    split = step == SPLIT  # Re + (1 - Re) weights: the two children's throughputs add up to f * adj within rounding
    assert np.allclose(got["child_adj"][:n][split] + got["child_adj"][n:][split], (col * adj)[split], rtol=1e-14, atol=0)

    # defaults: adj3 = NULL is (1,1,1), path = NULL is 1; keys = NULL is the derived key
    for k in ARRAYS:
        assert np.array_equal(plain[k], ones[k]), k
    assert np.array_equal(plain["child_path"][:n], np.where(plain["step"] >= REFLECT, 2, 0)) and \
        np.array_equal(plain["child_path"][n:], np.where(plain["step"] == SPLIT, 3, 0))
    dk = default_keys(99, 1000, n)
    assert np.array_equal(nokeys["child_keys"][:n], np.where(has_r, dk, np.uint64(0)))
    assert np.array_equal(nokeys["child_keys"][n:], np.where(has_t, dk, np.uint64(0)))
    for k in ARRAYS:
        if k != "child_keys":
            assert np.array_equal(nokeys[k], got[k]), k
    # three calls of 1, 63 and the remaining rays: the same arrays, every ray keeps its key through first_index
    for k in ARRAYS:
        if k.startswith("child_"):
            joined = np.concatenate([p[k][:len(p["step"])] for p in parts] + [p[k][len(p["step"]):] for p in parts])
        else:
            joined = np.concatenate([p[k] for p in parts])
        assert np.array_equal(joined, nokeys[k]), k
    assert sum(int(p["counters"][_capi.CNT_RAYS]) for p in parts) == int(nokeys["counters"][_capi.CNT_RAYS])


# ---- 3. total internal reflection -------------------------------------------------------------------------------------------
def test_total_internal_reflection(gpu_ready):
    """256 rays that start inside c2's glass sphere and meet its surface beyond the critical angle (sin > 1/1.33 + 0.05): the
    step is REFLECT, the reflected child's throughput is the input adj bit for bit (main.cpp:144), the refracted slot is empty."""
    import cgraytracing_amd as cg
    objs = scenes.scene_c2()
    gi = next(i for i, ob in enumerate(objs) if ob.transparency >= 1e-4)
    C, R = np.array(objs[gi].center, float), float(objs[gi].radius)
    rng = np.random.default_rng(3)
    n = 256
    u = rng.normal(size=(n, 3))
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.sqrt((w * w).sum(axis=1))[:, None]
    sin = rng.uniform(1 / 1.33 + 0.05, 0.98, n)
    cos = np.sqrt(1 - sin * sin)
    d = cos[:, None] * u + sin[:, None] * w
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    org = C + R * u - d * (R * cos)[:, None]  # the middle of the chord that ends at C + R u
    assert (np.sqrt(((org - C) ** 2).sum(axis=1)) < R).all()
    ddn = -(d * u).sum(axis=1)  # against the normal turned towards the ray
    cos2t = 1 - 1.33 * 1.33 * (1 - ddn * ddn)
    sure = cos2t < 0
    assert sure.sum() >= 200, int(sure.sum())
    adj = rng.uniform(0.01, 1.0, (n, 3))
    with cg.Scene(objs) as sc:
        _note(sc, "c2")
        got = _bounce(sc, org, d, adj, rng.integers(1, 1 << 20, n).astype(np.uint32))
    print("TIR: %d of %d rays by construction, steps %s" % (sure.sum(), n, np.bincount(got["step"], minlength=4).tolist()))
    assert (got["hit_obj"][sure] == gi).all()
    assert (got["step"][sure] == REFLECT).all()
    assert np.array_equal(got["child_adj"][:n][sure], adj[sure])
    for k in ("child_org", "child_dir", "child_adj", "child_path", "child_keys"):
        assert not got[k][n:][sure].any(), k
    assert (got["child_dir"][:n][sure] != 0).any(axis=1).all() and not got["value"][sure].any()
    # the normal is turned against the ray (it leaves the glass): it points to the centre
    assert ((got["normal"][sure] * u[sure]).sum(axis=1) < -0.999).all()


# ---- 4. deeper than 5 ------------------------------------------------------------------------------------------------------------
def test_deeper_than_five(gpu_ready):
    """c2 at 48x27 to depth 7, which the full trace does not reach: the Hitpoints with path < 32 are exactly the depth-5 tree's
    (the capture's records), and some root has a Hitpoint beyond it."""
    import cgraytracing_amd as cg
    with cg.Scene(scenes.scene_c2()) as sc:
        _note(sc, "c2")
        org, dirs, keys = sc.camera_rays(48, 27, 1, scenes.cam_dof(), 12345)
        five = check_against_full_trace(sc, org, dirs, keys, 5, "c2 48x27", need=())
        seven = wavefront(sc, org, dirs, keys, 7)
    near = seven["path"] < 32
    print("depth 7: %d Hitpoints, %d of them beyond depth 5 in %d roots, rays per level %s" %
          (len(near), int((~near).sum()), len(np.unique(seven["root"][~near])), seven["per_level"]))
    assert (~near).sum() >= 1 and seven["path"].max() >= 64
    assert near.sum() == len(five["root"])
    for k in ("root", "path", "value", "pos", "normal"):
        assert np.array_equal(seven[k][near], five[k]), k
    assert seven["per_level"][:5] == five["per_level"]


# ---- 5. SPILL rows, STATS and the table ----------------------------------------------------------------------------------------
def _forty_objects():
    """test_gpu_rays.test_more_objects_than_lds_holds's scene of every kind but Bezier"""
    objs = scenes.planes(scenes.stone_small_texture(True)) + scenes.many_spheres(38, 3)[5:]
    objs.insert(9, scenes.TriangleMesh.from_triangles(scenes.pyramid_tris(0.6, (-6.0, -13.0, 36.0)), (0.6, 0.7, 0.9), 0.0, 0.0))
    objs.append(scenes.TriangleMesh.from_triangles(scenes.bunny_tris() * 0.5 + np.tile([6.0, -6.0, 12.0], 3), (1.0, 1.0, 1.0), 0.8, 0.5))
    assert len(objs) == 40
    return objs


SPILL_CASES = [
    ("spheres_1000", lambda: scenes.many_spheres(1000, 11), None, "TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=1", 64, 32),
    ("forty_objects_7_resident", _forty_objects, "7", "TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=1", 64, 48),
]


@pytest.mark.parametrize("name,mk,lds_objs,expect,W,H", SPILL_CASES, ids=[c[0] for c in SPILL_CASES])
def test_more_objects_than_lds_holds(gpu_ready, monkeypatch, name, mk, lds_objs, expect, W, H):
    """Test 1's comparison where objects are read from beyond the LDS list: 1 000 spheres (768 resident), and the 40-object scene
    of every kind with 7 objects resident (the general loop's staging record; the step's materials come through load_mat's
    SPILL path)."""
    import cgraytracing_amd as cg
    if lds_objs:
        monkeypatch.setenv("CGRT_LDS_OBJS", lds_objs)
    with cg.Scene(mk()) as sc:
        v = _note(sc, name)
        assert expect in v, v
        org, dirs, keys = sc.camera_rays(W, H, 1, scenes.cam_dof(), 9)
        check_against_full_trace(sc, org, dirs, keys, 5, name, need=(HITPOINT,))


def test_stats_counters(gpu_ready):
    """CGRT_RAYS_STATS: the same arrays, and the node and triangle tests of one bounce call are the nearest-hit query's for the
    same rays (a lane counts the tests of its own walk)."""
    import cgraytracing_amd as cg
    import torch
    with cg.Scene(scenes.scene_c3(True)) as sc:
        v = _note(sc, "c3_glass_bunny (stats)", stats=True)
        assert "STATS=1" in v, v
        org, dirs, keys = sc.camera_rays(48, 48, 1, scenes.cam_dof(), 12345)
        plain = sc.bounce(org, dirs, keys=keys)
        st = sc.bounce(org, dirs, keys=keys, stats=True)
        q = sc.trace_rays(org, dirs, keys, want=("hit",), stats=True)
        torch.cuda.synchronize()
        for k in ARRAYS:
            assert torch.equal(plain[k], st[k]), k
        c_plain, c_st, c_q = (x["counters"].cpu().numpy() for x in (plain, st, q))
        print("node / triangle tests: bounce %d / %d, nearest-hit query %d / %d" %
              (c_st[_capi.CNT_NODE_TESTS], c_st[_capi.CNT_TRI_TESTS], c_q[_capi.CNT_NODE_TESTS], c_q[_capi.CNT_TRI_TESTS]))
        assert c_plain[_capi.CNT_NODE_TESTS] == 0 and c_plain[_capi.CNT_TRI_TESTS] == 0
        assert c_st[_capi.CNT_NODE_TESTS] == c_q[_capi.CNT_NODE_TESTS] > 0 and c_st[_capi.CNT_TRI_TESTS] == c_q[_capi.CNT_TRI_TESTS] > 0
        assert c_st[_capi.CNT_RAYS] == c_q[_capi.CNT_RAYS] == org.shape[0] and np.array_equal(c_st[:2], c_plain[:2])


# ---- 6. device tensors, out= reuse, a stream of the caller's ------------------------------------------------------------------
def test_tensors_streams_and_host_form(gpu_ready):
    """Preallocated outputs used twice on a stream of our own, counters added to, and the numpy form: the same bits; shapes of
    0, 1, 63, 64 and 65 rays; arguments refused before any launch."""
    import cgraytracing_amd as cg
    import torch
    with cg.Scene(_bezier_scene(True)) as sc:
        _note(sc, "bezier_glass")
        dev = torch.device("cuda", sc.device)
        org, dirs, keys = sc.camera_rays(32, 32, 1, scenes.cam_dof(), 7)
        n = org.shape[0]
        rng = np.random.default_rng(4)
        adj = torch.from_numpy(rng.uniform(0.1, 1.0, (n, 3))).to(dev)
        path = torch.from_numpy(rng.integers(1, 1 << 10, n).astype(np.int32)).to(dev)
        base = sc.bounce(org, dirs, adj, path, keys)
        torch.cuda.synchronize()
        assert int((base["step"] == SPLIT).sum()) >= 16 and int((base["step"] == HITPOINT).sum()) >= 64
        host = sc.bounce_host(org.cpu().numpy(), dirs.cpu().numpy(), adj.cpu().numpy(), path.cpu().numpy().view(np.uint32),
                              keys.cpu().numpy().view(np.uint64))
        for k in ARRAYS:
            h = host[k].view(np.int32) if host[k].dtype == np.uint32 else host[k].view(np.int64) if host[k].dtype == np.uint64 else host[k]
            assert np.array_equal(base[k].cpu().numpy(), h), k
        assert host["nrays"] == n == int(base["counters"][_capi.CNT_RAYS].item())
        assert host["nhp"] == int((base["step"] == HITPOINT).sum()) == int(base["counters"][_capi.CNT_HITPOINTS].item())
        # out= on a stream of our own, twice into the same tensors; counters are added to
        out = {k: torch.full_like(v, 99) for k, v in base.items() if k != "counters"}
        cnt = torch.zeros(8, dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            r1 = sc.bounce(org, dirs, adj, path, keys, out=out, counters=cnt)
            r2 = sc.bounce(org, dirs, adj, path, keys, out=out, counters=cnt, stream=stream.cuda_stream)
        stream.synchronize()
        assert all(r1[k] is out[k] and r2[k] is out[k] for k in out) and r2["counters"] is cnt
        for k in ARRAYS:
            assert torch.equal(out[k], base[k]), k
        assert int(cnt[_capi.CNT_RAYS].item()) == 2 * n
        # 0, 1, 63, 64, 65 rays
        for m in (1, 63, 64, 65):
            part = sc.bounce(org[:m].contiguous(), dirs[:m].contiguous(), adj[:m].contiguous(), path[:m].contiguous(), keys[:m].contiguous())
            for k in ARRAYS:
                want = torch.cat([base[k][:m], base[k][n:n + m]]) if k.startswith("child_") else base[k][:m]
                assert torch.equal(part[k], want), (m, k)
        e = torch.empty((0, 3), dtype=torch.float64, device=dev)
        none = sc.bounce(e, e)
        assert none["step"].shape == (0,) and none["child_org"].shape == (0, 3) and int(none["counters"].sum().item()) == 0
        # refused before any launch
        cnt.zero_()
        bad = [dict(org=org.float()), dict(dirs=dirs[:64].contiguous()), dict(adj=adj.float()), dict(adj=adj[:64].contiguous()),
               dict(path=path.long()), dict(path=path[:64].contiguous()), dict(keys=keys.int()), dict(want=("colour",)), dict(want=()),
               dict(out=dict(step=torch.zeros(n, dtype=torch.int32, device=dev))), dict(out=dict(child_org=out["child_org"][:n]))]
        for kw in bad:
            args = dict(org=org, dirs=dirs, adj=adj, path=path, keys=keys, counters=cnt)
            args.update(kw)
            with pytest.raises(ValueError):
                sc.bounce(**args)
        torch.cuda.synchronize()
        assert int(cnt.sum().item()) == 0


def test_example_wavefront_tinted_glass(gpu_ready, tmp_path):
    """examples/wavefront_tinted_glass.py at a small size: it writes a PNG, reaches depth 8, and with sigma = 0 its depth-5
    image is the full trace's sum, bit for bit."""
    import sys
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import wavefront_tinted_glass as ex
    out = str(tmp_path / "tinted.png")
    W, H = 64, 36
    info = ex.main(out, W=W, H=H, spp=1)
    rgb = np.asarray(Image.open(out).convert("RGB"))
    assert rgb.shape == (H, W, 3) and rgb.max() > rgb.min()
    assert info["levels"] == 8 and info["rays"][0] == W * H and info["rays"][7] > 0 and info["tinted"] > 0, info
    plain = ex.main(str(tmp_path / "plain.png"), W=W, H=H, spp=1, depth=5, sigma=0.0, check=True)
    assert plain["equals_trace_rays"] is True


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_every_table_entry_is_launched(gpu_ready, monkeypatch):
    """Every nearest-hit row of CGRT_RAY_VARIANTS (read from cgrt_variants.h) is launched as a bounce_rays_kernel on a small grid
    of camera rays, STATS included, agrees there with the nearest-hit query and the materials, and nothing outside the table is
    ever asked for -- by this test or by the others of this file."""
    import cgraytracing_amd as cg
    import torch
    import variants
    table = {(t, b, p, s, sp, nt) for t, b, g, p, s, sp, f, nt in variants.ray_variants() if f}
    assert len(table) >= 7
    launches = [(c[0], c[1], False, None) for c in FULL_CASES] + [(c[0], c[1], False, c[2]) for c in SPILL_CASES]
    launches += [("c3_glass_bunny (stats)", lambda: scenes.scene_c3(True), True, None), ("dragon (stats)", scenes.scene_dragon, True, None),
                 ("textured_walls", scenes.scene_textured_walls, False, None), ("room_800", lambda: scenes.room_with_objects(800, 5), False, None)]
    seen = {}
    for label, mk, stats, lds_objs in launches:
        if lds_objs:
            monkeypatch.setenv("CGRT_LDS_OBJS", lds_objs)
        objs = mk()
        with cg.Scene(objs) as sc:
            org, dirs, keys = sc.camera_rays(16, 9, 1, scenes.cam_dof(), 3)
            q = sc.trace_rays(org, dirs, keys, want=("hit",))
            res = sc.bounce(org, dirs, keys=keys, stats=stats)
            torch.cuda.synchronize()
            v = sc.bounce_variant(stats=stats)
            seen.setdefault(tuple(int(p.split("=")[1]) for p in v[v.index("<") + 1:-1].split(",")), label)
            assert int(res["counters"][_capi.CNT_RAYS].item()) == 144
            assert torch.equal(res["hit_obj"], q["hit_obj"]) and torch.equal(res["hit_t"], q["hit_t"]), label
            obj = res["hit_obj"].cpu().numpy()
            diffuse = np.array([o >= 0 and objs[o].reflection < 1e-4 and objs[o].transparency < 1e-4 for o in obj])
            step = res["step"].cpu().numpy()
            assert np.array_equal(step == HITPOINT, diffuse) and np.array_equal(step == NONE, obj < 0), label
        if lds_objs:
            monkeypatch.delenv("CGRT_LDS_OBJS")
    print("\n".join("%s  <- %s" % (v, seen.get(v)) for v in sorted(table)))
    assert set(seen) == table, dict(never_launched=sorted(table - set(seen)), not_in_table=sorted(set(seen) - table))
    assert set(_SEEN) <= table, sorted(set(_SEEN) - table)
