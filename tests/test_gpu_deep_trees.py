"""GPU: full-depth glass ray trees -- the third pending level -- in every kernel that carries the recursion of trace().

trace_grid_body, trace_rays_body and its capture form keep a lane's waiting refracted rays on a stack: two levels in LDS
(kLdsLevels), a third in scratch (`Pending deep[2]`), a register for the sibling of a leaf, the packed word
`depth_left << 8 | path` and the 4-bit `seq` of the capture label.  The third level is used only when the primary ray, its
reflected child and that child's reflected child all split; test_deep_trees_host.py shows from the oracle alone that the scenes
of this file do that on every ray (camera inside a glass sphere) or on more than a tenth of the rays, and that the scenes the
rest of the suite renders almost never do.  Everything here is compared bit for bit with the CPU oracle, except the Bezier
scene, whose bar is test_gpu_parity.BEZ_SCENE_BAR and whose three kernels must agree with each other bit for bit.

Kernel families the scenes select (asserted in test_variants_cover_the_families, printed by every test):
  inside_glass, glass_cluster   planes and spheres   TREES=0, SPH=0, NT=256
  inside_glass_c2               spheres only         SPH=1, NT=256
  inside_glass_mesh             glass mesh, its tree cached in LDS   TREES=1, BEZ=0, NT=256
  inside_glass_spill            769 objects, planes first: the general SPILL body   TREES=1, BEZ=1, SPILL=1, NT=256
  inside_glass_sphere_spill     769 spheres: the sphere loop's SPILL body   SPH=1, SPILL=1, NT=256
  inside_glass_vase             Bezier: one-wave workgroups   TREES=1, BEZ=1, NT=64
Every entry is a GLASS=1 one.  Not reached: the STATS variants (a counter switch, the same stack code; test_gpu_rays
test_stats_counters holds them to the plain variants bit for bit) and the FIRST variants (one scene walk, no stack).

The split-samples mode shares a tile's samples between workgroups only from 32 samples per pixel on (frame_plan), so that one
test renders 32 samples; its reference is the oracle's chunk sums added in chunk order, which is the order
finalize_chunks_kernel documents -- bit for bit as well."""
import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32
from cgraytracing_amd import _capi
from test_deep_trees_host import DEEP_SCENES, H, KLDS, SEED, W, glass_around_camera
from test_gpu_parity import BEZ_SCENE_BAR, _canon, bezier_report
from test_gpu_rays import oracle_nearest, oracle_per_ray

pytestmark = pytest.mark.gpu

FORCE_REORDER = 16  # CGRT_GRID_FORCE_REORDER


def inside_glass_sphere_spill():
    """An all-sphere scene beyond the LDS list, the sphere around the camera last"""
    objs = scenes.many_spheres(KLDS, 31) + [glass_around_camera()]
    assert len(objs) == KLDS + 1
    return objs


NONBEZ = DEEP_SCENES[:-1] + [("inside_glass_sphere_spill", inside_glass_sphere_spill, DEEP_SCENES[0][2])]
NONBEZ_IDS = [c[0] for c in NONBEZ]
VASE = DEEP_SCENES[-1]
assert VASE[0] == "inside_glass_vase"
SPHERE_SCENES = [c for c in NONBEZ if c[0] in ("inside_glass", "inside_glass_c2", "glass_cluster")]

# what the launch tables must select: (substrings of kernel_variant, of rays_variant / capture_variant)
FAMILY = {
    "inside_glass": ("TREES=0,BEZ=0,", "GLASS=1,SPH=0,", "NT=256>"),
    "glass_cluster": ("TREES=0,BEZ=0,", "GLASS=1,SPH=0,", "NT=256>"),
    "inside_glass_c2": ("TREES=0,BEZ=0,", "GLASS=1,SPH=1,", "NT=256>"),
    "inside_glass_mesh": ("TREES=1,BEZ=0,", "GLASS=1,SPH=0,", "NT=256>"),
    "inside_glass_spill": ("TREES=1,BEZ=1,", "GLASS=1,SPH=0,", "SPILL=1"),
    "inside_glass_sphere_spill": ("TREES=0,BEZ=0,", "GLASS=1,SPH=1,", "SPILL=1"),
    "inside_glass_vase": ("TREES=1,BEZ=1,", "GLASS=1,SPH=0,", "NT=64>"),
}

_ORACLE = {}


def oracle_grid(orc, name, mk, cam_name, cam, spp, depth=5, **kw):
    """The oracle's eye pass, computed once per case and shared (read only)"""
    key = (name, cam_name, spp, depth, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        o = BackendScene(orc, mk())
        _ORACLE[key] = o.trace_grid(cam, W, H, spp, depth, SEED, **kw)
        o.close()
    return _ORACLE[key]


def check_family(name, *variants):
    for v in variants:
        print("%s: %s" % (name, v))
        assert all(part in v for part in FAMILY[name]), (name, v)


def eye_exact(got, want, spp, what, ref32=None):
    assert got["nrays"] == want["nrays"], "%s: rays %d vs %d" % (what, got["nrays"], want["nrays"])
    assert np.array_equal(got["nhit"], want["nhit"]), "%s: per-pixel hitpoint counts" % what
    ref = to_acc32(want["acc_sum"], spp) if ref32 is None else ref32
    bad = np.argwhere((got["rgb"] != ref).any(axis=2))
    assert len(bad) == 0, "%s: %d pixels differ, first (row, col) %s: %s vs %s" % (
        what, len(bad), bad[0], got["rgb"][tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("name,mk,cams", NONBEZ, ids=NONBEZ_IDS)
def test_grid_image_order_and_scheduled(gpu_ready, orc, name, mk, cams):
    """cgrt_trace_grid at spp 1 and 2 (image order) and at spp 4 and 6 (the probe, the heavy-tile unit queue and the ordered
    sum; asked for, since scenes without a tree are scheduled only on request; a SPILL launch stays in image order)"""
    import cgraytracing_amd as cg
    spill = "spill" in name
    with cg.Scene(mk()) as sc:
        for cam_name, cam in cams:
            for spp in (1, 2, 4, 6):
                v = sc.kernel_variant(W, H, spp, cam, flags=FORCE_REORDER)
                check_family(name, v)
                assert v.startswith("trace_grid_sched_kernel<" if spp >= 4 and not spill else "trace_grid_kernel<"), v
                got = sc.trace_grid_host(W, H, spp, cam, 5, SEED, force_reorder=True)
                eye_exact(got, oracle_grid(orc, name, mk, cam_name, cam, spp), spp, "%s %s spp %d" % (name, cam_name, spp))


@pytest.mark.parametrize("name,mk,cams", NONBEZ, ids=NONBEZ_IDS)
def test_grid_split_samples(gpu_ready, orc, name, mk, cams):
    """CGRT_GRID_SPLIT_SAMPLES at 32 samples per pixel, the fewest at which it splits: two workgroups per tile with 16
    samples each, their fp64 sums added in chunk order.  The reference is the oracle's two chunk sums added in that order;
    rays and hit counts are the unsplit pass's.  In image order (reorder=False): a scheduled launch sums its heavy tiles
    sample by sample and the others by chunks, and which tiles are heavy is a matter of measured cost.  (A SPILL launch
    ignores the switch: one chunk, the sequential sum.)"""
    import cgraytracing_amd as cg
    spp, chunk = 32, 16
    with cg.Scene(mk()) as sc:
        for cam_name, cam in cams:
            check_family(name, sc.kernel_variant(W, H, spp, cam, flags=4 | 8))
            parts = [oracle_grid(orc, name, mk, cam_name, cam, chunk, sample0=c * chunk) for c in range(spp // chunk)]
            want = dict(nrays=sum(p["nrays"] for p in parts), nhit=parts[0]["nhit"] + parts[1]["nhit"])
            if "spill" in name:
                ref = to_acc32(oracle_grid(orc, name, mk, cam_name, cam, spp)["acc_sum"], spp)
            else:
                ref = to_acc32((0.0 + parts[0]["acc_sum"]) + parts[1]["acc_sum"], spp)
            got = sc.trace_grid_host(W, H, spp, cam, 5, SEED, split_samples=True, reorder=False)
            eye_exact(got, want, spp, "%s %s split samples" % (name, cam_name), ref32=ref)


@pytest.mark.parametrize("name,mk,cams", NONBEZ, ids=NONBEZ_IDS)
def test_grid_two_stripes(gpu_ready, orc, name, mk, cams):
    """Two ranks' block-cyclic stripes of 8 rows, image order (spp 2) and scheduled (spp 4): each rank's rows are the
    oracle's rows, and the ranks' ray counts add up"""
    import cgraytracing_amd as cg
    from cgraytracing_amd.dist import global_row, local_rows
    S, N = 8, 2
    rows = local_rows(H, S, 0, N)
    with cg.Scene(mk()) as sc:
        for cam_name, cam in cams:
            for spp in (2, 4):
                want = oracle_grid(orc, name, mk, cam_name, cam, spp)
                ref = to_acc32(want["acc_sum"], spp)
                nrays = 0
                for r in range(N):
                    check_family(name, sc.kernel_variant(W, H, spp, cam, rows=rows, stripe=(S, r, N), flags=FORCE_REORDER))
                    got = sc.trace_grid_host(W, H, spp, cam, 5, SEED, rows=rows, stripe=(S, r, N), force_reorder=True)
                    g = np.array([global_row(j, S, r, N) for j in range(rows)])
                    assert (g < H).all()
                    assert np.array_equal(got["nhit"], want["nhit"][g]), (name, cam_name, spp, r)
                    assert np.array_equal(got["rgb"], ref[g]), (name, cam_name, spp, r)
                    nrays += got["nrays"]
                assert nrays == want["nrays"]


@pytest.mark.parametrize("name,mk,cams", SPHERE_SCENES, ids=[c[0] for c in SPHERE_SCENES])
def test_grid_tile_order_on_and_off(gpu_ready, orc, name, mk, cams):
    """The image-order launch with its tiles over glass first (tile_order_kernel ran: the order is read back) and row-major"""
    import cgraytracing_amd as cg
    with cg.Scene(mk()) as sc:
        for cam_name, cam in cams:
            for spp in (1, 2):
                want = oracle_grid(orc, name, mk, cam_name, cam, spp)
                for tile_order in (True, False):
                    got = sc.trace_grid_host(W, H, spp, cam, 5, SEED, tile_order=tile_order)
                    order = sc.last_tile_order()
                    assert (order is not None) == tile_order, (name, tile_order)
                    if order is not None:
                        n = ((W + 31) // 32) * ((H + 7) // 8)
                        assert np.array_equal(np.sort(order["list"]), np.arange(n, dtype=np.uint32))
                        print("%s %s: tiles of classes < c: %s" % (name, cam_name, order["plan"].tolist()))
                    eye_exact(got, want, spp, "%s %s spp %d tile_order=%s" % (name, cam_name, spp, tile_order))


def test_grid_every_depth_inside_glass(gpu_ready, orc):
    """max_depth 1 to 5 with the camera inside the sphere: the stack holds 0, 0, 1, 2, 3 rays on every lane
    (test_deep_trees_host.py); depth 1 selects the variant without pending-ray code"""
    import cgraytracing_amd as cg
    name, mk, cams = DEEP_SCENES[0]
    with cg.Scene(mk()) as sc:
        for cam_name, cam in cams:
            for depth in (1, 2, 3, 4, 5):
                for spp in (2, 4):
                    v = sc.kernel_variant(W, H, spp, cam, depth, flags=FORCE_REORDER)
                    print("depth %d spp %d: %s" % (depth, spp, v))
                    assert ("GLASS=1" in v) == (depth > 1), v
                    got = sc.trace_grid_host(W, H, spp, cam, depth, SEED, force_reorder=True)
                    want = oracle_grid(orc, name, mk, cam_name, cam, spp, depth=depth)
                    eye_exact(got, want, spp, "%s %s depth %d spp %d" % (name, cam_name, depth, spp))
                    assert got["nhp"] == W * H * spp * (depth - 1)


def _np(res):
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if "nhit" in out:
        out["nhit"] = out["nhit"].view(np.uint32)
    return out


@pytest.mark.parametrize("name,mk,cams", NONBEZ, ids=NONBEZ_IDS)
def test_trace_rays_per_ray(gpu_ready, orc, name, mk, cams):
    """The camera's rays as a ray list: fp64 acc, nhit and the nearest hit per ray equal the oracle's; a permuted list gives
    the permuted results; a list whose length is no multiple of 64 gives the same per ray"""
    import cgraytracing_amd as cg
    import torch
    spp = 2
    objs = mk()
    with cg.Scene(objs) as sc:
        check_family(name, sc.rays_variant(5))
        for cam_name, cam in cams:
            acc, nhit, nrays = oracle_per_ray(orc, objs, cam, W, H, spp, 5, SEED)
            org, dirs, keys = sc.camera_rays(W, H, spp, cam, SEED)
            n = org.shape[0]
            o, obj, t, nrm = oracle_nearest(orc, objs, org.cpu().numpy(), dirs.cpu().numpy())
            o.close()
            got = _np(sc.trace_rays(org, dirs, keys, max_depth=5, seed=SEED))
            bad = np.nonzero((got["acc"] != acc).any(axis=1))[0]
            assert len(bad) == 0, "%s %s: %d rays differ in fp64, first %d: %s vs %s" % (name, cam_name, len(bad), bad[0], got["acc"][bad[0]], acc[bad[0]])
            assert np.array_equal(got["nhit"], nhit)
            assert int(got["counters"][_capi.CNT_RAYS]) == nrays and int(got["counters"][_capi.CNT_HITPOINTS]) == int(nhit.sum())
            assert np.array_equal(got["hit_obj"], obj) and np.array_equal(got["hit_t"], t) and np.array_equal(got["hit_normal"], nrm)
            perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(org.device)
            shuf = _np(sc.trace_rays(org[perm].contiguous(), dirs[perm].contiguous(), keys[perm].contiguous(), max_depth=5, seed=SEED))
            m = n - 37
            assert m % 64 != 0
            part = _np(sc.trace_rays(org[:m].contiguous(), dirs[:m].contiguous(), keys[:m].contiguous(), max_depth=5, seed=SEED))
            perm = perm.cpu().numpy()
            for k in ("acc", "nhit", "hit_obj", "hit_t", "hit_normal"):
                assert np.array_equal(shuf[k], got[k][perm]), ("permuted", k)
                assert np.array_equal(part[k], got[k][:m]), ("ragged", k)


@pytest.mark.parametrize("name,mk,cams", NONBEZ, ids=NONBEZ_IDS)
def test_hitpoint_captures(gpu_ready, orc, name, mk, cams):
    """cgrt_trace_rays_hitpoints: sorted by label (ray << 4 | seq), seq runs 0 .. nhit - 1 in every ray and the records are the
    oracle's Hitpoint stream in emission order; their f summed in seq order is trace_rays' acc; a short buffer still counts
    everything.  The grid's capture (the eye pass of the photon map) holds the same records."""
    import cgraytracing_amd as cg
    spp = 2
    with cg.Scene(mk()) as sc:
        check_family(name, sc.capture_variant(5))
        vg = sc.kernel_variant(W, H, spp, cams[1][1], hitpoints=True)
        print("%s: %s" % (name, vg))
        assert "TREES=1,BEZ=1," in vg and "GLASS=1" in vg and "HPS=1" in vg
        for cam_name, cam in cams:
            want = oracle_grid(orc, name, mk, cam_name, cam, spp, capture=True)
            assert want["nhp"] == len(want["hp"])
            wray = want["hp_smp"] * (W * H) + want["hp_pix"]
            worder = np.argsort(wray, kind="stable")  # by ray, emission order kept within a ray
            org, dirs, keys = sc.camera_rays(W, H, spp, cam, SEED)
            n = org.shape[0]
            cap = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=5, seed=SEED)
            assert cap["count"] == len(cap["hp"]) == want["nhp"]
            order = np.lexsort([cap["seq"], cap["ray"]])
            ray, seq, hp = cap["ray"][order], cap["seq"][order], cap["hp"][order]
            nhit = np.bincount(wray, minlength=n)
            start = np.concatenate([[0], np.cumsum(nhit)[:-1]])
            assert np.array_equal(ray, wray[worder])
            assert np.array_equal(seq, np.arange(len(ray)) - start[ray]), "seq has gaps or repeats"
            bad = np.nonzero((hp != want["hp"][worder]).any(axis=1))[0]
            assert len(bad) == 0, "%s %s: %d records differ, first: ray %d seq %d" % (name, cam_name, len(bad), ray[bad[0]], seq[bad[0]])
            full = _np(sc.trace_rays(org, dirs, keys, max_depth=5, seed=SEED, want=("acc", "nhit")))
            acc = np.zeros((n, 3))
            for k in range(int(nhit.max())):
                sel = seq == k
                acc[ray[sel]] += hp[sel, 0:3]
            assert np.array_equal(acc, full["acc"]) and np.array_equal(full["nhit"], nhit.astype(np.uint32))
            small = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=5, seed=SEED, cap=100)
            assert small["count"] == want["nhp"] and len(small["hp"]) == 100
            grid = sc.trace_grid_hitpoints(W, H, spp, cam, 5, SEED)
            assert grid["count"] == want["nhp"]
            a, b = _canon(grid["hp"], grid["pix"], grid["smp"]), _canon(want["hp"], want["hp_pix"], want["hp_smp"])
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), "grid capture"
            gorder = np.lexsort([grid["seq"], grid["smp"] * (W * H) + grid["pix"]])
            assert np.array_equal(grid["hp"][gorder], want["hp"][worder]) and np.array_equal(grid["seq"][gorder], seq), "grid capture's seq"


def test_ppm_sessions_inside_glass_c2(gpu_ready, orc):
    """A photon-mapping session over the camera's rays equals the grid session bit for bit, and both the oracle's render"""
    import cgraytracing_amd as cg
    name, mk, cams = DEEP_SCENES[1]
    assert name == "inside_glass_c2"
    nph = 4000
    for cam_name, cam in cams:
        o = BackendScene(orc, mk())
        want = o.ppm(cam, W, H, 1, 5, seed=SEED, nphotons=nph)
        o.close()
        with cg.Scene(mk()) as sc:
            org, dirs, keys = sc.camera_rays(W, H, 1, cam, SEED)
            with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=1, seed=SEED, nphotons=nph) as ses:
                img, hp, inf = ses.image(), ses.hitpoints(), ses.info()
            with sc.ppm_session(W, H, 1, cam, 5, SEED, nphotons=nph) as ses:
                gimg, ghp, ginf = ses.image(), ses.hitpoints(), ses.info()
        assert np.array_equal(img, gimg), cam_name
        assert np.array_equal(hp, ghp), "table order"  # spp 1: the ray index is the pixel index
        assert inf["hp_count"] == ginf["hp_count"] == want["n"] and inf["n_events"] == ginf["n_events"]
        assert np.array_equal(gimg, want["image"]), "%s: %d pixels differ from the oracle" % (cam_name, int((gimg != want["image"]).any(axis=2).sum()))


def test_bezier_vase_inside_glass(gpu_ready, orc):
    """BEZ+GLASS, one-wave workgroups: the path label of every ray of the full tree feeds the key of its Newton start stream.
    The grid (image order at spp 2, scheduled at spp 4), the ray list and the capture agree bit for bit: the capture's f added
    per ray in seq order is trace_rays' acc, and added per pixel in (sample, seq) order, scaled and rounded, it is the grid's
    image.  Against the oracle the bar is test_bezier_scene_vs_oracle's, for the grid per pixel and for the rays per ray."""
    import cgraytracing_amd as cg
    name, mk, cams = VASE
    objs = mk()
    with cg.Scene(objs) as sc:
        for cam_name, cam in cams:
            for spp in (2, 4):
                check_family(name, sc.kernel_variant(W, H, spp, cam), sc.rays_variant(5), sc.capture_variant(5))
                org, dirs, keys = sc.camera_rays(W, H, spp, cam, SEED)
                n = org.shape[0]
                grid = sc.trace_grid_host(W, H, spp, cam, 5, SEED)
                full = _np(sc.trace_rays(org, dirs, keys, max_depth=5, seed=SEED))
                cap = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=5, seed=SEED)
                nhit = full["nhit"].astype(np.int64)
                assert cap["count"] == len(cap["hp"]) == int(nhit.sum()) == grid["nhp"]
                assert int(full["counters"][_capi.CNT_RAYS]) == grid["nrays"]
                order = np.lexsort([cap["seq"], cap["ray"]])
                ray, seq, hp = cap["ray"][order], cap["seq"][order], cap["hp"][order]
                start = np.concatenate([[0], np.cumsum(nhit)[:-1]])
                assert np.array_equal(np.bincount(ray, minlength=n), nhit)
                assert np.array_equal(seq, np.arange(len(ray)) - start[ray])
                acc, pix_sum = np.zeros((n, 3)), np.zeros((H * W, 3))
                for k in range(int(nhit.max())):
                    sel = seq == k
                    acc[ray[sel]] += hp[sel, 0:3]
                assert np.array_equal(acc, full["acc"]), "capture vs ray list"
                for s in range(spp):  # a pixel's Hitpoints in the reference's order: sample by sample, emission order within
                    for k in range(int(nhit.max())):
                        sel = (seq == k) & (ray // (H * W) == s)
                        pix_sum[ray[sel] % (H * W)] += hp[sel, 0:3]
                assert np.array_equal(grid["nhit"], nhit.reshape(spp, H, W).sum(axis=0).astype(np.uint32))
                assert np.array_equal(grid["rgb"], to_acc32(pix_sum.reshape(H, W, 3), spp)), "grid vs capture"
                # the oracle
                want = oracle_grid(orc, name, mk, cam_name, cam, spp)
                frac, linf, gap = bezier_report("inside_glass_vase_%s_spp%d" % (cam_name, spp), grid["rgb"], to_acc32(want["acc_sum"], spp),
                                                grid["nrays"], want["nrays"])
                assert frac >= BEZ_SCENE_BAR[0] and gap <= BEZ_SCENE_BAR[1], (frac, gap)
                if spp == 2:
                    oacc, onhit, onrays = oracle_per_ray(orc, objs, cam, W, H, spp, 5, SEED)
                    err = np.abs(full["acc"] - oacc).max(axis=1)
                    rfrac = 1.0 - float((err >= 1e-4).mean())
                    print("%s %s rays: within 1e-4 %.6f, Linf %.3e, bit-equal %.6f" % (name, cam_name, rfrac, err.max(), float((full["acc"] == oacc).all(axis=1).mean())))
                    assert rfrac >= BEZ_SCENE_BAR[0]


def test_variants_cover_the_families(gpu_ready):
    """Every scene selects a GLASS=1 entry of its family in the three launch tables, and between them the scenes reach the
    sphere, plane-and-sphere, tree, Bezier and both SPILL bodies and both workgroup sizes"""
    import cgraytracing_amd as cg
    seen = set()
    for name, mk, cams in NONBEZ + [VASE]:
        with cg.Scene(mk()) as sc:
            st = sc.stats()
            vs = [sc.kernel_variant(W, H, 2, cams[1][1]), sc.kernel_variant(W, H, 4, cams[1][1], flags=FORCE_REORDER), sc.rays_variant(5),
                  sc.capture_variant(5)]
        check_family(name, *vs)
        assert all("GLASS=1" in v for v in vs)
        seen.add(FAMILY[name])
        if name == "inside_glass_mesh":
            assert st["n_trees"] == 1 and 0 < st["n_nodes"] <= 256, st  # kNodeCache: the tree is staged in LDS
        if "spill" in name:
            assert st["n_objects"] == KLDS + 1
    assert len(seen) == 6
