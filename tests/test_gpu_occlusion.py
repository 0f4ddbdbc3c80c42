"""Occlusion queries on the GPU (cgrt_occlusion_rays): occluded[i] = some object's intersect() length < tmax[i].

The sharp edge is tested against the CPU oracle's composition of intersect() (main.cpp:52-62): tmax is built from the oracle's
own distance t -- half of it, t exactly, the next double above t, twice t, no limit -- so the outcome is fixed by construction
and the strict `<` is met on every hit.  Every wave holds all five kinds: lanes that are done at once, lanes done late and
lanes never done share the walks.  Where the oracle is slow or statistical (Bezier objects, a thousand objects) the same
construction runs on the GPU's own nearest-hit query."""
import os

import numpy as np
import pytest

import scenes
from cgraytracing_amd import _capi
from test_gpu_rays import RANDOM_SCENES, _bezier_scene, oracle_nearest, random_rays

pytestmark = pytest.mark.gpu

NO_LIMIT = 1e10  # the kernels' "no hit yet"
_SEEN = {}       # occlusion_rays_kernel variants launched by the tests of this file -> the scene that did (read by the last test)


def _note(sc, label, stats=False):
    v = sc.occlusion_variant(stats=stats)
    assert v.startswith("occlusion_rays_kernel<"), v
    _SEEN.setdefault(tuple(int(p.split("=")[1]) for p in v[v.index("<") + 1:-1].split(",")), label)
    return v


def _subset(walls):
    """Every 8th ray of random_rays(walls, 2024) and 256 of each of its special groups (axis-parallel, starting on a wall,
    built to miss): 7 768 rays, 121 blocks of 64 and 24 rays."""
    org, dirs, _ = random_rays(walls, 2024)
    idx = np.concatenate([np.arange(0, len(org), 8)] + [g + 2 * np.arange(256) + 1 for g in (50000, 52000, 54000)])
    assert len(idx) <= 8192 and len(idx) % 64 != 0
    return np.ascontiguousarray(org[idx]), np.ascontiguousarray(dirs[idx])


def five_kinds(obj, t):
    """tmax of ray i by i % 5: 0.5 t, t, nextafter(t, inf), 2 t, no limit; no limit for a miss.  Returns (tmax, expected)."""
    kind = np.arange(len(t)) % 5
    tmax = np.choose(kind, [0.5 * t, t, np.nextafter(t, np.inf), 2.0 * t, np.full(len(t), NO_LIMIT)])
    tmax = np.where(obj >= 0, tmax, NO_LIMIT)
    want = ((obj >= 0) & (t < tmax)).astype(np.uint8)
    hits = obj >= 0
    # condition, not measurement: the construction gives 40 % / 60 % of the hits
    assert hits.any() and min(want[hits].mean(), 1.0 - want[hits].mean()) >= 0.30, want[hits].mean()
    assert not want[~hits].any()
    return np.ascontiguousarray(tmax), want


def _gpu(sc, org, dirs, tmax=None, keys=None, **kw):
    import torch
    dev = torch.device("cuda", sc.device)
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    res = sc.occluded(t(org), t(dirs), t(tmax), t(keys), **kw)
    torch.cuda.synchronize()
    return res["occluded"].cpu().numpy(), res["counters"].cpu().numpy()


_ORACLE = {}


def _oracle(orc, key, objs, walls):
    """(org, dirs, oracle hit_obj, hit_t) of the subset for the object list `objs`, computed once per key"""
    if key not in _ORACLE:
        org, dirs = _subset(walls)
        o, obj, t, _ = oracle_nearest(orc, objs, org, dirs)
        o.close()
        _ORACLE[key] = (org, dirs, obj, t)
    return _ORACLE[key]


def _report(name, variant, got, want):
    bad = np.nonzero(got != want)[0]
    print("%s: %s, %d rays, occluded %d, differing %d %s" % (name, variant, len(want), int(want.sum()), len(bad), bad[:10].tolist()))


@pytest.mark.parametrize("name,mk,walls", RANDOM_SCENES, ids=[c[0] for c in RANDOM_SCENES])
def test_sharp_edge_against_oracle(gpu_ready, orc, name, mk, walls):
    import cgraytracing_amd as cg
    objs = mk()
    org, dirs, obj, t = _oracle(orc, name, objs, walls)
    tmax, want = five_kinds(obj, t)
    n = len(org)
    with cg.Scene(objs) as sc:
        variant = _note(sc, name)
        got, cnt = _gpu(sc, org, dirs, tmax)
        _report(name, variant, got, want)
        assert np.array_equal(got, want)
        assert int(cnt[_capi.CNT_RAYS]) == n and int(cnt[_capi.CNT_HITPOINTS]) == 0 and int(cnt[_capi.CNT_WAVE_ITERS]) > 0
        assert int(cnt[_capi.CNT_NODE_TESTS]) == 0 and int(cnt[_capi.CNT_TRI_TESTS]) == 0
        # no limit
        got, cnt = _gpu(sc, org, dirs, None)
        assert np.array_equal(got, (obj >= 0).astype(np.uint8))
        assert int(cnt[_capi.CNT_RAYS]) == n and int(cnt[_capi.CNT_HITPOINTS]) == 0
        # STATS: the same bits; node and triangle tests are counted where the scene has a tree (printed beside the query's)
        _note(sc, name + " (stats)", stats=True)
        got, cnt = _gpu(sc, org, dirs, tmax, stats=True)
        assert np.array_equal(got, want)
        import torch
        dev = torch.device("cuda", sc.device)
        q = sc.trace_rays(torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev), want=("hit",), stats=True)["counters"].cpu().numpy()
        print("%s: node / triangle tests: occlusion %d / %d, nearest-hit query %d / %d" %
              (name, cnt[_capi.CNT_NODE_TESTS], cnt[_capi.CNT_TRI_TESTS], q[_capi.CNT_NODE_TESTS], q[_capi.CNT_TRI_TESTS]))
        if name != "c2":
            assert "STATS=1" in sc.occlusion_variant(stats=True)
            assert int(cnt[_capi.CNT_NODE_TESTS]) > 0 and int(cnt[_capi.CNT_TRI_TESTS]) > 0


SKIP_SCENES = [
    ("c2", scenes.scene_c2, "spheres"),
    ("c3_glass_bunny", lambda: scenes.scene_c3(True), "planes"),
    ("glass_bump_floor", scenes.scene_glass_bump_floor, "planes"),
    ("textured_walls", scenes.scene_textured_walls, "planes"),  # planes and spheres, no tree: the plain variant
]


@pytest.mark.parametrize("name,mk,walls", SKIP_SCENES, ids=[c[0] for c in SKIP_SCENES])
def test_skip_transparent_against_oracle(gpu_ready, orc, name, mk, walls):
    """CGRT_RAYS_SKIP_TRANSPARENT: the oracle's composition over the objects whose transparency is < 1e-4.  The scenes that
    are not among RANDOM_SCENES are also run without the flag (a transparent bump floor's tree; the plain variant)."""
    import cgraytracing_amd as cg
    objs = mk()
    opaque = [ob for ob in objs if ob.transparency < 1e-4]
    assert 0 < len(opaque) < len(objs)
    org, dirs, obj, t = _oracle(orc, name + "/opaque", opaque, walls)
    tmax, want = five_kinds(obj, t)
    with cg.Scene(objs) as sc:
        variant = _note(sc, name)
        got, cnt = _gpu(sc, org, dirs, tmax, skip_transparent=True)
        _report(name + " (skip)", variant, got, want)
        assert np.array_equal(got, want)
        assert int(cnt[_capi.CNT_RAYS]) == len(org)
        got, _ = _gpu(sc, org, dirs, None, skip_transparent=True)
        assert np.array_equal(got, (obj >= 0).astype(np.uint8))
        if name not in [c[0] for c in RANDOM_SCENES]:
            org, dirs, obj, t = _oracle(orc, name, objs, walls)
            tmax, want = five_kinds(obj, t)
            got, _ = _gpu(sc, org, dirs, tmax)
            _report(name, variant, got, want)
            assert np.array_equal(got, want)
        else:
            # the transparent object does block some ray that nothing else blocks in time: the flag is observable
            full = _ORACLE.get(name)
            if full is not None:
                tm_full, want_full = five_kinds(full[2], full[3])
                got_full, _ = _gpu(sc, org, dirs, tm_full)
                got_skip, _ = _gpu(sc, org, dirs, tm_full, skip_transparent=True)
                assert np.array_equal(got_full, want_full) and (got_skip <= got_full).all() and (got_skip < got_full).any()


def _forty_objects():
    """test_gpu_rays.test_more_objects_than_lds_holds's scene of every kind, and a Bezier vase at its end"""
    objs = scenes.planes(scenes.stone_small_texture(True)) + scenes.many_spheres(38, 3)[5:]
    objs.insert(9, scenes.TriangleMesh.from_triangles(scenes.pyramid_tris(0.6, (-6.0, -13.0, 36.0)), (0.6, 0.7, 0.9), 0.0, 0.0))
    objs.append(scenes.TriangleMesh.from_triangles(scenes.bunny_tris() * 0.5 + np.tile([6.0, -6.0, 12.0], 3), (1.0, 1.0, 1.0), 0.8, 0.5))
    objs.append(scenes.vase_bezier())
    return objs


QUERY_SCENES = [
    # name, scene, CGRT_LDS_OBJS, what the variant's name must hold
    ("bezier_mirror", lambda: _bezier_scene(False), None, "BEZ=1,SPH=0,STATS=0,SPILL=0,NT=64"),
    ("bezier_glass", lambda: _bezier_scene(True), None, "BEZ=1,SPH=0,STATS=0,SPILL=0,NT=64"),
    ("spheres_1000", lambda: scenes.many_spheres(1000, 11), None, "TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=1"),
    ("room_800", lambda: scenes.room_with_objects(800, 5), None, "TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=1"),
    ("forty_objects_7_resident", _forty_objects, "7", "TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=1"),
]


@pytest.mark.parametrize("name,mk,lds_objs,expect", QUERY_SCENES, ids=[c[0] for c in QUERY_SCENES])
def test_equals_own_nearest_hit_query(gpu_ready, monkeypatch, name, mk, lds_objs, expect):
    """occluded == hit_obj >= 0 and hit_t < tmax of cgrt_trace_rays on the same rays and keys: camera rays of a 64x32 grid at
    spp 2 with their own keys (the Bezier draws are the query's), the five kinds of tmax built from the query's hit_t; with
    and without CGRT_RAYS_SKIP_TRANSPARENT against each other where the flag cannot matter."""
    import cgraytracing_amd as cg
    import torch
    if lds_objs:
        monkeypatch.setenv("CGRT_LDS_OBJS", lds_objs)
    objs = mk()
    with cg.Scene(objs) as sc:
        variant = _note(sc, name)
        assert expect in variant, variant
        org, dirs, keys = sc.camera_rays(64, 32, 2, scenes.cam_dof(), 7)
        q = sc.trace_rays(org, dirs, keys, want=("hit",))
        torch.cuda.synchronize()
        obj, t = q["hit_obj"].cpu().numpy(), q["hit_t"].cpu().numpy()
        tmax, want = five_kinds(obj, t)
        got, cnt = _gpu(sc, org, dirs, tmax, keys)
        _report(name, variant, got, want)
        assert np.array_equal(got, want)
        assert int(cnt[_capi.CNT_RAYS]) == org.shape[0] and int(cnt[_capi.CNT_HITPOINTS]) == 0
        got, _ = _gpu(sc, org, dirs, None, keys)
        assert np.array_equal(got, (obj >= 0).astype(np.uint8))
        # every kind of object is a blocker somewhere
        kinds = {objs[i].kind for i in np.unique(obj[want == 1])}
        print("%s: blockers' kinds %s" % (name, sorted(kinds)))
        assert kinds == {ob.kind for ob in objs}, kinds
        # CGRT_RAYS_SKIP_TRANSPARENT with tmax just above the nearest hit: a ray whose nearest object is opaque keeps its 1, and
        # the flag only ever takes blockers away
        near = np.ascontiguousarray(np.where(obj >= 0, np.nextafter(t, np.inf), NO_LIMIT))
        full, _ = _gpu(sc, org, dirs, near, keys)
        skip, _ = _gpu(sc, org, dirs, near, keys, skip_transparent=True)
        opaque_first = np.array([o >= 0 and objs[o].transparency < 1e-4 for o in obj])
        assert np.array_equal(full, (obj >= 0).astype(np.uint8))
        assert (skip[opaque_first] == 1).all() and (skip <= full).all()
        if any(not ob.transparency < 1e-4 for ob in objs):
            assert (skip < full).any()


def test_shapes_and_rays_that_are_not_rays(gpu_ready):
    """n of 0, 1, 63, 64, 65; dir == 0 rays give 0 and are not counted; a NaN or <= 0 tmax gives 0 (planes and triangles return
    no length below zero; where a sphere does, test_sharp_edge_against_oracle[c2] holds the answer against the oracle's)."""
    import cgraytracing_amd as cg
    import torch
    objs = scenes.scene_dragon()
    with cg.Scene(objs) as sc:
        dev = torch.device("cuda", sc.device)
        org, dirs, keys = sc.camera_rays(13, 10, 1, scenes.cam_pinhole(), 5)  # 130 rays, every one hits a wall or the dragon
        base, cnt = _gpu(sc, org, dirs)
        assert base.all() and int(cnt[_capi.CNT_RAYS]) == 130
        for n in (1, 63, 64, 65):
            got, cnt = _gpu(sc, org[:n].contiguous(), dirs[:n].contiguous())
            assert got.shape == (n,) and got.all() and int(cnt[_capi.CNT_RAYS]) == n
        e = torch.empty((0, 3), dtype=torch.float64, device=dev)
        none = sc.occluded(e, e)
        assert none["occluded"].shape == (0,) and none["occluded"].dtype == torch.uint8 and int(none["counters"].sum().item()) == 0
        # every third ray is not a ray
        d0 = dirs.clone()
        d0[::3] = 0.0
        got, cnt = _gpu(sc, org, d0)
        want = np.ones(130, np.uint8)
        want[::3] = 0
        assert np.array_equal(got, want) and int(cnt[_capi.CNT_RAYS]) == int(want.sum())
        # tmax that admits nothing, mixed with tmax that admits everything
        bad = np.array([np.nan, 0.0, -0.0, -1.0, -np.inf])
        tm = np.full(130, np.inf)
        tm[::2] = bad[np.arange(65) % 5]
        got, cnt = _gpu(sc, org, dirs, tm)
        want = np.ones(130, np.uint8)
        want[::2] = 0
        assert np.array_equal(got, want) and int(cnt[_capi.CNT_RAYS]) == 130
        # a whole call of them launches and walks nothing
        got, cnt = _gpu(sc, org, dirs, np.full(130, np.nan))
        assert not got.any() and int(cnt[_capi.CNT_WAVE_ITERS]) == 0
        with pytest.raises(ValueError):
            sc.occluded(org, dirs, torch.ones(129, dtype=torch.float64, device=dev))
        with pytest.raises(ValueError):
            sc.occluded(org, dirs.float())
        with pytest.raises(ValueError):
            sc.occluded(org, dirs, out=torch.zeros(130, dtype=torch.int32, device=dev))


def test_independent_of_order_and_split(gpu_ready):
    """A permuted ray set gives the permuted result, split calls (keys; first_index without keys) equal one call, out= and a
    stream of the caller's work, and the host form equals the device form -- on a scene with Bezier draws, where keys matter."""
    import cgraytracing_amd as cg
    import torch
    with cg.Scene(_bezier_scene(False)) as sc:
        dev = torch.device("cuda", sc.device)
        org, dirs, keys = sc.camera_rays(64, 32, 1, scenes.cam_dof(), 7)
        n = org.shape[0]
        q = sc.trace_rays(org, dirs, keys, want=("hit",))
        tmax, want = five_kinds(q["hit_obj"].cpu().numpy(), q["hit_t"].cpu().numpy())
        tm = torch.from_numpy(tmax).to(dev)
        base, _ = _gpu(sc, org, dirs, tm, keys)
        assert np.array_equal(base, want)
        perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(dev)
        shuf, _ = _gpu(sc, org[perm].contiguous(), dirs[perm].contiguous(), tm[perm].contiguous(), keys[perm].contiguous())
        assert np.array_equal(shuf, base[perm.cpu().numpy()])
        cuts = [0, 777, 777 + 64 * 11 + 1, n]
        parts = [_gpu(sc, org[a:b].contiguous(), dirs[a:b].contiguous(), tm[a:b].contiguous(), keys[a:b].contiguous()) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), base)
        assert sum(int(p[1][_capi.CNT_RAYS]) for p in parts) == n
        # without keys the default key is a function of first_index + i
        q3 = sc.trace_rays(org, dirs, None, seed=3, want=("hit",))
        tmax3, want3 = five_kinds(q3["hit_obj"].cpu().numpy(), q3["hit_t"].cpu().numpy())
        tm3 = torch.from_numpy(tmax3).to(dev)
        whole, _ = _gpu(sc, org, dirs, tm3, None, seed=3)
        assert np.array_equal(whole, want3)
        parts = [_gpu(sc, org[a:b].contiguous(), dirs[a:b].contiguous(), tm3[a:b].contiguous(), None, seed=3, first_index=a)[0]
                 for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), whole)
        # out= (a tensor, or a dict as trace_rays takes) on a stream of our own
        stream = torch.cuda.Stream(dev)
        out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            res = sc.occluded(org, dirs, tm, keys, out=out)
            res2 = sc.occluded(org, dirs, tm, keys, out={"occluded": out}, stream=stream.cuda_stream)
        stream.synchronize()
        assert res["occluded"] is out and res2["occluded"] is out and np.array_equal(out.cpu().numpy(), base)
        assert int(res["counters"][_capi.CNT_RAYS].item()) == n
        # the numpy form
        host = sc.occluded_host(org.cpu().numpy(), dirs.cpu().numpy(), tmax, keys.cpu().numpy().view(np.uint64))
        assert np.array_equal(host["occluded"], base) and host["nrays"] == n
        host = sc.occluded_host(org.cpu().numpy(), dirs.cpu().numpy(), None, keys.cpu().numpy().view(np.uint64), skip_transparent=True)
        dev_skip, _ = _gpu(sc, org, dirs, None, keys, skip_transparent=True)
        assert np.array_equal(host["occluded"], dev_skip)


def test_example_shadow_rays(gpu_ready, tmp_path):
    """examples/shadow_rays.py at a small size: it writes a PNG; some hits are in shadow, some are lit."""
    import sys
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import shadow_rays as ex
    out = str(tmp_path / "shadow_rays.png")
    W, H = 64, 36
    info = ex.main(out, W=W, H=H, spp=1)
    rgb = np.asarray(Image.open(out).convert("RGB"))
    assert rgb.shape == (H, W, 3) and rgb.max() > rgb.min()
    assert W * H // 2 < info["shadow_rays"] <= W * H and 0 < info["blocked"] < info["shadow_rays"], info


def _table_variants():
    """The flag tuples (TREES, BEZ, SPH, STATS, SPILL, NT) of the occlusion kernels: one per FIRST entry of CGRT_RAY_VARIANTS,
    read from cgrt_variants.h itself."""
    import variants
    out = variants.occlusion_variants()
    assert len(out) >= 7
    return set(out)


def test_every_table_entry_is_launched(gpu_ready, monkeypatch):
    """Every instantiation of occlusion_rays_kernel (the list is read from the source) is launched on a small grid of camera rays
    by the scenes and flags the tests of this file use, gives the answer of the nearest-hit query there, and nothing outside
    the table is ever asked for."""
    import cgraytracing_amd as cg
    import torch
    launches = [(n, mk, False, None) for n, mk, _ in RANDOM_SCENES] + [(n + " (stats)", mk, True, None) for n, mk, _ in RANDOM_SCENES]
    launches += [(n, mk, False, None) for n, mk, _ in SKIP_SCENES] + [(n, mk, False, lds) for n, mk, lds, _ in QUERY_SCENES]
    seen = {}
    for label, mk, stats, lds_objs in launches:
        if lds_objs:
            monkeypatch.setenv("CGRT_LDS_OBJS", lds_objs)
        with cg.Scene(mk()) as sc:
            org, dirs, keys = sc.camera_rays(16, 9, 1, scenes.cam_dof(), 3)
            q = sc.trace_rays(org, dirs, keys, want=("hit",))
            res = sc.occluded(org, dirs, None, keys, stats=stats)
            torch.cuda.synchronize()
            v = sc.occlusion_variant(stats=stats)
            seen.setdefault(tuple(int(p.split("=")[1]) for p in v[v.index("<") + 1:-1].split(",")), label)
            assert int(res["counters"][_capi.CNT_RAYS].item()) == 144
            assert torch.equal(res["occluded"], (q["hit_obj"] >= 0).to(torch.uint8)), label
        if lds_objs:
            monkeypatch.delenv("CGRT_LDS_OBJS")
    table = _table_variants()
    print("\n".join("%s  <- %s" % (v, seen.get(v)) for v in sorted(table)))
    assert set(seen) == table, dict(never_launched=sorted(table - set(seen)), not_in_table=sorted(set(seen) - table))
    assert set(_SEEN) <= table, sorted(set(_SEEN) - table)
