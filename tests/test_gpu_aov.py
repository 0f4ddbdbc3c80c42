"""Grid AOVs on the GPU (cgrt_trace_grid_aov): a frame's first-hit albedo, normal, depth, coverage and object id.

The contract is a composition of calls that are each pinned to the oracle -- cgrt_camera_rays, the nearest-hit cgrt_trace_rays
without its sign pass, cgrt_ray_hit_attributes' colour -- folded per pixel in sample order: the grid kernel must give its bits.
The frames are 45x19 (partial tiles in both directions at both workgroup sizes) unless a test says otherwise."""
import numpy as np
import pytest

import scenes
from cgraytracing_amd import _capi
from cgraytracing_amd.scene import Sphere, TriangleMesh
from test_gpu_parity import BEZ_SCENE_BAR
from test_gpu_posed_camera import posed
from test_gpu_rays import _bezier_scene

pytestmark = pytest.mark.gpu
W, H, SEED = 45, 19, 12345
NAMES = ("albedo", "normal", "depth", "hits", "obj_id")


def _room_with_mesh():
    mesh = TriangleMesh.from_triangles(scenes.pyramid_tris(1.0, (0.0, -5.0, 30.0)), (0.6, 0.7, 0.9), 0.0, 0.0)
    return scenes.room_with_objects(800, 5, mesh=mesh)


SCENES = {
    "c1_spheres": scenes.scene_c1,
    "c2_glass": scenes.scene_c2,
    "pyramid_glass": lambda: scenes.scene_pyramid(True),
    "dragon_diffuse": scenes.scene_dragon,
    "c3_bunny_glass_chess": lambda: scenes.scene_c3(True),
    "glass_bump_floor": scenes.scene_glass_bump_floor,
    "plain_planes_chess": lambda: scenes.planes(scenes.chessboard_texture(False)),
    "spheres_1000": lambda: scenes.many_spheres(1000, 11),
    "room_800_mesh": _room_with_mesh,
    "bezier_mirror": lambda: _bezier_scene(False),
}
ROWS = {"aov_grid_kernel<TREES=1,BEZ=1,SPH=0,SPILL=0,NT=64>", "aov_grid_kernel<TREES=1,BEZ=0,SPH=0,SPILL=0,NT=256>",
        "aov_grid_kernel<TREES=0,BEZ=0,SPH=1,SPILL=0,NT=256>", "aov_grid_kernel<TREES=0,BEZ=0,SPH=0,SPILL=0,NT=256>",
        "aov_grid_kernel<TREES=0,BEZ=0,SPH=1,SPILL=1,NT=256>", "aov_grid_kernel<TREES=1,BEZ=1,SPH=0,SPILL=1,NT=256>"}
VIEWS = ("pinhole", "lens", "identity", "turned", "lookat")


@pytest.fixture(scope="module")
def committed():
    """name -> the committed scene, built once for the module's tests"""
    import cgraytracing_amd as cg
    made = {}

    def get(name):
        if name not in made:
            made[name] = cg.Scene(SCENES[name]())
        return made[name]

    yield get
    for sc in made.values():
        sc.close()


def camera(view):
    if view in ("pinhole", "lens"):
        return scenes.cam_pinhole() if view == "pinhole" else scenes.cam_dof()
    return posed(scenes.cam_dof(), view)


def aov(sc, cam, w=W, h=H, spp=3, seed=SEED, **kw):
    """trace_grid_aov as numpy (hits as uint32), counters included"""
    import torch
    res = sc.trace_grid_aov(w, h, spp, cam, seed, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if "hits" in out:
        out["hits"] = out["hits"].view(np.uint32)
    return out


def composed(sc, cam, w=W, h=H, spp=3, seed=SEED, sample_offset=0, spp_total=None, **kw):
    """The contract, in numpy: the camera's rays, their nearest hits without the sign pass and the colours there, the normal
    turned against the ray, summed per pixel in fp64 in sample order from +0.0, scaled by 1 / spp_total and rounded once."""
    import torch
    org, dirs, keys = sc.camera_rays(w, h, spp, cam, seed, sample_offset=sample_offset, **kw)
    hit = sc.trace_rays(org, dirs, keys, seed=seed, want=("hit",), sign_pass=False)
    col = sc.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=("color",))
    torch.cuda.synchronize()
    rows = org.shape[0] // (spp * w)
    d = dirs.cpu().numpy().reshape(spp, rows, w, 3)
    ids = hit["hit_obj"].cpu().numpy().reshape(spp, rows, w)
    t = hit["hit_t"].cpu().numpy().reshape(spp, rows, w)
    n = hit["hit_normal"].cpu().numpy().reshape(spp, rows, w, 3)
    c = col["color"].cpu().numpy().reshape(spp, rows, w, 3)
    is_hit = ids >= 0
    nd = scenes.ref_dot(n, d)
    # a condition on the inputs, not a tolerance: the flip is undefined up to sign where the ray grazes
    assert not (is_hit & (nd == 0.0)).any(), "a traced ray has dot(n, d) == 0 exactly"
    m = np.where((nd > 0)[..., None], -n, n)
    alb, nrm, dep = np.zeros((rows, w, 3)), np.zeros((rows, w, 3)), np.zeros((rows, w))
    for k in range(spp):  # (a miss adds +0.0, which changes no sum that started from +0.0)
        alb = alb + np.where(is_hit[k][..., None], c[k], 0.0)
        nrm = nrm + np.where(is_hit[k][..., None], m[k], 0.0)
        dep = dep + np.where(is_hit[k], t[k], 0.0)
    inv = 1.0 / float(spp_total if spp_total else spp)
    return dict(albedo=(alb * inv).astype(np.float32), normal=(nrm * inv).astype(np.float32), depth=(dep * inv).astype(np.float32),
                hits=is_hit.sum(axis=0).astype(np.uint32), obj_id=np.where(is_hit[0], ids[0], -1).astype(np.int32), traced=int((d != 0).any(axis=-1).sum()))


def assert_same(got, want, what):
    for k in NAMES:
        bad = np.argwhere(got[k] != want[k])
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


# ---- 1. the composition identity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SCENES if n != "bezier_mirror"])
def test_aov_is_the_composition_bit_for_bit(gpu_ready, committed, name):
    """Every scene class but Bezier under the pinhole, the thin lens and the identity, TURNED and look-at poses: all five buffers
    equal the composition at spp 3, sample_offset 2, spp_total 7; the identity pose equals the unposed call; the rays counted
    are the image's."""
    sc = committed(name)
    for view in VIEWS:
        cam = camera(view)
        want = composed(sc, cam, spp=3, sample_offset=2, spp_total=7)
        got = aov(sc, cam, spp=3, sample_offset=2, spp_total=7)
        print(name, view, sc.aov_variant(W, H, cam), "hits", int(got["hits"].sum()), "of", want["traced"])
        assert_same(got, want, (name, view))
        assert int(got["counters"][_capi.CNT_RAYS]) == want["traced"] == 3 * W * H
        assert int(got["counters"][_capi.CNT_HITPOINTS]) == 0
        assert got["hits"].sum() > 0
        if view == "identity":
            assert_same(got, aov(sc, scenes.cam_dof(), spp=3, sample_offset=2, spp_total=7), (name, "identity pose"))


def test_every_row_of_the_list_is_launched(gpu_ready, committed):
    """The names aov_variant reports over this file's scenes are the six rows of CGRT_AOV_VARIANTS, each the nearest-hit row
    rays_variant reports for the same scene."""
    seen = {}
    for name in SCENES:
        sc = committed(name)
        v = sc.aov_variant(W, H)
        seen.setdefault(v, name)
        r = sc.rays_variant(1, want=("hit",))
        flags = dict(p.split("=") for p in r[r.index("<") + 1:-1].split(","))
        assert flags["FIRST"] == "1" and flags["STATS"] == "0" and flags["GLASS"] == "0"
        assert v == "aov_grid_kernel<TREES=%s,BEZ=%s,SPH=%s,SPILL=%s,NT=%s>" % tuple(flags[k] for k in ("TREES", "BEZ", "SPH", "SPILL", "NT")), (name, v, r)
    print("\n".join("%s  <- %s" % kv for kv in sorted(seen.items())))
    assert set(seen) == ROWS


# ---- 2. the Bezier row ------------------------------------------------------------------------------------------------
BEZ_SCENES = [("mirror_vase", lambda: _bezier_scene(False)), ("glass_vase", lambda: _bezier_scene(True)),
              ("c5", lambda: scenes.scene_c5(scenes.stone_small_texture(True)))]


@pytest.mark.parametrize("name,mk", BEZ_SCENES, ids=[b[0] for b in BEZ_SCENES])
def test_bezier_row_against_the_composition(gpu_ready, name, mk):
    """C5-shaped scenes, 96x96 spp 2 under the lens, seed 7 (test_bezier_scene_vs_oracle's frame): whether Newton's outcome is
    independent of which 64 rays share a wave across the two kernels is not known, so the bar is the project's
    BEZ_SCENE_BAR[0] -- the fraction of pixels with all five buffers bit-equal to the composition.  The count is printed."""
    import cgraytracing_amd as cg
    with cg.Scene(mk()) as sc:
        cam = scenes.cam_dof()
        variant = sc.aov_variant(96, 96, cam)
        want = composed(sc, cam, 96, 96, 2, 7)
        got = aov(sc, cam, 96, 96, 2, 7)
    same = np.ones((96, 96), bool)
    for k in NAMES:
        e = got[k] == want[k]
        same &= e.all(axis=-1) if e.ndim == 3 else e
    vase = int((want["obj_id"] == int(want["obj_id"].max())).sum())
    print("%s: %s, %d of %d pixels bit-equal in all five buffers (%.6f), %d pixels see the vase first" %
          (name, variant, int(same.sum()), same.size, same.mean(), vase))
    assert variant == "aov_grid_kernel<TREES=1,BEZ=1,SPH=0,SPILL=0,NT=64>"
    assert vase > 50, "no primary ray reaches the vase"
    assert same.mean() >= BEZ_SCENE_BAR[0]
    assert int(got["counters"][_capi.CNT_RAYS]) == 2 * 96 * 96


# ---- 3. the anchor to the oracle-pinned eye pass ----------------------------------------------------------------------
def test_albedo_is_the_eye_pass_where_nothing_reflects(gpu_ready):
    """A room with a textured floor, diffuse spheres and the diffuse pyramid: every ray tree is its primary Hitpoint with adj = 1,
    so at max_depth 5 and spp 3 trace_grid's rgb IS the albedo and its nhit the coverage, bit for bit."""
    import cgraytracing_amd as cg
    import torch
    objs = scenes.planes(scenes.chessboard_texture(False)) + [
        Sphere((-9.0, -14.0, 26), 6, (0.9, 0.3, 0.2), 0.0, 0.0), Sphere((11.0, -15.0, 22), 5, (0.2, 0.8, 0.4), 0.0, 0.0),
        TriangleMesh.from_triangles(scenes.pyramid_tris(1.0, (0.0, -5.0, 30.0)), (0.6, 0.7, 0.9), 0.0, 0.0)]
    with cg.Scene(objs) as sc:
        for cam in (scenes.cam_pinhole(), scenes.cam_dof()):
            rgb, nhit, _ = sc.trace_grid(W, H, 3, cam, 5, SEED)
            torch.cuda.synchronize()
            got = aov(sc, cam, spp=3)
            assert np.array_equal(got["albedo"], rgb.cpu().numpy())
            assert np.array_equal(got["hits"], nhit.cpu().numpy().view(np.uint32))
            assert len(np.unique(got["obj_id"])) >= 6 and got["hits"].min() == 3  # a closed room: every sample hits


# ---- 4. ACCUMULATE ------------------------------------------------------------------------------------------------------
def test_accumulate_adds_in_fp32(gpu_ready, committed):
    """Passes (sample_offset 0, spp 2) and (sample_offset 2, spp 3, accumulate) at spp_total 5 into the same buffers: the float
    buffers are the fp32 sum of the two passes rendered separately, hits their sum, obj_id sample 2's."""
    import torch
    sc, cam = committed("c2_glass"), scenes.cam_dof()
    a = aov(sc, cam, spp=2, sample_offset=0, spp_total=5)
    b = aov(sc, cam, spp=3, sample_offset=2, spp_total=5)
    res = sc.trace_grid_aov(W, H, 2, cam, SEED, sample_offset=0, spp_total=5)
    out = {k: res[k] for k in NAMES}
    sc.trace_grid_aov(W, H, 3, cam, SEED, sample_offset=2, spp_total=5, out=out, accumulate=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("albedo", "normal", "depth"):
        assert np.array_equal(got[k], a[k] + b[k]), k  # (numpy adds float32 arrays in float32)
        assert (a[k] + b[k]).dtype == np.float32
    assert np.array_equal(got["hits"].view(np.uint32), a["hits"] + b["hits"])
    assert np.array_equal(got["obj_id"], b["obj_id"])
    assert (a["obj_id"] != b["obj_id"]).any(), "the two passes' first samples see the same objects everywhere"
    # buffers the call makes itself start from zero
    c = aov(sc, cam, spp=3, sample_offset=2, spp_total=5, accumulate=True)
    assert_same(c, b, "accumulate into fresh buffers")


# ---- 5. stripes ---------------------------------------------------------------------------------------------------------
def test_striped_rows_and_padding(gpu_ready, committed):
    """67x45, rows=16, stripe=(8, 2, 3) -- share 2 of 3 in stripes of 8 rows: local rows 0-7 are global rows 16-23, local rows
    8-15 global rows 40-47, of which 45-47 lie beyond the image.  The rows inside equal the contiguous frame's, the three
    padding rows are zero and -1; under accumulate the padding rows are left as they were."""
    import torch
    for name in ("c2_glass", "dragon_diffuse"):
        sc, cam = committed(name), scenes.cam_dof()
        full = aov(sc, cam, 67, 45, spp=2)
        part = aov(sc, cam, 67, 45, spp=2, rows=16, stripe=(8, 2, 3))
        for k in NAMES:
            assert part[k].shape[:2] == (16, 67)
            assert np.array_equal(part[k][:8], full[k][16:24]), (name, k)
            assert np.array_equal(part[k][8:13], full[k][40:45]), (name, k)
            assert (part[k][13:] == (-1 if k == "obj_id" else 0)).all(), (name, k)
        assert int(part["counters"][_capi.CNT_RAYS]) == 2 * 67 * 13
        dev = torch.device("cuda", sc.device)
        out = dict(albedo=torch.full((16, 67, 3), 7.0, dtype=torch.float32, device=dev), depth=torch.full((16, 67), 7.0, dtype=torch.float32, device=dev),
                   hits=torch.full((16, 67), 7, dtype=torch.int32, device=dev), obj_id=torch.full((16, 67), 7, dtype=torch.int32, device=dev))
        sc.trace_grid_aov(67, 45, 2, cam, SEED, rows=16, stripe=(8, 2, 3), want=tuple(out), out=out, accumulate=True)
        torch.cuda.synchronize()
        for k, v in out.items():
            v = v.cpu().numpy()
            assert (v[13:] == 7).all(), (name, k)
            if k != "obj_id":
                assert np.array_equal(v[:13].view(part[k].dtype), (part[k][:13] + np.asarray(7, part[k].dtype))), (name, k)
            else:
                assert np.array_equal(v[:13], part[k][:13])


# ---- 6. counters and the handle's state -----------------------------------------------------------------------------------
def test_counters_and_handle_state(gpu_ready):
    """CGRT_CNT_RAYS grows by spp x the pixels inside the image and _HITPOINTS not at all, on counters that already hold
    something; what a preceding trace_grid left in the handle -- whether its tile order was reused, the eye kernels it launched
    -- reads the same after the AOV call, and the next trace_grid reuses the cached order as if nothing had run between."""
    import cgraytracing_amd as cg
    import torch
    with cg.Scene(scenes.scene_c2()) as sc:
        cam = scenes.cam_dof()
        sc.trace_grid(96, 54, 4, cam, 5, SEED)
        rgb, _, cnt = sc.trace_grid(96, 54, 4, cam, 5, SEED)
        torch.cuda.synchronize()
        reused, launches = sc.last_tile_order_reused(), sc.last_eye_launches()
        before = cnt.cpu().numpy().copy()
        res = sc.trace_grid_aov(W, H, 3, cam, SEED, counters=cnt)
        none = sc.trace_grid_aov(W, H, 3, cam, SEED, want=("hits",), out=dict(hits=res["hits"]), counters=cnt, stream=0)
        torch.cuda.synchronize()
        after = cnt.cpu().numpy()
        assert after[_capi.CNT_RAYS] - before[_capi.CNT_RAYS] == 2 * 3 * W * H
        assert after[_capi.CNT_HITPOINTS] == before[_capi.CNT_HITPOINTS] and before[_capi.CNT_HITPOINTS] > 0
        assert after[_capi.CNT_WAVE_ITERS] > before[_capi.CNT_WAVE_ITERS]
        assert (after[3:] == before[3:]).all()
        assert none["hits"] is res["hits"]
        assert sc.last_tile_order_reused() == reused and np.array_equal(sc.last_eye_launches(), launches)
        again, _, _ = sc.trace_grid(96, 54, 4, cam, 5, SEED)
        torch.cuda.synchronize()
        assert sc.last_tile_order_reused() == reused and np.array_equal(sc.last_eye_launches(), launches)
        assert torch.equal(again, rgb)
        # only the arrays asked for are written
        only = aov(sc, cam, want=("depth", "obj_id"))
        assert sorted(only) == ["counters", "depth", "obj_id"]
        assert_same(dict(aov(sc, cam), **only), aov(sc, cam), "a subset of the buffers")


# ---- the host layers' examples ----------------------------------------------------------------------------------------------
def test_cpp_host_wrapper_render_aov(gpu_ready):
    """examples/aov_host.cpp over include/cgrt_host.hpp's render_aov and DeformingScene::render_aov: the program checks every
    pixel's albedo, depth and normal against the scene it built (two planes, a diffuse and a glass sphere)."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cgraytracing_amd", "cgrt_aov_host")
    assert os.path.exists(exe), "build it with make -C cgraytracing_amd/csrc all"
    out = subprocess.run([exe, "--width", "45", "--height", "35"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: 1575 pixels -- floor "), out.stdout


def test_example_aov_buffers(gpu_ready, tmp_path):
    """examples/aov_buffers.py at a small size: three PNGs, one ray per sample, and C2's mirror and glass spheres among the
    objects first seen (its diffuse sphere stands behind them, at z = 60 below the floor sphere's horizon)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import aov_buffers
    got = aov_buffers.main(str(tmp_path / "aov"), 96, 54, 2)
    assert got["rays"] == 2 * 96 * 54 and {6, 7} <= set(got["objects"]) and -1 not in got["objects"]
    for k in ("albedo", "normal", "depth"):
        assert os.path.getsize(str(tmp_path / ("aov_%s.png" % k))) > 200
