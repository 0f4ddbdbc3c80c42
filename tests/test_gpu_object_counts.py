"""GPU: scenes of 255 to 1 100 top-level objects against the CPU oracle, on every launch whose LDS grows with the object count.

Up to kLdsObjsMax = 768 objects are staged in LDS by every workgroup; the SPILL variants read the rest from HBM.  How many fit
depends on what else a launch keeps in LDS, so the counts below straddle each launch family's limit.  The arithmetic, from
cgrt_types.h / cgrt_wg_lds.h / cgrt_bezier.hpp: ObjRec 128 B; pending-ray levels 2 x 19 456 = 38 912 B; BezLds 7 872 B, one
per wave (4 waves); the cached tree <= 256 x 32 B (the glass bunny's 255 nodes: 8 160 B; an opaque mesh's triangle-level
hierarchy is larger and not cached); the wide walk's stack 256 x 16 x 8 = 32 768 B; a workgroup may use 163 840 B, its
kernel's static __shared__ included (the eye kernels: S = 336 B).

  * 255 / 257: 256 objects are 32 768 B, so beside the wide walk's 32 KiB stack (primary_walk_kernel finishing units) 257
    objects pass the 64 KiB that needs the dynamic-LDS opt-in and 255 do not.
  * 600: past the opt-in on every family, below every other limit.
  * The most general variant (Hitpoint capture, so ppm_render's eye pass too; the eye pass beyond 768 objects unless all are
    spheres) needs R*128 + 38 912 + 4*7 872 + nodes + S <= 163 840 for R resident objects:
      without a cached tree  R <= (163 840 - 70 400 - 336) / 128 = 727  -> 727 / 728, and 730 / 732;
      with the glass bunny's R <= (163 840 - 78 560 - 336) / 128 = 663  -> 663 / 664, and 666 / 668.
    Beyond that it keeps R - 4 objects (723 / 659) in LDS beside one staging record per wave and runs SPILL.  Before that fix
    these launches asked for the whole list (up to 169 216 B beyond 768 objects, 177 376 B with the glass bunny) and could not start.
  * 768 / 769: kLdsObjsMax, the spill boundary of every other launch.
  * 1 100: far beyond it.

Exact duplicates of a sphere straddle 256, 659, 723, 730 and 768 (the earlier object must win: main.cpp:57).  Every case
asserts which kernel variant ran (kernel_variant), so that a change of the thresholds cannot turn one case into a copy of
another; none of them lowers the resident count through CGRT_LDS_OBJS."""
import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32
from test_gpu_parity import BEZ_SCENE_BAR, _canon, bezier_report

pytestmark = pytest.mark.gpu

W, H, SEED = 64, 48, 9
KLDS = 768  # kLdsObjsMax
CAPTURE_MAX = {"plain": 727, "bunny": 663}  # the general variant's resident limit without / with the glass bunny's cached tree
DUPS = [(255, 257), (658, 660), (722, 724), (729, 731), (767, 769)]
PPM = dict(W=48, H=36, nphotons=3000)


def _bunny(glass):
    return scenes.TriangleMesh.from_triangles(scenes.bunny_tris() * 0.5 + np.tile([6.0, -6.0, 12.0], 3), (1.0, 1.0, 1.0),
                                              0.8 if glass else 0.0, 0.5 if glass else 0.0)


def _pyramid():
    return scenes.TriangleMesh.from_triangles(scenes.pyramid_tris(0.6, (-6.0, -13.0, 36.0)), (0.6, 0.7, 0.9), 0.0, 0.0)


def _vase():
    return scenes.vase_bezier()


def _scene(kind, n):
    if kind == "A":
        return scenes.room_with_objects(n, 100 + n, dup_pairs=DUPS)
    if kind == "B":
        return scenes.room_with_objects(n, 200 + n, mesh=_bunny(False), dup_pairs=DUPS)
    if kind == "C":
        return scenes.room_with_objects(n, 300 + n, mesh=_pyramid(), floor_tex=scenes.stone_small_texture(True), dup_pairs=DUPS)
    if kind == "D":
        return scenes.room_with_objects(n, 400 + n, mesh=_bunny(True), dup_pairs=DUPS)
    if kind == "E":
        return scenes.room_with_objects(n, 500 + n, mesh=_vase(), dup_pairs=DUPS)
    if kind == "F":
        return scenes.room_with_objects(n, 600 + n, mesh=_bunny(False), dup_pairs=DUPS)
    raise ValueError(kind)


def _eye_exact(got, want, spp, what):
    assert got["nrays"] == want["nrays"], "%s: rays %d vs %d" % (what, got["nrays"], want["nrays"])
    assert np.array_equal(got["nhit"], want["nhit"]), "%s: per-pixel hitpoint counts" % what
    ref = to_acc32(want["acc_sum"], spp)
    assert np.array_equal(got["rgb"], ref), "%s: %d pixels differ" % (what, int((got["rgb"] != ref).any(axis=2).sum()))


def _capture_exact(sc, want, cam, spp, what):
    """want: the oracle's trace with capture=True.  Identical multisets of {f, pos, normal} records, bit for bit."""
    r = sc.trace_grid_hitpoints(W, H, spp, cam, 5, SEED)
    assert r["count"] == len(want["hp"]), "%s: %d hitpoints vs %d" % (what, r["count"], len(want["hp"]))
    a = _canon(r["hp"], r["pix"], r["smp"])
    b = _canon(want["hp"], want["hp_pix"], want["hp_smp"])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "%s: hitpoint pixels / samples" % what
    assert np.array_equal(a[0], b[0]), "%s: hitpoint records differ" % what


def _ppm_exact(sc, o, what):
    cam = scenes.cam_pinhole()
    want = o.ppm(cam, PPM["W"], PPM["H"], 1, 5, nphotons=PPM["nphotons"])
    got = sc.ppm_render(PPM["W"], PPM["H"], 1, cam, 5, 12345, nphotons=PPM["nphotons"])
    nd = int((got["image"] != want["image"]).any(axis=2).sum())
    print("%s: ppm_render hitpoints %d vs %d, %d pixels differ" % (what, got["count"], want["n"], nd))
    assert got["count"] == want["n"] and nd == 0, what


def _capture_spills(sc, n, cam, spp, tree):
    """The Hitpoint capture's variant: SPILL exactly when n passes the general variant's resident limit."""
    v = sc.kernel_variant(W, H, spp, cam, hitpoints=True)
    assert v.startswith("trace_grid_kernel<TREES=1,BEZ=1,") and "HPS=1" in v, v
    assert ("SPILL=1" in v) == (n > CAPTURE_MAX[tree]), (n, v)
    return "SPILL=1" in v


def _eye_variant(sc, n, spp, cam, sched, flags=0):
    """cgrt_trace_grid's variant: SPILL beyond kLdsObjsMax (image order, the general body unless all are spheres), else the
    scheduled form when `sched`, else image order."""
    v = sc.kernel_variant(W, H, spp, cam, flags=flags)
    if n > KLDS:
        assert v.startswith("trace_grid_kernel<TREES=1,BEZ=1,") and v.endswith("SPILL=1>"), (n, v)
    else:
        assert "SPILL" not in v and v.startswith("trace_grid_sched_kernel" if sched else "trace_grid_kernel"), (n, v)
    return v


FORCE_REORDER = 16  # CGRT_GRID_FORCE_REORDER


@pytest.mark.parametrize("n", [255, 257, 600, 666, 668, 727, 728, 730, 732, 768, 769, 1100])
def test_room_and_spheres(gpu_ready, orc, n):
    """A: the room's five planes and spheres of all three materials, n objects: the eye pass in image order (spp 2) and
    scheduled (spp 4, forced: a scene of planes and spheres is left in image order by default), the Hitpoint capture, and at
    four counts ppm_render, whose eye pass is the capture."""
    import cgraytracing_amd as cg
    objs = _scene("A", n)
    cam = scenes.cam_dof()
    o = BackendScene(orc, objs)
    want2 = o.trace_grid(cam, W, H, 2, 5, SEED, capture=True)
    want4 = o.trace_grid(cam, W, H, 4, 5, SEED)
    with cg.Scene(objs) as sc:
        _eye_variant(sc, n, 2, cam, sched=False)
        _eye_exact(sc.trace_grid_host(W, H, 2, cam, 5, SEED), want2, 2, "A%d image order" % n)
        _eye_variant(sc, n, 4, cam, sched=True, flags=FORCE_REORDER)
        _eye_exact(sc.trace_grid_host(W, H, 4, cam, 5, SEED, force_reorder=True), want4, 4, "A%d scheduled" % n)
        spill = _capture_spills(sc, n, cam, 2, "plain")
        _capture_exact(sc, want2, cam, 2, "A%d capture" % n)
        if n in (600, 732, 769, 1100):
            assert _capture_spills(sc, n, scenes.cam_pinhole(), 1, "plain") == spill
            _ppm_exact(sc, o, "A%d" % n)
    o.close()


@pytest.mark.parametrize("n", [257, 600, 666, 668, 727, 728, 732, 768, 769, 1100])
def test_room_opaque_bunny_and_spheres(gpu_ready, orc, n):
    """B: the room, an opaque bunny and spheres.  At spp 4 the scheduled launch: the probe, the heavy-tile unit queue,
    primary_walk_kernel finishing units (all n objects staged beside its 32 KiB stack: past 64 KiB from 257 objects on) and
    the light tiles on the second stream; image order at spp 2; the capture (the opaque bunny's triangle-level hierarchy is
    too large for the node cache, so its limit is the plain one); ppm_render at two counts."""
    import cgraytracing_amd as cg
    objs = _scene("B", n)
    cam = scenes.cam_dof()
    o = BackendScene(orc, objs)
    want2 = o.trace_grid(cam, W, H, 2, 5, SEED, capture=True)
    want4 = o.trace_grid(cam, W, H, 4, 5, SEED)
    with cg.Scene(objs) as sc:
        _eye_variant(sc, n, 4, cam, sched=True)
        _eye_exact(sc.trace_grid_host(W, H, 4, cam, 5, SEED), want4, 4, "B%d scheduled" % n)
        _eye_variant(sc, n, 2, cam, sched=False)
        _eye_exact(sc.trace_grid_host(W, H, 2, cam, 5, SEED), want2, 2, "B%d image order" % n)
        _capture_spills(sc, n, cam, 2, "plain")
        _capture_exact(sc, want2, cam, 2, "B%d capture" % n)
        if n in (728, 769):
            _capture_spills(sc, n, scenes.cam_pinhole(), 1, "plain")
            _ppm_exact(sc, o, "B%d" % n)
    o.close()


@pytest.mark.parametrize("n", [257, 768, 769])
def test_bump_floor_pyramid_and_spheres(gpu_ready, orc, n):
    """C: the room with the bump-mapped stone floor, an opaque pyramid and spheres, spp 4: primary_walk_kernel filling the
    table only (a bump floor: finish = 0) and the light variant that runs only the height-field walk; SPILL at 769."""
    import cgraytracing_amd as cg
    objs = _scene("C", n)
    cam = scenes.cam_dof()
    o = BackendScene(orc, objs)
    want = o.trace_grid(cam, W, H, 4, 5, SEED)
    o.close()
    with cg.Scene(objs) as sc:
        _eye_variant(sc, n, 4, cam, sched=True)
        _eye_exact(sc.trace_grid_host(W, H, 4, cam, 5, SEED), want, 4, "C%d" % n)


@pytest.mark.parametrize("n", [663, 664, 666, 668, 768, 769])
def test_glass_bunny_and_spheres(gpu_ready, orc, n):
    """D: a glass bunny (its 255-node tree cached in LDS; pending-ray levels beside up to 768 objects), the room and spheres:
    the eye pass at spp 4 (scheduled) and spp 2 (image order), SPILL at 769; the capture, whose limit the cached tree lowers
    to 663 resident objects; ppm_render at two counts."""
    import cgraytracing_amd as cg
    objs = _scene("D", n)
    cam = scenes.cam_dof()
    o = BackendScene(orc, objs)
    want2 = o.trace_grid(cam, W, H, 2, 5, SEED, capture=True)
    want4 = o.trace_grid(cam, W, H, 4, 5, SEED)
    with cg.Scene(objs) as sc:
        v = _eye_variant(sc, n, 4, cam, sched=True)
        assert "GLASS=1" in v
        _eye_exact(sc.trace_grid_host(W, H, 4, cam, 5, SEED), want4, 4, "D%d scheduled" % n)
        _eye_variant(sc, n, 2, cam, sched=False)
        _eye_exact(sc.trace_grid_host(W, H, 2, cam, 5, SEED), want2, 2, "D%d image order" % n)
        _capture_spills(sc, n, cam, 2, "bunny")
        _capture_exact(sc, want2, cam, 2, "D%d capture" % n)
        if n in (664, 769):
            _capture_spills(sc, n, scenes.cam_pinhole(), 1, "bunny")
            _ppm_exact(sc, o, "D%d" % n)
    o.close()


@pytest.mark.parametrize("n", [257, 769])
def test_bezier_vase_and_spheres(gpu_ready, orc, n):
    """E: the Bezier vase, the room and spheres at spp 4: one-wave workgroups (BezLds beside the object list) at 257, the
    general SPILL variant (four waves' BezLds) at 769.  Bezier parity is statistical: BEZ_SCENE_BAR."""
    import cgraytracing_amd as cg
    objs = _scene("E", n)
    cam = scenes.cam_dof()
    o = BackendScene(orc, objs)
    want = o.trace_grid(cam, W, H, 4, 5, SEED)
    o.close()
    with cg.Scene(objs) as sc:
        v = _eye_variant(sc, n, 4, cam, sched=True)
        assert ("NT=64" in v) == (n <= KLDS), v
        got = sc.trace_grid_host(W, H, 4, cam, 5, SEED)
    frac, linf, gap = bezier_report("object_counts_vase_%d" % n, got["rgb"], to_acc32(want["acc_sum"], 4), got["nrays"],
                                    want["nrays"])
    assert frac >= BEZ_SCENE_BAR[0] and gap <= BEZ_SCENE_BAR[1], (frac, gap)


@pytest.mark.parametrize("n", [56, 57, 768, 769])
def test_photon_paths_with_many_objects(gpu_ready, orc, n):
    """F: photon paths through the room, an opaque bunny and spheres.  photon_trace_kernel keeps the wide walk's first stack
    entries in LDS up to 56 objects (photon_lds_stack) and not from 57 on; 768 / 769 is its spill boundary."""
    import cgraytracing_amd as cg
    objs = _scene("F", n)
    want = BackendScene(orc, objs).photon_events(1000, 4096)
    with cg.Scene(objs) as sc:
        st = sc.stats()
        assert st["n_objects"] == n and st["n_meshes"] == 1
        # the eye pass's variant says the same about the LDS list: all n objects resident up to 768
        _eye_variant(sc, n, 2, scenes.cam_dof(), sched=False)
        got = sc.photon_events(1000, 4096)
    assert got.shape == want.shape and len(want) > 4000, (got.shape, want.shape)
    assert np.array_equal(got, want)
