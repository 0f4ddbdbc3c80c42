"""Planes in general position and the plane run's decision bound on the GPU, against the CPU oracle, bit for bit.

Every plane the older tests put on a device has a normal that is exactly +-e_k: ObjRec.axis >= 0, the one-subtraction form of
plane_len, and the leading run tested as a group by plane_run (cgrt_scene_walk.hpp).  Here the general form of plane_len runs
(oblique normals, normals not of unit length, which reach reflect / refract unnormalised as in the reference, normals next to
an axis), the ballot that sends zero numerators and denominators of the fast path to the general expression sees waves of every
composition, two planes of a run stand at distance ratios around plane_run's bound 1 + 2^-14, exact ties are met between a plane
in front of the run, the run's planes and later objects, and the same scenes go through every consumer: the nearest-hit query,
the any-hit kernel, the full trace, the frame kernels with their light-tile and primary-walk launches, and photon tracing.

The arbiter is the oracle's per-object intersect() composed as main.cpp:52-62 composes it (test_gpu_rays.oracle_nearest), its
trace_grid and photon_events; tests/test_planes_general_host.py pins it to the compiled reference on these very planes and
checks that every input is what it claims to be.  A hit is a hit that trace() can accept: len > 0 and len < 1e10.  No tolerance
appears in this file.

The vase of front_tie_room and front_oblique_room stands behind the back wall (scenes.hidden_vase) and the rays are kept in front
of it: it selects the Bezier kernels -- the only ones, with the height-field launch, that compile the tie rule for planes in
front of the run -- while no answer depends on a Newton draw; every ray's oracle winner is then something else than the vase
(asserted), which is more than the 95 % a vase in view would have had to leave.

Measured on an MI355X: 0 mismatches in all 56 tests, the file in under four seconds.  Mutations, each built once by hand and
run against this file (the failing tests, and how many rays or pixels differ):
  (i)   1.00006103515625f in plane_run replaced by 1.0000001f: 17 tests -- every case of test_ratio_sweep_nearer_floor_wins and
        test_room_nearest_hit_equals_oracle for the five rooms with a run -- each on 3 to 7 rays of the `edges` group, where two
        walls' exact distances lie within a few ulps.  No floor pair and no near_edges ray fails: two planes on one axis share
        the reciprocal and their estimates cannot swap, and beside an edge the estimates were never wrong by more than the gap.
        The floor pairs and near_edges hold a bound that is wrong by more than that; the literal 1.0000001f is caught at the ties.
  (ii)  the __ballot(zero) fallback of plane_len dropped: test_bump_floor_parallel_rays_take_the_sign_of_the_general_form
        alone, 72 of 4 000 parallel rays and 26 of the 4 032 interleaved ones hit a bump where the reference never looks for one.
        No other test can see it: without a bump tree neither infinity nor either zero is ever an accepted hit.
  (iii) add_plane classifying every normal on an axis as axis-aligned, (0, 2, 0) included: 5 tests -- axis_triple (563, 244,
        294 and 713 lengths of classes a, b, f and g) and nonunit_room in the query (2 150 rays), the full trace (1 022 rays),
        the frames (273 pixels in all) and photon_events (14 525 events for 14 655).  axis_nonunit and axis_half do NOT fail, and
        cannot: doubling or halving both dot products is exact, so for these two normals the fast path returns the general
        form's bits (that is what test_fast_path_equals_the_general_path rests on); a factor of 3 or 7 is not exact.
  (iv)  the FRONT tie clause of intersect_scene removed: front_tie_room with the vase in the query (1 717 rays: the run's floor
        wins) and in the frames (405 to 482 pixels), and bump_front_room's scheduled spp-5 frame (8 pixels, in the height-field
        launch); front_tie_room_no_vase passes, as it must -- its kernels leave a run behind another plane to the loop."""
import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32
from cgraytracing_amd import _capi
from scenes import K_INF
from test_gpu_device_math import same_bits
from test_gpu_object_counts import FORCE_REORDER
from test_gpu_occlusion import _gpu as occluded_gpu
from test_gpu_rays import _cam_off_axis, oracle_nearest, oracle_per_ray, trace_camera

pytestmark = pytest.mark.gpu

SEED = 20261  # make_golden.PLANES_SEED: the host test checks these very rays
PLANES = scenes.general_planes()
W, H = 64, 48


def _hex(v):
    return [float(x).hex() for x in np.atleast_1d(v)]


# ---- function level: one plane -----------------------------------------------------------------------------------------
_ONE = {}


def _one_plane(orc, name):
    """{class: (org, dirs, oracle (accepted hit, len, normal), GPU (hit, len, normal))} for one plane, computed once"""
    import cgraytracing_amd as cg
    if name not in _ONE:
        plane = dict(PLANES)[name]
        cl = scenes.plane_ray_classes(plane, SEED)
        o = BackendScene(orc, [plane])
        out = {}
        with cg.Scene([plane]) as sc:
            for c, (org, dirs) in sorted(cl.items()):
                hit, ln, nv = o.intersect_batch(0, org, dirs)
                out[c] = (org, dirs, ((hit != 0) & (ln < K_INF), ln, nv), sc.intersect_rays(0, org, dirs))
        o.close()
        _ONE[name] = out
    return _ONE[name]


@pytest.mark.parametrize("name", [p[0] for p in PLANES])
def test_one_plane_intersect_equals_oracle(gpu_ready, orc, name):
    """Scene.intersect_rays(0, ...) on a one-plane scene for every plane of general_planes() and every ray class: the hit flag,
    and on the hits len and the returned normal -- the plane's own, whatever its length, -0.0 components included -- bit for
    bit."""
    total = 0
    for c, (org, dirs, (acc, ln, nv), (ghit, glen, gnv)) in _one_plane(orc, name).items():
        bad_hit = np.nonzero((ghit != 0) != acc)[0]
        bad_len = np.nonzero(acc & ~same_bits(glen, ln))[0]
        bad_nrm = np.nonzero(acc & ~same_bits(gnv, nv).all(axis=1))[0]
        print("%-17s %s: %4d rays, hits %4d, hit flags differing %d, len %d %s, normal %d %s" %
              (name, c, len(org), int(acc.sum()), len(bad_hit), len(bad_len),
               [(_hex(org[i]), _hex(dirs[i]), _hex(glen[i]), _hex(ln[i])) for i in bad_len[:2]], len(bad_nrm),
               [(_hex(gnv[i]), _hex(nv[i])) for i in bad_nrm[:2]]))
        total += len(bad_hit) + len(bad_len) + len(bad_nrm)
    assert total == 0


def test_bump_floor_parallel_rays_take_the_sign_of_the_general_form(gpu_ready, orc):
    """The bump floor alone with scenes.bump_parallel_rays: the one observable consequence of the ballot fallback in plane_len.
    A ray exactly parallel to the floor has len = +-inf; +inf is a hit (len > 0) for which the bump tree is consulted, and a
    bump is nearer than +inf.  The sign is that of the three-term sum d . n, which differs from d.y's for d.y = -0.0 beside a
    positive d.x or d.z: without the fallback those rays would walk the bumps and some would hit.
    Scene.intersect_rays and Scene.trace_rays(want=("hit",)): hit flag, hit_obj and len equal the oracle's, bit for bit.  The
    normal is held to what include/cgrt.h promises of an opaque bump floor's triangles -- the vector is right and its sign is
    that of one improvement, along the ray; the reference's own sign follows the parity of its walk's improvement counter,
    which a level ray through several bumps makes even now and then --: every component has the oracle's bits, or every
    component the oracle's bits negated while the oracle's normal points against the ray and the GPU's along it."""
    import cgraytracing_amd as cg
    plane = scenes.bump_floor_plane()
    total = 0
    with cg.Scene([plane]) as sc:
        variant = sc.rays_variant(5, want=("hit",))
        for c, (org, dirs) in sorted(scenes.bump_parallel_rays(SEED).items()):
            o, obj, t, nrm = oracle_nearest(orc, [plane], org, dirs)
            o.close()
            ghit, glen, _ = sc.intersect_rays(0, org, dirs)
            bad_hit = np.nonzero((ghit != 0) != (obj >= 0))[0]
            bad_len = np.nonzero((obj >= 0) & (ghit != 0) & ~same_bits(glen, t))[0]
            q = _query(sc, org, dirs)
            gn = q["hit_normal"]
            turned = same_bits(gn, -nrm).all(axis=1) & ((nrm * dirs).sum(axis=1) < 0) & ((gn * dirs).sum(axis=1) > 0) & (obj >= 0)
            bad_q = np.nonzero((q["hit_obj"] != obj) | ~same_bits(q["hit_t"], t) | ~(same_bits(gn, nrm).all(axis=1) | turned))[0]
            print("bump_floor %s: %s, %d rays, parallel %d, hits %d; probe: hit flags differing %d %s, len %d; query: normals with "
                  "the sign of one improvement where the reference counted an even number %d, differing %d %s" %
                  (c, variant, len(org), int((dirs[:, 1] == 0).sum()), int((obj >= 0).sum()), len(bad_hit),
                   [(_hex(org[i]), _hex(dirs[i]), int(ghit[i]), _hex(glen[i])) for i in bad_hit[:2]], len(bad_len), int(turned.sum()),
                   len(bad_q), [(int(i), int(q["hit_obj"][i]), int(obj[i]), _hex(gn[i]), _hex(nrm[i])) for i in bad_q[:3]]))
            total += len(bad_hit) + len(bad_len) + len(bad_q)
    assert "TREES=1" in variant, variant
    assert total == 0


def test_fast_path_equals_the_general_path(gpu_ready, orc):
    """The same geometry down both paths of plane_len on the GPU itself: axis_unit beside axis_nonunit and axis_half (normals
    (0, 2, 0) and (0, 0.5, 0): general form, both dot products doubled or halved, which is exact --
    tests/test_planes_general_host.py asserts it for the oracle) and beside the two axis_negzero planes (fast path, the
    signed-zero edge).  On every ray whose numerator and denominator are non-zero the GPU's answers are axis_unit's: the same
    hit and the same double."""
    base = _one_plane(orc, "axis_unit")
    plane = dict(PLANES)["axis_unit"]
    for other in ("axis_nonunit", "axis_half", "axis_negzero_up", "axis_negzero_down"):
        for c, (org, dirs, _, (ghit, glen, _)) in sorted(_one_plane(orc, other).items()):
            borg, bdirs, _, (bhit, blen, _) = base[c]
            assert np.array_equal(org, borg) and np.array_equal(dirs, bdirs)  # one seed, one geometry: the same rays
            num, den, _ = scenes.plane_terms(plane, org, dirs)
            ok = (num != 0) & (den != 0)
            bad = np.nonzero(ok & ((ghit != bhit) | ((bhit != 0) & ~same_bits(glen, blen))))[0]
            print("axis_unit vs %-17s %s: %4d rays with non-zero operands, differing %d %s" %
                  (other, c, int(ok.sum()), len(bad), [(_hex(glen[i]), _hex(blen[i])) for i in bad[:3]]))
            assert len(bad) == 0


def test_surface_colors_on_textured_oblique_planes(gpu_ready, orc):
    """Scene.surface_colors on a textured oblique plane against the oracle's getSurfaceColor: the texture's normal equal to the
    plane's (Texture::color falls through to `return false` for most points) and (0, 1, 0) on the oblique plane; a texel and
    the flat colour each on at least 5 % of the points."""
    import cgraytracing_amd as cg
    for name, plane, pts in scenes.textured_oblique_cases():
        want = BackendScene(orc, [plane]).surface_color_batch(0, pts)
        with cg.Scene([plane]) as sc:
            got = sc.surface_colors(0, pts)
        flat = (want == np.asarray(plane.surfaceColor)).all(axis=1)
        bad = np.nonzero(~same_bits(got, want).all(axis=1))[0]
        print("%s: %d points, flat colour %d, texel %d, differing %d %s" %
              (name, len(pts), int(flat.sum()), int((~flat).sum()), len(bad), [(_hex(pts[i]), _hex(got[i]), _hex(want[i])) for i in bad[:3]]))
        assert 0.05 <= flat.mean() <= 0.95
        assert len(bad) == 0


# ---- scene walk: rooms ---------------------------------------------------------------------------------------------------
ROOMS = ["tilted_room", "nonunit_room", "front_tie_room", "front_tie_room_no_vase", "front_oblique_room", "behind_tie_room",
         "twin_in_run", "glass_wall_room"]
VASE_ROOMS = ("front_tie_room", "front_oblique_room")
_ROOM = {}


def _room_rays(name, objs):
    """the room's ray set: room_rays with the degenerate classes taken against the run's floor (tilted_room: the floor before the
    rotation, and every ray rotated with the walls), behind_tie_room's own rays appended"""
    floor = scenes.room_walls()[0]
    org, dirs, groups = scenes.room_rays(SEED, floor, tilt=name == "tilted_room", floor_origins=name.startswith("ratio_sweep"),
                                         in_front=name in VASE_ROOMS)
    if name == "behind_tie_room":
        o2, d2, _ = scenes.behind_tie_rays()
        groups["tangent"] = slice(len(org), len(org) + len(o2))
        org, dirs = np.concatenate([org, o2]), np.concatenate([dirs, d2])
    assert len(org) <= 20000
    return np.ascontiguousarray(org), np.ascontiguousarray(dirs), groups


def _room(orc, name, objs=None):
    """(objs, org, dirs, groups, oracle hit_obj / hit_t / hit_normal), once per room"""
    if name not in _ROOM:
        objs = scenes.run_rooms()[name] if objs is None else objs
        org, dirs, groups = _room_rays(name, objs)
        o, obj, t, nrm = oracle_nearest(orc, objs, org, dirs)
        o.close()
        _ROOM[name] = (objs, org, dirs, groups, obj, t, nrm)
    return _ROOM[name]


def _query(sc, org, dirs):
    import torch
    dev = torch.device("cuda", sc.device)
    res = sc.trace_rays(torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev), want=("hit",))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _compare_hits(name, variant, groups, got, obj, t, nrm):
    """prints the counts per group and returns the number of rays whose hit_obj, hit_t or hit_normal differs in a bit"""
    bad = (got["hit_obj"] != obj) | ~same_bits(got["hit_t"], t) | ~same_bits(got["hit_normal"], nrm).all(axis=1)
    print("%s: %s" % (name, variant))
    for g, sl in groups.items():
        idx = np.nonzero(bad[sl])[0] + sl.start
        print("  %-10s %5d rays, hits %5d, differing %d %s" %
              (g, sl.stop - sl.start, int((obj[sl] >= 0).sum()), len(idx),
               [(int(i), int(got["hit_obj"][i]), int(obj[i]), _hex(got["hit_t"][i]), _hex(t[i])) for i in idx[:3]]))
    return int(bad.sum())


@pytest.mark.parametrize("name", ROOMS)
def test_room_nearest_hit_equals_oracle(gpu_ready, orc, name):
    """Scene.trace_rays(want=("hit",)) on the rooms of scenes.run_rooms(): hit_obj, hit_t and hit_normal equal the oracle's, bit
    for bit, on random, axis-parallel, wall-bound, edge- and corner-bound, far and degenerate rays (scenes.room_rays).  What
    each room adds is asserted on the oracle's side, so that the case is known to be met."""
    import cgraytracing_amd as cg
    objs, org, dirs, groups, obj, t, nrm = _room(orc, name)
    with cg.Scene(objs) as sc:
        variant = sc.rays_variant(5, want=("hit",))
        got = _query(sc, org, dirs)
    n_bad = _compare_hits(name, variant, groups, got, obj, t, nrm)
    floor_t = None
    if name in VASE_ROOMS:
        assert "BEZ=1" in variant, variant
        assert (obj != len(objs) - 1).all()  # no ray's winner is the vase: all of them are compared
    if name.endswith("no_vase") or name in ("behind_tie_room", "twin_in_run", "glass_wall_room", "tilted_room", "nonunit_room"):
        assert "BEZ=0" in variant, variant
    if name.startswith("front_tie_room"):
        # the front plane keeps its tie with the run's floor: index 0, normal (0, 2, 0), on every floor-bound ray
        assert (obj != 1).all() and (obj == 0).sum() > 3000
        assert (nrm[obj == 0] == np.array([0.0, 2.0, 0.0])).all()
    if name == "front_oblique_room":
        assert (obj == 0).sum() > 500 and (obj == 1).sum() > 500
    if name == "behind_tie_room":
        assert (obj != 5).all() and (obj == 0).sum() > 3000  # the run's floor keeps the tie against the later plane
        tg = groups["tangent"]
        assert (obj[tg] == 6).any() and (obj[tg] == 0).any()  # the rim and the axis: the sphere here, the floor there
    if name == "twin_in_run":
        assert (obj != 1).all() and (obj == 0).sum() > 3000
    if name in ("tilted_room", "nonunit_room"):
        assert all((obj == i).sum() > 1000 for i in range(5))
    assert n_bad == 0


@pytest.mark.parametrize("k", scenes.RATIO_KS)
def test_ratio_sweep_nearer_floor_wins(gpu_ready, orc, k):
    """Two floors of one run at y = -12 and y = -12 r, r - 1 = 2^-14 k, around plane_run's bound: the fp32 estimates may pick
    the winner only when the second smallest exceeds the smallest by more than 1 + 2^-14, and every other lane must take the
    planes one by one.  From origins above both floors the nearer one, y = -12, wins on every floor-bound ray; for k = 0 the
    first in the list; in both list orders; and everything equals the oracle."""
    import cgraytracing_amd as cg
    n_bad = 0
    for swapped in (False, True):
        name = "ratio_sweep_%g%s" % (k, "_swapped" if swapped else "")
        objs, org, dirs, groups, obj, t, nrm = _room(orc, name, scenes.ratio_sweep_room(k, swapped))
        with cg.Scene(objs) as sc:
            variant = sc.rays_variant(5, want=("hit",))
            got = _query(sc, org, dirs)
        n_bad += _compare_hits(name, variant, groups, got, obj, t, nrm)
        near, far = (4, 0) if swapped else (0, 4)
        inside = org[:, 1] > -12.0  # above both floors
        on_floor = (got["hit_obj"] == near) | (got["hit_obj"] == far)
        wrong = inside & (got["hit_obj"] == (far if k > 0 else 4))
        print("  rays that end on a floor %d, of them from above both %d, the farther (k = 0: the later) floor winning %d" %
              (int(on_floor.sum()), int((on_floor & inside).sum()), int(wrong.sum())))
        assert (on_floor & inside).sum() > 2500 and not wrong.any()
    assert n_bad == 0


TMAX = (0.5, 5.0, 20.0, 1e10)


@pytest.mark.parametrize("name", ROOMS + ["ratio_sweep_1", "ratio_sweep_0.000976562_swapped"])
def test_room_occlusion_equals_oracle(gpu_ready, orc, name):
    """Scene.occluded on the same rooms and rays for tmax in {0.5, 5, 20, 1e10}: occluded = the oracle's nearest accepted length
    < tmax (as tests/test_gpu_occlusion.py derives it), through the any-hit kernel's own use of the run (run_sure / mine /
    usable, cgrt_occlusion.hpp).  With CGRT_RAYS_SKIP_TRANSPARENT on nonunit_room (the glass sphere) and on glass_wall_room, whose
    transparent wall stands inside the run, so that the run is not usable: the oracle over the opaque objects."""
    import cgraytracing_amd as cg
    if name.startswith("ratio_sweep"):
        k = next(k for k in scenes.RATIO_KS if "%g" % k == name.split("_")[2])
        objs, org, dirs, groups, obj, t, nrm = _room(orc, name, scenes.ratio_sweep_room(k, name.endswith("swapped")))
    else:
        objs, org, dirs, groups, obj, t, nrm = _room(orc, name)
    cases = [(False, obj, t)]
    if name in ("nonunit_room", "glass_wall_room"):
        opaque = [i for i, ob in enumerate(objs) if ob.transparency < 1e-4]
        assert 0 < len(opaque) < len(objs)
        o, obj2, t2, _ = oracle_nearest(orc, [objs[i] for i in opaque], org, dirs)
        o.close()
        assert (obj2 != obj).any() or (t2 != t).any()
        cases.append((True, obj2, t2))
    n_bad = 0
    with cg.Scene(objs) as sc:
        variant = sc.occlusion_variant()
        for skip, wobj, wt in cases:
            for tmax in TMAX:
                want = ((wobj >= 0) & (wt < tmax)).astype(np.uint8)
                got, _ = occluded_gpu(sc, org, dirs, np.full(len(org), tmax), skip_transparent=skip)
                bad = np.nonzero(got != want)[0]
                print("%s: %s, skip_transparent %d, tmax %g: %d rays, occluded %d, differing %d %s" %
                      (name, variant, skip, tmax, len(org), int(want.sum()), len(bad), bad[:8].tolist()))
                n_bad += len(bad)
                if tmax < 1e10:
                    assert 0 < want.sum() < (wobj >= 0).sum()  # the limit cuts some hits off and leaves some
    assert n_bad == 0


@pytest.mark.parametrize("name", ["tilted_room", "nonunit_room"])
def test_full_trace_equals_oracle(gpu_ready, orc, name):
    """Scene.trace_rays(max_depth=5) on an off-axis thin-lens camera's rays (96x72, spp 2) against the oracle's eye pass per ray
    (test_gpu_rays.oracle_per_ray): acc and nhit exact.  The mirror wall reflects about a normal that is oblique resp. of length
    three, nonunit_room's glass sphere sends refracted rays to walls whose normals have lengths 2, 0.5, 0.25 and 7."""
    import cgraytracing_amd as cg
    objs, cam = scenes.run_rooms()[name], _cam_off_axis()
    acc, nhit, nrays = oracle_per_ray(orc, objs, cam, 96, 72, 2, 5, SEED)
    with cg.Scene(objs) as sc:
        variant = sc.rays_variant(5)
        got, _ = trace_camera(sc, cam, 96, 72, 2, 5, SEED)
    bad = np.nonzero((got["acc"] != acc).any(axis=1) | (got["nhit"] != nhit))[0]
    print("%s: %s, %d primary rays, %d rays, %d Hitpoints, differing %d %s" %
          (name, variant, len(acc), nrays, int(nhit.sum()), len(bad), [(int(i), _hex(got["acc"][i]), _hex(acc[i])) for i in bad[:3]]))
    assert nrays > len(acc) * 1.1  # secondary rays: the normals did reach reflect / refract
    assert len(bad) == 0 and int(got["counters"][_capi.CNT_RAYS]) == nrays


def _frame(orc, objs, cam, spp, seed=SEED, **kw):
    import cgraytracing_amd as cg
    want = BackendScene(orc, objs).trace_grid(cam, W, H, spp, 5, seed=seed)
    with cg.Scene(objs) as sc:
        variant = sc.kernel_variant(W, H, spp, cam, flags=FORCE_REORDER if kw.get("force_reorder") else 0)
        got = sc.trace_grid_host(W, H, spp, cam, 5, seed, **kw)
    ref = to_acc32(want["acc_sum"], spp)
    px = int((got["rgb"] != ref).any(axis=2).sum()) + int((got["nhit"] != want["nhit"]).sum())
    print("  spp %d %s: %s, rays %d vs %d, pixels differing %d" % (spp, kw, variant, got["nrays"], want["nrays"], px))
    return variant, px + abs(got["nrays"] - want["nrays"])


@pytest.mark.parametrize("name", ["tilted_room", "nonunit_room", "front_tie_room"])
def test_frames_equal_oracle(gpu_ready, orc, name):
    """Scene.trace_grid_host at 64x48, spp 1 and 5 (image order and the scheduled path), pinhole and thin lens: nrays, nhit and
    rgb equal the oracle's trace_grid exactly."""
    objs = scenes.run_rooms()[name]
    print(name)
    n_bad = 0
    for cam in (scenes.cam_pinhole(), scenes.cam_dof()):
        for spp in (1, 5):
            n_bad += _frame(orc, objs, cam, spp)[1]
    n_bad += _frame(orc, objs, scenes.cam_dof(), 5, force_reorder=True)[1]
    assert n_bad == 0


def test_bump_floor_and_general_plane_in_front_of_the_run(gpu_ready, orc):
    """bump_front_room: an opaque bump floor, then a ceiling whose normal has length two, then a run of three walls, and a mirror
    sphere; 64x48 at spp 1 and 5 and at spp 5 in the forced scheduled form, exact against the oracle (nrays, nhit, rgb: the
    fields of test_plane_group_test_edges_corners_and_degenerate_rays).  Both planes stand in front of the run: in the
    kernels that compile the tie rule (FRONT: the height-field launch and the Bezier variants) the run is tested first and the two
    meet its winner.
    That the light tiles' launch is the HFONLY variant cannot be read from Python -- no entry point names the launch plan's
    kernels beyond kernel_variant's main launch --; it follows from the scene's traits, which tests/native/plane_runs.cpp's
    build evaluates for this very list (every plane diffuse, the floor's tree a height field, a mirror sphere: light_ok =
    light_hf_only = 1, as tests/test_gpu_hfonly_cached_tree.py argues for its room), and the scheduled form is asserted."""
    objs = scenes.run_rooms()["bump_front_room"]
    n_bad = 0
    for spp in (1, 5):
        n_bad += _frame(orc, objs, scenes.cam_pinhole(), spp)[1]
        n_bad += _frame(orc, objs, scenes.cam_dof(), spp)[1]
    variant, bad = _frame(orc, objs, scenes.cam_dof(), 5, force_reorder=True)
    assert variant.startswith("trace_grid_sched_kernel<TREES=1"), variant
    assert n_bad + bad == 0


@pytest.mark.parametrize("name", ["tilted_room", "nonunit_room"])
def test_photon_events_equal_oracle(gpu_ready, orc, name):
    """photon_events(0, 4096): photon tracing through intersect_scene on general-form planes, every diffuse hit's position,
    normal and flux exact.  The light at (0, 19.999, 20) lies outside these rooms (above the ceiling, behind the back wall);
    the planes are unbounded, so its photons meet them from outside all the same: more than 4 000 events (16 336 and 14 655)."""
    import cgraytracing_amd as cg
    objs = scenes.run_rooms()[name]
    want = BackendScene(orc, objs).photon_events(0, 4096)
    with cg.Scene(objs) as sc:
        got = sc.photon_events(0, 4096)
    print("%s: %d events (oracle %d)" % (name, len(got), len(want)))
    assert len(want) > 4000 and got.shape == want.shape
    bad = np.nonzero(~same_bits(got, want).all(axis=1))[0]
    assert len(bad) == 0, (bad[:5], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("replaced", sorted(scenes.MESH_RUNS))
def test_primary_walk_with_general_form_planes(gpu_ready, orc, replaced):
    """An opaque mesh behind five planes is the primary-walk kernel's scene (cgrt_primwalk.hpp): with one plane's normal doubled
    the run shrinks to four (replaced = 4), stands behind a general-form plane (0) or disappears (2), and the kernel's own
    plane code meets general-form planes.  64x48, spp 4, pinhole and thin lens, exact against the oracle."""
    objs = scenes.mesh_behind_planes(replaced)
    print("plane %d replaced: run %s" % (replaced, scenes.MESH_RUNS[replaced]))
    n_bad = sum(_frame(orc, objs, cam, 4, seed=9)[1] for cam in (scenes.cam_pinhole(), scenes.cam_dof()))
    assert n_bad == 0
