"""GPU: every compiled eye kernel is launched here and held to the oracle -- the census of CGRT_EYE_VARIANTS and
CGRT_EYE_POSED_VARIANTS (cgrt_variants.h), of the rows' scheduled forms (SCHED=1) and of primary_walk_kernel<DOF>.

Scene.kernel_variant() names a frame's main launch only.  Scene.last_eye_launches() reads back every eye kernel the last eye pass
on the handle launched -- the probe, the light tiles' launch on the second stream, the diffuse launch, the relay's cost probe (the
START twin), the LTAB twins, the primary walk --, as the header's own columns.  Each case below renders one small frame, compares
it with the CPU oracle bit for bit (eye_exact of test_gpu_deep_trees.py: rays, per-pixel Hitpoint counts, the image), and files
what it launched under its label; test_every_eye_kernel_is_launched then holds the set of launches against the lists read from
the header (tests/variants.py).  There is no allow-list: a row no case reaches fails the test.

Frames are 40 x 18 pixels: 1 1/4 tiles of 32 across and 2 1/4 tiles of 8 down (2 1/2 wave tiles of 16, 4 1/2 of 4), so every
launch has full tiles and tiles cut on the right and at the bottom; the suite's two cameras see the spheres, the meshes and the
vase in the lower half of such a frame.  Image order at 2 samples, the scheduled form at 4
(the fewest at which eye_choice schedules); the relay at 32 and its promotion at 48, the fewest at which relay_chunks cuts a
tile into 2 and 3 chunks, with CGRT_GRID_SAMPLE_RELAY, which lifts relay_engaged's tile count -- no form here needs a larger frame.

Bezier cases cannot be bit-exact against the oracle: they get test_gpu_parity.BEZ_SCENE_BAR through
bezier_report, and their image-order and scheduled launches must agree with each other bit for bit.  Posed rows are rendered
under two views each: the identity pose against the oracle as above (the contract test_gpu_posed_camera.py states), and that
file's TURNED pose against the Hitpoint records of trace_rays_hitpoints over the posed camera_rays, folded per pixel sample by
sample in fp64 by that file's fold helper -- the chain to the oracle its docstring describes."""
import numpy as np
import pytest

import scenes
import variants
from backends import BackendScene, to_acc32
from cgraytracing_amd import _capi
from test_gpu_deep_trees import eye_exact
from test_gpu_parity import BEZ_SCENE_BAR, _canon, bezier_report
from test_gpu_posed_camera import _fold, posed, rays
from test_gpu_rays import _bezier_scene, _bump_sphere_scene

pytestmark = pytest.mark.gpu

W, H, SEED = 40, 18, 12345
RAYS = _capi.CNT_RAYS


PIN, DOF = scenes.cam_pinhole, scenes.cam_dof


def _hfonly_room():
    """The scene of test_gpu_hfonly_cached_tree.py: a glass pyramid (the cached tree) over the opaque stone bump floor"""
    pyramid = scenes.TriangleMesh.from_triangles(scenes.pyramid_tris(0.6, (-6.0, -13.0, 36.0)), (0.6, 0.7, 0.9), 0.8, 0.5)
    return scenes.room_with_objects(12, 312, mesh=pyramid, floor_tex=scenes.stone_small_texture(True))


def bez_mirror():
    return _bezier_scene(False)


def bez_glass():
    return _bezier_scene(True)


def c3_glass():
    return scenes.scene_c3(True)


def pyramid_glass():
    return scenes.scene_pyramid(True)


def spheres_1000():
    return scenes.many_spheres(1000, 11)


def room_800():
    return scenes.room_with_objects(800, 5)


RELAY = dict(sample_relay=True, relay_start="cost")

# (label, scene factory, camera, keywords of trace_grid_host -- or hitpoints=True: the capture; both=True: the default launch and
# the same frame with reorder=False; pose=True: a posed row, under two views --, spp, depth).  Every frame is 40 x 18 (above).
CASES = [
    # ---- Bezier scenes, one-wave workgroups: 4 samples, scheduled by default and in image order on request ----
    ("bez_mirror_pin", bez_mirror, PIN, dict(both=True), 4, 5),
    ("bez_mirror_dof", bez_mirror, DOF, dict(both=True), 4, 5),
    ("bez_glass_pin", bez_glass, PIN, dict(both=True), 4, 5),
    ("bez_glass_dof", bez_glass, DOF, dict(both=True), 4, 5),
    # ---- meshes: image order at 2 samples; scheduled at 4 with the probe, the light tiles' launch and the primary walk ----
    ("dragon_pin_image", scenes.scene_dragon, PIN, {}, 2, 5),
    ("dragon_dof_image", scenes.scene_dragon, DOF, {}, 2, 5),
    ("dragon_pin_sched", scenes.scene_dragon, PIN, {}, 4, 5),
    ("dragon_dof_sched", scenes.scene_dragon, DOF, {}, 4, 5),
    ("c3_pin_image", c3_glass, PIN, {}, 2, 5),
    ("c3_dof_image", c3_glass, DOF, {}, 2, 5),
    ("c3_pin_sched", c3_glass, PIN, {}, 4, 5),
    ("c3_dof_sched", c3_glass, DOF, {}, 4, 5),
    ("c3_dof_depth1_sched", c3_glass, DOF, {}, 4, 1),  # GLASS=0 on a glass scene
    ("pyramid_glass_dof_image", pyramid_glass, DOF, {}, 2, 5),
    ("glass_bump_floor_dof_sched", scenes.scene_glass_bump_floor, DOF, {}, 4, 5),
    # ... with STATS, each beside its plain twin
    ("dragon_pin_stats_image", scenes.scene_dragon, PIN, dict(stats=True), 2, 5),
    ("dragon_dof_stats_image", scenes.scene_dragon, DOF, dict(stats=True), 2, 5),
    ("dragon_pin_stats_sched", scenes.scene_dragon, PIN, dict(stats=True), 4, 5),
    ("dragon_dof_stats_sched", scenes.scene_dragon, DOF, dict(stats=True), 4, 5),
    ("c3_pin_stats_image", c3_glass, PIN, dict(stats=True), 2, 5),
    ("c3_dof_stats_image", c3_glass, DOF, dict(stats=True), 2, 5),
    ("c3_pin_stats_sched", c3_glass, PIN, dict(stats=True), 4, 5),
    ("c3_dof_stats_sched", c3_glass, DOF, dict(stats=True), 4, 5),
    # ... and the light tiles' HFONLY launch beside the scheduled form: opaque bump floors
    ("bump_sphere_pin_sched", _bump_sphere_scene, PIN, {}, 4, 5),
    ("bump_sphere_dof_sched", _bump_sphere_scene, DOF, {}, 4, 5),
    ("hfonly_room_pin_sched", _hfonly_room, PIN, {}, 4, 5),
    ("hfonly_room_dof_sched", _hfonly_room, DOF, {}, 4, 5),
    # ---- sphere scenes: the pair kernel in tile order, one sphere a trip, without glass, scheduled on request ----
    ("c2_pin_pair", scenes.scene_c2, PIN, {}, 2, 5),
    ("c2_dof_pair", scenes.scene_c2, DOF, {}, 2, 5),
    ("c2_pin_no_pairs", scenes.scene_c2, PIN, dict(sphere_pairs=False), 2, 5),
    ("c2_dof_no_pairs", scenes.scene_c2, DOF, dict(sphere_pairs=False), 2, 5),
    ("c2_pin_depth1", scenes.scene_c2, PIN, {}, 2, 1),
    ("c1_dof_image", scenes.scene_c1, DOF, {}, 2, 5),
    ("c2_pin_sched", scenes.scene_c2, PIN, dict(force_reorder=True), 4, 5),
    ("c2_dof_sched", scenes.scene_c2, DOF, dict(force_reorder=True), 4, 5),
    ("c1_pin_sched", scenes.scene_c1, PIN, dict(force_reorder=True), 4, 5),
    ("c2_dof_depth1_sched", scenes.scene_c2, DOF, dict(force_reorder=True), 4, 1),
    # ... the second, terminal-diffuse launch (frame_plan: a sphere scene in tile order that asks for it, whatever its size)
    ("c2_pin_diffuse_tiles", scenes.scene_c2, PIN, dict(diffuse_tiles=True), 2, 5),
    ("c2_dof_diffuse_tiles", scenes.scene_c2, DOF, dict(diffuse_tiles=True), 2, 5),
    # ... the lens table's LTAB twin (frame_plan: the pair kernel under a lens; written wherever the launch stands when asked for)
    ("c2_dof_lens_table", scenes.scene_c2, DOF, dict(lens_table=True), 2, 5),
    # ... the sample relay: 32 samples, the fewest relay_chunks cuts in two; by the list, and by cost with the START twin as the
    # probe and as the frame (under a lens the table is written beside the probe: START and LTAB)
    ("c2_pin_relay_list", scenes.scene_c2, PIN, dict(sample_relay=True), 32, 5),
    ("c2_pin_relay_cost", scenes.scene_c2, PIN, RELAY, 32, 5),
    ("c2_dof_relay_cost", scenes.scene_c2, DOF, RELAY, 32, 5),
    ("c2_dof_relay_cost_no_table", scenes.scene_c2, DOF, dict(RELAY, lens_table=False), 32, 5),
    # ... and its promotion: 48 samples, the fewest relay_chunks(spp, 4) cuts in more chunks (3) than the base relay's 2
    ("c2_dof_relay_boost", scenes.scene_c2, DOF, dict(RELAY, relay_boost=True), 48, 5),
    # ---- planes, and planes with spheres ----
    ("planes_pin_image", scenes.planes, PIN, {}, 2, 5),
    ("planes_dof_image", scenes.planes, DOF, {}, 2, 5),
    ("planes_pin_sched", scenes.planes, PIN, dict(force_reorder=True), 4, 5),
    ("planes_dof_sched", scenes.planes, DOF, dict(force_reorder=True), 4, 5),
    ("walls_pin_image", scenes.scene_textured_walls, PIN, {}, 2, 5),
    ("walls_dof_image", scenes.scene_textured_walls, DOF, {}, 2, 5),
    ("walls_pin_sched", scenes.scene_textured_walls, PIN, dict(force_reorder=True), 4, 5),
    ("walls_dof_sched", scenes.scene_textured_walls, DOF, dict(force_reorder=True), 4, 5),
    # ---- more objects than the LDS list holds: the sphere loop's SPILL body and the general one ----
    ("spheres_1000_pin", spheres_1000, PIN, {}, 2, 5),
    ("spheres_1000_dof", spheres_1000, DOF, {}, 2, 5),
    ("spheres_1000_pin_depth1", spheres_1000, PIN, {}, 2, 1),
    ("spheres_1000_dof_depth1", spheres_1000, DOF, {}, 2, 1),
    ("room_800_pin", room_800, PIN, {}, 2, 5),
    ("room_800_dof", room_800, DOF, {}, 2, 5),
    # ---- the Hitpoint capture, every object resident and not ----
    ("c2_pin_hps", scenes.scene_c2, PIN, dict(hitpoints=True), 2, 5),
    ("c3_dof_hps", c3_glass, DOF, dict(hitpoints=True), 2, 5),
    ("spheres_1000_pin_hps", spheres_1000, PIN, dict(hitpoints=True), 2, 5),
    ("room_800_dof_hps", room_800, DOF, dict(hitpoints=True), 2, 5),
    # ---- posed rows (CGRT_EYE_POSED_VARIANTS), each under the identity pose and TURNED ----
    ("posed_bez_mirror_pin", bez_mirror, PIN, dict(pose=True, both=True), 4, 5),
    ("posed_bez_mirror_dof", bez_mirror, DOF, dict(pose=True, both=True), 4, 5),
    ("posed_bez_glass_pin", bez_glass, PIN, dict(pose=True, both=True), 4, 5),
    ("posed_bez_glass_dof", bez_glass, DOF, dict(pose=True, both=True), 4, 5),
    ("posed_dragon_pin", scenes.scene_dragon, PIN, dict(pose=True, both=True), 4, 5),
    ("posed_dragon_dof", scenes.scene_dragon, DOF, dict(pose=True, both=True), 4, 5),
    ("posed_c3_pin", c3_glass, PIN, dict(pose=True, both=True), 4, 5),
    ("posed_c3_dof", c3_glass, DOF, dict(pose=True, both=True), 4, 5),
    ("posed_c2_pin", scenes.scene_c2, PIN, dict(pose=True), 2, 5),
    ("posed_c2_dof", scenes.scene_c2, DOF, dict(pose=True), 2, 5),
    ("posed_c1_pin", scenes.scene_c1, PIN, dict(pose=True), 2, 5),
    ("posed_c2_dof_depth1", scenes.scene_c2, DOF, dict(pose=True), 2, 1),
    ("posed_planes_pin", scenes.planes, PIN, dict(pose=True), 2, 5),
    ("posed_planes_dof", scenes.planes, DOF, dict(pose=True), 2, 5),
    ("posed_walls_pin", scenes.scene_textured_walls, PIN, dict(pose=True), 2, 5),
    ("posed_walls_dof", scenes.scene_textured_walls, DOF, dict(pose=True), 2, 5),
    ("posed_spheres_1000_pin", spheres_1000, PIN, dict(pose=True), 2, 5),
    ("posed_spheres_1000_dof", spheres_1000, DOF, dict(pose=True), 2, 5),
    ("posed_room_800_pin", room_800, PIN, dict(pose=True), 2, 5),
    ("posed_room_800_dof", room_800, DOF, dict(pose=True), 2, 5),
    ("posed_c2_pin_hps", scenes.scene_c2, PIN, dict(pose=True, hitpoints=True), 2, 5),
    ("posed_c3_dof_hps", c3_glass, DOF, dict(pose=True, hitpoints=True), 2, 5),
    ("posed_spheres_1000_dof_hps", spheres_1000, DOF, dict(pose=True, hitpoints=True), 2, 5),
    ("posed_room_800_pin_hps", room_800, PIN, dict(pose=True, hitpoints=True), 2, 5),
]
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)

LAUNCHES = {}  # label -> [the tuples of last_eye_launches() after each of the case's eye passes]
_ORACLE_SCENES, _ORACLE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _oracle_scenes():
    yield
    for o in _ORACLE_SCENES.values():
        o.close()
    _ORACLE_SCENES.clear()


def oracle(orc, mk, cam, spp, depth, capture=False):
    """The oracle's eye pass over the case's frame, computed once and shared (read only); its scene is built once per factory"""
    key = (mk, cam.lens_radius, spp, depth, capture)
    if key not in _ORACLE:
        if mk not in _ORACLE_SCENES:
            _ORACLE_SCENES[mk] = BackendScene(orc, mk())
        _ORACLE[key] = _ORACLE_SCENES[mk].trace_grid(cam, W, H, spp, depth, SEED, capture=capture)
    return _ORACLE[key]


def _file(label, sc):
    got = sc.last_eye_launches()
    assert got, "%s: the eye pass recorded no launch" % label
    LAUNCHES.setdefault(label, []).extend(got)
    return got


def _bezier_bar(what, rgb, ref32, nrays, nrays_want):
    frac, linf, gap = bezier_report("eye_variants_" + what.replace("/", "_"), rgb, ref32, nrays, nrays_want)
    assert frac >= BEZ_SCENE_BAR[0] and gap <= BEZ_SCENE_BAR[1], (what, frac, linf, gap)


def _ray_records(sc, cam, spp, depth):
    """The posed view's reference: the Hitpoint records of trace_rays_hitpoints over the posed camera_rays (label = sample * pixels
    + pixel, position in the ray tree), their fold per pixel, the per-pixel counts and the rays traced"""
    org, dirs, keys = sc.camera_rays(W, H, spp, cam, SEED)
    r = sc.trace_rays_hitpoints(org, dirs, keys, max_depth=depth, seed=SEED)
    assert r["count"] == len(r["hp"])
    npix = W * H
    pix, smp = r["ray"] % npix, r["ray"] // npix
    rgb = _fold(r["hp"], pix, smp, r["seq"], npix, spp).reshape(H, W, 3)
    nhit = np.bincount(pix, minlength=npix).astype(np.uint32).reshape(H, W)
    _, rnhit, rcnt = rays(sc, cam, W, H, spp, depth)
    assert np.array_equal(nhit, rnhit.sum(axis=0).astype(np.uint32)), "capture_rays and trace_rays disagree on the Hitpoint counts"
    return dict(rgb=rgb, nhit=nhit, nrays=int(rcnt[RAYS]), rec=r, pix=pix, smp=smp)


def _check_capture(what, g, want_hp, want_pix, want_smp, want_n):
    assert g["count"] == want_n == len(g["hp"]), "%s: %d Hitpoints vs %d" % (what, g["count"], want_n)
    a, b = _canon(g["hp"], g["pix"], g["smp"]), _canon(want_hp, want_pix, want_smp)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "%s: pixels and samples of the Hitpoint stream" % what
    assert np.array_equal(a[0], b[0]), "%s: Hitpoint records differ" % what


def _check_form(what, sc, kw, cam, spp, got):
    """The frame took the form its case is in the list for -- it did relay, promote, read a lens table, hand tiles to the diffuse
    launch --, so that the twin it launched ran the code that sets it apart"""
    if kw.get("sample_relay"):
        relay = sc.last_sample_relay()
        assert relay["tiles"] > 0 and relay["chunks"] == 2 and relay["parked_values"] > 0, (what, relay)
        if kw.get("relay_start") == "cost":
            start = sc.last_relay_start()
            assert start is not None and start["t"] > 0 and not start["reused"] and start["wcost"].any(), (what, start)
            assert [t[13] for t in got] == [1, 1], (what, got)  # the cost probe and the frame: START twins both
        if kw.get("relay_boost"):
            boost = sc.last_relay_boost()
            assert boost is not None and boost["k_boost"] == 3 and boost["boost_cap"] > 0, (what, boost)
    tabled = cam.lens_radius > 0 and (kw.get("lens_table") or (kw.get("relay_start") == "cost" and kw.get("lens_table") is None))
    if tabled:
        table = sc.last_lens_table()
        assert table["entries"] > 0 and not table["reused"] and got[-1][14] == 1, (what, table, got)
    elif "lens_table" in kw or kw.get("sample_relay"):
        assert sc.last_lens_table()["entries"] == 0 and not any(t[14] for t in got), (what, got)
    if kw.get("diffuse_tiles"):
        assert sc.last_diffuse_tiles() > 0 and [t[11] for t in got] == [0, 1], (what, got)  # the main launch, then the DIFF one
    if spp < 4 and not kw and cam.pose is None and got[0][12]:  # the pair kernel in tile order: class 3 by the body inside it
        assert sc.last_inkernel_diffuse_tiles() > 0, what


def run_case(orc, label, mk, cam_of, kw, spp, depth):
    import cgraytracing_amd as cg

    kw = dict(kw)
    is_posed, both, capture = kw.pop("pose", False), kw.pop("both", False), kw.pop("hitpoints", False)
    bezier = mk in (bez_mirror, bez_glass)
    LAUNCHES.pop(label, None)
    with cg.Scene(mk()) as sc:
        for view in (("identity", "turned") if is_posed else (None,)):
            what = label if view is None else "%s/%s" % (label, view)
            cam = cam_of() if view is None else posed(cam_of(), view)
            ref = _ray_records(sc, cam, spp, depth) if view == "turned" else None
            if capture:
                g = sc.trace_grid_hitpoints(W, H, spp, cam, depth, SEED)
                got = _file(label, sc)
                assert [t[0] for t in got] == [0] and got[0][7] == 1 and got[0][15] == int(is_posed), (what, got)
                if ref is None:
                    want = oracle(orc, mk, cam_of(), spp, depth, capture=True)
                    _check_capture(what, g, want["hp"], want["hp_pix"], want["hp_smp"], want["nhp"])
                else:  # labels coincide by construction: the records, sorted by label, are equal in all their doubles
                    r = ref["rec"]
                    glab, rlab = ((g["smp"] * (W * H) + g["pix"]) << 4) | g["seq"], (r["ray"] << 4) | r["seq"]
                    go, ro = np.argsort(glab, kind="stable"), np.argsort(rlab, kind="stable")
                    assert g["count"] == r["count"] and np.array_equal(glab[go], rlab[ro]), what
                    assert np.array_equal(g["hp"][go], r["hp"][ro]), "%s: Hitpoint records differ" % what
                continue
            frames = {}
            for form, extra in ((("default", {}), ("image", dict(reorder=False))) if both else (("default", {}),)):
                frames[form] = sc.trace_grid_host(W, H, spp, cam, depth, SEED, **dict(kw, **extra))
                got = _file(label, sc)
                assert all(t[15] == int(is_posed) for t in got), (what, got)
                _check_form(what, sc, kw, cam, spp, got)
                if both:  # the default launch of these cases is the scheduled one
                    assert (1 in [t[0] for t in got]) == (form == "default"), (what, form, got)
            want = oracle(orc, mk, cam_of(), spp, depth) if ref is None else ref
            ref32 = to_acc32(want["acc_sum"], spp) if ref is None else want["rgb"]
            for form, got in frames.items():
                assert float(np.abs(got["rgb"]).max()) > 0, "%s %s: the view sees nothing" % (what, form)
                if bezier:
                    _bezier_bar("%s_%s" % (what, form), got["rgb"], ref32, got["nrays"], want["nrays"])
                else:
                    eye_exact(got, want, spp, "%s %s" % (what, form), ref32=ref32)
            if both:
                a, b = frames["default"], frames["image"]
                assert np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["nhit"], b["nhit"]) and a["nrays"] == b["nrays"], \
                    "%s: the scheduled and the image-order launch differ" % what
            if kw.get("stats"):  # the plain twin: the same image and the same rays and Hitpoints; STATS counts its walks
                st = frames["default"]
                plain = sc.trace_grid_host(W, H, spp, cam, depth, SEED, **dict(kw, stats=False))
                _file(label, sc)
                assert np.array_equal(st["rgb"], plain["rgb"]) and np.array_equal(st["nhit"], plain["nhit"]), what
                assert np.array_equal(st["counters"][:2], plain["counters"][:2]), what
                assert st["counters"][_capi.CNT_NODE_TESTS] > 0 and st["counters"][_capi.CNT_TRI_TESTS] > 0, st["counters"]
                assert plain["counters"][_capi.CNT_NODE_TESTS] == 0 and plain["counters"][_capi.CNT_TRI_TESTS] == 0


@pytest.mark.parametrize("label,mk,cam_of,kw,spp,depth", CASES, ids=IDS)
def test_eye_case(gpu_ready, orc, label, mk, cam_of, kw, spp, depth):
    run_case(orc, label, mk, cam_of, kw, spp, depth)
    print("%s: %s" % (label, sorted(set(LAUNCHES[label]))))


def test_record_is_the_last_eye_pass_in_launch_order(gpu_ready):
    """last_eye_launches() holds one eye pass, in launch order: a scheduled frame's probe, light-tile launch, primary walk and
    scheduled launch; it is cleared by the next eye pass on the handle, whichever entry point runs it -- trace_grid, the Hitpoint
    capture, a PPM session's eye pass, each pass of an SPPM session -- and left alone by a ray query."""
    import cgraytracing_amd as cg

    with cg.Scene(scenes.scene_dragon()) as sc:
        assert sc.last_eye_launches() == []
        sc.trace_grid_host(W, H, 4, PIN(), 5, SEED)
        tree, plain = (1, 0, 0, 0, 0, 0, 0, 256) + (0,) * 7, (0, 0, 0, 0, 0, 0, 0, 256) + (0,) * 7
        assert sc.last_eye_launches() == [(0,) + tree, (0,) + plain, (2, 0, 0, 0) + (0,) * 12, (1,) + tree]
        sc.trace_grid_host(W, H, 2, DOF(), 5, SEED)
        tree_dof = (1, 0, 1) + tree[3:]
        assert sc.last_eye_launches() == [(0,) + tree_dof]
        org, dirs, keys = sc.camera_rays(W, H, 1, PIN(), SEED)
        sc.trace_rays(org, dirs, keys)
        assert sc.last_eye_launches() == [(0,) + tree_dof]
        capture = (1, 1, 0, 1, 0, 0, 1, 256) + (0,) * 7  # (the scene has no glass: the capture's kernel is the general one)
        sc.trace_grid_hitpoints(W, H, 1, PIN(), 5, SEED)
        assert sc.last_eye_launches() == [(0,) + capture]
        sc.trace_grid_host(W, H, 2, DOF(), 5, SEED)
        with sc.ppm_session(W, H, 1, PIN(), 5, SEED, nphotons=0):
            assert sc.last_eye_launches() == [(0,) + capture]
        capture_dof = (1, 1, 1) + capture[3:]
        with sc.sppm_session(W, H, 1, DOF(), initial_radius=2.0) as ses:
            sc.trace_grid_host(W, H, 2, PIN(), 5, SEED)
            ses.add_passes(2, 500)
            assert sc.last_eye_launches() == [(0,) + capture_dof]
        turned = posed(PIN(), "turned")
        sc.trace_grid_host(W, H, 4, turned, 5, SEED)  # posed: no light split, no primary walk
        assert sc.last_eye_launches() == [(0,) + tree[:14] + (1,), (1,) + tree[:14] + (1,)]


def expected_launches():
    """{(kind, TREES .. LTAB, POSE)} the header defines: kind 0 for every row of both lists, kind 1 for every row with SCHED=1,
    kind 2 -- primary_walk_kernel, which fills DOF only -- for DOF 0 and 1"""
    want = set()
    for pose, rows in ((0, variants.eye_variants()), (1, variants.posed_eye_variants())):
        for v in rows:
            want.add((0,) + v[:14] + (pose,))
            if v[14]:
                want.add((1,) + v[:14] + (pose,))
    for dof in (0, 1):
        want.add((2, 0, 0, dof) + (0,) * 12)
    return want


def test_every_eye_kernel_is_launched(gpu_ready, orc):
    """The launches of all cases together are the instantiations the header defines, in both kinds, and nothing else.  A case
    that has not run in this session (a selection by -k) is run here; what it asserts about its frame is its own test's."""
    for case in CASES:
        if case[0] not in LAUNCHES:
            try:
                run_case(orc, *case)
            except AssertionError as e:
                print("%s: %s" % (case[0], str(e).split("\n")[0]))
    seen = {}
    for label in IDS:
        for t in LAUNCHES.get(label, []):
            seen.setdefault(t, label)
    want = expected_launches()
    kinds = ("trace_grid_kernel", "trace_grid_sched_kernel", "primary_walk_kernel")
    print("kind, TREES BEZ DOF GLASS SPH STATS HPS NT SPILL HFONLY DIFF PAIR START LTAB, POSE  <- the first case that launched it")
    print("\n".join("%-23s %s POSE=%d  <- %s" % (kinds[v[0]], " ".join("%d" % x for x in v[1:15]), v[15], seen.get(v)) for v in sorted(want)))
    assert set(seen) == want, "never_launched: %s\nnot_in_table: %s" % (sorted(want - set(seen)), sorted((t, seen[t]) for t in set(seen) - want))
