"""CPU: what the ray and grid entry points answer to bad arguments -- (return code, cgrt_last_error()) of every call of a cross
product of faults, against a table recorded from the library before the checks were merged into check_ray_list and
check_grid_rows (tests/golden/ray_arg_errors.json).  Needs no device: every call is refused, or has nothing to do, before one is
touched (an uncommitted scene, null handles)."""
import ctypes as C
import itertools
import json
import os

import numpy as np

import scenes
from cgraytracing_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_arg_errors.json")
SEED = 12345
N_RAYS = (-1, 0, 4, 2 ** 36 + 1)
DEPTHS = (0, 5, 6)
# (width, height, rows, row_offset, stripe_rows, stripe_rank, stripe_nranks, spp, sample_offset, spp_total, max_depth), lens
# radius.  GRIDS: cgrt_camera_rays refuses each -- test_rays_host.py's four bad grids, then one fault each of the conditions left,
# then every fault at once (the first one wins).  CAMERA_GRIDS: good for cgrt_camera_rays, which reads neither spp_total nor
# max_depth (its device form, which would launch, is not called on these), the last four bad for an eye pass.
GRIDS = [
    ((0, 8, 8, 0, 0, 0, 1, 1, 0, 1, 5), 0.0), ((8, 8, 8, 0, 0, 0, 1, 0, 0, 1, 5), 0.0), ((8, 8, 8, 0, 4, 0, 2, 1, 0, 1, 5), 0.0),
    ((8, 8, 8, -1, 0, 0, 1, 1, 0, 1, 5), 0.0),
    ((8, 0, 8, 0, 0, 0, 1, 1, 0, 1, 5), 0.0), ((8, 8, 0, 0, 0, 0, 1, 1, 0, 1, 5), 0.0), ((8, 8, 8, 0, 0, 0, 1, 1, -1, 1, 5), 0.0),
    ((8, 8, 8, 0, 0, 0, 2, 1, 0, 1, 5), 0.0), ((8, 8, 8, 0, 8, 2, 2, 1, 0, 1, 5), 0.0), ((8, 8, 8, 0, 8, -1, 2, 1, 0, 1, 5), 0.0),
    ((8, 8, 8, 0, 0, 0, 1, 1, 0, 1, 5), -1.0), ((8, 8, 8, 0, 0, 0, 1, 1, 0, 1, 5), float("nan")),
    ((2 ** 20, 8, 2 ** 20, 0, 0, 0, 1, 2 ** 20, 0, 2 ** 20, 5), 0.0),
    ((0, 8, 8, -1, 4, 5, 2, 0, -1, 0, 9), -1.0),
]
CAMERA_GRIDS = [
    ((8, 8, 8, 0, 0, 0, 1, 1, 0, 1, 5), 0.5), ((8, 8, 8, 0, 0, 0, 1, 1, 0, 0, 5), 0.0), ((8, 8, 8, 0, 0, 0, 1, 1, 0, 1, 0), 0.0),
    ((8, 8, 8, 0, 0, 0, 1, 1, 0, 1, 6), 0.0), ((8, 8, 8, 0, 8, 1, 2, 2, 1, 0, 9), 0.0),
]


def _outcomes(L, sc):
    """{entry point: [(rc, message or "") of every case, in the fixed order of the loops below]}; sc: an uncommitted scene."""
    org = np.zeros((4, 3), np.float64)
    dirs = np.tile([0.0, 0.0, 1.0], (4, 1))
    acc, hit_t, tmax = np.zeros((4, 3), np.float64), np.zeros(4, np.float64), np.ones(4, np.float64)
    hit_obj, occluded = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    cnt, count, name = np.zeros(8, np.uint64), C.c_uint64(0), C.create_string_buffer(256)
    out = {}

    def note(entry, rc):
        out.setdefault(entry, []).append((int(rc), L.cgrt_last_error().decode() if rc else ""))

    for scene, have_rays, have_out, n, have_org, have_dir, depth, own in itertools.product(
            (None, sc), (False, True), (False, True), N_RAYS, (False, True), (False, True), DEPTHS, (0, 1)):
        def rays(flags=0):
            r = _capi.Rays(n, org.ctypes.data if have_org else None, dirs.ctypes.data if have_dir else None, None, 0, SEED, depth, flags)
            return C.byref(r) if have_rays else None
        # own: a full trace or a nearest-hit query; occluded given or null; hit_obj given or null
        res = _capi.RayResults(None if own else acc.ctypes.data, None, hit_obj.ctypes.data, hit_t.ctypes.data, None)
        res = C.byref(res) if have_out else None
        note("cgrt_trace_rays", L.cgrt_trace_rays(scene, rays(), res, cnt.ctypes.data, None))
        note("cgrt_trace_rays_host", L.cgrt_trace_rays_host(scene, rays(), res, cnt.ctypes.data))
        for flags in (0, _capi.RAYS_HITPOINTS):
            note("cgrt_trace_rays_variant", L.cgrt_trace_rays_variant(scene, rays(flags), res, name, 256))
        note("cgrt_trace_rays_variant", L.cgrt_trace_rays_variant(scene, rays(), res, None, 256))
        note("cgrt_trace_rays_variant", L.cgrt_trace_rays_variant(scene, rays(), res, name, 0))
        note("cgrt_trace_rays_hitpoints", L.cgrt_trace_rays_hitpoints(scene, rays(), None, 4 if own else 0, C.byref(count) if have_out else None))
        occ = _capi.Occlusion(tmax.ctypes.data, None if own else occluded.ctypes.data)
        occ = C.byref(occ) if have_out else None
        note("cgrt_occlusion_rays", L.cgrt_occlusion_rays(scene, rays(), occ, cnt.ctypes.data, None))
        note("cgrt_occlusion_rays_host", L.cgrt_occlusion_rays_host(scene, rays(), occ, cnt.ctypes.data))
        note("cgrt_occlusion_rays_variant", L.cgrt_occlusion_rays_variant(scene, rays(), name if have_out else None, 0 if own else 256))
        att = _capi.HitAttributes(None, None, acc.ctypes.data, None)
        att = C.byref(att) if have_out else None
        obj = None if own else hit_obj.ctypes.data
        note("cgrt_ray_hit_attributes", L.cgrt_ray_hit_attributes(scene, rays(), obj, hit_t.ctypes.data, att, None))
        note("cgrt_ray_hit_attributes_host", L.cgrt_ray_hit_attributes_host(scene, rays(), obj, hit_t.ctypes.data, att))
        note("cgrt_ray_hit_attributes_host", L.cgrt_ray_hit_attributes_host(scene, rays(), hit_obj.ctypes.data, None if own else hit_t.ctypes.data, att))

    rgb = np.zeros((8, 8, 3), np.float32)
    for (g, lens), good in [(x, False) for x in GRIDS] + [(x, True) for x in CAMERA_GRIDS]:
        for have_cam, have_grid in itertools.product((False, True), (False, True)):
            cam = _capi.Camera((C.c_double * 3)(0, 0, -10), 10.0, 20.0, lens)
            cam = C.byref(cam) if have_cam else None
            grid = _capi.Grid(*g, 0, SEED)
            grid = C.byref(grid) if have_grid else None
            note("cgrt_camera_rays_host", L.cgrt_camera_rays_host(cam, grid, None, None, None))
            if not (good and have_cam and have_grid):  # a good call of the device form would launch
                note("cgrt_camera_rays", L.cgrt_camera_rays(cam, grid, None, None, None, None))
            for scene in (None, sc):
                note("cgrt_trace_grid", L.cgrt_trace_grid(scene, cam, grid, rgb.ctypes.data, None, None, None))
                note("cgrt_trace_grid_host", L.cgrt_trace_grid_host(scene, cam, grid, rgb.ctypes.data, None, None))
                note("cgrt_trace_grid_host", L.cgrt_trace_grid_host(scene, cam, grid, None, None, None))
                note("cgrt_trace_grid_variant", L.cgrt_trace_grid_variant(scene, cam, grid, name, 256))
                note("cgrt_trace_grid_hitpoints", L.cgrt_trace_grid_hitpoints(scene, cam, grid, None, 0, C.byref(count)))

    for scene, obj, n, have in itertools.product((None, sc), (-1, 0, 99), (-1, 0, 4), (False, True)):
        p = org.ctypes.data if have else None
        note("cgrt_intersect_rays", L.cgrt_intersect_rays(scene, obj, p, p, None, n, hit_obj.ctypes.data, hit_t.ctypes.data, acc.ctypes.data))
        note("cgrt_surface_colors", L.cgrt_surface_colors(scene, obj, p, n, acc.ctypes.data))
    for op, have_in, have_out, n in itertools.product((_capi.PROBE_SQRT, 3, 99), (False, True), (False, True), (-1, 0, 2 ** 28 + 1)):
        note("cgrt_math_probe", L.cgrt_math_probe(0, op, hit_t.ctypes.data if have_in else None, n, hit_t.ctypes.data if have_out else None))
    return out


def _run():
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        return _outcomes(_capi.lib(), sc._h)
    finally:
        sc.close()


def record():
    """Writes the table from the library that is loaded -- run by hand on the commit whose answers are to be kept (a development
    build: CGRT_LIB and CGRT_DEV_LIBS=1), never by pytest: python -c "import test_ray_args_host as t; t.record()"."""
    calls = _run()
    outcomes = sorted({o for v in calls.values() for o in v})
    table = {"outcomes": [list(o) for o in outcomes], "calls": {k: [outcomes.index(o) for o in v] for k, v in sorted(calls.items())}}
    with open(GOLDEN, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")


def test_first_error_of_every_bad_call_is_the_recorded_one():
    """Null scene, rays or output; n of -1, 0, 4 and 2^36 + 1; null org3 or dir3; max_depth 0, 5 and 6; a full trace against a
    nearest-hit query; a null `occluded`, hit_obj or hit_t; a null name and cap 0; bad grids (test_rays_host.py's four and one
    per remaining condition) and good ones -- over cgrt_trace_rays and its host, variant and Hitpoint forms, the occlusion and
    hit-attribute entry points, cgrt_camera_rays(_host), the cgrt_trace_grid family, cgrt_intersect_rays, cgrt_surface_colors and
    cgrt_math_probe: the return code and the text of cgrt_last_error() of every call are the recorded ones, in particular which
    fault is reported first."""
    table = json.load(open(GOLDEN))
    want = {k: [tuple(table["outcomes"][i]) for i in v] for k, v in table["calls"].items()}
    got = _run()
    assert sorted(got) == sorted(want)
    total = 0
    for entry in sorted(got):
        assert len(got[entry]) == len(want[entry]), entry
        diff = [(i, g, w) for i, (g, w) in enumerate(zip(got[entry], want[entry])) if g != w]
        assert not diff, (entry, len(diff), diff[:5])
        total += len(got[entry])
    assert total >= 10000, total
    assert not [(k, o) for k, v in got.items() for o in v if o[0] == -3], "a call got as far as the device (CGRT_ERR_DEVICE)"
    assert {o[1] for v in got.values() for o in v} >= {
        "", "null argument", "negative ray count", "null org3 / dir3", "max_depth must be 1..5", "scene not committed",
        "more than 2^36 rays in one call", "null occluded", "empty grid", "bad sample range", "bad stripe_rank", "bad row_offset",
        "stripe_rows must be a positive multiple of 8", "lens_radius must be >= 0", "more than 2^38 camera rays in one call"}
