"""ctypes binding of libcgrt.so (include/cgrt.h).  There is no fallback: if the HIP library has not been
built (``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C cgraytracing_amd/csrc``) importing
this module raises."""
from __future__ import annotations

import ctypes as C
import os

import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CGRT_VERSION = 112  # include/cgrt.h: the ABI this binding was written against
# Development hook: CGRT_LIB names another build of the same ABI (make exp / make fma: other occupancy or contraction choices)
# and is honoured ONLY together with CGRT_DEV_LIBS=1 -- a stray variable must not swap the product's library.
LIB_PATH = os.path.join(_HERE, "libcgrt.so")
if os.environ.get("CGRT_LIB"):
    if os.environ.get("CGRT_DEV_LIBS") == "1":
        LIB_PATH = os.environ["CGRT_LIB"]
        print("cgraytracing_amd: DEVELOPMENT library %s (CGRT_LIB + CGRT_DEV_LIBS=1)" % LIB_PATH, file=sys.stderr)
    else:
        print("cgraytracing_amd: CGRT_LIB ignored (set CGRT_DEV_LIBS=1 to load a development build)", file=sys.stderr)

CGRT_OK = 0
CGRT_NCOUNTERS = 8
CNT_RAYS, CNT_HITPOINTS, CNT_WAVE_ITERS, CNT_NODE_TESTS, CNT_TRI_TESTS = 0, 1, 2, 3, 4


class CgrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libcgrt error %d: %s" % (code, msg))
        self.code = code


class Camera(C.Structure):
    _fields_ = [("cam", C.c_double * 3), ("half_width", C.c_double), ("focus_plane", C.c_double),
                ("lens_radius", C.c_double)]


class PosedCamera(C.Structure):  # cgrt_posed_camera: with GRID_POSED a call's camera argument points at its `base`
    _fields_ = [("base", Camera), ("origin", C.c_double * 3), ("right", C.c_double * 3), ("up", C.c_double * 3),
                ("forward", C.c_double * 3)]  # 144 bytes


class Grid(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rows", C.c_int32), ("row_offset", C.c_int32),
                ("stripe_rows", C.c_int32), ("stripe_rank", C.c_int32), ("stripe_nranks", C.c_int32),
                ("spp", C.c_int32), ("sample_offset", C.c_int32), ("spp_total", C.c_int32),
                ("max_depth", C.c_int32), ("flags", C.c_int32), ("seed", C.c_uint64)]


# Grid.flags: one name per CGRT_GRID_* enumerator of include/cgrt.h (tests/test_capi_host.py compares them with the header)
GRID_STATS, GRID_ACCUMULATE, GRID_SPLIT_SAMPLES, GRID_NO_REORDER, GRID_FORCE_REORDER, GRID_HITPOINTS = 1, 2, 4, 8, 16, 32
GRID_NO_TILE_ORDER, GRID_DIFFUSE_TILES, GRID_NO_SPHERE_PAIRS, GRID_NO_SPHERE_MASKS = 64, 128, 256, 512
GRID_SAMPLE_RELAY, GRID_NO_SAMPLE_RELAY, GRID_SAMPLE_RELAY_4 = 1024, 2048, 4096
GRID_RELAY_MIRROR, GRID_RELAY_NO_MIRROR = 8192, 16384
GRID_RELAY_CHUNKS_FIRST, GRID_RELAY_MIRROR_FIRST, GRID_RELAY_INTERLEAVED, GRID_RELAY_ORDER_MASK = 32768, 65536, 98304, 98304
GRID_NO_LENS_STAGE, GRID_NO_SURE_TILES = 131072, 262144
GRID_RELAY_COST_START, GRID_NO_RELAY_COST_START, GRID_RELAY_BOOST, GRID_NO_RELAY_BOOST = 524288, 1048576, 2097152, 4194304
GRID_NO_LENS_TABLE, GRID_LENS_TABLE = 8388608, 16777216
GRID_NO_INSIDE_TRIPS = 33554432
GRID_POSED = 67108864


class Photons(C.Structure):
    _fields_ = [("light", C.c_double * 3), ("jitter", C.c_double), ("power", C.c_double), ("alpha", C.c_double),
                ("nphotons", C.c_int64), ("hashsize", C.c_int32), ("batch", C.c_int32), ("seed", C.c_uint64),
                ("initial_radius", C.c_double), ("pair_cap", C.c_int64)]


class PpmResult(C.Structure):
    _fields_ = [("image", C.c_void_p), ("rgb8", C.c_void_p), ("hp16", C.c_void_p), ("hp_cap", C.c_uint64),
                ("hp_count", C.c_uint64), ("n_events", C.c_uint64), ("n_pairs", C.c_uint64), ("n_batch_halvings", C.c_uint64),
                ("ms_eye", C.c_double),
                ("ms_table", C.c_double), ("ms_photons", C.c_double), ("ms_gather", C.c_double)]


class PpmSessionInfo(C.Structure):
    _fields_ = [("photons_done", C.c_int64), ("hp_count", C.c_uint64), ("n_events", C.c_uint64), ("n_pairs", C.c_uint64),
                ("n_batch_halvings", C.c_uint64), ("device_bytes", C.c_int64), ("ms_eye", C.c_double), ("ms_table", C.c_double),
                ("ms_photons", C.c_double), ("ms_last_add", C.c_double), ("ms_last_image", C.c_double)]


PPM_SESSION_NO_LOOKAHEAD = 1


class SppmSessionInfo(C.Structure):
    _fields_ = [("passes", C.c_int64), ("photons_done", C.c_int64), ("hp_count", C.c_uint64), ("n_events", C.c_uint64),
                ("n_pairs", C.c_uint64), ("n_batch_halvings", C.c_uint64), ("device_bytes", C.c_int64), ("ms_eye", C.c_double),
                ("ms_table", C.c_double), ("ms_photons", C.c_double), ("ms_update", C.c_double)]


class SceneStats(C.Structure):
    _fields_ = [("n_objects", C.c_int32), ("n_spheres", C.c_int32), ("n_planes", C.c_int32),
                ("n_meshes", C.c_int32), ("n_beziers", C.c_int32), ("n_textures", C.c_int32),
                ("n_trees", C.c_int32), ("committed", C.c_int32), ("n_triangles", C.c_int64),
                ("n_nodes", C.c_int64), ("device_bytes", C.c_int64), ("scene_bytes_fp64", C.c_int64)]


class BuildInfo(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n_device_trees", C.c_int32), ("ms_host_build", C.c_double),
                ("ms_device_build", C.c_double), ("ms_commit", C.c_double)]


BUILD_HOST, BUILD_DEVICE = 0, 1


class RefitInfo(C.Structure):
    _fields_ = [("refits", C.c_int64), ("nwide", C.c_int32), ("ntris", C.c_int32), ("plan_built", C.c_int32),
                ("ms_plan", C.c_double), ("geometry_gen", C.c_uint64)]  # 40 bytes


class RebuildInfo(C.Structure):
    _fields_ = [("rebuilds", C.c_int64), ("nwide", C.c_int32), ("stack_need", C.c_int32), ("balanced", C.c_int32),
                ("levels", C.c_int32), ("readbacks", C.c_int32), ("pad_", C.c_int32), ("ms_last", C.c_double),
                ("scratch_bytes", C.c_int64)]  # 48 bytes


class TreeCost(C.Structure):
    _fields_ = [("node_cost", C.c_double), ("tri_cost", C.c_double), ("root_area", C.c_double)]  # 24 bytes


class Rays(C.Structure):
    _fields_ = [("n", C.c_int64), ("org3", C.c_void_p), ("dir3", C.c_void_p), ("keys", C.c_void_p),
                ("first_index", C.c_int64), ("seed", C.c_uint64), ("max_depth", C.c_int32), ("flags", C.c_int32)]


class RayResults(C.Structure):
    _fields_ = [("acc3", C.c_void_p), ("nhit", C.c_void_p), ("hit_obj", C.c_void_p), ("hit_t", C.c_void_p),
                ("hit_normal3", C.c_void_p)]


class HitAttributes(C.Structure):
    _fields_ = [("prim", C.c_void_p), ("uv2", C.c_void_p), ("color3", C.c_void_p), ("material2", C.c_void_p)]


class GridAov(C.Structure):
    _fields_ = [("albedo3", C.c_void_p), ("normal3", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p),
                ("obj_id", C.c_void_p)]  # 40 bytes


class Occlusion(C.Structure):
    _fields_ = [("tmax", C.c_void_p), ("occluded", C.c_void_p)]


class Bounce(C.Structure):
    _fields_ = [("adj3", C.c_void_p), ("path", C.c_void_p), ("step", C.c_void_p), ("hit_obj", C.c_void_p), ("hit_t", C.c_void_p),
                ("pos3", C.c_void_p), ("normal3", C.c_void_p), ("value3", C.c_void_p), ("child_org3", C.c_void_p),
                ("child_dir3", C.c_void_p), ("child_adj3", C.c_void_p), ("child_path", C.c_void_p), ("child_keys", C.c_void_p),
                ("reserved", C.c_void_p * 2)]  # 15 pointers, 120 bytes


class Wavefront(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("pad_", C.c_int32), ("min_adj", C.c_double), ("work_bytes", C.c_int64),
                ("acc3", C.c_void_p), ("nhit", C.c_void_p), ("hp9", C.c_void_p), ("hp_ray", C.c_void_p), ("hp_path", C.c_void_p),
                ("hp_cap", C.c_uint64), ("reserved", C.c_void_p * 2)]  # 88 bytes


WAVEFRONT_MAX_DEPTH = 31


class RayPixels(C.Structure):
    _fields_ = [("width", C.c_int32), ("rows", C.c_int32), ("spp", C.c_int32), ("pad_", C.c_int32), ("pixel", C.c_void_p)]


class Hitpoints(C.Structure):
    _fields_ = [("n", C.c_int64), ("hp9", C.c_void_p), ("ray", C.c_void_p), ("path", C.c_void_p), ("pixel", C.c_void_p),
                ("width", C.c_int32), ("rows", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("reserved", C.c_void_p * 2)]  # 72 bytes


class PhotonRays(C.Structure):
    _fields_ = [("n", C.c_int64), ("org3", C.c_void_p), ("dir3", C.c_void_p), ("flux3", C.c_void_p), ("keys", C.c_void_p),
                ("draws", C.c_void_p)]


RAYS_STATS = 1
RAYS_NO_SIGN_PASS = 2
RAYS_HITPOINTS = 4
RAYS_SKIP_TRANSPARENT = 8
STEP_NONE, STEP_HITPOINT, STEP_REFLECT, STEP_SPLIT = 0, 1, 2, 3  # cgrt_bounce.step
PROBE_SQRT, PROBE_NORMALIZED, PROBE_SPHERE_LEN, PROBE_SPHERE_LEN_PAIR = 0, 1, 2, 4  # cgrt_math_probe's op (3 is none)
PROBE_INSIDE_LOOP = 5  # cgrt_inside_probe's op

# every symbol include/cgrt.h declares, with its signature
_DP = C.POINTER(C.c_double)
SIGNATURES = {
    "cgrt_version": (C.c_int, []),
    "cgrt_last_error": (C.c_char_p, []),
    # (the posed camera; a library built before it has no such symbol and is refused at load)
    "cgrt_look_at": (C.c_int, [_DP, _DP, _DP, C.c_double, C.c_double, C.c_double, C.POINTER(PosedCamera)]),
    "cgrt_scene_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "cgrt_scene_destroy": (None, [C.c_void_p]),
    "cgrt_scene_set_build": (C.c_int, [C.c_void_p, C.c_int]),
    "cgrt_scene_build_info": (C.c_int, [C.c_void_p, C.POINTER(BuildInfo)]),
    "cgrt_scene_add_sphere": (C.c_int, [C.c_void_p, _DP, C.c_double, _DP, C.c_double, C.c_double]),
    "cgrt_scene_add_texture": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _DP, _DP, C.c_double,
                                         C.c_double, C.c_int]),
    "cgrt_scene_add_plane": (C.c_int, [C.c_void_p, _DP, _DP, _DP, C.c_double, C.c_double, C.c_int]),
    "cgrt_scene_add_mesh_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double, _DP, _DP, C.c_double, C.c_double,
                                           C.c_int]),
    "cgrt_scene_add_mesh_triangles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _DP, C.c_double, C.c_double,
                                                C.c_int]),
    "cgrt_scene_add_bezier": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _DP, _DP, C.c_double, C.c_double]),
    "cgrt_scene_commit": (C.c_int, [C.c_void_p, C.c_int]),
    "cgrt_scene_get_stats": (C.c_int, [C.c_void_p, C.POINTER(SceneStats)]),
    "cgrt_scene_tree_sizes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]),
    "cgrt_scene_tree_dump": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_trace_grid": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "cgrt_unpermute_stripes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "cgrt_trace_grid_host": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "cgrt_trace_grid_hitpoints": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.c_void_p, C.c_uint64,
                                            C.POINTER(C.c_uint64)]),
    "cgrt_ppm_render": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.POINTER(Photons),
                                  C.POINTER(PpmResult)]),
    "cgrt_ppm_session_create": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.POINTER(Photons), C.c_int,
                                          C.POINTER(C.c_void_p)]),
    "cgrt_ppm_session_create_rays": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(RayPixels), C.POINTER(Photons), C.c_int,
                                               C.POINTER(C.c_void_p)]),
    "cgrt_ppm_session_create_hitpoints": (C.c_int, [C.c_void_p, C.POINTER(Hitpoints), C.POINTER(Photons), C.c_int,
                                                    C.POINTER(C.c_void_p)]),
    "cgrt_ppm_session_destroy": (None, [C.c_void_p]),
    "cgrt_ppm_session_add_photons": (C.c_int, [C.c_void_p, C.c_int64]),
    "cgrt_ppm_session_add_photon_rays": (C.c_int, [C.c_void_p, C.POINTER(PhotonRays)]),
    "cgrt_photon_emit": (C.c_int, [C.POINTER(Photons), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "cgrt_photon_emit_host": (C.c_int, [C.POINTER(Photons), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cgrt_photon_ray_events": (C.c_int, [C.c_void_p, C.POINTER(PhotonRays), C.c_uint64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cgrt_ppm_session_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_ppm_session_image_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_ppm_session_hitpoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cgrt_ppm_session_get_info": (C.c_int, [C.c_void_p, C.POINTER(PpmSessionInfo)]),
    "cgrt_sppm_session_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Photons), C.c_int32,
                                           C.POINTER(C.c_void_p)]),
    "cgrt_sppm_session_destroy": (None, [C.c_void_p]),
    "cgrt_sppm_session_pass_grid": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.c_int64]),
    "cgrt_sppm_session_pass_rays": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.c_void_p, C.c_int64]),
    "cgrt_sppm_session_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_sppm_session_image_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_sppm_session_pixels": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cgrt_sppm_session_last_hitpoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cgrt_sppm_session_get_info": (C.c_int, [C.c_void_p, C.POINTER(SppmSessionInfo)]),
    "cgrt_sppm_update_host": (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_void_p]),
    "cgrt_sppm_check_host": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Photons), C.c_int32, C.POINTER(Grid)]),
    "cgrt_tonemap_rgb8": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cgrt_write_png": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_void_p]),
    "cgrt_photon_events": (C.c_int, [C.c_void_p, C.POINTER(Photons), C.c_int, C.c_int64, C.c_int32, C.c_void_p,
                                     C.c_void_p]),
    "cgrt_scene_bvh_dump": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "cgrt_scene_bvh_order": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_void_p]),
    "cgrt_scene_wide_dump": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "cgrt_scene_refit_mesh": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cgrt_scene_refit_mesh_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "cgrt_scene_refit_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RefitInfo)]),
    "cgrt_scene_refit_plan_host": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "cgrt_scene_rebuild_mesh": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cgrt_scene_rebuild_mesh_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "cgrt_scene_rebuild_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RebuildInfo)]),
    "cgrt_scene_mesh_cost": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cgrt_scene_mesh_cost_host": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(TreeCost)]),
    "cgrt_scene_mesh_bounds_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_void_p,
                                              C.c_int32, C.POINTER(C.c_int32)]),
    "cgrt_lens_samples": (C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]),
    "cgrt_surface_colors": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cgrt_trace_grid_variant": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.c_char_p, C.c_size_t]),
    "cgrt_scene_last_tile_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "cgrt_scene_last_sphere_masks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "cgrt_scene_last_sure_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "cgrt_scene_last_sample_relay": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "cgrt_scene_last_relay_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cgrt_scene_last_eye_launches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "cgrt_relay_start_host": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "cgrt_scene_last_relay_start": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "cgrt_scene_last_relay_boost": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_int64]),
    "cgrt_relay_boost_host": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_uint64)]),
    "cgrt_scene_last_lens_stage": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "cgrt_scene_last_lens_table": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "cgrt_scene_last_tile_order_reused": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "cgrt_trace_grid_diffuse_variant": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    "cgrt_scene_last_diffuse_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "cgrt_scene_last_inkernel_diffuse_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "cgrt_trace_rays": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(RayResults), C.c_void_p, C.c_void_p]),
    "cgrt_trace_rays_host": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(RayResults), C.c_void_p]),
    "cgrt_ray_hit_attributes": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.c_void_p, C.c_void_p, C.POINTER(HitAttributes), C.c_void_p]),
    "cgrt_ray_hit_attributes_host": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.c_void_p, C.c_void_p, C.POINTER(HitAttributes)]),
    "cgrt_trace_rays_variant": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(RayResults), C.c_char_p, C.c_size_t]),
    "cgrt_trace_rays_hitpoints": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cgrt_occlusion_rays": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(Occlusion), C.c_void_p, C.c_void_p]),
    "cgrt_occlusion_rays_host": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(Occlusion), C.c_void_p]),
    "cgrt_occlusion_rays_variant": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.c_char_p, C.c_size_t]),
    "cgrt_bounce_rays": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(Bounce), C.c_void_p, C.c_void_p]),
    "cgrt_bounce_rays_host": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(Bounce), C.c_void_p]),
    "cgrt_bounce_rays_variant": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.c_char_p, C.c_size_t]),
    "cgrt_wavefront_rays": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(Wavefront), C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "cgrt_wavefront_rays_host": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.POINTER(Wavefront), C.c_void_p, C.POINTER(C.c_uint64)]),
    "cgrt_wavefront_rays_variant": (C.c_int, [C.c_void_p, C.POINTER(Rays), C.c_char_p, C.c_size_t]),
    "cgrt_scene_last_wavefront": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "cgrt_scene_last_wavefront_rays": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cgrt_camera_rays": (C.c_int, [C.POINTER(Camera), C.POINTER(Grid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_camera_rays_host": (C.c_int, [C.POINTER(Camera), C.POINTER(Grid), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_trace_grid_aov": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.POINTER(GridAov), C.c_void_p, C.c_void_p]),
    "cgrt_trace_grid_aov_host": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.POINTER(GridAov), C.c_void_p]),
    "cgrt_trace_grid_aov_variant": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Grid), C.c_char_p, C.c_size_t]),
    "cgrt_intersect_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "cgrt_math_probe": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "cgrt_scene_inside_spheres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "cgrt_inside_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
}

_lib = None


def lib():
    """The loaded library; raises if libcgrt.so is missing (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "cgraytracing_amd: %s not found -- build the HIP library first "
                "(make -C cgraytracing_amd/csrc, or __graft_entry__.build()). There is no CPU fallback." % LIB_PATH)
        # Load order matters where PyTorch is in the process: libtorch_hip needs "libamdhip64.so" (its bundled copy, found by
        # RPATH) while libcgrt.so needs "libamdhip64.so.7".  With torch first, our NEEDED entry matches the SONAME of the copy
        # already loaded and the process has ONE HIP runtime; with libcgrt.so first, torch's name matches nothing loaded, a
        # second runtime comes in and one of the two then finds "no ROCm-capable device".  So torch, when importable, goes first
        # -- deliberately, also for the torch-free entry points (trace_grid_host, ppm_render): the cost is torch's import time.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.cgrt_version() != CGRT_VERSION:  # same symbols, other struct layouts: refuse rather than corrupt memory
            raise ImportError("cgraytracing_amd: %s is ABI version %d, this binding needs %d -- rebuild it (make -C cgraytracing_amd/csrc)"
                              % (LIB_PATH, L.cgrt_version(), CGRT_VERSION))
        _lib = L
    return _lib


def check(rc):
    if rc < 0:
        raise CgrtError(rc, lib().cgrt_last_error().decode("utf-8", "replace"))
    return rc
