/*
 * cgrt.h -- C ABI of libcgrt.so, the MI355X (gfx950) implementation of the image-grid eye-ray pass of
 * haoyuzhao123/CGRayTracing.
 *
 * The reference has no plugin / FFI seam; the boundary this library replaces is the call
 *
 *     trace(camorg, dir, objs, Vec3(), Vec3(1,1,1), true, 0, htable, w, h);        main.cpp:209 (DoF form :207)
 *
 * inside the pixel/sample loop of render() (main.cpp:185-219), together with everything that call reaches:
 * trace() main.cpp:42-100,129-157 and the intersect()/getSurfaceColor() virtuals of headers/objects.h,
 * headers/bezier.h and headers/texture.h.  One cgrt_trace_grid() call replaces the whole loop nest for a
 * set of image rows.  The scene-building entry points mirror the reference constructors one to one so that
 * a host program can keep main()'s scene code shape.
 *
 * Conventions: plain C, no C++ or torch types.  Every function returns CGRT_OK (0) or a negative error code
 * and never exits or throws; cgrt_last_error() gives the message for the calling thread.  Object handles are
 * not thread-safe; distinct scenes may be used concurrently from different host threads / devices.
 * Threading: launches on ONE scene handle must be ordered by the caller (same stream, or events between streams) --
 * a handle owns device scratch that consecutive launches reuse (CGRT_GRID_SPLIT_SAMPLES chunk sums; the schedule of a
 * cost-ordered frame; the tile order of an image-order one; the queue counter of cgrt_trace_rays, cgrt_trace_rays_hitpoints and cgrt_ppm_session_create_rays, which
 * are such launches (cgrt_occlusion_rays and cgrt_bounce_rays use that counter too); cgrt_ray_hit_attributes is one too: its first call that asks for `prim` builds a table the handle keeps;
 * cgrt_wavefront_rays uses the queue counter and keeps its work memory on the handle, and it synchronises its stream, so it cannot be stream-captured;
 * cgrt_scene_refit_mesh WRITES the scene's device arrays and keeps a plan and arrival counters on the handle: every launch that reads the scene is ordered against it;
 * cgrt_scene_rebuild_mesh WRITES them too, keeps its build scratch on the handle, and it synchronises its stream, so it cannot be stream-captured).
 * All geometry is IEEE double, like the reference (Vec3 = 3 x double, vec3.h:11-30).
 */
#ifndef CGRT_H
#define CGRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGRT_VERSION 112 /* 110: cgrt_photons.initial_radius / .pair_cap, cgrt_ppm_result.n_batch_halvings,
                            cgrt_surface_colors, cgrt_trace_grid_variant; 111: cgrt_scene_wide_dump;
                            112: cgrt_scene_set_build, cgrt_scene_build_info (row f3: structures built on the device);
                            added since without a new number, like the cgrt_ppm_session_* calls: cgrt_trace_rays,
                            cgrt_trace_rays_host, cgrt_trace_rays_variant, cgrt_camera_rays, cgrt_camera_rays_host (caller-supplied rays);
                            cgrt_trace_rays_hitpoints, cgrt_ppm_session_create_rays (photon mapping of caller-supplied rays);
                            cgrt_ppm_session_add_photon_rays, cgrt_photon_emit, cgrt_photon_emit_host, cgrt_photon_ray_events
                            (caller-supplied photons); cgrt_hit_attributes, cgrt_ray_hit_attributes, cgrt_ray_hit_attributes_host
                            (hit attributes of caller-supplied rays); cgrt_occlusion, CGRT_RAYS_SKIP_TRANSPARENT,
                            cgrt_occlusion_rays, cgrt_occlusion_rays_host, cgrt_occlusion_rays_variant (occlusion queries);
                            cgrt_bounce, CGRT_STEP_*, cgrt_bounce_rays, cgrt_bounce_rays_host, cgrt_bounce_rays_variant
                            (bounce queries); cgrt_wavefront, cgrt_wavefront_rays, cgrt_wavefront_rays_host,
                            cgrt_wavefront_rays_variant, cgrt_scene_last_wavefront, cgrt_scene_last_wavefront_rays
                            (wavefront trace); cgrt_hitpoints, cgrt_ppm_session_create_hitpoints (photon mapping of
                            caller-supplied Hitpoints); the cgrt_sppm_session_ calls, cgrt_sppm_update_host, cgrt_sppm_check_host
                            (stochastic progressive photon mapping); cgrt_posed_camera, CGRT_GRID_POSED, cgrt_look_at
                            (posed camera: a library without them has no cgrt_look_at symbol, and CGRT_GRID_POSED was an
                            unknown bit that it ignored); cgrt_scene_refit_mesh, cgrt_scene_refit_mesh_host, cgrt_refit_info,
                            cgrt_scene_refit_info, cgrt_scene_refit_plan_host (refit of committed opaque meshes);
                            cgrt_scene_rebuild_mesh, cgrt_scene_rebuild_mesh_host, cgrt_rebuild_info, cgrt_scene_rebuild_info,
                            cgrt_tree_cost, cgrt_scene_mesh_cost, cgrt_scene_mesh_cost_host (in-place rebuild of device-built
                            opaque meshes, and the tree cost that tells when one pays); cgrt_scene_mesh_bounds_host (a
                            mesh's bounding and cover spheres as the device holds them, for verification) */

enum {
    CGRT_OK = 0,
    CGRT_ERR_INVALID = -1,     /* bad argument / bad handle state                                       */
    CGRT_ERR_IO = -2,          /* mesh file unreadable or malformed                                     */
    CGRT_ERR_DEVICE = -3,      /* HIP runtime error (no GPU, allocation or launch failure)              */
    CGRT_ERR_UNSUPPORTED = -4, /* feature combination not available in this build                        */
    CGRT_ERR_LIMIT = -5        /* scene exceeds a documented limit (e.g. top-level objects per scene)    */
};

typedef struct cgrt_scene cgrt_scene; /* opaque; owns host copies and device buffers */

/* Camera and lens constants of render(), main.cpp:178-181,188-206. */
typedef struct cgrt_camera {
    double cam[3];      /* camorg, main.cpp:181: (0,0,-10)                                              */
    double half_width;  /* the literal 10.0 of main.cpp:188-189: image plane z=0 spans x in [-hw,hw)    */
    double focus_plane; /* main.cpp:178: 20.0                                                            */
    double lens_radius; /* main.cpp:179: 1.5.  0 selects the pinhole call main.cpp:209, >0 the thin-lens
                           call main.cpp:207 with neworg = cam + disc(radius) (sampling.h:35-43)         */
} cgrt_camera;

/* A camera with a position and an orientation: `base` is the camera IN ITS OWN FRAME, exactly as above (image plane z = 0 of
 * that frame, view along its +z), and the frame is placed in the world: a point p of the frame lies at
 *     M(p) = ((origin + right * p.x) + up * p.y) + forward * p.z          (per component, in this order, no contraction).
 * A pinhole ray starts at M(cam) towards M(pixel); a thin-lens ray starts at M(lens point) towards M(focus point): the
 * direction is normalised from WORLD points, so it is unit to the standard of the built-in camera's whatever the last bits of
 * the basis are.  Keys, lens draws and sample order are the built-in camera's.  For the identity frame (origin 0, unit axes)
 * every M(p) is p and the rays are the built-in camera's, bit for bit.
 * WITH CGRT_GRID_POSED IN grid->flags, THE `cam` ARGUMENT OF EVERY ENTRY THAT TAKES (cam, grid) POINTS AT THE `base` OF A
 * cgrt_posed_camera (the sockaddr idiom): cgrt_trace_grid and its _host and _variant forms, cgrt_trace_grid_hitpoints,
 * cgrt_camera_rays and cgrt_camera_rays_host, cgrt_ppm_render, cgrt_ppm_session_create, cgrt_sppm_session_pass_grid.
 * WITHOUT THE FLAG NOTHING CHANGES AND NO BYTE BEYOND THE 48 OF cgrt_camera IS READ.
 * The 12 numbers must be finite, every axis of length 1 within 1e-9 and every pair of axes orthogonal within 1e-9 (dot
 * product), else CGRT_ERR_INVALID.  No handedness is demanded: a mirrored basis (right x up = -forward) mirrors the image. */
typedef struct cgrt_posed_camera {
    cgrt_camera base;  /* the camera in ITS OWN frame, exactly as cgrt_camera                                  */
    double origin[3];  /* world position of the camera frame's (0,0,0)                                         */
    double right[3], up[3], forward[3]; /* world directions of the frame's +x, +y, +z: orthonormal               */
} cgrt_posed_camera;   /* 144 bytes */

/* Host only, plain fp64: fills `out` so that the eye lies at `eye`, the centre of the image looks at `target`, the
 * horizontal field of view is fov_x_deg, the plane of sharp focus lies focus_distance from the eye along `forward` and row 0
 * is the bottom row:  forward = normalize(target - eye), right = normalize(up_hint x forward), up = forward x right,
 * and with D = |target - eye|: origin = target (the image plane passes through the target), base = {cam (0,0,-D), half_width
 * D tan(fov_x/2), focus_plane focus_distance - D, lens_radius}.  With eye (0,0,-10), target (0,0,0), up_hint (0,1,0) and 90
 * degrees this is the built-in camera's frame (origin 0, the unit axes) and its eye.  The eye maps to M(base.cam) = target -
 * forward * D, which is `eye` up to the rounding of that expression.  CGRT_ERR_INVALID: eye == target, up_hint parallel to the view or zero,
 * fov_x_deg outside (0, 180), focus_distance not > 0, lens_radius negative, anything not finite. */
int cgrt_look_at(const double eye[3], const double target[3], const double up_hint[3], double fov_x_deg, double focus_distance,
                 double lens_radius, cgrt_posed_camera *out);

/* Which part of the W x H x spp grid one call renders.  Compile-time constants of the reference
 * (width,height main.cpp:28-29; MAX_DEPTH :35; num_of_samples :177) become fields here. */
typedef struct cgrt_grid {
    int32_t width, height;  /* global image; row 0 is the BOTTOM row (main.cpp:185,189)                  */
    int32_t rows;           /* local rows rendered by this call = rows of the output buffers             */
    int32_t row_offset;     /* contiguous mode (stripe_nranks <= 1): first global row                    */
    int32_t stripe_rows;    /* block-cyclic mode: stripe height in rows (multiple of 8)                  */
    int32_t stripe_rank;    /*   local row j is global row ((j/S)*nranks + rank)*S + j%S                 */
    int32_t stripe_nranks;  /*   rows that fall beyond `height` are left zero                            */
    int32_t spp;            /* samples traced by this call                                               */
    int32_t sample_offset;  /* index of the first sample (keys the lens stream)                          */
    int32_t spp_total;      /* normaliser: output = sum / spp_total (== spp for a single pass)           */
    int32_t max_depth;      /* MAX_DEPTH, main.cpp:35 (1..5)                                             */
    int32_t flags;          /* bit set of CGRT_GRID_* below                                              */
    uint64_t seed;          /* seed of the counter-based lens / Bezier streams                           */
} cgrt_grid;

enum {
    CGRT_GRID_STATS = 1,      /* also count tree-node and triangle tests (CGRT_CNT_NODE_TESTS / _TRI_TESTS)          */
    CGRT_GRID_ACCUMULATE = 2, /* rgb += this pass instead of rgb = this pass: progressive multi-pass rendering with
                                 sample_offset / spp_total, the fp32 replacement for the reference's average.cpp,
                                 which averages nine uint8 images with truncating division (average.cpp:21-64)     */
    CGRT_GRID_NO_REORDER = 8, /* render every tile in image order by its own workgroup.  By default a launch of >= 4 samples
                                 per pixel on a scene with a mesh, bump floor or Bezier object is cost-scheduled: one sample of
                                 every 16x4-pixel wave tile is traced first to measure it; tiles that alone would hold a wave
                                 slot for more than 1/32 of the frame's ideal duration are HEAVY and are rendered through a
                                 queue of (pixel, sample) units that any free lane of any heavy wave takes, their Hitpoint
                                 values parked in HBM and added per pixel afterwards in the reference's order (sample by
                                 sample, emission order inside a sample); the other tiles follow in image order.  Image, hit
                                 counts and counters are bit-identical either way; this flag exists to measure the difference
                                 and to test both paths.  Device memory: up to 12 GiB (at most 1/8 of the device) of parked
                                 values per scene handle, sized by the largest launch (CGRT_DEFER_BYTES overrides)    */
    CGRT_GRID_FORCE_REORDER = 16, /* cost-schedule sphere-only scenes too (off by default: measured no gain on them)    */
    CGRT_GRID_NO_TILE_ORDER = 64, /* image-order launches only: start the tiles in row-major order.  By default an image-order
                                 launch over a scene of spheres and planes with 1..16 reflecting or refracting spheres is
                                 preceded by one small kernel that lists the 32x8-pixel tiles whose primary rays may reach
                                 such a sphere in front of the others (refracting first), and the tiles are started in that
                                 order, so that the frame's longest tiles do not start late.  Every pixel is computed by
                                 the same code either way: image, hit counts and counters are identical                */
    CGRT_GRID_DIFFUSE_TILES = 128, /* image-order launches of sphere-only scenes in tile order, opt-in: the tiles none of whose
                                 primary rays can reach a reflecting or refracting sphere (class 3 of the order) are rendered by
                                 a second launch beside the main one, with a variant in which every ray ends at its first hit
                                 (no normal, no material dispatch, no pending-ray storage; more waves per SIMD).  Same image,
                                 hit counts and counters either way; cgrt_scene_last_diffuse_tiles reads back how many tiles
                                 it took.  Off by default: it executes fewer instructions, but on the measured frame the
                                 longest workgroup bounds the frame and runs slower beside the denser launch */
    CGRT_GRID_NO_SPHERE_PAIRS = 256, /* image-order launches of sphere-only scenes with a refracting sphere that the tile order
                                 serves: by default their kernel tests the spheres two at a time, as two independent
                                 instruction chains (",PAIR=1," in cgrt_trace_grid_variant's name), and in tile order the
                                 class-3 tiles -- those CGRT_GRID_DIFFUSE_TILES would hand to a second launch -- take the
                                 terminal-diffuse body inside that one launch (cgrt_scene_last_inkernel_diffuse_tiles).  This
                                 flag restores the loop over one sphere at a time and the full body for every tile.  Same
                                 image, hit counts and counters either way; it exists to test one against the other      */
    CGRT_GRID_NO_SPHERE_MASKS = 512, /* the terminal-diffuse body (CGRT_GRID_DIFFUSE_TILES, or inside the main launch: see
                                 CGRT_GRID_NO_SPHERE_PAIRS) over a scene of at most 32 spheres and nothing else: by default the
                                 ordering kernel also finds, per 16x4-pixel wave tile, the spheres that some primary ray of the
                                 tile may meet, and the body tests only those (cgrt_scene_last_sphere_masks).  This flag
                                 restores the loop over every sphere.  Same image, hit counts and counters either way; it
                                 exists to test one against the other                                                  */
    CGRT_GRID_SAMPLE_RELAY = 1024, /* the sample relay of the one-launch form above (",PAIR=1," in tile order; not with
                                 CGRT_GRID_DIFFUSE_TILES or CGRT_GRID_SPLIT_SAMPLES), at 32 samples or more: the tiles some
                                 primary ray of which may meet a refracting sphere are rendered by 2 workgroups (up to 4: CGRT_GRID_SAMPLE_RELAY_4), each
                                 with a contiguous chunk of >= 16 samples.  The first sums its chunk; the others park their
                                 Hitpoint values in emission order in an area on the scene handle (sized by the largest
                                 launch: at most 4 GiB and an eighth of the device; without it the launch goes unrelayed), and
                                 the last of a tile's workgroups to finish adds them to the first chunk's sums in chunk order
                                 inside the launch -- the unsplit loop's sequence of additions, so image, hit counts, rays
                                 and Hitpoints are bit-identical; CGRT_CNT_WAVE_ITERS differs (see there).  By default the
                                 relay is engaged when the launch has at least 4 tiles per compute unit, and then in the form
                                 measured fastest (CGRT_GRID_RELAY_MIRROR, interleaved); this flag engages it whatever the
                                 tile count, for those tiles only (cgrt_scene_last_sample_relay tells what a launch did) ... */
    CGRT_GRID_NO_SAMPLE_RELAY = 2048, /* ... and this one switches it off                                              */
    CGRT_GRID_SAMPLE_RELAY_4 = 4096, /* the relay cuts a tile's samples into up to 4 chunks instead of 2, the default: measured
                                 on the 1920x1080 frame at 64 samples, two workgroups a tile gain more than four, which park
                                 half as many values again                                        */
    CGRT_GRID_RELAY_MIRROR = 8192, /* the relay's extent: the tiles that may see a reflecting sphere only (class 2 of the tile
                                 order) are rendered by several workgroups too -- every tile in front of class 3, as many as
                                 the area holds ... */
    CGRT_GRID_RELAY_NO_MIRROR = 16384, /* ... or only those that may see a refracting sphere.  Neither flag: a launch with
                                 CGRT_GRID_SAMPLE_RELAY relays the latter, a launch that relays by default the extent
                                 measured to be the faster.  Same bits either way                  */
    CGRT_GRID_RELAY_CHUNKS_FIRST = 32768, /* the relay's launch order, a two-bit field (CGRT_GRID_RELAY_ORDER_MASK): the workgroups
                                 of the tiles that may see a refracting sphere in front of those of class 2 ...          */
    CGRT_GRID_RELAY_MIRROR_FIRST = 65536, /* ... behind them ...                                                           */
    CGRT_GRID_RELAY_INTERLEAVED = 98304, /* ... or the two merged in proportion.  0: chunks first with CGRT_GRID_SAMPLE_RELAY,
                                 the measured order by default.  cgrt_scene_last_relay_form tells what a launch used       */
    CGRT_GRID_RELAY_ORDER_MASK = 98304,
    CGRT_GRID_RELAY_COST_START = 524288, /* the relay's workgroups of classes 0-2 start longest first, by a probed cost: once per
                                 camera, seed and depth the launch's kernel runs the first samples of those tiles storing
                                 nothing but each wave's iteration count, and a small kernel ranks the workgroups by tile cost
                                 x samples (cgrt_scene_last_relay_start).  The same workgroups run the same bodies: image, hit
                                 counts and all counters are identical.  The default of a launch that relays by default and
                                 names no order; a launch on a captured stream goes without ...                          */
    CGRT_GRID_NO_RELAY_COST_START = 1048576, /* ... and this one switches it off: the order the flags above name           */
    CGRT_GRID_RELAY_BOOST = 2097152, /* a launch with a start table (see CGRT_GRID_RELAY_COST_START) at 48 samples or more: the
                                 relayed tiles whose workgroups are long -- tile cost x samples of a chunk above a share of
                                 the frame's work per workgroup slot (CGRT_RELAY_BOOST=num/den, default 3/4) -- are PROMOTED:
                                 rendered by 3 or 4 workgroups of >= 16 samples instead of 2, parked in a second area on the
                                 handle (at most 3 GiB, both areas within an eighth of the device; the heaviest tiles where it
                                 is short, CGRT_RELAY_BOOST_TILES bounds it).  The additions keep the unsplit loop's order:
                                 image, hit counts, rays and Hitpoints are bit-identical, CGRT_CNT_WAVE_ITERS differs.  A
                                 launch without a table promotes nothing (cgrt_scene_last_relay_boost tells) ...          */
    CGRT_GRID_NO_RELAY_BOOST = 4194304, /* ... and this one switches promotion off (as the knob CGRT_RELAY_BOOST=off does where
                                 no flag speaks); off wins                                                               */
    CGRT_GRID_NO_LENS_STAGE = 131072, /* the terminal-diffuse body inside the main launch (see CGRT_GRID_NO_SPHERE_PAIRS) under a
                                 thin-lens camera: by default a wave finds the accepted lens draws of its next 16 samples
                                 ahead of their use -- attempt 1 of every sample without divergence, then the rejected ones,
                                 every lane on its own (sample, attempt) stream -- and keeps them in LDS the launch already
                                 owns (cgrt_scene_last_lens_stage).  This flag restores one rejection loop per sample, run at
                                 the pace of the wave's unluckiest lane.  The same lens points: same image, hit counts and
                                 counters either way; it exists to test one against the other.  The second launch of
                                 CGRT_GRID_DIFFUSE_TILES always draws sample by sample                                    */
    CGRT_GRID_NO_LENS_TABLE = 8388608, /* the full and the parking body of a glass sphere scene's one-launch tile order (see
                                 CGRT_GRID_NO_SPHERE_PAIRS) under a thin-lens camera: by default a small kernel ahead of the
                                 frame finds the accepted lens draw of every sample of the tiles that may see a mirror or a
                                 glass sphere and leaves it in a table on the handle (8 bytes a pixel and sample, at most
                                 CGRT_LENS_TABLE_BYTES, default 256 MiB; the list's first entries where it is short), and those
                                 tiles' workgroups read their draws there instead of running the rejection loop in lockstep.
                                 The table is kept with the tile order and reused while order, seed, sample_offset and spp
                                 stand (cgrt_scene_last_lens_table): the gain is that of a launch repeated with exactly these.
                                 Writing the table costs more than reading it saves in one frame, so by default a launch
                                 writes it only where that is hidden: on the handle's second stream, beside the cost probe of a
                                 relay that starts by cost (see CGRT_GRID_RELAY_COST_START) -- the first frame of a camera or
                                 a seed.  A launch that finds neither its draws in the table nor a probe to write them beside
                                 -- a pass of a progressive render, whose sample_offset moves -- runs the loop, in the kernels
                                 that have no table code, as under this flag or the knob CGRT_LENS_TABLE=off.  The same lens
                                 points: same image, hit counts and counters either way.  Independent of
                                 CGRT_GRID_NO_LENS_STAGE, which is class 3's.  A captured launch, or one whose table cannot be
                                 allocated, goes without                                                                   */
    CGRT_GRID_LENS_TABLE = 16777216, /* ... and with this flag (or the knob CGRT_LENS_TABLE=on) every such launch that does not
                                 find its draws in the table writes them, ahead of its frame, whether or not anything hides
                                 that: for tests and measurements.  CGRT_GRID_NO_LENS_TABLE wins over it                    */
    CGRT_GRID_NO_SURE_TILES = 262144, /* the terminal-diffuse body, where it has sphere masks (see CGRT_GRID_NO_SPHERE_MASKS, which
                                 implies this flag): by default a second small kernel behind the ordering kernel proves, per
                                 16x4-pixel wave tile of a class-3 tile, whether every primary ray of it -- any pixel, any lens
                                 point -- hits one and the same sphere first (most wave tiles that lie inside one wall), and
                                 such a wave adds that sphere's colour once per sample, addition after addition, without
                                 tracing anything (cgrt_scene_last_sure_tiles).  This flag restores the sample loop.  Same
                                 image, hit counts and counters either way -- CGRT_CNT_RAYS keeps counting the rays the loop
                                 would have traced; it exists to test one against the other                              */
    CGRT_GRID_NO_INSIDE_TRIPS = 33554432, /* the full and the parking body of a glass sphere scene's ",PAIR=1," launch: by default
                                 an iteration in which every lane's ray starts inside the scene's refracting sphere (the
                                 refracted child of an entering ray, the reflected child of a ray inside) tests only the
                                 spheres that ray can hit first -- the sphere itself and those not provably disjoint from it
                                 (cgrt_scene_inside_spheres) -- instead of all of them two at a time.  This flag, or the knob
                                 CGRT_INSIDE_TRIPS=off, restores the pair loop in the same kernel.  Same image, hit counts and
                                 counters either way, CGRT_CNT_WAVE_ITERS included                                       */
    CGRT_GRID_POSED = 67108864, /* 1 << 26: `cam` points at the `base` of a cgrt_posed_camera (see there), whose frame the primary
                                 rays start from.  A posed launch runs kernels of its own (",POSE=1" in cgrt_trace_grid_variant's
                                 name) in the image-order form CGRT_GRID_NO_TILE_ORDER gives, or cost-scheduled where the scene
                                 has a mesh, a bump floor or a Bezier object (the probe traces real rays).  What reasons about
                                 rays in the built-in frame is NOT USED by a posed launch in this version: the tile order of
                                 sphere scenes, sphere masks, sure tiles, the in-launch diffuse body and the pair loop
                                 (CGRT_GRID_DIFFUSE_TILES, _NO_SPHERE_PAIRS), the sample relay with its cost start and boost,
                                 the lens stage and the lens table; nor the light-tile split and the primary walk of scheduled
                                 launches (every tile is rendered by the full variant, no walk ahead), nor CGRT_GRID_FORCE_REORDER.
                                 Flags that ask for these are IGNORED, not refused -- each is "the same image either way" by
                                 its own contract --, the cgrt_scene_last_* readers report that nothing was taken, and the
                                 handle's cached tile order, cost probe and lens table, keyed by the built-in camera's six
                                 numbers, are neither reused nor overwritten.  CGRT_GRID_SPLIT_SAMPLES is supported with a
                                 pose (the same chunks, the same sums); CGRT_GRID_STATS on a mesh scene has no posed kernel:
                                 CGRT_ERR_UNSUPPORTED                                                                     */
    CGRT_GRID_HITPOINTS = 32, /* cgrt_trace_grid_variant only: name the launch of the Hitpoint capture
                                 (cgrt_trace_grid_hitpoints, the eye pass of cgrt_ppm_render) instead of cgrt_trace_grid's;
                                 ignored by the other calls                                                            */
    CGRT_GRID_SPLIT_SAMPLES = 4 /* let several workgroups share a tile's samples: each sums a contiguous chunk of the
                                 samples in fp64 and the chunk sums are added in chunk order by a second kernel.
                                 Reproducible, but the fp64 summation ORDER differs from the sample-by-sample sum
                                 (the last bit of a sum may differ before the rounding to fp32).  It fills the GPU
                                 when a few tiles carry most of the work and exactness of the last fp64 bit is not needed.
                                 (Round 1 forced it on for Bezier scenes; the cost scheduler above now balances them
                                 with the exact summation order, so it is purely opt-in.)                            */
};

/* indices into the uint64 counters[CGRT_NCOUNTERS] array written by cgrt_trace_grid (added to, not reset) */
enum {
    CGRT_CNT_RAYS = 0,      /* trace() invocations past the depth test (main.cpp:46)                     */
    CGRT_CNT_HITPOINTS = 1, /* Hitpoints the reference would have inserted (main.cpp:98)                 */
    CGRT_CNT_WAVE_ITERS = 2,/* wavefront loop iterations (x64 = lane slots; lane utilisation = rays/slots).
                               A measurement of the launch as it ran, not of the image: a launch that relays samples
                               (CGRT_GRID_SAMPLE_RELAY) runs a relayed tile's samples in several shorter waves and
                               counts their iterations, so it differs from the unrelayed launch's                */
    CGRT_CNT_NODE_TESTS = 3,/* tree nodes visited (lane granularity)                                     */
    CGRT_CNT_TRI_TESTS = 4, /* triangle tests                                                            */
    CGRT_NCOUNTERS = 8
};

typedef struct cgrt_scene_stats {
    int32_t n_objects, n_spheres, n_planes, n_meshes, n_beziers, n_textures, n_trees, committed;
    int64_t n_triangles;   /* leaf triangles over all trees (mesh + bump)                                */
    int64_t n_nodes;
    int64_t device_bytes;  /* bytes resident in HBM for this scene                                       */
    int64_t scene_bytes_fp64; /* S_scene of SURVEY.md section 8d: 88/sphere, 100/plane, 56/node + 72/tri, 3/texel */
} cgrt_scene_stats;

int cgrt_version(void);
const char *cgrt_last_error(void);

/* ---- scene construction; each add_* returns the object's position in `objs` (>= 0) or an error (< 0).
 *      Order matters exactly as in vector<Object*> objs (main.cpp:355-366): on equal hit distance the
 *      earlier object wins (main.cpp:57). */
int cgrt_scene_create(cgrt_scene **out);
void cgrt_scene_destroy(cgrt_scene *s);

/* ---- row f3 of SURVEY.md section 8: WHERE the acceleration structures of OPAQUE owners are built -------------------------
 * CGRT_BUILD_HOST (default): KDTree::buildKdTree's leaf order (objects.h:217-267, the same std::sort over the same
 * sequence), the bump mesh of objects.h:480-504 and the height field of texture.h:19-38 are produced on the host by the add_*
 * calls, bit for bit the reference's; the device hierarchies are derived from them.
 * CGRT_BUILD_DEVICE: for objects added AFTER this call whose transparency is < 1e-4, cgrt_scene_commit builds them on the
 * GPU instead -- a bump floor's heights, vertices and grid cells from the texture bytes; an opaque mesh's triangle-level
 * hierarchy from the triangle soup (Morton codes, radix sort, binary radix tree, 4-wide collapse), its bounding and cover
 * spheres.  Transparent owners keep the host build (their normals depend on the reference's leaf ORDER, quirk Q5).
 * Parity class of this mode: tolerance, not bit-exact -- every ray with a unique nearest hit gets the same hit, bit for
 * bit; exact ties (a ray through a shared edge or vertex) go to the lower construction index instead of the reference's
 * leaf-order rule, and heights use a correctly rounded exp where the reference's libm is only within 0.52 ulp.  The
 * verification dumps that describe the reference's tree (cgrt_scene_tree_dump, cgrt_scene_bvh_dump) are empty for a
 * device-built tree; cgrt_scene_wide_dump / cgrt_scene_bvh_order read the device's records back.
 * The environment variable CGRT_BUILD=device makes CGRT_BUILD_DEVICE the default of scenes created afterwards. */
enum { CGRT_BUILD_HOST = 0, CGRT_BUILD_DEVICE = 1 };
int cgrt_scene_set_build(cgrt_scene *s, int mode);

typedef struct cgrt_build_info {
    int32_t mode;            /* CGRT_BUILD_*                                                                              */
    int32_t n_device_trees;  /* trees the commit built on the device                                                      */
    double ms_host_build;    /* wall-clock the add_* calls spent building trees / bump meshes on the host                 */
    double ms_device_build;  /* wall-clock of the device builds inside cgrt_scene_commit (uploads of their inputs included) */
    double ms_commit;        /* wall-clock of cgrt_scene_commit as a whole                                                */
} cgrt_build_info;
int cgrt_scene_build_info(const cgrt_scene *s, cgrt_build_info *out);

/* Sphere(c, r, sc, refl, transp)                                                   objects.h:28-38 */
int cgrt_scene_add_sphere(cgrt_scene *s, const double c[3], double r, const double sc[3], double refl, double transp);

/* Texture(data, n, p, lx, ly, bump)   texture.h:19-38.  rgb = rows*cols*3 bytes as decoded (texel = byte/256,
 * main.cpp:303-316).  Returns a texture id for cgrt_scene_add_plane. */
int cgrt_scene_add_texture(cgrt_scene *s, const uint8_t *rgb, int rows, int cols, const double n[3],
                           const double p[3], double lx, double ly, int isbump);

/* Plane(p, n, sc, refl, transp, tx)   objects.h:480-504.  tex_id < 0: no texture.  A bump texture on a
 * plane with |n.y-1| < 1e-5 builds the displacement mesh and its tree (objects.h:482-503). */
int cgrt_scene_add_plane(cgrt_scene *s, const double p[3], const double n[3], const double sc[3], double refl,
                         double transp, int tex_id);

/* TriangleMesh(filename, a, b, sc, refl, transp, typeofdata)   objects.h:338-403: the three text formats,
 * vertex -> (x, y, -z) * a + b.  A missing file yields an empty mesh like the reference; a malformed file
 * is CGRT_ERR_IO (the reference's behaviour there is undefined). */
int cgrt_scene_add_mesh_file(cgrt_scene *s, const char *filename, double a, const double b[3], const double sc[3],
                             double refl, double transp, int typeofdata);
/* Same object from ntri*9 doubles (pa, pb, pc per triangle, already transformed). */
int cgrt_scene_add_mesh_triangles(cgrt_scene *s, const double *tri9, int ntri, const double sc[3], double refl,
                                  double transp, int typeofdata);

/* Bezier(points, pos, sc, refl, transp)   bezier.h:44-71; 1..6 control points. */
int cgrt_scene_add_bezier(cgrt_scene *s, const double *cp3, int ncp, const double pos[3], const double sc[3],
                          double refl, double transp);

/* Builds the trees (KDTree::buildKdTree, objects.h:217-267, same leaf order), flattens the scene and uploads
 * it to HIP device `device`.  Must be called once before tracing; the scene is immutable afterwards, except for the vertices of
 * an opaque mesh (cgrt_scene_refit_mesh below). */
int cgrt_scene_commit(cgrt_scene *s, int device);
int cgrt_scene_get_stats(const cgrt_scene *s, cgrt_scene_stats *out);

/* ---- host-side prerequisites exposed for verification (tree fingerprints, loader output) ----
 * tree index t: 0..n_trees-1 in object order (a mesh's tree, or a bump plane's tree).
 * node_lr_size: nnodes*3 int32 (left, right, triangle count) in the reference's node numbering;
 * leaf_ids: triangle ids of all leaves in node order; bbox: nnodes*6 (xmin,xmax,ymin,ymax,zmin,zmax).
 * tri9: the tree's triangles in construction order.  Any pointer may be NULL. */
int cgrt_scene_tree_sizes(const cgrt_scene *s, int t, int32_t *nnodes, int32_t *nleaftris, int32_t *ntris);
int cgrt_scene_tree_dump(const cgrt_scene *s, int t, int32_t *node_lr_size, int32_t *leaf_ids, double *bbox,
                         double *tri9);

/* The hierarchy the device actually traverses over the reference's leaves (a binned-SAH tree stored once per ray-direction
 * octant, children near-to-far): *nnodes = nodes per octant; box6 = 8*nnodes x {lo(3), hi(3)}
 * (grown and rounded outward to fp32); skip_leaf2 = 8*nnodes x {skip link relative to the octant's first node,
 * leaf = -1 for inner nodes else (first triangle in leaf order << 4) | count}.  Either array may be NULL
 * (call once with both NULL to size them). */
int cgrt_scene_bvh_dump(const cgrt_scene *s, int tree, int32_t *nnodes, float *box6, int32_t *skip_leaf2);
/* *tri_level = 1 when the owner is opaque and the hierarchy goes down to single triangles: leaf references of
 * cgrt_scene_bvh_dump then index the hierarchy's own triangle order, and order[j] (ntris entries, may be NULL) is the
 * leaf-order index of the triangle at position j; 0: leaf references index the reference's leaf order directly. */
int cgrt_scene_bvh_order(const cgrt_scene *s, int tree, int32_t *tri_level, int32_t *order);
/* The 4-wide form of a triangle-level hierarchy (what the device walks for an opaque owner; *nwide = 0 for other trees):
 * node i has up to four children, box24[(4*i + k)*6 ..] = lo[3], hi[3] of child k and ref4[4*i + k] = its reference --
 * >= 0 a leaf ((first triangle of the hierarchy's order << 4) | count), INT32_MIN an empty slot, otherwise ~(child node).
 * *stack_need = the deepest the walk's stack can get (always below 64).  Two-call protocol: box24 / ref4 may be NULL. */
int cgrt_scene_wide_dump(const cgrt_scene *s, int tree, int32_t *nwide, int32_t *stack_need, float *box24, int32_t *ref4);

/* ---- refit: new vertices for a committed OPAQUE mesh, on the device -----------------------------
 * The one thing that may change in a committed scene.  A mesh that moves (a squashed dragon, a cloth, a skinned bunny) keeps its
 * triangles and their order and gets new vertices: the topology of its 4-wide hierarchy stays, every box is recomputed bottom-up
 * by the builders' rule (the fp64 extent, grown, rounded outward to fp32), and the triangle records, the mesh's bounding sphere,
 * its cover spheres and its tree's error bound follow -- all by kernels, into the device arrays.
 *
 * tri9: ntri * 9 doubles in the layout of cgrt_scene_add_mesh_triangles (pa, pb, pc per triangle, in construction order, already
 * transformed); ntri must be the mesh's triangle count.  After the call every kernel that runs LATER ON `stream` sees the mesh
 * with these vertices.
 * cgrt_scene_refit_mesh: tri9 is a DEVICE pointer on the scene's device, read by the kernels (it must stay valid until they have
 * run; it is not inspected on the host).  The call is asynchronous: it launches kernels on `stream` and returns, with no host
 * read-back and no blocking copy -- except that the FIRST refit of a mesh builds its plan (parents, slots, arrival counts, the
 * triangle order's construction indices) once, which for a device-built tree reads the tree back, and uploads it with blocking
 * copies.  It is a launch on the scene handle (Threading above): the caller orders it against launches on other streams, and
 * against a cgrt_ppm_session's look-ahead batch (destroy the session, or create it with CGRT_PPM_SESSION_NO_LOOKAHEAD);
 * cgrt_trace_grid's own second stream forks from and joins its `stream`, so for it the same stream is order enough.  Two
 * refits enqueued back to back are both correct.
 * cgrt_scene_refit_mesh_host: tri9 is a host pointer; synchronous (null stream), and it refreshes the handle's host mirrors of
 * what the device now owns (the object's bounding sphere, the tree's error bound, the cover spheres, the triangles
 * cgrt_scene_tree_dump returns).  The device entry leaves those mirrors as they were.
 *
 * What may be refitted: a mesh object of a committed scene whose transparency is < 1e-4 and whose tree has the 4-wide form,
 * host-built or device-built.  An empty mesh with ntri == 0 is accepted and nothing is done.  Refused with CGRT_ERR_INVALID and
 * a cgrt_last_error that says which, before any device is touched: a null or uncommitted scene; an `obj` that is no object; a
 * sphere, a plane, a Bezier object; a bump floor; a transparent mesh (its improvement counter makes the reference's leaf order
 * observable, quirk Q5, and a refit cannot reproduce that order); a tree without the wide form (CGRT_TREE=ref); an ntri that
 * is not the mesh's; a null tri9 with ntri > 0.
 * Vertices: the caller supplies FINITE coordinates with |coordinate| < 1e30 -- the bound the box test's proof assumes
 * (DESIGN.md section 4.2); a device pointer's values are not checked.
 * Parity class: that of CGRT_BUILD_DEVICE -- tolerance, not bit-exact.  Every ray with a unique nearest hit gets the hit of a
 * scene freshly committed with the new vertices, bit for bit (boxes are supersets, the triangle test is the same code); exact
 * ties (a ray through a shared edge or vertex) keep the tie order the tree had BEFORE the refit: the lower construction index
 * for a device-built tree, the old leaf order for a host-built one.  Frame time may grow as the mesh moves away from the pose
 * the topology was built for: this call does not rebuild (profiles/refit_probe.json has the cost of two poses).
 * After a refit cgrt_scene_tree_dump and cgrt_scene_bvh_dump, which describe the reference's tree, are empty for the tree, as
 * for a device-built one; cgrt_scene_wide_dump and cgrt_scene_bvh_order read the device's records back.  A cgrt_ppm_session or
 * cgrt_sppm_session created before a refit holds Hitpoints or pixel statistics of the old geometry: its add_photons,
 * add_photon_rays, pass_grid and pass_rays return CGRT_ERR_INVALID ("the scene was refitted after this session was created");
 * its image, hitpoints and get_info calls go on working. */
int cgrt_scene_refit_mesh(cgrt_scene *s, int obj, const double *tri9, int ntri, void *stream);
int cgrt_scene_refit_mesh_host(cgrt_scene *s, int obj, const double *tri9, int ntri);
typedef struct cgrt_refit_info {
    int64_t refits;        /* refits of this mesh so far                                                               */
    int32_t nwide, ntris;  /* wide nodes and triangles of its tree                                                     */
    int32_t plan_built;    /* 1 once the first refit has built the plan                                                */
    double ms_plan;        /* wall-clock of building and uploading the plan, inside that first refit                   */
    uint64_t geometry_gen; /* refits of the SCENE so far: what the photon-mapping sessions remember                    */
} cgrt_refit_info;
int cgrt_scene_refit_info(const cgrt_scene *s, int obj, cgrt_refit_info *out);
/* The refit's plan of tree `tree`, for verification; host-built trees also before the commit.  Per wide node i: parent[i] (-1 for
 * the root, node 0), slot[i] (ref4[4*parent[i] + slot[i]] == ~i) and arrivals[i] (its inner children + 1).  Per position j of the
 * hierarchy's triangle order: src[j], the triangle's construction index (where tri9 holds it).  Two-call protocol as
 * cgrt_scene_wide_dump: with the four arrays NULL only *nwide and *ntris are written; a tree without the wide form gives 0, 0. */
int cgrt_scene_refit_plan_host(const cgrt_scene *s, int tree, int32_t *nwide, int32_t *ntris, int32_t *parent, int32_t *slot,
                               int32_t *arrivals, int32_t *src);

/* ---- rebuild: a new hierarchy for a committed, DEVICE-BUILT opaque mesh, in place -----------------
 * A refit keeps the topology of the pose the tree was built for, and frames get slower as the mesh moves away from it.
 * cgrt_scene_rebuild_mesh gives mesh object `obj` the vertices tri9 (n x 9 doubles, the layout and construction order of
 * cgrt_scene_add_mesh_triangles; the triangle count stays) and the hierarchy a fresh CGRT_BUILD_DEVICE commit of these vertices
 * builds: Morton sort, radix tree (or the balanced fallback, also on CGRT_DEVBUILD_BALANCED), the 4-wide form -- the same tree up
 * to the numbering of wide nodes inside a level, which comes from an atomic counter and is not fixed from run to run.  Triangle
 * records, wide nodes, the object's bounding sphere, the tree's error bound and its cover spheres are recomputed; the handle,
 * every other object and the hit-attribute table stay.  Parity class: that of CGRT_BUILD_DEVICE itself.
 * cgrt_scene_rebuild_mesh: tri9 is a DEVICE pointer on the scene's device.  The call enqueues on `stream` (a hipStream_t, NULL =
 * the null stream) and synchronises it -- the host needs the node count and the stack bound, a few words read back once per
 * batch of levels --, so it cannot be stream-captured.  Work enqueued earlier on the stream sees the old mesh, everything enqueued
 * after the call returns sees the new one.  The hierarchy is built in scratch memory and put in place by device-to-device
 * copies only once the host has seen that it fits the walk's stack: on any error return the committed scene is exactly as
 * before the call.  The scratch (sort keys, the binary tree, boxes, the level queue, staging records) is allocated by the mesh's
 * first rebuild, kept on the handle, counted in cgrt_scene_stats.device_bytes and freed with the scene; later rebuilds allocate
 * nothing.
 * cgrt_scene_rebuild_mesh_host: tri9 is a host pointer; null stream; it also refreshes the triangles cgrt_scene_tree_dump returns.
 * Both refresh the handle's host mirrors of the bounding sphere, the error bound and the cover spheres.
 * Accepted: an opaque mesh of a committed scene whose tree was built on the device.  Refused with CGRT_ERR_INVALID, before any
 * device is touched: everything cgrt_scene_refit_mesh refuses, and a mesh whose tree was built on the host (its arrays have
 * room for that one topology only, and its triangle records are in leaf order: commit the scene under CGRT_BUILD_DEVICE).
 * ntri == 0 is accepted and does nothing.
 * Afterwards: the mesh's refit plan is dropped and built again by its next refit (cgrt_refit_info.plan_built is 0 until then,
 * .refits keeps counting); the scene's geometry count grows by one, so photon-mapping sessions created before refuse as after a
 * refit.  Test aids, read at every build: CGRT_REBUILD_BATCH (levels enqueued per read-back, 1..64, default 8) and
 * CGRT_REBUILD_GRID (workgroups of a level's launch, default sized from ntri); they serve the commit's device build too. */
int cgrt_scene_rebuild_mesh(cgrt_scene *s, int obj, const double *tri9_dev, int ntri, void *stream);
int cgrt_scene_rebuild_mesh_host(cgrt_scene *s, int obj, const double *tri9, int ntri);
typedef struct cgrt_rebuild_info {
    int64_t rebuilds;           /* rebuilds of this mesh so far                                                        */
    int32_t nwide, stack_need;  /* the current tree: wide nodes, deepest the walk's stack can get                      */
    int32_t balanced;           /* 1: the last rebuild needed the balanced fallback                                    */
    int32_t levels, readbacks;  /* the last rebuild: levels of the 4-wide form, read-backs of the level counters       */
    int32_t pad_;
    double ms_last;             /* wall-clock of the last rebuild, its synchronisation included                        */
    int64_t scratch_bytes;      /* device memory the mesh's rebuilds keep on the handle                                */
} cgrt_rebuild_info;            /* 48 bytes */
int cgrt_scene_rebuild_info(const cgrt_scene *s, int obj, cgrt_rebuild_info *out);

/* The surface-area cost of the 4-wide hierarchy the device currently walks for opaque mesh `obj` (host-built, device-built,
 * refitted or rebuilt), read from the device's records.  With S(b) = 2(xy + yz + zx) of a slot's fp32 box, the extents taken
 * as (double)hi - (double)lo: root_area = S of the union of the root node's used slots; node_cost = 1 + the sum over inner
 * slots of S / root_area; tri_cost = the sum over leaf slots of count * S / root_area.  A caller's rule of thumb: rebuild when
 * tri_cost + node_cost exceeds some multiple of its value after the last build; the library picks no multiple.
 * cgrt_scene_mesh_cost: asynchronous on `stream`; cost3_dev = DEVICE room for {node_cost, tri_cost, root_area}.
 * cgrt_scene_mesh_cost_host: null stream, synchronises.  Refusals as for the refit, except that a transparent mesh is refused
 * as having no 4-wide hierarchy; an empty mesh gives zeros. */
typedef struct cgrt_tree_cost { double node_cost, tri_cost, root_area; } cgrt_tree_cost; /* 24 bytes */
int cgrt_scene_mesh_cost(const cgrt_scene *s, int obj, double *cost3_dev, void *stream);
int cgrt_scene_mesh_cost_host(const cgrt_scene *s, int obj, cgrt_tree_cost *out);

/* The bounds the device currently holds for opaque mesh `obj`, for verification: whichever of commit, refit and rebuild wrote them
 * last.  centre3 / s0: the bounding sphere (centre, squared radius); bmax: the tree's bound of |coordinate|; cover4: the mesh's
 * cover spheres, 4 doubles each (centre, radius), *n_cover of them.  cover4 == NULL is the sizing call; with cover4, cap is its
 * room in spheres.  Any other output may be NULL.  Null stream, synchronises (as cgrt_scene_wide_dump after a refit).  Refusals as
 * for cgrt_scene_mesh_cost, under the name "bounds"; an empty mesh has no cover sphere and s0 = -1. */
int cgrt_scene_mesh_bounds_host(const cgrt_scene *s, int obj, double centre3[3], double *s0, float *bmax, double *cover4, int32_t cap,
                                int32_t *n_cover);

/* ---- the hot path -------------------------------------------------------------------------------------
 * Renders grid->rows rows: for every pixel and sample it runs the reference's trace(flag=true) recursion
 * (iteratively) and writes
 *     rgb [rows*width*3] float : (1/spp_total) * sum over samples and diffuse hits of f*adj  (main.cpp:88)
 *     nhit[rows*width]   uint32: number of Hitpoints of the pixel (may be NULL)
 *     counters[CGRT_NCOUNTERS] uint64: totals, ADDED to the existing values (may be NULL)
 * rgb, nhit and counters are DEVICE pointers on the scene's device; the launch is asynchronous on `stream`
 * (a hipStream_t passed as void*, NULL = default stream).  Arithmetic is fp64 on the device; the only fp32
 * rounding is the final store. */
int cgrt_trace_grid(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, float *rgb,
                    uint32_t *nhit, uint64_t *counters, void *stream);

/* ---- caller-supplied rays -----------------------------------------------------------------------------------------
 * cgrt_trace_grid traces the rays its own camera makes (image plane z = 0, view along +z).  cgrt_trace_rays runs the same
 * trace(flag=true) recursion -- the same arithmetic in the same order -- for rays from a buffer: arbitrary cameras (make the
 * rays yourself, or take cgrt_camera_rays' and transform them), nearest-hit queries (picking, visibility), radiance probes. */
typedef struct cgrt_rays {
    int64_t n;               /* rays; 0 is valid and does nothing; more than 2^36: CGRT_ERR_LIMIT                           */
    const double *org3;      /* [n][3]                                                                                        */
    const double *dir3;      /* [n][3] used as given: trace() never normalises its dir (main.cpp:42); unit length is the
                                caller's contract.  A dir of exactly (0,0,0) marks a ray that is NOT traced: its results are
                                those of a miss and it is not counted                                                        */
    const uint64_t *keys;    /* [n] or NULL: key of ray i's Bezier draw streams (the k_smp of cgrt_rng.hpp).
                                NULL: sample_key(pixel_key(seed, first_index + i), 0)                                        */
    int64_t first_index;     /* only used when keys == NULL: lets a caller split a ray set over calls / GPUs                 */
    uint64_t seed;
    int32_t max_depth;       /* 1..5, as cgrt_grid.max_depth; not looked at by a nearest-hit query                           */
    int32_t flags;           /* bit set of CGRT_RAYS_*                                                                       */
} cgrt_rays;
enum {
    CGRT_RAYS_STATS = 1,       /* also count tree-node and triangle tests, like CGRT_GRID_STATS                              */
    CGRT_RAYS_NO_SIGN_PASS = 2,/* hit_normal3 of an opaque mesh: skip the pass that gives it the reference's sign (below); the
                                  vector is then right up to its sign, and the call costs one unpruned mesh walk per ray less */
    CGRT_RAYS_HITPOINTS = 4,   /* cgrt_trace_rays_variant only: name the launch of the Hitpoint capture (cgrt_trace_rays_hitpoints,
                                  the eye stage of cgrt_ppm_session_create_rays) instead of cgrt_trace_rays'; `out` is then not
                                  looked at and may be NULL.  Ignored by the other calls, as CGRT_GRID_HITPOINTS is              */
    CGRT_RAYS_SKIP_TRANSPARENT = 8 /* cgrt_occlusion_rays only: objects with transparency >= 1e-4 are no occluders (shadow rays
                                  through glass).  Ignored by the other calls                                                  */
};

typedef struct cgrt_ray_results {   /* every pointer may be NULL: only the arrays asked for are written */
    double   *acc3;        /* [n][3] sum over the ray tree's Hitpoints of f*adj (main.cpp:88), fp64, added in the reference's
                              emission order (reflect subtree, then refract); NOT divided by anything                       */
    uint32_t *nhit;        /* [n]    Hitpoints of the ray tree                                                              */
    int32_t  *hit_obj;     /* [n]    position in objs of the nearest object the ray itself hits (main.cpp:52-62: strict <,
                              the first object wins), -1 for none                                                            */
    double   *hit_t;       /* [n]    its distance; 0 when hit_obj = -1                                                       */
    double   *hit_normal3; /* [n][3] the normal intersect() returned, before the flip of main.cpp:73-76; 0 on a miss.
                              Spheres, planes, Bezier objects, transparent meshes and transparent bump floors: as the scene walk
                              finds it.  OPAQUE mesh: the reference takes the sign from the parity of its walk's improvement
                              counter (objects.h:321-327), which the pruned scene walk does not know; asking for this array on
                              a scene with an opaque mesh walked in its 4-wide form (the default build) adds a pass that
                              recounts it, unless CGRT_RAYS_NO_SIGN_PASS.  NOT recounted -- the vector is right, its sign is
                              that of ONE improvement (along the ray): an opaque mesh whose hierarchy is not the 4-wide one
                              (the CGRT_TREE=ref development build of the hierarchy) and the triangles of an opaque BUMP
                              FLOOR (a ray reaching the height field from above hits one triangle).  trace() turns an opaque
                              owner's normal against the ray in any case, so no radiance depends on the sign                */
} cgrt_ray_results;

/* DEVICE pointers on the scene's device; asynchronous on `stream`; counters (may be NULL) are ADDED to: CGRT_CNT_RAYS,
 * _HITPOINTS and _WAVE_ITERS (and, with CGRT_RAYS_STATS, the two test counters) mean what they mean for cgrt_trace_grid.
 * With acc3 and nhit both NULL the call is a NEAREST-HIT QUERY: one scene walk per ray, no shading.  Otherwise the full
 * recursion runs per ray.  A ray's results do not depend on the other rays of the call, on their order or on how a ray set
 * is split over calls (with keys, or first_index, kept alike).  This is a launch on the scene handle (Threading above). */
int cgrt_trace_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_results *out, uint64_t *counters, void *stream);
/* HOST pointers: allocates device buffers, runs, synchronises and copies back (counters are overwritten). */
int cgrt_trace_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_results *out, uint64_t *counters);
/* Name of the trace_rays_kernel instantiation cgrt_trace_rays would launch for (scene, rays, out), as cgrt_trace_grid_variant
 * names the eye pass's; only rays->n, max_depth, flags and which of out's pointers are NULL matter (no pointer is read). */
int cgrt_trace_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_results *out, char *name, size_t cap);

/* ---- hit attributes: what a caller needs to shade the hits of a nearest-hit query ----------------------------------
 * cgrt_trace_rays tells which object a ray hits, where and with which normal.  This call adds, per ray, the triangle and
 * the point on it, the reference's surface colour at the hit and the object's material.  It is a pass of its own behind the
 * query: hit_obj / hit_t are what cgrt_trace_rays wrote for the same rays (both required); of `rays` only n, org3 and dir3
 * are read.  Per ray i:
 *   a MISS -- hit_obj[i] outside [0, n_objs); -1 is the query's -- gives prim = -1 and zeros in every other array;
 *   color3    objs[hit_obj]->getSurfaceColor(P), P = org + dir * hit_t (main.cpp:68,77): the bits cgrt_surface_colors(hit_obj,
 *             P) gives -- the flat colour, except on a textured plane, which takes Texture::color inside the texture
 *             rectangle;
 *   material2 the object's reflection and transparency as given to its constructor;
 *   prim      hit object a TriangleMesh: the triangle's index in CONSTRUCTION order -- the order of
 *             cgrt_scene_add_mesh_triangles' tri9, of a file's faces and of cgrt_scene_tree_dump's tri9.  A plane with a bump
 *             floor, hit on its displacement mesh: the index in the bump mesh's construction order (objects.h:485-497), which
 *             is 2 * (i * (cols/3 - 1) + j) + k for triangle k of cell row i, column j, k = 0 for (a,b,c) and 1 for (d,b,c);
 *             again the order of that tree's tri9.  -1 in every other case: sphere, Bezier object, plain plane, the flat part of
 *             a bump plane, or an object none of whose triangles returns exactly hit_t (distances that are not the query's).
 *             Where several triangles of the object return exactly hit_t, prim is the one the scene walk's own tie rule picks
 *             (host-built tree: the reference's -- first inside a leaf, last leaf across leaves, objects.h:281,297;
 *             device-built: the lower construction index), so hit_normal3 is that triangle's normal up to sign;
 *   uv2       for prim >= 0 the reference's own quotients u = det3/det1, v = det4/det1 of Triangle::intersect
 *             (objects.h:101-105; determinants associated as vec3.h:95-97, e1 = pa-pb, e2 = pa-pc, s = pa-org).  By Cramer's
 *             rule the hit point is (1-u-v)*pa + u*pb + v*pc: interpolate per-vertex data with these weights.  Zeros where
 *             prim = -1.
 * n == 0 is valid and does nothing (the scene is not even looked at); more than 2^36 rays: CGRT_ERR_LIMIT.  A null scene,
 * an uncommitted scene, null rays, out, hit_obj or hit_t: CGRT_ERR_INVALID, before any device is touched. */
typedef struct cgrt_hit_attributes {   /* every pointer may be NULL: only the arrays asked for are written */
    int32_t *prim;       /* [n]    */
    double  *uv2;        /* [n][2] */
    double  *color3;     /* [n][3] */
    double  *material2;  /* [n][2]  {reflection, transparency} */
} cgrt_hit_attributes;   /* 32 bytes */

/* DEVICE pointers on the scene's device; asynchronous on `stream`.  With prim or uv2 the winning object's tree is walked
 * again per ray (an opaque owner's walk is pruned at hit_t, a transparent owner's costs what the query's cost); color3 and
 * material2 alone walk nothing.  The first call on a handle that asks for prim builds the leaf-to-construction table on the
 * host and uploads it with a blocking copy (4 bytes per triangle, owned by the handle, counted in
 * cgrt_scene_stats.device_bytes from then on): make that call outside a stream capture.  A launch on the scene handle
 * (Threading above). */
int cgrt_ray_hit_attributes(const cgrt_scene *s, const cgrt_rays *rays, const int32_t *hit_obj, const double *hit_t,
                            const cgrt_hit_attributes *out, void *stream);
/* HOST pointers: allocates device buffers, runs, synchronises and copies back, like cgrt_trace_rays_host. */
int cgrt_ray_hit_attributes_host(const cgrt_scene *s, const cgrt_rays *rays, const int32_t *hit_obj, const double *hit_t,
                                 const cgrt_hit_attributes *out);

/* ---- occlusion queries: "is anything between these two points?" ----------------------------------------------------
 * Shadow rays to a light, ambient occlusion, mutual visibility, culling a custom emitter's photons.  Per ray i
 *   occluded[i] = 1 exactly when some occluder's intersect() returns len < tmax[i] (strict), else 0,
 * where len is the value the nearest-hit query computes for that object and that ray, bit for bit.  The occluders are all
 * objects of the scene; with CGRT_RAYS_SKIP_TRANSPARENT those whose transparency is < 1e-4 (the "opaque" of the scene walk).
 * Without the flag this is hit_obj[i] >= 0 && hit_t[i] < tmax[i] of cgrt_trace_rays on the same org3, dir3 and keys /
 * first_index / seed; with it, the same expression over the scene without its transparent objects.  A tmax that is NaN
 * gives 0, and so does a tmax <= 0 wherever no object returns a length below zero (Sphere::intersect can, by a few ulps, for
 * a ray that starts on the sphere's surface, objects.h:45-68: the identity with the query holds there too); such a ray
 * still counts as traced.  A dir of exactly (0,0,0) marks a ray that is NOT traced: it gives 0 and is not counted, as in
 * cgrt_trace_rays.  Nothing but the bit is returned -- no blocker, no distance: which blocker a walk meets
 * first depends on the walk's order, the bit does not, so a ray's result does not depend on the other rays of the call, on
 * their order or on how a ray set is split over calls (with keys, or first_index, kept alike).
 * Of `rays`, max_depth is not looked at; CGRT_RAYS_NO_SIGN_PASS and CGRT_RAYS_HITPOINTS are ignored; CGRT_RAYS_STATS counts
 * node and triangle tests.  counters (may be NULL) are ADDED to: CGRT_CNT_RAYS by the rays traced, _WAVE_ITERS as usual;
 * _HITPOINTS is untouched.
 * A null scene, null rays or occ, a negative n, a null occluded: CGRT_ERR_INVALID; more than 2^36 rays: CGRT_ERR_LIMIT;
 * n == 0 is valid and does nothing (the scene is not even looked at); otherwise an uncommitted scene: CGRT_ERR_INVALID -- all
 * before any device is touched. */
typedef struct cgrt_occlusion {
    const double *tmax;   /* [n] or NULL.  NULL: no limit (the kernels' 1e10 "no hit yet"); larger values mean the same      */
    uint8_t *occluded;    /* [n] required: 1 or 0                                                                          */
} cgrt_occlusion;         /* 16 bytes */

/* DEVICE pointers on the scene's device; asynchronous on `stream`.  This is a launch on the scene handle (Threading above):
 * it uses the handle's ray-queue counter, like cgrt_trace_rays. */
int cgrt_occlusion_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_occlusion *occ, uint64_t *counters, void *stream);
/* HOST pointers: allocates device buffers, runs, synchronises and copies back (counters are overwritten). */
int cgrt_occlusion_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_occlusion *occ, uint64_t *counters);
/* Name of the occlusion_rays_kernel instantiation cgrt_occlusion_rays would launch for (scene, rays); only rays->flags matters. */
int cgrt_occlusion_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, char *name, size_t cap);

/* ---- bounce queries: one step of trace() for caller-supplied rays ---------------------------------------------------
 * The step between a hit and the next rays, for integrators written on top of the library.  Per ray i: one scene walk -- the
 * nearest-hit query's, keyed by (key, path[i]) --, then exactly what trace() does at that hit (main.cpp:64-157): the normal
 * flip, getSurfaceColor, and either the Hitpoint's value f * adj or the child rays with their throughput -- the mirror
 * direction, the Fresnel split with its Re and 1 - Re weights, total internal reflection, the 1e-4 offsets of the child
 * origins.  The expressions are those of cgrt_trace_rays' kernels in their order (one shared function), so a depth loop over
 * this call -- root rays with adj = (1,1,1) and path 1, the children fed back level by level -- visits the ray tree of
 * cgrt_trace_rays and produces its Hitpoints bit for bit: summed per root in emission order (depth first, the reflected
 * subtree before the refracted one; by path: compare the bits behind the leading 1, a prefix before its extensions) they
 * give acc3, and their {value3, pos3, normal3} are the records of cgrt_trace_rays_hitpoints.  Between two levels the caller
 * may do what the library does not: go deeper than 5, attenuate, cull, stop a subtree, shade some objects itself.
 *   THERE IS NO DEPTH LIMIT in this call: rays->max_depth is not looked at, a mirror or glass hit always yields its
 *   children, and the caller decides when to stop.
 *   step[i]   CGRT_STEP_NONE      a miss, or a ray that is not traced: dir = (0,0,0), as in every ray-list call, or a path of
 *                                 0 or >= 2^31; hit_obj = -1 and zeros in every other array; a ray not traced is not counted
 *             CGRT_STEP_HITPOINT  reflection < 1e-4 and transparency < 1e-4: value3 = f * adj (main.cpp:88); no child
 *             CGRT_STEP_REFLECT   a mirror (child_adj = f * adj * reflection, main.cpp:129-134), or total internal reflection
 *                                 in glass, where child_adj IS adj3[i], bit for bit (main.cpp:144): the reflected child only
 *             CGRT_STEP_SPLIT     glass: the reflected child with f * adj * Re and the refracted one with f * adj * (1 - Re)
 *   Child slots: slot i of the [2n] arrays is the reflected child of ray i, slot n + i its refracted child.  An absent child
 *   is zeros in child_org3 / child_dir3 / child_adj3, child_path 0 and child_keys 0 -- dir = 0 is the "not a ray" mark, so the
 *   five child arrays can be passed straight back as the next call's org3 / dir3 / adj3 / path / keys with n' = 2n; a caller
 *   may instead compact them first.  child_path is 2p for the reflected and 2p + 1 for the refracted child of a ray at
 *   path p (root 1): with the ray's key it keys a Bezier object's draws, as in the full trace.  child_keys is the parent's key
 *   (keys[i], or the one derived from seed and first_index + i).
 * A ray's results do not depend on the other rays of the call, on their order or on how a ray set is split over calls (with
 * keys, or first_index, kept alike).  Of `rays`, max_depth is not looked at; CGRT_RAYS_STATS counts node and triangle tests;
 * the other flags are ignored.  hit_normal3's sign pass has no part here: trace() turns an opaque owner's normal against the
 * ray in any case.  counters (may be NULL) are ADDED to: CGRT_CNT_RAYS by the rays traced, _HITPOINTS by the
 * CGRT_STEP_HITPOINT steps, _WAVE_ITERS as usual.
 * A null scene, null rays or bounce, a negative n: CGRT_ERR_INVALID; more than 2^36 rays: CGRT_ERR_LIMIT; n == 0 is valid and
 * does nothing (the scene is not even looked at); otherwise an uncommitted scene: CGRT_ERR_INVALID -- all before any device is
 * touched.  With every output pointer NULL the call returns CGRT_OK and launches nothing. */
enum {
    CGRT_STEP_NONE = 0,      /* miss, or a ray that is not traced (dir = 0)                                                  */
    CGRT_STEP_HITPOINT = 1,  /* diffuse hit: value3 = f * adj (main.cpp:88); no child                                        */
    CGRT_STEP_REFLECT = 2,   /* mirror, or total internal reflection: the reflected child only                               */
    CGRT_STEP_SPLIT = 3      /* glass: reflected and refracted child                                                         */
};
typedef struct cgrt_bounce {
    /* in, each may be NULL */
    const double   *adj3;       /* [n][3] the ray's throughput, trace()'s adj; NULL: (1,1,1)                                 */
    const uint32_t *path;       /* [n] position in the ray tree: root 1, reflected child 2p, refracted 2p+1; NULL: 1;
                                   0 or >= 2^31: CGRT_STEP_NONE, not traced                                                  */
    /* out, each may be NULL; only the arrays asked for are written */
    uint8_t  *step;             /* [n] CGRT_STEP_*                                                                           */
    int32_t  *hit_obj;          /* [n] as cgrt_ray_results                                                                   */
    double   *hit_t;            /* [n]                                                                                       */
    double   *pos3, *normal3;   /* [n][3] P = org + dir * t and the normal AFTER the flip of main.cpp:73-76, for every hit;
                                   zeros for CGRT_STEP_NONE                                                                  */
    double   *value3;           /* [n][3] f * adj for CGRT_STEP_HITPOINT, else zeros                                         */
    double   *child_org3, *child_dir3, *child_adj3;  /* [2n][3] the child slots (above)                                      */
    uint32_t *child_path;       /* [2n] 2p / 2p+1; 0 for an absent child                                                     */
    uint64_t *child_keys;       /* [2n] the parent's key; 0 for an absent child                                              */
    void     *reserved[2];      /* not looked at; set to NULL: room for two more arrays without another layout               */
} cgrt_bounce;                  /* 15 pointers, 120 bytes */

/* DEVICE pointers on the scene's device; asynchronous on `stream`.  This is a launch on the scene handle (Threading above):
 * it uses the handle's ray-queue counter, like cgrt_trace_rays. */
int cgrt_bounce_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_bounce *bounce, uint64_t *counters, void *stream);
/* HOST pointers: allocates device buffers, runs, synchronises and copies back (counters are overwritten). */
int cgrt_bounce_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_bounce *bounce, uint64_t *counters);
/* Name of the bounce_rays_kernel instantiation cgrt_bounce_rays would launch for (scene, rays); only rays->flags matters. */
int cgrt_bounce_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, char *name, size_t cap);

/* ---- wavefront trace: caller-supplied rays to any depth, inside the library -----------------------------------------
 * The depth loop over cgrt_bounce_rays, on the device: every ray of the list is traced to wf->max_depth levels (1..31, as far
 * as path < 2^31 reaches), one launch per level.  A level's surviving children are appended to a ray queue in device work
 * memory, its Hitpoints are parked with their place in the ray tree; after the last level (or the first empty one) the parked
 * Hitpoints are sorted into emission order and each ray's values are added in that order in fp64 from 0.  For max_depth <= 5
 * acc3, nhit, CGRT_CNT_RAYS / _HITPOINTS and the records are cgrt_trace_rays' and cgrt_trace_rays_hitpoints' bit for bit; for
 * any depth they are those of the caller's loop over cgrt_bounce_rays summed in emission order.
 *   Rays: every rule of the ray-list calls holds -- dir = (0,0,0) marks a ray that is not traced and not counted, with zero
 *   results; keys, or first_index and seed, key the draws; at most 2^36 rays; CGRT_RAYS_STATS counts node and triangle tests;
 *   the other flags and rays->max_depth are not looked at.
 *   min_adj: a child whose throughput has max(x, y, z) < min_adj is not spawned (the test is strict: 0 drops nothing, and
 *   children with adj == 0 are kept -- the full trace's bits and counts).
 *   work_bytes: the rays are processed in slices in ray order; a slice whose queue or parked list does not fit the work memory
 *   is redone in halves (nothing of it has been written, its counters are added only when it finishes).  The results never
 *   depend on work_bytes.  A single ray whose tree does not fit: CGRT_ERR_LIMIT, the message names the bytes needed and given.
 *   0 = room for a level of 2n rays and 8n Hitpoints, at most min(1 GiB, an eighth of the device's memory).
 *   Records: hp9 / hp_ray / hp_path get all rays' Hitpoints by ray index, then emission order; records at or beyond hp_cap
 *   are dropped, *hp_count counts them all.
 * counters (may be NULL) are ADDED to: CGRT_CNT_RAYS and _HITPOINTS are deterministic and equal the bounce loop's sums;
 * CGRT_CNT_WAVE_ITERS measures the run and may differ from run to run (the order in which waves append to the queues is not
 * fixed, so a level's rays meet different lanes; no result depends on that order).
 * A null scene, rays or wf, a negative n, max_depth outside 1..31, a negative or NaN min_adj, a negative work_bytes, hp_cap > 0
 * with hp9, hp_ray and hp_path all NULL: CGRT_ERR_INVALID; more than 2^36 rays: CGRT_ERR_LIMIT; n == 0 is valid and does
 * nothing (the scene is not even looked at); otherwise an uncommitted scene: CGRT_ERR_INVALID -- all before any device is
 * touched. */
typedef struct cgrt_wavefront {
    int32_t  max_depth;   /* 1..31; rays->max_depth is not looked at                                                       */
    int32_t  pad_;
    double   min_adj;     /* >= 0; a child whose child_adj has max(x,y,z) < min_adj (strict) is not spawned; 0 drops nothing */
    int64_t  work_bytes;  /* device work memory for ray queues and parked Hitpoints; 0 = automatic.  The result never
                             depends on it                                                                                 */
    /* out, DEVICE pointers (HOST in the _host form), each may be NULL */
    double   *acc3;       /* [n][3] as cgrt_ray_results.acc3: fp64 sum from 0 in emission order                            */
    uint32_t *nhit;       /* [n]                                                                                           */
    double   *hp9;        /* [hp_cap][9] {value3, pos3, normal3 after the flip}                                            */
    int64_t  *hp_ray;     /* [hp_cap] the record's ray                                                                     */
    uint32_t *hp_path;    /* [hp_cap] its place in the ray's tree                                                          */
    uint64_t  hp_cap;     /* records beyond it are dropped (the last ones); *hp_count still counts them                    */
    void     *reserved[2];/* not looked at; set to NULL                                                                    */
} cgrt_wavefront;         /* 88 bytes */

/* DEVICE pointers on the scene's device.  The call enqueues on `stream` and SYNCHRONISES it: the host reads a few counters
 * back after every level of every slice, and once at the end.  It therefore cannot be captured into a graph.  This is a launch
 * on the scene handle (Threading above): it uses the handle's ray-queue counter and work memory the handle keeps.
 * hp_count (HOST, may be NULL): Hitpoints produced. */
int cgrt_wavefront_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_wavefront *wf, uint64_t *counters,
                        uint64_t *hp_count, void *stream);
/* HOST pointers: allocates device buffers, runs, synchronises and copies back (counters are overwritten). */
int cgrt_wavefront_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_wavefront *wf, uint64_t *counters,
                             uint64_t *hp_count);
/* Name of the wavefront_step_kernel instantiation cgrt_wavefront_rays would launch for (scene, rays); only rays->flags
 * matters. */
int cgrt_wavefront_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, char *name, size_t cap);
/* What the last cgrt_wavefront_rays on the handle did: slices finished, slices redone in halves, and the deepest level that
 * traced a ray; rays31 (may be NULL): rays traced per level, [31], over the finished slices.  Any pointer may be NULL. */
int cgrt_scene_last_wavefront(const cgrt_scene *s, int64_t *slices, int64_t *halvings, int32_t *levels);
int cgrt_scene_last_wavefront_rays(const cgrt_scene *s, int64_t *rays31);

/* The primary rays cgrt_trace_grid starts for sample `sample_offset + k`, k in [0, spp), of every pixel of the grid's rows
 * (contiguous or striped): ray index = (k * rows + local row) * width + w.  org3 / dir3 / keys as in cgrt_rays (any may be
 * NULL); pixels of rows beyond `height` in a striped grid get org = cam, dir = 0, key = 0 and are not traced by
 * cgrt_trace_rays.  max_depth, spp_total and flags are ignored.  More than 2^38 rays: CGRT_ERR_LIMIT.
 * DEVICE pointers on the current device, asynchronous on `stream`. */
int cgrt_camera_rays(const cgrt_camera *cam, const cgrt_grid *grid, double *org3, double *dir3, uint64_t *keys, void *stream);
/* The same bits evaluated on the HOST into host buffers; needs no GPU (like cgrt_lens_samples). */
int cgrt_camera_rays_host(const cgrt_camera *cam, const cgrt_grid *grid, double *org3, double *dir3, uint64_t *keys);

/* ---- grid AOVs: a frame's feature buffers -- albedo, shading normal, depth, coverage and object id of the first hit ------
 * What a denoiser, a compositor, a picker or a debug view asks of a frame, by one launch over the grid: the pixel is the lane,
 * no ray is written to memory.  It is the composition cgrt_camera_rays -> cgrt_trace_rays (nearest-hit query) ->
 * cgrt_ray_hit_attributes folded per pixel, bit for bit:
 *   rays    for the pixel at local row j, column w and k in [0, spp): the ray, key included, that cgrt_camera_rays writes at
 *           index (k * rows + j) * width + w -- pinhole or thin lens, the built-in or a posed camera (CGRT_GRID_POSED),
 *           contiguous or striped rows;
 *   hit     (id_k, t_k, n_k) = the nearest-hit query's hit_obj, hit_t and hit_normal3 for that ray and key; on an opaque mesh
 *           n_k as the pruned scene walk gives it (CGRT_RAYS_NO_SIGN_PASS), since the flip below does not depend on its sign.
 *           A hit contributes c_k = cgrt_ray_hit_attributes' color3 at P = org + dir * t_k, m_k = n_k turned against the ray
 *           (main.cpp:73-76: dot(n, dir) > 0 ? -n : n) and t_k itself; a miss contributes nothing;
 *   sums    in fp64 from +0.0, in the order k = 0, 1, ...;
 *   albedo3, normal3, depth   (float)(sum * (1 / spp_total)); with CGRT_GRID_ACCUMULATE added to the destination in fp32,
 *           exactly as cgrt_trace_grid stores rgb.  normal3 is a mean of unit vectors, not a unit vector;
 *   hits    the samples that hit; added to under CGRT_GRID_ACCUMULATE, else overwritten.  The mean depth over the hits is
 *           depth * spp_total / hits;
 *   obj_id  id_0, the object sample `sample_offset` hits, or -1; every call overwrites it;
 *   rows of a striped grid beyond `height` get zeros and -1; under CGRT_GRID_ACCUMULATE they are left untouched.
 * max_depth is not looked at (0 is as good as 5).  Of the flags only CGRT_GRID_ACCUMULATE and CGRT_GRID_POSED are honoured:
 * every other one is "same image either way" by its own contract and is ignored, CGRT_GRID_STATS too.
 * counters: CGRT_CNT_RAYS is added to by the rays traced (spp per pixel of the image) and CGRT_CNT_WAVE_ITERS by the waves'
 * iterations; CGRT_CNT_HITPOINTS and the rest are untouched.
 * Errors: the argument checks are cgrt_trace_grid's (max_depth apart); a null scene, cam, grid or out and an uncommitted scene
 * give CGRT_ERR_INVALID; everything is refused before a device is touched.  With every pointer of `out` NULL the call is
 * CGRT_OK and launches nothing.
 * A launch on the scene handle (Threading above).  It leaves the handle's cached tile order, cost probe and lens table and
 * every cgrt_scene_last_* record as they were. */
typedef struct cgrt_grid_aov {   /* every pointer may be NULL: only the arrays asked for are written */
    float    *albedo3;  /* [rows][width][3] */
    float    *normal3;  /* [rows][width][3] */
    float    *depth;    /* [rows][width]    */
    uint32_t *hits;     /* [rows][width]    */
    int32_t  *obj_id;   /* [rows][width]    */
} cgrt_grid_aov;        /* 40 bytes */
/* DEVICE pointers on the scene's device; asynchronous on `stream`. */
int cgrt_trace_grid_aov(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_grid_aov *out,
                        uint64_t *counters, void *stream);
/* HOST pointers: allocates device buffers, runs, synchronises and copies back, like cgrt_trace_grid_host (counters are
 * overwritten, not added to).  The device buffers are the call's own, so CGRT_GRID_ACCUMULATE has nothing to add to and is
 * ignored: the arrays are overwritten. */
int cgrt_trace_grid_aov_host(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_grid_aov *out,
                             uint64_t *counters);
/* The kernel instantiation cgrt_trace_grid_aov launches for (scene, cam, grid), e.g.
 * "aov_grid_kernel<TREES=0,BEZ=0,SPH=1,SPILL=0,NT=256>": the row the nearest-hit query of the same scene runs. */
int cgrt_trace_grid_aov_variant(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, char *name, size_t cap);

/* Row e of SURVEY.md section 8: the un-permute that follows the framebuffer gather.  shares = n_present buffers
 * [rows_local][width][channels] float, share-major (share r's local row j is global row ((j / stripe_rows) * nshares + r) *
 * stripe_rows + j % stripe_rows, as in cgrt_grid); frame = [height][width][channels].  Rows of shares >= n_present are
 * written as zero.  DEVICE pointers on the current device; asynchronous on `stream`. */
int cgrt_unpermute_stripes(const float *shares, int n_present, int nshares, int width, int height, int stripe_rows,
                           int rows_local, int channels, float *frame, void *stream);

/* Convenience form with HOST output buffers: allocates device scratch, runs, synchronises and copies back
 * (counters are overwritten, not added to). */
int cgrt_trace_grid_host(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, float *rgb,
                         uint32_t *nhit, uint64_t *counters);

/* The Hitpoint stream the reference would have inserted into its hash table (main.cpp:87-98, hash.h:43-54), for
 * the same grid: up to `cap` records of 10 doubles {f(3) = surface colour * adj, pos(3), normal(3), label} are written
 * to the HOST buffer hp10 in no particular order; label = ((sample_index * (rows*width) + local pixel index) << 4) |
 * position of the hitpoint in that sample's emission order.  *count
 * receives the number of hitpoints produced (if > cap the excess was dropped).  This is the hand-off a photon pass
 * would consume and what parity tests compare with the reference's own records. */
int cgrt_trace_grid_hitpoints(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, double *hp10,
                              uint64_t cap, uint64_t *count);

/* The same hand-off for caller-supplied rays: the Hitpoints of every ray tree of `rays` (DEVICE pointers, as for
 * cgrt_trace_rays; max_depth always counts), up to `cap` records of 10 doubles {f(3), pos(3), normal(3), label} into the HOST
 * buffer hp10, in no particular order; normal is the one AFTER the flip of main.cpp:73-76, as the grid form stores it;
 * label = (ray index << 4) | position of the Hitpoint in the ray tree's emission order.  *count = Hitpoints produced (the
 * excess over cap was dropped).  The sum of a ray's f in emission order is cgrt_ray_results.acc3 of that ray, bit for bit.
 * CGRT_RAYS_STATS / CGRT_RAYS_NO_SIGN_PASS are ignored.  Runs on the null stream and synchronises; a launch on the scene handle. */
int cgrt_trace_rays_hitpoints(const cgrt_scene *s, const cgrt_rays *rays, double *hp10, uint64_t cap, uint64_t *count);

/* ---- row f1 of SURVEY.md section 8: the photon pass and final gather, render() main.cpp:223-258 ----------------
 * Constants of the reference as fields.  The reference races eight OpenMP threads over time-seeded rand(); what is
 * implemented is its SERIAL meaning (photons in index order, photon i on the keyed stream (seed, i)), which the
 * compiled reference reproduces on one thread and which golden vectors pin bit for bit. */
typedef struct cgrt_photons {
    double light[3];   /* lightorg, main.cpp:180: (0, 19.999, 20)                                                  */
    double jitter;     /* main.cpp:240-241: emitter half extent 2.0 (a, b = u*4-2)                                  */
    double power;      /* main.cpp:246: 700 (flux = power * 4*PI per channel)                                      */
    double alpha;      /* main.cpp:36: 0.7                                                                         */
    int64_t nphotons;  /* photons in total (reference: num_photon * num_threads = 20 480 000, main.cpp:223-224)     */
    int32_t hashsize;  /* main.cpp:184: 1000001 (bucket collisions are part of the semantics, hash.h:32-37)         */
    int32_t batch;     /* photons traced per batch (0 = default 1048576); does not change the result               */
    uint64_t seed;
    double initial_radius; /* radius every Hitpoint starts with and, through it, the hash cell length (hash.h:25-26).
                            * The reference ties both to its compile-time `height`: r = 200.0/height (main.cpp:84,183),
                            * 200/768 as committed.  0 selects 200/768; a host mirroring a reference built for another
                            * height passes that build's 200.0/height                                               */
    int64_t pair_cap;  /* capacity of the per-batch (hitpoint, photon hit) pair buffer; 0 = automatic (128 per hitpoint,
                        * between 4 M and 128 M).  A batch whose pairs do not fit is redone in halves -- the result does
                        * not depend on it; tests set it low to drive that path                                     */
} cgrt_photons;

/* What cgrt_ppm_render hands back; every pointer is a HOST buffer owned by the caller and may be NULL. */
typedef struct cgrt_ppm_result {
    double *image;     /* rows*width*3: image[h][w] = sum over the pixel's hitpoints of flux / (PI * r2 * nphotons * spp),
                        * row 0 = bottom (main.cpp:252-258)                                                        */
    uint8_t *rgb8;     /* rows*width*3: the PNG pixels of main.cpp:403-412 -- top row first, gammaCorr() per channel
                        * (row f2; same values as cgrt_tonemap_rgb8(image))                                        */
    double *hp16;      /* hp_cap x 16: per hitpoint {pixel*spp+sample, emission index, f(3), pos(3), normal(3), flux(3),
                        * r2, n} in the reference's table order (bucket, then insertion order)                     */
    uint64_t hp_cap;
    uint64_t hp_count; /* out: hitpoints the eye pass produced                                                     */
    uint64_t n_events; /* out: diffuse photon hits processed (main.cpp:103-125 executions)                         */
    uint64_t n_pairs;  /* out: (hitpoint, photon hit) candidate pairs replayed                                      */
    uint64_t n_batch_halvings; /* out: times a batch overflowed the pair buffer and was redone in halves            */
    double ms_eye, ms_table, ms_photons, ms_gather; /* out: device time of the four stages, milliseconds            */
} cgrt_ppm_result;

/* Eye pass + photon pass + final gather (+ tone map) for grid: the whole of render(), main.cpp:169-258, and the pixel
 * loop of main(), main.cpp:403-412.
 * Sharding (multi-GPU): a hitpoint's history depends only on the ordered photon hits that reach it, never on other
 * hitpoints, so a rank may own just the rows of its grid (a band, or block-cyclic stripes as in cgrt_trace_grid):
 * it traces ALL photons but keeps, searches and updates only its own hitpoints, and its image rows are bit-identical
 * to the same rows of a single full-frame call.  rgb8 needs contiguous rows (it flips them); hp16[0] is
 * local_pixel*spp + sample. */
int cgrt_ppm_render(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_photons *ph,
                    cgrt_ppm_result *out);

/* ---- resumable photon mapping: a live render() that photons are added to --------------------------------------
 * A session keeps what cgrt_ppm_render frees when it returns: the hitpoint table, the pair buffers, the photon producer and
 * a per-pixel index of the hitpoints.  Photon i draws from the keyed stream (seed, i) and a hitpoint replays its events in
 * photon order, so after add_photons calls totalling k photons the image, rgb8 and hitpoints are those of cgrt_ppm_render
 * with nphotons = k and the same other fields, bit for bit, whatever the chunk sizes, batch, pair_cap or halvings.
 * A batch is applied whole or not at all: a failing add_photons (CGRT_ERR_LIMIT when one photon's pairs exceed the pair
 * buffer, say) leaves the state of the first photons_done photons and the session usable.
 * Lifetime and ordering: the scene must outlive its sessions; calls on a session, and on the sessions of one scene, are
 * ordered by the caller like launches on one scene handle (see Threading above).  add_photons and image run on the null
 * stream and synchronise, like cgrt_ppm_render; image_device runs on the caller's stream and the next add_photons waits for it.
 * Device memory: up to ~3 GiB of pair buffers plus two event buffers of batch * 8 * 89 bytes stay allocated while the
 * session lives (cgrt_ppm_session_info.device_bytes). */
typedef struct cgrt_ppm_session cgrt_ppm_session; /* opaque */
enum {
    CGRT_PPM_SESSION_NO_LOOKAHEAD = 1 /* by default, when add_photons (or create) ends, the trace of the next batch from
                                         `done` is enqueued on the session's producer stream, sized as the first batch of a call
                                         of as many photons as the one that just ended ([done, done + batch) after create); a
                                         next call that starts with exactly that batch uses it, any other drops it.  This flag
                                         turns that off. */
};
/* Eye pass + table for grid (same rows / stripes rules as cgrt_ppm_render), then ph->nphotons photons (0 allowed).  ph's
 * other fields (light, jitter, power, alpha, hashsize, seed, initial_radius, batch, pair_cap) are fixed for the session's
 * life.  A grid without hitpoints is valid (its image is zero). */
int cgrt_ppm_session_create(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_photons *ph,
                            int flags, cgrt_ppm_session **out);

/* A session whose Hitpoints come from caller-supplied rays (any camera; probe rays) instead of the grid's own.  The rays
 * are bound to the image the session gathers into by */
typedef struct cgrt_ray_pixels {
    int32_t width, rows;   /* the image the session gathers into: npix = width * rows texels (< 2^31), row 0 = bottom, as
                              cgrt_ppm_result.image; rgb8 flips rows with these                                            */
    int32_t spp;           /* normaliser of the final gather: flux / (PI * r2 * nphotons * spp), main.cpp:256 (>= 1)         */
    int32_t pad_;
    const int64_t *pixel;  /* [n] DEVICE, or NULL.  Texel of ray i in [0, npix); -1 (any negative value): the ray belongs to
                              no texel and is not traced.  NULL: ray i belongs to texel i % npix -- cgrt_camera_rays' ray order */
} cgrt_ray_pixels;
/* Order contract: inside a hash bucket the Hitpoints stand in the insertion order of a serial loop over texels, for each
 * texel over its rays in ray-index order, for each ray in emission order.  For rays in cgrt_camera_rays' order with pixel ==
 * NULL that is the reference's pixel-major, then sample, then emission order: such a session is cgrt_ppm_session_create's on
 * the same grid bit for bit -- image, rgb8, hitpoints, table order -- except that hp16[0] of a ray session is the RAY INDEX
 * (a grid session's is pixel*spp + sample).  The photons' depth limit is rays->max_depth.  A ray with dir = (0,0,0) or
 * without a texel is not traced.  rays' pointers and px->pixel are DEVICE pointers on the scene's device, read before the call
 * returns; CGRT_RAYS_STATS / CGRT_RAYS_NO_SIGN_PASS are ignored.  Every cgrt_ppm_session_* call works on the session as on a
 * grid session's.  The eye stage is a launch on the scene handle (Threading above).  2^31 Hitpoints or more: CGRT_ERR_LIMIT. */
int cgrt_ppm_session_create_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_pixels *px,
                                 const cgrt_photons *ph, int flags, cgrt_ppm_session **out);
/* A session whose Hitpoints are caller-supplied RECORDS instead of the library's own full trace of a grid or of rays: the
 * records cgrt_wavefront_rays returns (any eye depth to 31, min_adj), records a caller shaded or culled between bounce levels,
 * or Hitpoints that come from no ray at all (irradiance probes at given points and normals).  There is no eye stage. */
typedef struct cgrt_hitpoints {
    int64_t n;              /* records; 0 is valid (a session whose image is zero); 2^31 or more: CGRT_ERR_LIMIT      */
    const double   *hp9;    /* [n][9] {value3 = f*adj, pos3, normal3 after the flip}: cgrt_wavefront.hp9's layout;
                               required when n > 0                                                                     */
    const int64_t  *ray;    /* [n] or NULL: id of the ray (or probe) the record belongs to, 0 .. 2^36-1; NULL: i        */
    const uint32_t *path;   /* [n] or NULL: place in that ray's tree (cgrt_bounce: root 1, 2p, 2p+1); NULL: 1          */
    const int64_t  *pixel;  /* [n] or NULL: texel the record gathers into; NULL: ray % (width*rows)                    */
    int32_t width, rows;    /* the image, as cgrt_ray_pixels (npix < 2^31, row 0 = bottom)                             */
    int32_t spp;            /* the gather's normaliser (>= 1)                                                          */
    int32_t max_depth;      /* the PHOTONS' depth limit, 1..5 (a ray session takes it from rays->max_depth)            */
    void *reserved[2];      /* not looked at; NULL                                                                     */
} cgrt_hitpoints;           /* 72 bytes */
/* The arrays are DEVICE pointers on the scene's device, written on the null stream or finished before the call; they are read
 * before the call returns (it runs on the null stream and synchronises, like cgrt_ppm_session_create_rays).
 * Dropped records: a record whose texel is negative or >= npix, whose path is 0 or >= 2^31, whose ray is negative or >= 2^36,
 * or whose pos has a coordinate that is not finite is dropped -- not kept, not counted, in no result.
 * cgrt_ppm_session_info.hp_count is the number of records kept.
 * Order contract: inside a hash bucket (the bucket of pos) the kept records stand by texel ascending, then by ray ascending,
 * then by path in emission order (the paths compared as bit strings behind their leading 1, reflected before refracted, a
 * prefix before its extensions), then by position in the input.  The result depends on the set of records, never on their
 * order in the arrays; input order matters only among records equal in texel, ray and path.  Any number of records per ray.
 * hp16[0] is the record's ray; hp16[1] is its rank among the kept records of that ray in the order above (a double with no
 * 4-bit limit).
 * Equivalence: all records cgrt_wavefront_rays returns at max_depth <= 5 for a ray set, passed with pixel NULL or pixel[i] =
 * ray_pixel[ray[i]], give cgrt_ppm_session_create_rays' session on those rays bit for bit: image, rgb8, hitpoints, n_events.
 * Every cgrt_ppm_session_* call works on the session as on a ray session; its ms_eye is 0.
 * Before any device is touched: a null s, hps, ph or out, n < 0, n > 0 with a null hp9, non-positive width, rows or spp,
 * max_depth outside 1..5, unknown flags, bad ph, an uncommitted scene (whatever n is: the session traces photons through
 * it): CGRT_ERR_INVALID; npix >= 2^31 or n >= 2^31: CGRT_ERR_LIMIT. */
int cgrt_ppm_session_create_hitpoints(const cgrt_scene *s, const cgrt_hitpoints *hps, const cgrt_photons *ph,
                                      int flags, cgrt_ppm_session **out);
/* Waits for anything in flight, then frees the session.  NULL is ignored. */
void cgrt_ppm_session_destroy(cgrt_ppm_session *p);
/* Traces photons [done, done + count) and applies them; returns when they are applied.  count >= 0. */
int cgrt_ppm_session_add_photons(cgrt_ppm_session *p, int64_t count);
/* ---- caller-supplied photons: light a session from any emitter ---------------------------------------------------------
 * cgrt_ppm_session_add_photons traces the photons of the reference's one jittered point light (cgrt_photons.light / jitter /
 * power).  cgrt_ppm_session_add_photon_rays traces photons whose start the caller made: spot, area, coloured or several
 * lights, a light in a fixture.  Past its start a photon runs trace(flag=false) unchanged (main.cpp:101-165). */
typedef struct cgrt_photon_rays {
    int64_t n;              /* photons; 0 is valid and does nothing; more than 2^36: CGRT_ERR_LIMIT                        */
    const double *org3;     /* [n][3]                                                                                      */
    const double *dir3;     /* [n][3] used as given (unit length is the caller's contract).  Exactly (0,0,0): the photon is
                               emitted but goes nowhere -- not traced, no event, yet COUNTED (an emitter that sends part of
                               its power where no photon is wanted keeps its normalisation)                                */
    const double *flux3;    /* [n][3] the flux trace(flag=false) starts with (main.cpp:246: 700*4*PI in each channel)       */
    const uint64_t *keys;   /* [n] or NULL: key of the stream the photon's bounces draw from (half-sphere directions, the
                               glass roulette, Bezier starts).  NULL: stream_key(session seed, photon index, 0, 'phot'), the
                               built-in emitter's                                                                          */
    const uint32_t *draws;  /* [n] or NULL: draws of that stream already consumed (Stream::n of cgrt_rng.hpp).  NULL: 0      */
} cgrt_photon_rays;
/* The photons take the indices [photons_done, photons_done + n) and are applied in that order; photons_done advances by n,
 * photons with dir = 0 included, and the gather stays flux / (PI * r2 * photons_done * spp).  The depth limit, alpha, hashsize,
 * initial_radius, batch and pair_cap are the session's; a batch is applied whole or not at all, and the result does not depend
 * on how a photon set is split over calls, batches or halvings.  Calls of add_photons and add_photon_rays may be mixed on one
 * session.  pr's arrays are DEVICE pointers on the scene's device (written on the null stream or finished), read before the call
 * returns.  No batch is traced ahead when the call ends (the next photons are not known), and a batch that an earlier
 * add_photons traced ahead is dropped.  Multi-GPU: every rank is given the same photons. */
int cgrt_ppm_session_add_photon_rays(cgrt_ppm_session *p, const cgrt_photon_rays *pr);
/* The built-in emitter as a producer of such photons: origin, direction, flux, stream key and stream position of photons
 * [first, first + count) of ph (light, jitter, power and seed are read) -- the values of main.cpp:240-246 as
 * cgrt_ppm_session_add_photons computes them (one inline function is the kernel's emission and both forms here).  draws is the
 * stream position behind the rejection-sampled direction: at least 5, and it differs per photon.  add_photon_rays of these
 * arrays at photons_done = first is add_photons(count) bit for bit.  Any pointer may be NULL; count > 2^36: CGRT_ERR_LIMIT.
 * DEVICE pointers on the current device, asynchronous on `stream`. */
int cgrt_photon_emit(const cgrt_photons *ph, int64_t first, int64_t count, double *org3, double *dir3, double *flux3,
                     uint64_t *keys, uint32_t *draws, void *stream);
/* The same bits evaluated on the HOST into host buffers; needs no GPU. */
int cgrt_photon_emit_host(const cgrt_photons *ph, int64_t first, int64_t count, double *org3, double *dir3, double *flux3,
                          uint64_t *keys, uint32_t *draws);

/* Final gather at the current photon count (main.cpp:252-258), as cgrt_ppm_result.image / .rgb8.  HOST buffers; either may be
 * NULL.  CGRT_ERR_INVALID before the first photon (the reference's flux / (PI r2 0)); rgb8 with stripes: CGRT_ERR_UNSUPPORTED. */
int cgrt_ppm_session_image(const cgrt_ppm_session *p, double *image, uint8_t *rgb8);
/* Same into DEVICE buffers on the session's device, enqueued on `stream` (a hipStream_t as void*, NULL = null stream). */
int cgrt_ppm_session_image_device(const cgrt_ppm_session *p, double *image, uint8_t *rgb8, void *stream);
/* Up to cap hp16 records (layout and table order of cgrt_ppm_result.hp16) of the current state; *count = hitpoints. */
int cgrt_ppm_session_hitpoints(const cgrt_ppm_session *p, double *hp16, uint64_t cap, uint64_t *count);
typedef struct cgrt_ppm_session_info {
    int64_t photons_done;                                   /* photons applied                                       */
    uint64_t hp_count, n_events, n_pairs, n_batch_halvings; /* as cgrt_ppm_result; sums over all photons so far       */
    int64_t device_bytes;                                   /* device memory the session holds                        */
    double ms_eye, ms_table;                                /* device time of the eye pass and table (at create)      */
    double ms_photons;                                      /* photon stage, summed over create and every add_photons */
    double ms_last_add, ms_last_image;                      /* the last add_photons (or create), the last gather     */
} cgrt_ppm_session_info;
int cgrt_ppm_session_get_info(const cgrt_ppm_session *p, cgrt_ppm_session_info *out);

/* ---- stochastic progressive photon mapping (Hachisuka & Jensen 2009): an eye pass per photon pass -----------------------
 * Every cgrt_ppm_session keeps its eye pass's Hitpoints for the whole render, each with a radius, count and flux of its own:
 * memory grows with the sample count, and depth of field, antialiasing and glass edges never converge past that fixed sample
 * set.  Here the statistics belong to the TEXEL, every pass traces fresh eye samples and a fresh photon batch, and the texel's
 * radius shrinks once per pass: memory is one pass's Hitpoints plus 8 doubles per texel, whatever the number of passes.
 * A session owns, per texel p of a width x rows image, N (starts 0), R2 (starts r0^2; r0 and the hash cell length come from
 * initial_radius as for every photon session) and tau[3] (starts 0); and photons_done and passes (start 0).  A pass takes an
 * eye-ray set and a photon count M >= 0:
 *   1. Capture: the Hitpoints of the rays as cgrt_ppm_session_create (a grid) or cgrt_ppm_session_create_rays (rays) captures
 *      them, in the same table (bucket order, per-pixel index); every Hitpoint searches with its texel's current R2.
 *   2. Photons [photons_done, photons_done + M) of the session's keyed stream (seed, i), traced and searched in batches as
 *      cgrt_ppm_session_add_photons does.  The radius is constant during a pass, so the pairs that pass the search's two tests
 *      -- dot(n_h, n_e) > 1e-4 and |pos - P|^2 <= R2 -- are the accepted set.  The candidate multiset is the photon pass's
 *      own, the reference's two quirks included: hash cells slightly shorter than r0 (hash.h:25-26; a photon within R2 of a
 *      Hitpoint but two cells away is not a candidate) and a bucket walked once per colliding cell (hash.h:35-37; with a small
 *      hashsize a photon can count twice for one Hitpoint).
 *   3. Per Hitpoint h, a left fold from 0 over its pairs in slot order (photon, then path segment), across the batches:
 *      Phi_h = Phi_h + f_h * flux_e * (1 / PI);  M_h += 1.
 *   4. Per texel, a left fold from 0 over its Hitpoints in the per-pixel index order: Phi_p += Phi_h;  M_p += M_h.
 *   5. Only where M_p > 0, in fp64, in this order:  Nn = N + alpha * M_p;  g = Nn / (N + M_p);  R2 = R2 * g;
 *      tau = (tau + Phi_p) * g;  N = Nn.
 *   6. photons_done += M; passes += 1 -- also when the rays produce no Hitpoint; M = 0 captures, counts the pass and changes
 *      nothing else of the texels' N, R2 and tau.
 * image[p] = tau * (1 / (PI * R2 * (photons_done * spp))), row 0 = bottom; rgb8 as cgrt_ppm_session_image's.
 * A batch is applied whole or not at all; the state after a pass does not depend on batch, pair_cap or halvings; a failing pass
 * leaves the texels, photons_done and passes of the pass before (its Hitpoints are gone: last_hitpoints then gives none) and
 * the session usable.  A texel's history depends only on its own rays and on all photons, so block-cyclic stripes give the rows
 * of the full frame, every rank tracing all photons.  Radii only shrink, which keeps the session's hash grid valid: alpha
 * must lie in (0, 1].
 * Lifetime, ordering and streams as for cgrt_ppm_session: passes, image and pixels run on the null stream and synchronise;
 * image_device runs on the caller's stream and the next pass waits for it.  Device memory: the texels, the last pass's table
 * (freed before the next pass captures), the pair buffers (they grow to the largest pass's need), two event buffers. */
typedef struct cgrt_sppm_session cgrt_sppm_session; /* opaque */
/* ph->nphotons is not looked at; ph's other fields are fixed for the session's life.  photon_depth: the photons' depth limit,
 * 1..5.  flags: 0.  Before any device is touched: a null ph, s or out, non-positive width, rows or spp, photon_depth outside
 * 1..5, bad ph (as cgrt_ppm_session_create), alpha not in (0, 1] (NaN included), flags != 0, an uncommitted scene (the last of
 * the checks): CGRT_ERR_INVALID; 2^31 texels or more: CGRT_ERR_LIMIT. */
int cgrt_sppm_session_create(const cgrt_scene *s, int32_t width, int32_t rows, int32_t spp, int32_t photon_depth,
                             const cgrt_photons *ph, int32_t flags, cgrt_sppm_session **out);
/* Waits for anything in flight, then frees the session.  NULL is ignored. */
void cgrt_sppm_session_destroy(cgrt_sppm_session *p);
/* A pass whose eye rays are the built-in camera's: grid->width, rows and spp must be the session's; sample_offset, seed,
 * max_depth (the eye depth) and the scheduling flags are the caller's (a renderer passes sample_offset = passes * spp).  The
 * first pass fixes the stripes (stripe_rows, stripe_rank, stripe_nranks; a contiguous grid is one value whatever those fields
 * hold); a later pass with other stripes is CGRT_ERR_INVALID, as are a grid cgrt_ppm_session_create refuses and nphotons < 0
 * -- all before any device is touched. */
int cgrt_sppm_session_pass_grid(cgrt_sppm_session *p, const cgrt_camera *cam, const cgrt_grid *grid, int64_t nphotons);
/* A pass over caller-supplied rays: ray i belongs to texel pixel[i] ([n] DEVICE int64; negative: the ray is not traced), or
 * with pixel == NULL to texel i % (width * rows).  Every rule of cgrt_ppm_session_create_rays holds: DEVICE arrays read before
 * the call returns, dir = (0,0,0) is not traced, keys, the order contract; rays->max_depth is the eye depth, 1..5. */
int cgrt_sppm_session_pass_rays(cgrt_sppm_session *p, const cgrt_rays *rays, const int64_t *pixel, int64_t nphotons);
/* The image at the current state.  HOST buffers; either may be NULL.  CGRT_ERR_INVALID before the first photon (tau / (PI R2 0));
 * rgb8 on a striped session: CGRT_ERR_UNSUPPORTED. */
int cgrt_sppm_session_image(const cgrt_sppm_session *p, double *image, uint8_t *rgb8);
/* Same into DEVICE buffers on the session's device, enqueued on `stream` (a hipStream_t as void*, NULL = null stream). */
int cgrt_sppm_session_image_device(const cgrt_sppm_session *p, double *image, uint8_t *rgb8, void *stream);
/* The texels: px8 is a HOST buffer of [width * rows][8] doubles = {N, R2, tau[3], M_p of the last pass, Hitpoints of the last
 * pass, 0}. */
int cgrt_sppm_session_pixels(const cgrt_sppm_session *p, double *px8);
/* Up to cap hp16 records of the LAST pass's table, in cgrt_ppm_session_hitpoints' layout and order, with flux = Phi_h, r2 = the
 * radius the pass searched with, n = M_h; *count = its Hitpoints. */
int cgrt_sppm_session_last_hitpoints(const cgrt_sppm_session *p, double *hp16, uint64_t cap, uint64_t *count);
typedef struct cgrt_sppm_session_info {
    int64_t passes, photons_done;
    uint64_t hp_count;                            /* Hitpoints of the last pass                                        */
    uint64_t n_events, n_pairs, n_batch_halvings; /* as cgrt_ppm_result; sums over all passes so far                   */
    int64_t device_bytes;                         /* device memory the session holds now                               */
    double ms_eye, ms_table, ms_photons, ms_update; /* device time of the last pass's four stages, milliseconds        */
} cgrt_sppm_session_info;
int cgrt_sppm_session_get_info(const cgrt_sppm_session *p, cgrt_sppm_session_info *out);
/* Host only, no GPU.  cgrt_sppm_update_host: step 5 for one texel, the very function the kernel calls; out5 = {N, R2, tau[3]}.
 * cgrt_sppm_check_host: the argument checks of cgrt_sppm_session_create that need no scene and, where grid is not NULL, of a
 * first pass's grid against such a session. */
int cgrt_sppm_update_host(double N, double R2, const double *tau3, double M, const double *phi3, double alpha, double *out5);
int cgrt_sppm_check_host(int32_t width, int32_t rows, int32_t spp, int32_t photon_depth, const cgrt_photons *ph, int32_t flags,
                         const cgrt_grid *grid);

/* ---- row f2 of SURVEY.md section 8: tone map, flip, PNG (util.h:45-47, main.cpp:403-412) ----------------------
 * rgb8[(height-1-h)*width + w][c] = int(pow(1 - exp(-image[h][w][c]), 1/2.2) * 255 + .5) computed on `device`;
 * HOST buffers.  NaN and negative inputs give 0 (the reference's int(NaN) is undefined). */
int cgrt_tonemap_rgb8(int device, const double *image, int width, int height, uint8_t *rgb8);

/* 8-bit RGB PNG, rows top to bottom, like stbi_write_png("test.png", width, height, 3, data, width*3) at main.cpp:412.
 * Self-contained encoder (stored deflate blocks; no zlib dependency).  Host only. */
int cgrt_write_png(const char *path, int width, int height, const uint8_t *rgb8);

/* Verification probe for photon paths: the diffuse hits (the events the serial loop of main.cpp:103-125 processes) of
 * photons [first, first+count): events9 = count*8 slots of 9 doubles {P(3), n(3), flux(3)}, slot = (photon-first)*8 +
 * path segment; valid = one byte per slot.  HOST buffers. */
int cgrt_photon_events(const cgrt_scene *s, const cgrt_photons *ph, int max_depth, int64_t first, int32_t count,
                       double *events9, uint8_t *valid);

/* The same probe for caller-supplied photons: pr's arrays are HOST pointers here, pr->n <= 2^20; seed and first_index make the
 * default stream key (seed, first_index + i) where pr->keys is NULL.  events9 = n*8 slots, valid = n*8 bytes, as above. */
int cgrt_photon_ray_events(const cgrt_scene *s, const cgrt_photon_rays *pr, uint64_t seed, int64_t first_index, int max_depth,
                           double *events9, uint8_t *valid);

/* Function-level probe used by parity tests: objs[obj]->intersect(org, dir, len, normal) for n rays on the
 * device (host pointers; keys: per-ray stream key for Bezier draws, may be NULL). */
int cgrt_intersect_rays(const cgrt_scene *s, int obj, const double *org3, const double *dir3, const uint64_t *keys,
                        int n, int32_t *hit, double *len, double *normal3);

/* Function-level probe: objs[obj]->getSurfaceColor(P) for n points on the device -- the flat colour, or for a textured
 * plane Texture::color (texture.h:39-72: three axis-aligned orientations, nearest texel) with the flat colour outside
 * the texture rectangle (objects.h:533-539).  HOST buffers, n*3 doubles each. */
int cgrt_surface_colors(const cgrt_scene *s, int obj, const double *points3, int n, double *colors3);

/* Name of the trace_grid_kernel instantiation cgrt_trace_grid would launch for (scene, cam, grid) -- the kernel name a
 * rocprofv3 kernel trace shows; written NUL-terminated into name[cap].  With CGRT_GRID_HITPOINTS in grid->flags: the
 * instantiation the Hitpoint capture launches (",SPILL=1" when objects beyond the ones it keeps in LDS are read from HBM). */
int cgrt_trace_grid_variant(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, char *name, size_t cap);

/* Verification / development aid: the tile order the LAST cgrt_trace_grid on this handle started its tiles in (see
 * CGRT_GRID_NO_TILE_ORDER).  *n_tiles = the number of 32x8 tiles it ordered, 0 when that launch ran no ordering kernel (then
 * nothing else is written).  With cap >= *n_tiles: synchronises the device and copies to HOST memory (each may be NULL)
 * plan5[c] = tiles of classes < c (c = 0..4; classes: 0 centre on a refracting sphere, 1 may see a refracting sphere, 2 may
 * see a reflecting sphere, 3 the rest), list[i] = the tile (ty * ceil(width / 32) + tx) workgroup i rendered, cls[t] = class
 * of tile t. */
int cgrt_scene_last_tile_order(const cgrt_scene *s, uint32_t *plan5, uint32_t *list, uint8_t *cls, int64_t cap, int64_t *n_tiles);

/* The sphere masks of that launch (see CGRT_GRID_NO_SPHERE_MASKS): *n_wave_tiles = the number of 16x4 wave tiles
 * (ceil(width / 16) x ceil(rows / 4), numbered wy * ceil(width / 16) + wx) it wrote a mask for, 0 when it wrote none.  With
 * cap >= *n_wave_tiles: synchronises the device and copies them to HOST memory; bit i of masks[wave tile] = sphere i (in the
 * order the objects were added) may be met by a primary ray of the wave tile. */
int cgrt_scene_last_sphere_masks(const cgrt_scene *s, uint32_t *masks, int64_t cap, int64_t *n_wave_tiles);
/* The sure tiles of that launch (see CGRT_GRID_NO_SURE_TILES), in the same form: sure[wave tile] = the sphere every primary ray of
 * the wave tile hits first, or 255 -- none proven, or the wave tile's 32x8 tile is not of class 3.  *n_wave_tiles = 0 when the
 * launch wrote none. */
int cgrt_scene_last_sure_tiles(const cgrt_scene *s, uint8_t *sure, int64_t cap, int64_t *n_wave_tiles);
/* Whether the LAST cgrt_trace_grid on the handle ran no ordering kernel because the order (and masks) it had computed for the
 * same camera, frame geometry, rows and stripe were still in the handle's buffer: *reused = 1, else 0.  An order depends on
 * nothing else -- not on the seed, the samples or the depth -- so the passes of a progressive render compute it once.
 * The stored order lives in the handle's launch scratch: as for every launch on a handle, the caller orders launches on one
 * handle, and launches of one handle that are in flight together on different streams must use the same camera and frame.
 * A handle one of whose launches was captured into a graph (hipStreamBeginCapture) reuses nothing from then on: a captured
 * launch runs later, and again at every replay. */
int cgrt_scene_last_tile_order_reused(const cgrt_scene *s, int32_t *reused);

/* The terminal-diffuse launch beside cgrt_trace_grid's main launch (see CGRT_GRID_DIFFUSE_TILES): the name of its kernel
 * instantiation for (scene, cam, grid), or an empty string when the grid launches none; and, for the LAST cgrt_trace_grid on
 * the handle, the number of tiles that launch rendered (synchronises the device; 0: none was issued). */
int cgrt_trace_grid_diffuse_variant(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, char *name, size_t cap);
int cgrt_scene_last_diffuse_tiles(const cgrt_scene *s, int64_t *n_tiles);
/* The same count for the one-launch form (see CGRT_GRID_NO_SPHERE_PAIRS): the tiles of the LAST cgrt_trace_grid on the handle
 * whose workgroups ran the terminal-diffuse body inside the main launch (synchronises the device; 0: none did). */
int cgrt_scene_last_inkernel_diffuse_tiles(const cgrt_scene *s, int64_t *n_tiles);
/* The sample relay of the LAST cgrt_trace_grid on the handle (see CGRT_GRID_SAMPLE_RELAY; synchronises the device): *tiles =
 * the tiles it rendered by several workgroups (0: it did not relay), *chunks = the workgroups of each, *parked_values = the
 * Hitpoint values (3 doubles each) that went through the relay area. */
int cgrt_scene_last_sample_relay(const cgrt_scene *s, int64_t *tiles, int32_t *chunks, int64_t *parked_values);
/* The form of that relay: *mirror = 1 when the class-2 tiles were relayed too (CGRT_GRID_RELAY_MIRROR), *order = 0 chunks
 * first, 1 mirror first, 2 interleaved; both -1 when the launch did not relay. */
int cgrt_scene_last_relay_form(const cgrt_scene *s, int32_t *mirror, int32_t *order);
/* The start table of that relay (see CGRT_GRID_RELAY_COST_START; synchronises the device): *t = the workgroups of classes 0-2
 * it ordered by cost, 0 when the launch had no table; *n_wave_tiles = the wave tiles of the launch, *reused = 1 when probe and
 * table were those of an earlier launch.  With start_cap >= *t: start[b] = entry << 2 | chunk of workgroup b, to HOST memory;
 * with cost_cap >= *n_wave_tiles: wcost[wave tile] = the probe's iteration count (0: not probed, a class-3 tile).  A launch with
 * promoted tiles (cgrt_scene_last_relay_boost) returns its full table: a promoted tile's chunks 0 .. k_boost - 1 are all in it
 * and *t is the true count of its workgroups. */
int cgrt_scene_last_relay_start(const cgrt_scene *s, uint32_t *start, int64_t start_cap, uint32_t *wcost, int64_t cost_cap, int64_t *t,
                                int64_t *n_wave_tiles, int32_t *reused);
/* Lens points staged ahead of the sample loop by the LAST cgrt_trace_grid on the handle (see CGRT_GRID_NO_LENS_STAGE;
 * synchronises the device): *lds_tiles = the tiles whose workgroups staged their lens draws in LDS batches, *area_tiles = the
 * tiles that staged them in device memory (no launch does: always 0).  Both 0: every lens point came from the per-sample loop. */
int cgrt_scene_last_lens_stage(const cgrt_scene *s, int64_t *lds_tiles, int64_t *area_tiles);
/* The lens table of the LAST cgrt_trace_grid on the handle (see CGRT_GRID_NO_LENS_TABLE; synchronises the device): *entries = the
 * entries of the tile-order list whose workgroups read their lens draws from the table (its tiles of classes 0-2 below the
 * capacity), *capacity = the entries the table held (CGRT_LENS_TABLE_BYTES / (spp x 2048 bytes), at most the tiles), *reused = 1
 * when the launch found the table written by an earlier one (same order, seed, sample_offset, spp and capacity) and ran no
 * lens_table_kernel.  All 0: the launch read no table, or it returned an error. */
int cgrt_scene_last_lens_table(const cgrt_scene *s, int64_t *entries, int64_t *capacity, int32_t *reused);
/* The committed scene's inside spheres (see CGRT_GRID_NO_INSIDE_TRIPS; a scene trait: no launch, no device): *n = its refracting
 * spheres as the trait holds them -- 0 for a scene with more than one, with more than 32 objects or with an object that is no
 * sphere -- and for k < min(*n, cap): index[k] = the sphere's place in the object list, mask[k] = bit j set for every sphere j a ray
 * that starts inside it can hit first (itself, and every sphere not provably disjoint from it; all bits: the unchanged loop),
 * rin2[k] = the squared radius below which an origin counts as inside (0: none does). */
int cgrt_scene_inside_spheres(const cgrt_scene *s, int32_t *index, uint32_t *mask, double *rin2, int32_t cap, int32_t *n);
/* The eye kernels the LAST eye pass on the handle launched -- cgrt_trace_grid, cgrt_trace_grid_hitpoints, or the eye pass of a PPM
 * or SPPM session over a grid --, in launch order, probes included (host state: no launch, no synchronisation; at most 16 are
 * kept, CGRT_ERR_LIMIT beyond).  *n = the launches, and for i < min(*n, cap) rows[16 i ..] = the kind -- 0 trace_grid_kernel,
 * 1 trace_grid_sched_kernel, 2 primary_walk_kernel --, the instantiation's template flags in the order of the list of compiled
 * instantiations (cgrt_variants.h): TREES BEZ DOF GLASS SPH STATS HPS NT SPILL HFONLY DIFF PAIR START LTAB, then POSE.  A primary
 * walk fills DOF only.  Tells a test which instantiations it ran: cgrt_trace_grid_variant names the main launch alone. */
int cgrt_scene_last_eye_launches(const cgrt_scene *s, int32_t *rows, int64_t cap, int64_t *n);

/* Host evaluation of that table (cgrt_relay.h, the same inline code the kernels run; no GPU): for a list of n_tiles entries,
 * the first n01 of class 0 or 1 and the first n012 of classes 0-2 (cgrt_scene_last_tile_order's plan[2], plan[3], plan[4] and
 * list), an area of cap tiles relayed by k workgroups of chunk_spp samples each out of spp, extent 0 (classes 0 and 1) or 1
 * (class 2 too), and the wave tiles' costs of a grid `width` pixels wide and `rows` high: writes start[b] for b < *t, when
 * start_cap >= *t.  Lets a test recompute the table a launch read back. */
int cgrt_relay_start_host(int32_t k, int32_t chunk_spp, int32_t spp, int64_t cap, int32_t extent, int64_t n01, int64_t n012, int64_t n_tiles,
                          const uint32_t *list, const uint32_t *wcost, int32_t width, int32_t rows, uint32_t *start, int64_t start_cap,
                          int64_t *t);

/* Promotion in that launch (see CGRT_GRID_RELAY_BOOST; synchronises the device): *promoted = the tiles rendered by *k_boost
 * workgroups (0: none, or the launch did not promote), *boost_cap = the tiles the second area held, *cost_sum = S, the sum of
 * tile cost x samples over the tiles of classes 0-2 that the threshold *num / *den refers to, *wg_slots = the workgroup slots
 * it counted.  With slot_cap >= the launch's relayed tiles (cgrt_scene_last_sample_relay's *tiles): bslot[e] = boost slot + 1 of
 * list entry e, 0 where it was not promoted, to HOST memory.  For such a launch cgrt_scene_last_relay_start returns the whole
 * table, a promoted tile's *k_boost chunks included, with *t the true count of its workgroups; cgrt_scene_last_sample_relay
 * keeps *chunks as the base count, and *parked_values counts what went through both areas. */
int cgrt_scene_last_relay_boost(const cgrt_scene *s, int64_t *promoted, int32_t *k_boost, int64_t *boost_cap, uint64_t *cost_sum,
                                int32_t *num, int32_t *den, int32_t *wg_slots, uint32_t *bslot, int64_t slot_cap);
/* Host evaluation of the promoted set and its table (cgrt_relay.h; no GPU): cgrt_relay_start_host's arguments, then a promoted
 * tile's k_boost workgroups of boost_chunk_spp samples, the second area's boost_cap tiles and the threshold num / den over
 * wg_slots workgroup slots.  Writes start[b] for b < *t when start_cap >= *t, and bslot[e] for the relayed entries when
 * slot_cap >= their number; *promoted and *cost_sum as above. */
int cgrt_relay_boost_host(int32_t k, int32_t chunk_spp, int32_t spp, int64_t cap, int32_t extent, int64_t n01, int64_t n012, int64_t n_tiles,
                          const uint32_t *list, const uint32_t *wcost, int32_t width, int32_t rows, int32_t k_boost, int32_t boost_chunk_spp,
                          int64_t boost_cap, int32_t num, int32_t den, int32_t wg_slots, uint32_t *start, int64_t start_cap, uint32_t *bslot,
                          int64_t slot_cap, int64_t *t, int64_t *promoted, uint64_t *cost_sum);

/* Host evaluation of the lens stream (cgrt_rng.hpp, the same inline code the kernel runs): writes
 * uniform_sampling_circle(radius) (sampling.h:35-43) for n (pixel, sample) pairs as 3 doubles each.  Lets CPU-only
 * tests pin the stream against the reference's sampler without a GPU. */
int cgrt_lens_samples(uint64_t seed, const int64_t *pixel, const int32_t *sample, int n, double radius, double *out3);

/* Function-level probe of the device math the fp64 parity rests on (tests/test_gpu_device_math.py): the very inline
 * functions the render kernels call, evaluated on `device` for n elements.  HOST buffers.
 *   CGRT_PROBE_SQRT        in[n]     -> out[n]    = the kernels' fp64 square root (sqrt(), correctly rounded)
 *   CGRT_PROBE_NORMALIZED  in[n][3]  -> out[n][3] = Vec3::normalize (vec3.h:35-43)
 *   CGRT_PROBE_SPHERE_LEN  in[n][10] -> out[n]    = len of Sphere::intersect (objects.h:45-68) for {centre(3), radius2,
 *                                                   rayorig(3), raydir(3)}; a miss gives 1e10 (the kernels' "no hit yet")
 *   CGRT_PROBE_SPHERE_LEN_PAIR in[n][14] -> out[n][2] = the same for two spheres at once, as the pair loop computes them:
 *                                                   {centre A(3), radius2 A, centre B(3), radius2 B, rayorig(3), raydir(3)}
 * Launch geometry is part of the contract, because these functions decide per WAVE which form they take: element i is handled
 * by thread i % 256 of block i / 256, so elements 64k .. 64k+63 are the 64 lanes of one wave, and a lane with i >= n leaves
 * before the call -- the last wave decides with its live lanes only.
 * CGRT_ERR_INVALID: unknown op, null pointer, n < 0 (checked before any device is touched); n == 0 does nothing;
 * more than 2^28 elements: CGRT_ERR_LIMIT. */
enum { CGRT_PROBE_SQRT = 0, CGRT_PROBE_NORMALIZED = 1, CGRT_PROBE_SPHERE_LEN = 2, CGRT_PROBE_SPHERE_LEN_PAIR = 4 /* 3: not an op */ };
int cgrt_math_probe(int device, int op, const double *in, int64_t n, double *out);
/* The same for a routine that needs a scene: CGRT_PROBE_INSIDE_LOOP runs the ",PAIR=1," kernels' sphere loop over the committed
 * scene's spheres for n rays {rayorig(3), raydir(3)}, laid out over the waves as above, once as the pair loop alone and once with
 * the scene's inside spheres (see CGRT_GRID_NO_INSIDE_TRIPS), as a launch with the feature on hands them to its kernel:
 *   out[n][5] = {t, id of the pair loop (1e10, -1: no hit), t, id of the guarded loop, 1 where the element's wave took the
 *                one-by-one loop over the mask, else 0}
 * CGRT_ERR_UNSUPPORTED: the scene is not one the pair loop serves (an object that is no sphere, or more than the resident list
 * holds); CGRT_ERR_INVALID / CGRT_ERR_LIMIT as cgrt_math_probe. */
enum { CGRT_PROBE_INSIDE_LOOP = 5 };
int cgrt_inside_probe(const cgrt_scene *s, int op, const double *rays, int64_t n, double *out);

#ifdef __cplusplus
}
#endif
#endif /* CGRT_H */
