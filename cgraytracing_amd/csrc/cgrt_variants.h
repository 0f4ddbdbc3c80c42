// The kernel variants that are compiled, once, in plain C++ (no HIP): the template flags of the eye kernels and of the ray-list
// kernels, the two lists of instantiations as X-macros, and the dynamic LDS of a variant's launch.  cgrt_hip.hip and
// cgrt_ray_queries.hpp expand the lists into their dispatch tables -- only these instantiations are compiled (every combination
// of the flags would multiply the library's build time and size) --, tests/native/wg_lds.cpp and tests/native/rays_plan.cpp walk
// them on the CPU, and the GPU tests read them from this file (tests/variants.py).
#ifndef CGRT_VARIANTS_H
#define CGRT_VARIANTS_H
#include "cgrt_frame.h"  // kThreads
#include "cgrt_wg_lds.h"

#ifndef CGRT_BEZ_WAVES
#define CGRT_BEZ_WAVES 2
#endif
static constexpr int kBezWaves = CGRT_BEZ_WAVES;  // waves per SIMD the Bezier variants are compiled for
#ifndef CGRT_TREE_WAVES
#define CGRT_TREE_WAVES 3
#endif
#ifndef CGRT_SCHED_TREE_WAVES
#define CGRT_SCHED_TREE_WAVES CGRT_TREE_WAVES
#endif
static constexpr int kTreeWaves = CGRT_TREE_WAVES;             // ... the tree-capable tile kernels
static constexpr int kSchedTreeWaves = CGRT_SCHED_TREE_WAVES;  // ... the tree-capable scheduled kernels (unit queue + tile queue)

// ---- the eye kernels ----
// The template flags of a trace_grid_kernel / trace_grid_sched_kernel instantiation
struct EyeFlags {
    bool trees, bez, dof, glass, sph, stats, hps, spill, hfonly;
    int nt;  // threads per workgroup: 256 (32x8-pixel tiles) or 64 (Bezier scenes: one-wave workgroups on 16x4 tiles)
    bool diff = false;  // the terminal-diffuse body (sphere scenes' class-3 tiles)
    bool pair = false;  // the sphere loop two spheres a trip, class-3 tiles by the diffuse body in the same launch (glass sphere scenes)
    bool start = false;  // a PAIR variant's twin that reads the relay's start table and serves as its cost probe (cgrt_relay.h)
    bool ltab = false;  // a thin-lens PAIR variant's twin whose full and parking bodies read the lens table (cgrt_lens_stage.h)
    constexpr int id() const {
        return (int)trees | (int)bez << 1 | (int)dof << 2 | (int)glass << 3 | (int)sph << 4 | (int)stats << 5 | (int)hps << 6 |
               (int)spill << 7 | (int)hfonly << 8 | (nt == 64 ? 1 << 9 : 0) | (int)diff << 10 | (int)pair << 11 | (int)start << 12 | (int)ltab << 13;
    }
};
// image order, the probe and the scheduled form: Bezier scenes share the tree-capable variants (one-wave workgroups)
static constexpr EyeFlags image_flags(bool trees, bool bez, bool dof, bool glass, bool sph, bool stats) {
    return {trees, bez, dof, glass, sph, stats, false, false, false, bez ? 64 : kThreads};
}
// the sphere loop reading the objects beyond the LDS list from `objs`
static constexpr EyeFlags spill_sph_flags(bool dof, bool glass) { return {false, false, dof, glass, true, false, false, true, false, kThreads}; }
// the most general body (trees, Bezier, pending rays): the Hitpoint capture (hps) and the eye pass's SPILL form
static constexpr EyeFlags general_flags(bool dof, bool hps, bool spill) { return {true, true, dof, true, false, false, hps, spill, false, kThreads}; }
// the light tiles: no Bezier or pending-ray code; with trees beside bump-mapped planes, or only their height-field walk (hfonly)
static constexpr EyeFlags light_flags(bool trees, bool dof, bool hfonly) { return {trees, false, dof, false, false, false, false, false, hfonly, kThreads}; }
// the diffuse tiles of a sphere-only scene: the sphere loop, every ray ends at its first hit
static constexpr EyeFlags diffuse_flags(bool dof) { return {false, false, dof, false, true, false, false, false, false, kThreads, true}; }

// The instantiations of the eye kernels that are launched, one X(...) each; SCHED: trace_grid_sched_kernel runs these flags too
// (its own flags are the first six and NT)
//    TREES BEZ DOF GLASS SPH STATS HPS NT SPILL HFONLY DIFF PAIR START LTAB | SCHED
#define CGRT_EYE_VARIANTS(X)                                                                                                        \
    /* image order, the probe and the scheduled form (the light variants are the tree and plain ones without GLASS or STATS) */     \
    X(1, 1, 0, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1) X(1, 1, 0, 1, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1)                                 \
    X(1, 1, 1, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1) X(1, 1, 1, 1, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1)                                 \
    X(1, 0, 0, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(1, 0, 0, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(1, 0, 1, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(1, 0, 1, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(1, 0, 0, 0, 0, 1, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(1, 0, 0, 1, 0, 1, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(1, 0, 1, 0, 0, 1, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(1, 0, 1, 1, 0, 1, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(0, 0, 0, 0, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(0, 0, 0, 1, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(0, 0, 1, 0, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(0, 0, 1, 1, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(0, 0, 0, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(0, 0, 0, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(0, 0, 1, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(0, 0, 1, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    /* SPILL: spheres, and the general body; the Hitpoint capture (general, HPS) with and without SPILL */                          \
    X(0, 0, 0, 0, 1, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0) X(0, 0, 0, 1, 1, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0)                               \
    X(0, 0, 1, 0, 1, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0) X(0, 0, 1, 1, 1, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0)                               \
    X(1, 1, 0, 1, 0, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0) X(1, 1, 1, 1, 0, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0)                               \
    X(1, 1, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 0, 0, 0) X(1, 1, 1, 1, 0, 0, 1, 256, 0, 0, 0, 0, 0, 0, 0)                               \
    X(1, 1, 0, 1, 0, 0, 1, 256, 1, 0, 0, 0, 0, 0, 0) X(1, 1, 1, 1, 0, 0, 1, 256, 1, 0, 0, 0, 0, 0, 0)                               \
    /* light tiles beside bump-mapped planes that need only the height-field walk */                                                \
    X(1, 0, 0, 0, 0, 0, 0, 256, 0, 1, 0, 0, 0, 0, 0) X(1, 0, 1, 0, 0, 0, 0, 256, 0, 1, 0, 0, 0, 0, 0)                               \
    /* diffuse tiles of sphere-only scenes (class 3 of the tile order) */                                                           \
    X(0, 0, 0, 0, 1, 0, 0, 256, 0, 0, 1, 0, 0, 0, 0) X(0, 0, 1, 0, 1, 0, 0, 256, 0, 0, 1, 0, 0, 0, 0)                               \
    /* glass sphere scenes in image order: the pair loop, the class-3 tiles' diffuse body inside */                                 \
    X(0, 0, 0, 1, 1, 0, 0, 256, 0, 0, 0, 1, 0, 0, 0) X(0, 0, 1, 1, 1, 0, 0, 256, 0, 0, 0, 1, 0, 0, 0)                               \
    /* ... and their twins for a launch whose relay starts by cost: the start table's map, the cost probe */                        \
    X(0, 0, 0, 1, 1, 0, 0, 256, 0, 0, 0, 1, 1, 0, 0) X(0, 0, 1, 1, 1, 0, 0, 256, 0, 0, 0, 1, 1, 0, 0)                               \
    /* ... and the thin-lens ones' twins, plain and START, for a launch with a lens table: the bodies that read it */                \
    X(0, 0, 1, 1, 1, 0, 0, 256, 0, 0, 0, 1, 0, 1, 0) X(0, 0, 1, 1, 1, 0, 0, 256, 0, 0, 0, 1, 1, 1, 0)

// ---- the ray-list kernels (cgrt_rays.hpp, cgrt_occlusion.hpp, cgrt_bounce.hpp) ----
// The template flags of a trace_rays_kernel instantiation
struct RayFlags {
    bool trees, bez, glass, sph, stats, spill, first;
    int nt;  // threads per workgroup: 256, or 64 (Bezier scenes: one BezLds per workgroup, as the eye pass's one-wave form)
    constexpr int id() const {
        return (int)trees | (int)bez << 1 | (int)glass << 2 | (int)sph << 3 | (int)stats << 4 | (int)spill << 5 | (int)first << 6 |
               (nt == 64 ? 1 << 7 : 0);
    }
};
// The instantiations of trace_rays_kernel that are launched (rays_plan, cgrt_rays_plan.h), one X(...) each
//    TREES BEZ GLASS SPH STATS SPILL FIRST NT
#define CGRT_RAY_VARIANTS(X)                                                                                                          \
    /* the full trace: Bezier scenes (one-wave workgroups), meshes / bump floors (with and without STATS), spheres, plain scenes */   \
    X(1, 1, 0, 0, 0, 0, 0, 64) X(1, 1, 1, 0, 0, 0, 0, 64)                                                                             \
    X(1, 0, 0, 0, 0, 0, 0, 256) X(1, 0, 1, 0, 0, 0, 0, 256) X(1, 0, 0, 0, 1, 0, 0, 256) X(1, 0, 1, 0, 1, 0, 0, 256)                   \
    X(0, 0, 0, 1, 0, 0, 0, 256) X(0, 0, 1, 1, 0, 0, 0, 256) X(0, 0, 0, 0, 0, 0, 0, 256) X(0, 0, 1, 0, 0, 0, 0, 256)                   \
    /* SPILL: spheres, and the general body */                                                                                        \
    X(0, 0, 0, 1, 0, 1, 0, 256) X(0, 0, 1, 1, 0, 1, 0, 256) X(1, 1, 1, 0, 0, 1, 0, 256)                                               \
    /* the nearest-hit query: no GLASS variants */                                                                                    \
    X(1, 1, 0, 0, 0, 0, 1, 64) X(1, 0, 0, 0, 0, 0, 1, 256) X(1, 0, 0, 0, 1, 0, 1, 256) X(0, 0, 0, 1, 0, 0, 1, 256)                    \
    X(0, 0, 0, 0, 0, 0, 1, 256) X(0, 0, 0, 1, 0, 1, 1, 256) X(1, 1, 0, 0, 0, 1, 1, 256)
// The three derived families share a variant's flags, launch plan and table row:
// capture_rays_kernel<TREES, BEZ, GLASS, SPH, SPILL, NT> exists for every full-trace variant without STATS, ...
static constexpr bool has_capture(const RayFlags &f) { return !f.stats && !f.first; }
// ... occlusion_rays_kernel<TREES, BEZ, SPH, STATS, SPILL, NT> for every nearest-hit variant (none of which has GLASS), ...
static constexpr bool has_occlusion(const RayFlags &f) { return f.first; }
// ... and so does bounce_rays_kernel<TREES, BEZ, SPH, STATS, SPILL, NT>: one walk per ray, then one step of trace()
static constexpr bool has_bounce(const RayFlags &f) { return f.first; }

// ---- LDS of a launch ----
// A workgroup may use at most a CU's LDS (MI355X: 160 KiB): the kernel's static __shared__ bytes plus the dynamic bytes of
// the launch.  Each launch family's dynamic bytes come from one function below: the total of the layout its kernel carves up
// (wg_lds, cgrt_wg_lds.h) for the variant's flags.  The static bytes are the compiler's; the static_asserts use kStaticLdsAllowance.
static constexpr size_t kStaticLdsAllowance = 512;  // the eye kernels have 336 B (ROCm 7.2): wg_cnt, tile_entry, tl_rays, ...
static constexpr WgLdsAsk eye_ask(const EyeFlags &f) { return wg_ask_trace(f.nt, f.trees, f.bez, f.glass, f.spill, f.hfonly); }
static constexpr size_t eye_lds(const EyeFlags &f, size_t resident, size_t cached_nodes, bool wide) {
    return wg_lds(eye_ask(f), resident, cached_nodes, wide).total;
}
static constexpr size_t eye_lds(const EyeFlags &f, const cgrt::DeviceScene &d) { return wg_lds(eye_ask(f), d).total; }
// primary_walk_kernel stages `staged` objects; photon_trace_kernel takes the stack where photon_lds_stack asks for it
static constexpr size_t primary_walk_lds(size_t staged) { return wg_lds(wg_ask_primary_walk(), staged, 0, true).total; }
static constexpr size_t photon_lds(size_t resident, bool spill, bool bez, bool wide_stack) {
    return wg_lds(wg_ask_photon(bez, spill), resident, 0, wide_stack).total;
}
static constexpr WgLdsAsk rays_ask(const RayFlags &f) { return wg_ask_trace(f.nt, f.trees, f.bez, f.glass, f.spill, false); }
static constexpr size_t rays_lds(const RayFlags &f, size_t resident, size_t cached_nodes, bool wide) {
    return wg_lds(rays_ask(f), resident, cached_nodes, wide).total;
}
static constexpr size_t rays_lds(const RayFlags &f, const cgrt::DeviceScene &d) { return wg_lds(rays_ask(f), d).total; }

// The launch's copy of the scene with `resident` objects in LDS.  A run of planes tested as a group (plane_run) is read from
// the LDS list, so it ends inside it: a shorter run is the same test over fewer planes.
static constexpr cgrt::DeviceScene with_resident(const cgrt::DeviceScene &d, int resident) {
    cgrt::DeviceScene c = d;
    c.n_lds = resident;
    if (c.prun_end > resident) c.prun_end = resident;
    if (c.prun_end - c.prun_begin < 3) c.prun_begin = c.prun_end = 0;
    return c;
}

static constexpr bool fits_lds(size_t dyn) { return dyn + kStaticLdsAllowance <= cgrt::kLdsBytes; }
// Every launch that stages kLdsObjsMax objects fits beside its other LDS (the general variant lowers its count instead):
// the eye pass without SPILL, with and without glass (the light variants are the latter), ...
static_assert(fits_lds(eye_lds(image_flags(true, false, false, true, false, false), cgrt::kLdsObjsMax, cgrt::kNodeCache, true)) &&
                  fits_lds(eye_lds(image_flags(true, false, false, false, false, false), cgrt::kLdsObjsMax, cgrt::kNodeCache, true)),
              "eye pass, 256-thread and light variants");
// ... the one-wave Bezier variants, the sphere-only SPILL variant, ...
static_assert(fits_lds(eye_lds(image_flags(true, true, false, true, false, false), cgrt::kLdsObjsMax, cgrt::kNodeCache, true)),
              "eye pass, one-wave Bezier variants");
static_assert(fits_lds(eye_lds(spill_sph_flags(false, true), cgrt::kLdsObjsMax, 0, false)), "eye pass, SPILL_SPH");
// ... primary_walk_kernel (all objects staged when it finishes units; it runs only when none is spilled), the photon launches
static_assert(fits_lds(primary_walk_lds(cgrt::kLdsObjsMax)), "primary_walk_kernel");
static_assert(fits_lds(photon_lds(cgrt::kLdsObjsMax, true, true, false)), "photon_trace_kernel");
// ... and the ray-list launches: trees with and without pending rays, the one-wave Bezier form, the sphere loop with SPILL
static_assert(fits_lds(rays_lds(RayFlags{true, false, true, false, false, false, false, kThreads}, cgrt::kLdsObjsMax, cgrt::kNodeCache, true)) &&
                  fits_lds(rays_lds(RayFlags{true, false, false, false, false, false, false, kThreads}, cgrt::kLdsObjsMax, cgrt::kNodeCache, true)) &&
                  fits_lds(rays_lds(RayFlags{true, true, true, false, false, false, false, 64}, cgrt::kLdsObjsMax, cgrt::kNodeCache, true)) &&
                  fits_lds(rays_lds(RayFlags{false, false, true, true, false, true, false, kThreads}, cgrt::kLdsObjsMax, 0, false)),
              "trace_rays_kernel");
static_assert(fits_lds(rays_lds(RayFlags{true, true, true, false, false, true, false, kThreads}, 600, cgrt::kNodeCache, false)),
              "trace_rays_kernel, general variant: resident objects");
// The general variant keeps at least 600 objects resident whatever the scene.
static_assert(fits_lds(eye_lds(general_flags(false, false, true), 600, cgrt::kNodeCache, false)), "general variant: resident objects");

#endif
