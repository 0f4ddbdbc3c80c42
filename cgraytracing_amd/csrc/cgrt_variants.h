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
    bool pose = false;  // the kernels of a posed launch (CGRT_GRID_POSED): primary rays from the camera's frame in the world
    constexpr int id() const {
        return (int)trees | (int)bez << 1 | (int)dof << 2 | (int)glass << 3 | (int)sph << 4 | (int)stats << 5 | (int)hps << 6 |
               (int)spill << 7 | (int)hfonly << 8 | (nt == 64 ? 1 << 9 : 0) | (int)diff << 10 | (int)pair << 11 | (int)start << 12 | (int)ltab << 13 | (int)pose << 14;
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

// The instantiations with POSE that are launched (a list of its own: the one above is walked column by column by tools and
// tests), the same columns: the forms a posed launch can take -- image order for every scene class, the scheduled form for scenes
// with a tree or a Bezier object (sphere and plain scenes are never scheduled under a pose), SPILL and the Hitpoint capture.  No
// STATS, DIFF, PAIR, START, LTAB or HFONLY form: a posed launch has no tile order and no light split (cgrt_frame.h).  The
// spheres' SPILL form comes with GLASS only (eye_launch asks for it whatever the scene).
//    TREES BEZ DOF GLASS SPH STATS HPS NT SPILL HFONLY DIFF PAIR START LTAB | SCHED
#define CGRT_EYE_POSED_VARIANTS(X)                                                                                                  \
    /* image order and the scheduled form: Bezier (one wave), trees, spheres, plain scenes */                                       \
    X(1, 1, 0, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1) X(1, 1, 0, 1, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1)                                 \
    X(1, 1, 1, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1) X(1, 1, 1, 1, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 1)                                 \
    X(1, 0, 0, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(1, 0, 0, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(1, 0, 1, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1) X(1, 0, 1, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 1)                               \
    X(0, 0, 0, 0, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0) X(0, 0, 0, 1, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0)                               \
    X(0, 0, 1, 0, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0) X(0, 0, 1, 1, 1, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0)                               \
    X(0, 0, 0, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0) X(0, 0, 0, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0)                               \
    X(0, 0, 1, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0) X(0, 0, 1, 1, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0)                               \
    /* SPILL: spheres (GLASS), and the general body; the Hitpoint capture (general, HPS) with and without SPILL */                  \
    X(0, 0, 0, 1, 1, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0) X(0, 0, 1, 1, 1, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0)                               \
    X(1, 1, 0, 1, 0, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0) X(1, 1, 1, 1, 0, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0)                               \
    X(1, 1, 0, 1, 0, 0, 1, 256, 0, 0, 0, 0, 0, 0, 0) X(1, 1, 1, 1, 0, 0, 1, 256, 0, 0, 0, 0, 0, 0, 0)                               \
    X(1, 1, 0, 1, 0, 0, 1, 256, 1, 0, 0, 0, 0, 0, 0) X(1, 1, 1, 1, 0, 0, 1, 256, 1, 0, 0, 0, 0, 0, 0)
// a variant's posed form
static constexpr EyeFlags posed_flags(EyeFlags f) {
    f.pose = true;
    return f;
}

// The eye kernels one eye pass launched, in launch order, probes included: a fixed array (a pass issues at most six: probe, light
// tiles, primary walk, the frame, its diffuse launch, the relay's cost probe), nothing allocated on the launch path
enum EyeKernelKind { kEyeGrid = 0, kEyeSched = 1, kEyePrimaryWalk = 2 };  // trace_grid_kernel, trace_grid_sched_kernel, primary_walk_kernel
static constexpr int kEyeLogCols = 16;  // a row as cgrt_scene_last_eye_launches hands it out: the kind, the lists' 14 columns, POSE
struct EyeLaunchLog {
    static constexpr int kCap = 16;
    struct Entry {
        int kind;
        EyeFlags k;
    } e[kCap];
    int n = 0;
    bool overflow = false;
    void clear() { n = 0, overflow = false; }
    void add(int kind, const EyeFlags &k) {
        if (n < kCap) e[n++] = Entry{kind, k};
        else overflow = true;
    }
    // entry i as kind, TREES BEZ DOF GLASS SPH STATS HPS NT SPILL HFONLY DIFF PAIR START LTAB, POSE
    void row(int i, int32_t out[kEyeLogCols]) const {
        const EyeFlags &k = e[i].k;
        const int32_t v[kEyeLogCols] = {e[i].kind, k.trees, k.bez,  k.dof,  k.glass, k.sph,   k.stats, k.hps,
                                        k.nt,      k.spill, k.hfonly, k.diff, k.pair,  k.start, k.ltab,  k.pose};
        for (int c = 0; c < kEyeLogCols; c++) out[c] = v[c];
    }
};

// ---- the eye pass's choice of kernel ----
enum class EyeForm { Image, Sched, SpillSph, SpillGen, Capture, Light, LightHF, Diffuse };
// What the choice reads of a committed scene (DeviceScene's traits and the handle's order_ok), and the choice
struct EyeSceneTraits {
    bool all_spheres, has_mesh, has_bezier, has_glass, single_ray, order_ok;
    int n_objs, n_lds;
};
struct EyeChoice {
    EyeForm form;
    EyeFlags k;
};
// The form and the template flags of the eye pass's main launch for (scene, camera, grid): the Hitpoint capture (capture), else
// cgrt_trace_grid's.  The general forms (Capture, SpillGen) come back with k.spill set; eye_launch (cgrt_hip.hip) clears it where
// the scene's objects all stay resident.  force_reorder: the knob CGRT_FORCE_REORDER.
// A posed launch (CGRT_GRID_POSED) takes the same form with the POSE kernels of CGRT_EYE_POSED_VARIANTS, except: sphere and plain
// scenes stay in image order whatever the flags ask, without the pair loop (there is no tile order for it to serve), and the
// spheres' SPILL form is compiled with GLASS only.  No STATS kernel has POSE: such a launch is refused as unsupported.
static inline EyeChoice eye_choice(const EyeSceneTraits &d, const cgrt_camera &cam, const cgrt_grid &grid, bool force_reorder, bool capture) {
    const bool dof = cam.lens_radius > 0, glass = d.has_glass && grid.max_depth > 1;
    const bool spill = d.n_objs > d.n_lds;  // more top-level objects than the LDS list holds (kLdsObjsMax)
    const bool posed = (grid.flags & CGRT_GRID_POSED) != 0;
    EyeChoice c{};
    if (capture || (spill && !d.all_spheres)) {
        // the most general variant serves every scene, with as many objects resident as fit beside its other LDS; the
        // capture is a verification / hand-off path, not the hot path
        c.form = capture ? EyeForm::Capture : EyeForm::SpillGen;
        c.k = general_flags(dof, capture, true);
    } else if (spill) {
        c.form = EyeForm::SpillSph;
        c.k = spill_sph_flags(dof, glass || posed);
    } else {
        const bool bez = d.has_bezier, trees = d.has_mesh || bez;
        c.k = image_flags(trees, bez, dof, glass, !trees && d.all_spheres, (grid.flags & CGRT_GRID_STATS) != 0 && d.has_mesh && !bez);
        // Scenes of spheres and plain planes are left in image order: without a tree or a Newton solve behind a ray, a tile's
        // cost varies only with the size of its ray trees (<= 31 rays per sample), the per-lane sample loop already keeps 97 %
        // of the lanes busy, and measured on C2 the unit queue costs 13 % more VALU instructions (at 93 % VALU busy) and 0.9 GB
        // of deferred values per frame for a gain within the noise (4.0-4.2 ms either way); a room of five planes, 4096x4096
        // spp 4: 2.2 ms scheduled (probe and plan for nothing), 1.0 ms in image order.
        // The same holds when every ray tree is a single ray (diffuse planes, bump-mapped or not, and diffuse spheres): a room
        // with the stone floor, 8192 x 512 rows at spp 16: floor band 7.7 ms scheduled (every tile of a uniform frame counts as
        // heavy), 5.4 ms in image order; wall band 4.0 and 1.7 ms.
        const bool plain_scene = (!d.has_mesh && !d.has_bezier) || d.single_ray;  // has_mesh: any tree, a bump floor's included
        const size_t n_wt = (size_t)((grid.width + kWaveTileW - 1) / kWaveTileW) * ((grid.rows + kWaveTileH - 1) / kWaveTileH);
        const bool reorder = grid.spp >= 4 && !(grid.flags & CGRT_GRID_NO_REORDER) && n_wt > 1 && n_wt < (1u << 30) &&
                             (!plain_scene || (!posed && ((grid.flags & CGRT_GRID_FORCE_REORDER) || force_reorder)));
        c.form = reorder ? EyeForm::Sched : EyeForm::Image;
        // The image-order launch of a glass sphere scene the tile order serves (order_ok): its last waves, over the glass sphere,
        // each alone on a SIMD, are bound by the sphere loop's dependent chain -- two spheres a trip
        c.k.pair = c.form == EyeForm::Image && c.k.sph && c.k.glass && !c.k.stats && d.order_ok && !(grid.flags & CGRT_GRID_NO_SPHERE_PAIRS) && !posed;
    }
    c.k.pose = posed;
    return c;
}

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
