// The launch plan of the grid AOV pass (cgrt_trace_grid_aov) in plain C++ (no HIP): the instantiations of aov_grid_kernel
// (cgrt_aov.hpp) as an X-macro list of its own, the choice among them from the scene's traits, the objects resident in LDS, the
// dynamic LDS bytes, the workgroups and the names.  The pass is the nearest-hit query of the camera's own rays, one pixel a
// lane, so its choice IS rays_plan's for such a query (cgrt_rays_plan.h) -- the same flags, resident count and LDS layout --
// and only the workgroups differ: one per tile of the eye pass's tile grid instead of persistent ones over a ray queue.
// tests/native/aov_plan.cpp checks it on the CPU.
#ifndef CGRT_AOV_PLAN_H
#define CGRT_AOV_PLAN_H
#include "cgrt_rays_plan.h"

// The template flags of an aov_grid_kernel instantiation
struct AovFlags {
    bool trees, bez, sph, spill;
    int nt;  // threads per workgroup: 256 (32x8-pixel tiles), or 64 (Bezier scenes: one wave on a 16x4 tile, as the eye pass)
    constexpr int id() const { return (int)trees | (int)bez << 1 | (int)sph << 2 | (int)spill << 3 | (nt == 64 ? 1 << 4 : 0); }
};
// The instantiations that are launched, one X(...) each: the six nearest-hit rows of CGRT_RAY_VARIANTS without STATS --
// Bezier scenes (one-wave workgroups), meshes / bump floors, spheres, plain scenes, and SPILL: spheres, the general body
//    TREES BEZ SPH SPILL NT
#define CGRT_AOV_VARIANTS(X) \
    X(1, 1, 0, 0, 64) X(1, 0, 0, 0, 256) X(0, 0, 1, 0, 256) X(0, 0, 0, 0, 256) X(0, 0, 1, 1, 256) X(1, 1, 0, 1, 256)

// a nearest-hit row of the ray-list kernels as the AOV kernel's flags, and back
static constexpr AovFlags aov_flags(const RayFlags &r) { return {r.trees, r.bez, r.sph, r.spill, r.nt}; }
static constexpr RayFlags aov_ray_flags(const AovFlags &a) { return {a.trees, a.bez, false, a.sph, false, a.spill, true, a.nt}; }
static constexpr WgLdsAsk aov_ask(const AovFlags &a) { return wg_ask_trace(a.nt, a.trees, a.bez, false, a.spill, false); }

// What the device tells the plan: a workgroup's LDS limit and the general variant's own static bytes (read only where rays_general)
struct AovDevice {
    size_t lds_limit, general_static;
};
// One launch of aov_grid_kernel
struct AovPlan {
    AovFlags k;
    int resident;    // objects in LDS: the launch's copy of the scene is with_resident(traits, resident)
    size_t lds;      // dynamic LDS bytes
    bool xcd_tiles;  // block -> tile map (tile_of_block): XCD-aware super-tiles for scenes with a mesh, as the eye pass
    int blocks;      // workgroups: one per tile of the grid's rows (tile_grid_blocks)
    const char *what() const {  // the launch's name in a refusal
        return k.spill ? (k.sph ? "grid AOVs, SPILL (spheres)" : "grid AOVs, SPILL (general)") : (k.bez ? "grid AOVs (Bezier)" : "grid AOVs");
    }
    void name(char *buf, size_t cap) const {  // the instantiation's name, as cgrt_trace_grid_aov_variant reports it
        std::snprintf(buf, cap, "aov_grid_kernel<TREES=%d,BEZ=%d,SPH=%d,SPILL=%d,NT=%d>", (int)k.trees, (int)k.bez, (int)k.sph, (int)k.spill, k.nt);
    }
};

// the row: rays_plan's for a nearest-hit query of the same scene (no STATS; the count of rays does not enter the flags)
static inline AovFlags aov_choice(const cgrt::DeviceScene &d) {
    return aov_flags(rays_plan(d, RaysAsk{1, false, RaysKind::First, 1}, RaysDevice{1, cgrt::kLdsBytes, kStaticLdsAllowance}).k);
}
static inline AovPlan aov_plan(const cgrt::DeviceScene &d, int width, int rows, const AovDevice &dev) {
    const RaysPlan r = rays_plan(d, RaysAsk{1, false, RaysKind::First, 1}, RaysDevice{1, dev.lds_limit, dev.general_static});
    AovPlan p{};
    p.k = aov_flags(r.k);
    p.resident = r.resident;
    p.lds = r.lds;
    p.xcd_tiles = !p.k.spill && d.has_mesh != 0 && d.has_bezier == 0;
    p.blocks = tile_grid_blocks(width, rows, p.xcd_tiles, p.k.nt == 64 ? kWaveTileW : kTileW, p.k.nt == 64 ? kWaveTileH : kTileH);
    return p;
}

#endif
