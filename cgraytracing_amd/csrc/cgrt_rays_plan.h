// The launch plan of a ray-list query in plain C++ (no HIP): from the scene's traits, what is asked and three numbers of the
// device, the kernel variant (RayFlags, cgrt_variants.h), the objects resident in LDS, the dynamic LDS bytes, the persistent
// workgroups and the names.  cgrt_trace_rays, the Hitpoint capture over a ray buffer, cgrt_occlusion_rays, cgrt_bounce_rays and
// every level of cgrt_wavefront_rays (cgrt_ray_queries.hpp) launch what rays_plan decides; tests/native/rays_plan.cpp,
// bounce_plan.cpp and wavefront_plan.cpp check it on the CPU.
#ifndef CGRT_RAYS_PLAN_H
#define CGRT_RAYS_PLAN_H
#include <algorithm>
#include <cstdio>

#include "cgrt_variants.h"

// full trace, nearest-hit query, Hitpoint capture, any-hit query, one step of trace(), one level of the wavefront trace
enum class RaysKind { Full, First, Capture, Occlusion, Bounce, Wavefront };
struct RaysAsk {
    int max_depth;
    bool stats;  // CGRT_RAYS_STATS (the capture has no STATS form)
    RaysKind kind;
    long long n;  // rays
};
struct RaysDevice {
    int n_cu;
    size_t lds_limit;       // what a workgroup may use, static + dynamic
    size_t general_static;  // static LDS of the general variant's trace_rays_kernel (rays_general_flags); read only where rays_general
};
// the occlusion query, the bounce query and the wavefront trace's levels share the nearest-hit query's plan -- flags, resident
// objects, LDS
static constexpr bool rays_first(RaysKind k) {
    return k == RaysKind::First || k == RaysKind::Occlusion || k == RaysKind::Bounce || k == RaysKind::Wavefront;
}
// More top-level objects than the LDS list holds, not all of them spheres: the most general body (trees, Bezier, pending rays
// unless only the first hit is asked for), with as many objects resident as fit beside its other LDS; the rest are read from `objs`
static constexpr bool rays_general(const cgrt::DeviceScene &d) { return d.n_objs > d.n_lds && !d.all_spheres; }
static constexpr RayFlags rays_general_flags(bool first) { return {true, true, !first, false, false, true, first, kThreads}; }

// One launch of trace_rays_kernel or of its capture / occlusion / bounce form: the flags chosen from the scene's traits the way
// eye_launch chooses the eye pass's
struct RaysPlan {
    RayFlags k;
    int resident;   // objects in LDS: the launch's copy of the scene is with_resident(traits, resident)
    size_t lds;     // dynamic LDS bytes
    long long wgs;  // persistent workgroups: at most two chips' worth at the kernel's occupancy, fewer when the rays are few
    const char *what() const {  // the launch's name in a refusal
        return k.spill ? (k.sph ? "ray list, SPILL (spheres)" : "ray list, SPILL (general)") : (k.bez ? "ray list (Bezier)" : "ray list");
    }
    // the instantiation's name, as the *_variant entry points report it
    void name(RaysKind kind, char *buf, size_t cap) const {
        if (kind == RaysKind::Capture)
            std::snprintf(buf, cap, "capture_rays_kernel<TREES=%d,BEZ=%d,GLASS=%d,SPH=%d,SPILL=%d,NT=%d>", (int)k.trees, (int)k.bez,
                          (int)k.glass, (int)k.sph, (int)k.spill, k.nt);
        else if (kind == RaysKind::Occlusion)
            std::snprintf(buf, cap, "occlusion_rays_kernel<TREES=%d,BEZ=%d,SPH=%d,STATS=%d,SPILL=%d,NT=%d>", (int)k.trees, (int)k.bez,
                          (int)k.sph, (int)k.stats, (int)k.spill, k.nt);
        else if (kind == RaysKind::Bounce)
            std::snprintf(buf, cap, "bounce_rays_kernel<TREES=%d,BEZ=%d,SPH=%d,STATS=%d,SPILL=%d,NT=%d>", (int)k.trees, (int)k.bez,
                          (int)k.sph, (int)k.stats, (int)k.spill, k.nt);
        else if (kind == RaysKind::Wavefront)
            std::snprintf(buf, cap, "wavefront_step_kernel<TREES=%d,BEZ=%d,SPH=%d,STATS=%d,SPILL=%d,NT=%d>", (int)k.trees, (int)k.bez,
                          (int)k.sph, (int)k.stats, (int)k.spill, k.nt);
        else
            std::snprintf(buf, cap, "trace_rays_kernel<TREES=%d,BEZ=%d,GLASS=%d,SPH=%d,STATS=%d,SPILL=%d,FIRST=%d,NT=%d>", (int)k.trees,
                          (int)k.bez, (int)k.glass, (int)k.sph, (int)k.stats, (int)k.spill, (int)k.first, k.nt);
    }
};

static inline RaysPlan rays_plan(const cgrt::DeviceScene &d, const RaysAsk &ask, const RaysDevice &dev) {
    const bool first = rays_first(ask.kind), stats = ask.stats && ask.kind != RaysKind::Capture;
    const bool glass = !first && d.has_glass != 0 && ask.max_depth > 1;
    RaysPlan p{};
    p.resident = d.n_lds;
    if (rays_general(d)) {
        p.k = rays_general_flags(first);
        if (rays_lds(p.k, d) + dev.general_static > dev.lds_limit) {
            const long long room = (long long)dev.lds_limit - (long long)(dev.general_static + rays_lds(p.k, with_resident(d, 0)));
            p.resident = (int)std::max(0ll, std::min(room / (long long)sizeof(cgrt::ObjRec), (long long)d.n_lds));
        }
    } else if (d.n_objs > d.n_lds) {
        p.k = RayFlags{false, false, glass, true, false, true, first, kThreads};
    } else {
        const bool bez = d.has_bezier != 0, trees = d.has_mesh != 0 || bez;
        p.k = RayFlags{trees, bez, glass, !trees && d.all_spheres != 0, stats && d.has_mesh != 0 && !bez, false, first, bez ? 64 : kThreads};
    }
    p.lds = rays_lds(p.k, with_resident(d, p.resident));
    const long long waves_per_wg = p.k.nt / 64, n_blocks = (ask.n + 63) / 64;
    const long long chip = (long long)dev.n_cu * 4 * (p.k.bez ? kBezWaves : (p.k.trees ? kTreeWaves : 4)) / waves_per_wg;
    p.wgs = std::max(1ll, std::min((n_blocks + waves_per_wg - 1) / waves_per_wg, 2 * chip));
    return p;
}

#endif
