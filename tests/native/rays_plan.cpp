// The launch plan of the ray-list queries (cgrt_rays_plan.h: rays_plan) over every scene-trait combination scene_traits can
// produce, object counts on either side of the LDS list, both depths, STATS and the four kinds of query: the variant is a
// compiled one and has the kernel the kind needs, its LDS fits, the general variant's resident counts, the workgroup count
// against the written-out formula, the names against literal strings.  CPU build under ASan + UBSan, driven by
// tests/test_rays_plan_host.py.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "cgrt_rays_plan.h"

static int g_failed = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        if (a_ != b_) {                                                                                         \
            std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)

#define X(T, B, G, P, S, SP, F, NT) RayFlags{T != 0, B != 0, G != 0, P != 0, S != 0, SP != 0, F != 0, NT},
static const RayFlags kRays[] = {CGRT_RAY_VARIANTS(X)};
#undef X
static const RayFlags *compiled(const RayFlags &f) {
    for (const RayFlags &r : kRays)
        if (r.id() == f.id()) return &r;
    return nullptr;
}

// an MI355X: 256 CUs, 160 KiB a workgroup; the general variant's trace_rays_kernel has 336 B of static LDS
static const RaysDevice kDev{256, 163840, 336};
static const RaysKind kKinds[] = {RaysKind::Full, RaysKind::First, RaysKind::Capture, RaysKind::Occlusion};

// Every trait combination scene_traits (cgrt_build.cpp) can produce, as far as a ray launch reads it: a scene of spheres only
// has no tree and no Bezier object; a cached tree, a wide tree and has_mesh need a tree; n_lds is the object count up to 768, or
// fewer on request (CGRT_LDS_OBJS: 7 here); a run of planes lies inside the LDS list.  f(traits) for each.
template <class F>
static void for_each_traits(F f) {
    for (int n_objs : {1, 768, 769, 1000, 1 << 20})
        for (int lds_objs : {768, 7})
            for (int all_spheres = 0; all_spheres < 2; all_spheres++)
                for (int has_mesh = 0; has_mesh < (all_spheres ? 1 : 2); has_mesh++)
                    for (int has_bezier = 0; has_bezier < (all_spheres ? 1 : 2); has_bezier++)
                        for (int has_glass = 0; has_glass < 2; has_glass++)
                            for (int cached = 0; cached < (has_mesh ? 2 : 1); cached++)
                                for (int wide = 0; wide < (has_mesh ? 2 : 1); wide++)
                                    for (int prun = 0; prun < (all_spheres ? 1 : 2); prun++) {
                                        cgrt::DeviceScene d{};
                                        d.n_objs = n_objs;
                                        d.n_lds = n_objs < lds_objs ? n_objs : lds_objs;
                                        d.all_spheres = all_spheres;
                                        d.has_mesh = has_mesh;
                                        d.has_bezier = has_bezier;
                                        d.has_glass = has_glass;
                                        d.cached_tree = cached ? 0 : -1;
                                        d.cached_nodes = cached ? 255 : 0;
                                        d.has_wide = wide;
                                        if (prun && d.n_lds >= 5) d.prun_end = 5;
                                        f(d);
                                    }
}

static long long wgs_written_out(const RayFlags &k, long long n) {
    const long long blocks = (n + 63) / 64;                          // 64 rays a wave at a time
    const long long wgs = k.nt == 64 ? blocks : (blocks + 3) / 4;    // one or four waves a workgroup
    const long long per_simd = k.bez ? 2 : (k.trees ? 3 : 4);        // the kernels' occupancy (waves per SIMD)
    const long long chip = 256 * 4 * per_simd / (k.nt == 64 ? 1 : 4);  // workgroups that fill the chip
    return wgs < 1 ? 1 : (wgs > 2 * chip ? 2 * chip : wgs);
}

static void check_name(const cgrt::DeviceScene &d, RaysKind kind, int depth, bool stats, const char *want) {
    char buf[160];
    rays_plan(d, RaysAsk{depth, stats, kind, 1000}, kDev).name(kind, buf, sizeof(buf));
    if (std::strcmp(buf, want) != 0) {
        std::printf("FAIL name: %s, expected %s\n", buf, want);
        g_failed++;
    }
}

#ifndef RAYS_PLAN_NO_MAIN
int main() {
    long long inputs = 0;
    for_each_traits([&](const cgrt::DeviceScene &d) {
        for (int depth : {1, 5})
            for (int stats = 0; stats < 2; stats++)
                for (RaysKind kind : kKinds) {
                    const RaysPlan p = rays_plan(d, RaysAsk{depth, stats != 0, kind, 100000}, kDev);
                    inputs++;
                    const RayFlags *r = compiled(p.k);
                    CHECK_EQ(r != nullptr, 1);
                    if (!r) continue;
                    if (kind == RaysKind::Capture) CHECK_EQ(has_capture(*r), 1);
                    if (kind == RaysKind::Occlusion) CHECK_EQ(has_occlusion(*r), 1);
                    CHECK_EQ(p.k.first, kind == RaysKind::First || kind == RaysKind::Occlusion);
                    // the LDS is that of the variant's layout for the resident count, and fits: the general variant beside its
                    // kernel's own static bytes (its resident count is what is left of the limit), the others beside the allowance
                    CHECK_EQ(p.lds, rays_lds(p.k, (size_t)p.resident, d.cached_tree >= 0 ? (size_t)d.cached_nodes : 0, d.has_wide != 0));
                    const bool general = p.k.trees && p.k.bez && p.k.spill;
                    CHECK_EQ(general, d.n_objs > d.n_lds && !d.all_spheres);
                    if (general) CHECK_EQ(p.lds + kDev.general_static <= kDev.lds_limit, 1);
                    else CHECK_EQ(fits_lds(p.lds), 1);
                    CHECK_EQ(p.k.spill, d.n_objs > d.n_lds);
                    // resident objects: all of the scene's LDS list, except the general variant with pending rays beside a full
                    // list -- test_wg_lds_host.py's 727 / 663 (no tree / a 255-node tree cached) less the four staging records
                    // its SPILL form always has
                    const bool lowered = general && !p.k.first && d.n_lds == 768;
                    CHECK_EQ(p.resident, lowered ? (d.cached_tree >= 0 ? 663 - 4 : 727 - 4) : d.n_lds);
                    const cgrt::DeviceScene c = with_resident(d, p.resident);
                    CHECK_EQ(c.n_lds, p.resident);
                    CHECK_EQ(c.prun_end <= c.n_lds && (c.prun_end == 0 || c.prun_end - c.prun_begin >= 3), 1);
                    // persistent workgroups, against the formula written out
                    const long long chip_rays = wgs_written_out(p.k, 1ll << 36) / 2 * (p.k.nt == 64 ? 64 : 256);
                    for (long long n : {1ll, 64ll, 65ll, 1ll << 36, chip_rays - 64, chip_rays, chip_rays + 64, 2 * chip_rays - 64, 2 * chip_rays + 64}) {
                        const RaysPlan q = rays_plan(d, RaysAsk{depth, stats != 0, kind, n}, kDev);
                        CHECK_EQ(q.wgs, wgs_written_out(q.k, n));
                        CHECK_EQ(q.k.id(), p.k.id());
                        CHECK_EQ(q.lds, p.lds);
                    }
                }
    });
    CHECK_EQ(rays_plan(cgrt::DeviceScene{}, RaysAsk{5, false, RaysKind::Full, 1}, kDev).wgs, 1);
    CHECK_EQ(rays_plan(cgrt::DeviceScene{}, RaysAsk{5, false, RaysKind::Full, 65}, kDev).wgs, 1);
    CHECK_EQ(rays_plan(cgrt::DeviceScene{}, RaysAsk{5, false, RaysKind::Full, 257}, kDev).wgs, 2);
    CHECK_EQ(rays_plan(cgrt::DeviceScene{}, RaysAsk{5, false, RaysKind::Full, 1ll << 36}, kDev).wgs, 2048);

    // names and refusal names of fixed scenes
    cgrt::DeviceScene spheres{}, mesh{}, bez{}, many{}, room{};
    spheres.n_objs = spheres.n_lds = 9;
    spheres.all_spheres = spheres.has_glass = 1;
    mesh.n_objs = mesh.n_lds = 7;
    mesh.has_mesh = mesh.has_wide = 1;
    bez.n_objs = bez.n_lds = 7;
    bez.has_bezier = bez.has_glass = 1;
    many.n_objs = 1000;
    many.n_lds = 768;
    many.all_spheres = many.has_glass = 1;
    room.n_objs = 800;
    room.n_lds = 768;
    room.has_mesh = room.has_bezier = room.has_glass = 1;
    check_name(spheres, RaysKind::Full, 5, false, "trace_rays_kernel<TREES=0,BEZ=0,GLASS=1,SPH=1,STATS=0,SPILL=0,FIRST=0,NT=256>");
    check_name(spheres, RaysKind::Full, 1, true, "trace_rays_kernel<TREES=0,BEZ=0,GLASS=0,SPH=1,STATS=0,SPILL=0,FIRST=0,NT=256>");
    check_name(spheres, RaysKind::First, 5, false, "trace_rays_kernel<TREES=0,BEZ=0,GLASS=0,SPH=1,STATS=0,SPILL=0,FIRST=1,NT=256>");
    check_name(spheres, RaysKind::Capture, 5, true, "capture_rays_kernel<TREES=0,BEZ=0,GLASS=1,SPH=1,SPILL=0,NT=256>");
    check_name(spheres, RaysKind::Occlusion, 5, false, "occlusion_rays_kernel<TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=0,NT=256>");
    check_name(mesh, RaysKind::Full, 5, true, "trace_rays_kernel<TREES=1,BEZ=0,GLASS=0,SPH=0,STATS=1,SPILL=0,FIRST=0,NT=256>");
    check_name(mesh, RaysKind::Capture, 5, true, "capture_rays_kernel<TREES=1,BEZ=0,GLASS=0,SPH=0,SPILL=0,NT=256>");
    check_name(mesh, RaysKind::Occlusion, 5, true, "occlusion_rays_kernel<TREES=1,BEZ=0,SPH=0,STATS=1,SPILL=0,NT=256>");
    check_name(bez, RaysKind::Full, 5, true, "trace_rays_kernel<TREES=1,BEZ=1,GLASS=1,SPH=0,STATS=0,SPILL=0,FIRST=0,NT=64>");
    check_name(bez, RaysKind::Capture, 1, false, "capture_rays_kernel<TREES=1,BEZ=1,GLASS=0,SPH=0,SPILL=0,NT=64>");
    check_name(bez, RaysKind::Occlusion, 5, false, "occlusion_rays_kernel<TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=0,NT=64>");
    check_name(many, RaysKind::Full, 5, false, "trace_rays_kernel<TREES=0,BEZ=0,GLASS=1,SPH=1,STATS=0,SPILL=1,FIRST=0,NT=256>");
    check_name(many, RaysKind::Capture, 1, false, "capture_rays_kernel<TREES=0,BEZ=0,GLASS=0,SPH=1,SPILL=1,NT=256>");
    check_name(many, RaysKind::Occlusion, 5, true, "occlusion_rays_kernel<TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=1,NT=256>");
    check_name(room, RaysKind::Full, 1, true, "trace_rays_kernel<TREES=1,BEZ=1,GLASS=1,SPH=0,STATS=0,SPILL=1,FIRST=0,NT=256>");
    check_name(room, RaysKind::First, 5, true, "trace_rays_kernel<TREES=1,BEZ=1,GLASS=0,SPH=0,STATS=0,SPILL=1,FIRST=1,NT=256>");
    check_name(room, RaysKind::Capture, 5, false, "capture_rays_kernel<TREES=1,BEZ=1,GLASS=1,SPH=0,SPILL=1,NT=256>");
    check_name(room, RaysKind::Occlusion, 5, false, "occlusion_rays_kernel<TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=1,NT=256>");
    const RaysAsk full{5, false, RaysKind::Full, 1000};
    CHECK_EQ(std::strcmp(rays_plan(spheres, full, kDev).what(), "ray list"), 0);
    CHECK_EQ(std::strcmp(rays_plan(bez, full, kDev).what(), "ray list (Bezier)"), 0);
    CHECK_EQ(std::strcmp(rays_plan(many, full, kDev).what(), "ray list, SPILL (spheres)"), 0);
    CHECK_EQ(std::strcmp(rays_plan(room, full, kDev).what(), "ray list, SPILL (general)"), 0);
    std::printf("plans checked: %lld\n", inputs);
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
#endif
