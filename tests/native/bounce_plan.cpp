// The launch plan of the bounce query (cgrt_rays_plan.h: RaysKind::Bounce) over the trait sweep of rays_plan.cpp: it is the
// nearest-hit query's plan field for field -- flags, resident objects, LDS, workgroups --, its variant is a compiled one that
// has a bounce kernel, max_depth does not reach it, and the names are the literal strings.  CPU build under ASan + UBSan,
// driven by tests/test_bounce_plan_host.py.
#define RAYS_PLAN_NO_MAIN
#include "rays_plan.cpp"

int main() {
    long long inputs = 0;
    for_each_traits([&](const cgrt::DeviceScene &d) {
        for (int depth : {1, 5})
            for (int stats = 0; stats < 2; stats++)
                for (long long n : {1ll, 64ll, 65ll, 100000ll, 1ll << 36}) {
                    const RaysPlan b = rays_plan(d, RaysAsk{depth, stats != 0, RaysKind::Bounce, n}, kDev);
                    const RaysPlan f = rays_plan(d, RaysAsk{depth, stats != 0, RaysKind::First, n}, kDev);
                    inputs++;
                    CHECK_EQ(b.k.id(), f.k.id());
                    CHECK_EQ(b.k.nt, f.k.nt);
                    CHECK_EQ(b.resident, f.resident);
                    CHECK_EQ(b.lds, f.lds);
                    CHECK_EQ(b.wgs, f.wgs);
                    CHECK_EQ(std::strcmp(b.what(), f.what()), 0);
                    const RayFlags *r = compiled(b.k);
                    CHECK_EQ(r != nullptr, 1);
                    if (!r) continue;
                    CHECK_EQ(has_bounce(*r), 1);
                    CHECK_EQ(b.k.first, 1);
                    CHECK_EQ(b.k.glass, 0);  // no pending rays: the LDS has no pending level
                    CHECK_EQ(b.lds, rays_lds(b.k, (size_t)b.resident, d.cached_tree >= 0 ? (size_t)d.cached_nodes : 0, d.has_wide != 0));
                    // the depth is the caller's loop, not the launch's
                    const RaysPlan other = rays_plan(d, RaysAsk{depth == 1 ? 5 : 1, stats != 0, RaysKind::Bounce, n}, kDev);
                    CHECK_EQ(other.k.id(), b.k.id());
                    CHECK_EQ(other.lds, b.lds);
                    CHECK_EQ(other.wgs, b.wgs);
                }
    });
    // has_bounce is has_occlusion's rule: the nearest-hit rows, and only they
    int rows = 0;
    for (const RayFlags &r : kRays) {
        CHECK_EQ(has_bounce(r), r.first);
        rows += has_bounce(r);
    }
    CHECK_EQ(rows >= 7, 1);

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
    check_name(spheres, RaysKind::Bounce, 5, false, "bounce_rays_kernel<TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=0,NT=256>");
    check_name(spheres, RaysKind::Bounce, 1, true, "bounce_rays_kernel<TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=0,NT=256>");
    check_name(bez, RaysKind::Bounce, 5, false, "bounce_rays_kernel<TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=0,NT=64>");
    check_name(bez, RaysKind::Bounce, 5, true, "bounce_rays_kernel<TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=0,NT=64>");
    check_name(mesh, RaysKind::Bounce, 5, false, "bounce_rays_kernel<TREES=1,BEZ=0,SPH=0,STATS=0,SPILL=0,NT=256>");
    check_name(mesh, RaysKind::Bounce, 5, true, "bounce_rays_kernel<TREES=1,BEZ=0,SPH=0,STATS=1,SPILL=0,NT=256>");
    check_name(many, RaysKind::Bounce, 5, true, "bounce_rays_kernel<TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=1,NT=256>");
    check_name(room, RaysKind::Bounce, 5, false, "bounce_rays_kernel<TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=1,NT=256>");
    std::printf("plans checked: %lld\n", inputs);
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
