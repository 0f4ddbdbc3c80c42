// The launch plan of the grid AOV pass (cgrt_aov_plan.h: aov_choice, aov_plan) over every scene-trait combination scene_traits
// can produce (rays_plan.cpp's sweep): every choice is a row of CGRT_AOV_VARIANTS, every row is chosen by some class, each
// choice is rays_plan's nearest-hit row for the same traits, and the rows' LDS fits.  CPU build under ASan + UBSan, driven by
// tests/test_aov_host.py.
#define RAYS_PLAN_NO_MAIN
#include "rays_plan.cpp"

#include "cgrt_aov_plan.h"

#define X(T, B, P, SP, NT) AovFlags{T != 0, B != 0, P != 0, SP != 0, NT},
static const AovFlags kAov[] = {CGRT_AOV_VARIANTS(X)};
#undef X
static constexpr int kRows = (int)(sizeof(kAov) / sizeof(kAov[0]));

static int row_of(const AovFlags &f) {
    for (int i = 0; i < kRows; i++)
        if (kAov[i].id() == f.id()) return i;
    return -1;
}

int main() {
    CHECK_EQ(kRows, 6);
    CHECK_EQ(sizeof(cgrt_grid_aov), 40);
    // the list: distinct rows, each the flags of a compiled nearest-hit row of CGRT_RAY_VARIANTS without STATS -- and all of those
    int first_rows = 0;
    for (const RayFlags &r : kRays)
        if (r.first && !r.stats) {
            first_rows++;
            CHECK_EQ(row_of(aov_flags(r)) >= 0, 1);
        }
    CHECK_EQ(first_rows, kRows);
    for (int i = 0; i < kRows; i++) {
        const RayFlags *r = compiled(aov_ray_flags(kAov[i]));
        CHECK_EQ(r != nullptr, 1);
        for (int j = 0; j < i; j++) CHECK_EQ(kAov[i].id() != kAov[j].id(), 1);
        // the row's layout at a full object list (the general row: at the count it always keeps) fits a workgroup's LDS, and is
        // the nearest-hit row's
        const bool general = kAov[i].trees && kAov[i].bez && kAov[i].spill;
        const size_t resident = general ? 600 : (size_t)cgrt::kLdsObjsMax;
        for (int wide = 0; wide < 2; wide++) {
            CHECK_EQ(fits_lds(rays_lds(aov_ray_flags(kAov[i]), resident, cgrt::kNodeCache, wide != 0)), 1);
            CHECK_EQ(wg_lds(aov_ask(kAov[i]), resident, cgrt::kNodeCache, wide != 0).total,
                     rays_lds(aov_ray_flags(kAov[i]), resident, cgrt::kNodeCache, wide != 0));
        }
    }

    long long inputs = 0, chosen[kRows] = {};
    for_each_traits([&](const cgrt::DeviceScene &d) {
        inputs++;
        const AovFlags k = aov_choice(d);
        const int row = row_of(k);
        CHECK_EQ(row >= 0, 1);
        if (row < 0) return;
        chosen[row]++;
        const RaysPlan r = rays_plan(d, RaysAsk{5, false, RaysKind::First, 100000}, kDev);
        CHECK_EQ(aov_ray_flags(k).id(), r.k.id());
        // the launch: the nearest-hit query's resident objects and LDS, one workgroup per tile of the eye pass's grid
        const AovPlan p = aov_plan(d, 45, 19, AovDevice{kDev.lds_limit, kDev.general_static});
        CHECK_EQ(p.k.id(), k.id());
        CHECK_EQ(p.resident, r.resident);
        CHECK_EQ(p.lds, r.lds);
        CHECK_EQ(p.lds, wg_lds(aov_ask(k), with_resident(d, p.resident)).total);
        CHECK_EQ(p.lds + kDev.general_static <= kDev.lds_limit, 1);
        CHECK_EQ(p.xcd_tiles, d.n_objs <= d.n_lds && d.has_mesh && !d.has_bezier);
        const int tw = k.nt == 64 ? 16 : 32, th = k.nt == 64 ? 4 : 8;
        const int tiles = ((45 + tw - 1) / tw) * ((19 + th - 1) / th);
        if (p.xcd_tiles) CHECK_EQ(p.blocks >= tiles && p.blocks % (kXcds * kSuperTiles) == 0, 1);
        else CHECK_EQ(p.blocks, tiles);
        CHECK_EQ(aov_plan(d, 1, 1, AovDevice{kDev.lds_limit, kDev.general_static}).blocks, p.xcd_tiles ? kXcds * kSuperTiles : 1);
    });
    for (int i = 0; i < kRows; i++) CHECK_EQ(chosen[i] > 0, 1);

    // names of fixed scenes
    cgrt::DeviceScene spheres{}, mesh{}, bez{}, plain{}, many{}, room{};
    spheres.n_objs = spheres.n_lds = 9;
    spheres.all_spheres = spheres.has_glass = 1;
    mesh.n_objs = mesh.n_lds = 7;
    mesh.has_mesh = mesh.has_wide = 1;
    bez.n_objs = bez.n_lds = 7;
    bez.has_bezier = bez.has_glass = 1;
    plain.n_objs = plain.n_lds = 5;
    many.n_objs = 1000;
    many.n_lds = 768;
    many.all_spheres = many.has_glass = 1;
    room.n_objs = 800;
    room.n_lds = 768;
    room.has_mesh = room.has_bezier = room.has_glass = 1;
    const struct {
        const cgrt::DeviceScene *d;
        const char *name, *what;
    } named[] = {{&spheres, "aov_grid_kernel<TREES=0,BEZ=0,SPH=1,SPILL=0,NT=256>", "grid AOVs"},
                 {&mesh, "aov_grid_kernel<TREES=1,BEZ=0,SPH=0,SPILL=0,NT=256>", "grid AOVs"},
                 {&bez, "aov_grid_kernel<TREES=1,BEZ=1,SPH=0,SPILL=0,NT=64>", "grid AOVs (Bezier)"},
                 {&plain, "aov_grid_kernel<TREES=0,BEZ=0,SPH=0,SPILL=0,NT=256>", "grid AOVs"},
                 {&many, "aov_grid_kernel<TREES=0,BEZ=0,SPH=1,SPILL=1,NT=256>", "grid AOVs, SPILL (spheres)"},
                 {&room, "aov_grid_kernel<TREES=1,BEZ=1,SPH=0,SPILL=1,NT=256>", "grid AOVs, SPILL (general)"}};
    for (const auto &c : named) {
        char buf[160];
        const AovPlan p = aov_plan(*c.d, 1920, 1080, AovDevice{kDev.lds_limit, kDev.general_static});
        p.name(buf, sizeof(buf));
        if (std::strcmp(buf, c.name) != 0 || std::strcmp(p.what(), c.what) != 0) {
            std::printf("FAIL name: %s / %s, expected %s / %s\n", buf, p.what(), c.name, c.what);
            g_failed++;
        }
    }
    std::printf("traits checked: %lld\n", inputs);
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
