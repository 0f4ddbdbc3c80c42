// CPU test of the sphere masks' candidate test (cgraytracing_amd/csrc/cgrt_sphere_mask.h), built with ASan + UBSan and
// -ffp-contract=off by tests/test_sphere_mask_host.py.
//
// CONSERVATIVE (may never fail): for a set of frames, cameras and scenes every pixel of every wave tile is enumerated with 33 lens
// points -- the centre, 16 on the rim at radius 1 - 2^-40, 16 pseudo-random -- and no sphere that sphere_surely_missed() drops may
// pass both of sphere_len's tests (cgrt_scene_walk.hpp, restated below in the device's operation order) for any of those rays.
// NOT VACUOUS: on the C2 frame at 1920x1080 the wave tiles of class 3 keep at most 3.5 of the 8 spheres on average (the exact
// minimum, from the rays themselves, is 2.95).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cgrt_sphere_mask.h"

static int failed = 0;
#define CHECK(c, ...)                                                  \
    do {                                                               \
        if (!(c)) {                                                    \
            if (failed++ < 20) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                              \
    } while (0)

struct Sph {
    double c[3], r;
    bool special, transp;
};
static std::vector<Sph> c2_scene() {  // tests/scenes.py scene_c2
    return {{{0.0, -10020, 0}, 10000, false, false}, {{10020, 0.0, 0}, 10000, false, false}, {{-10020, 0.0, 0}, 10000, false, false},
            {{0.0, 0.0, 10040}, 10000, false, false}, {{0.0, 10020, 0}, 10000, false, false}, {{-15.0, -20.0, 60}, 10, false, false},
            {{10.0, -13.0, 30}, 7, true, false},      {{-8.0, -13.0, 25}, 7, true, true}};
}
static cgrt_camera camera(double x, double y, double z, double lens, double focus = 20.0) {
    cgrt_camera c{};
    c.cam[0] = x; c.cam[1] = y; c.cam[2] = z;
    c.half_width = 10.0;
    c.focus_plane = focus;
    c.lens_radius = lens;
    return c;
}
static GridParams frame(const cgrt_camera &cam, int W, int H, int rows = 0, int stripe_rows = 0, int rank = 0, int nranks = 1) {
    cgrt_grid gr{};
    gr.width = W; gr.height = H; gr.rows = rows ? rows : H;
    gr.stripe_rows = stripe_rows; gr.stripe_rank = rank; gr.stripe_nranks = nranks;
    gr.spp = 1; gr.spp_total = 1; gr.max_depth = 5;
    return grid_params(&cam, &gr);
}

// sphere_len's two tests (cgrt_scene_walk.hpp): true = the ray gets a distance from the sphere
static bool sphere_len_finite(const Sph &s, Vec3d o, Vec3d d) {
    const double r2 = s.r * s.r;  // what the scene stores (ObjRec::s0)
    const Vec3d l = vec3d(s.c[0] - o.x, s.c[1] - o.y, s.c[2] - o.z);
    const double tca = dot3d(l, d), l2 = dot3d(l, l);
    if (tca < 0 && l2 > r2) return false;
    const double d2 = l2 - tca * tca;
    return !(d2 > r2);
}

static std::vector<double> lens_points() {  // 33 (sx, sy) with sx^2 + sy^2 < 1
    std::vector<double> p = {0.0, 0.0};
    const double rim = 1.0 - 0x1p-40;
    for (int k = 0; k < 16; k++) {
        const double a = 2 * 3.14159265358979323846 * k / 16;
        p.push_back(std::cos(a) * rim);
        p.push_back(std::sin(a) * rim);
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;
    while (p.size() < 2 * 33) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const double sx = (double)(x >> 11) * 0x1p-52 - 1, sy = (double)((x * 0x9E3779B97F4A7C15ull) >> 11) * 0x1p-52 - 1;
        if (sx * sx + sy * sy < 1) { p.push_back(sx); p.push_back(sy); }
    }
    return p;
}

struct Tally {
    long long wave_tiles = 0, class3 = 0, class3_candidates = 0, dropped = 0, rays = 0;
};
// every `row_step`-th wave-tile row of the frame
static Tally run(const char *name, const GridParams &g, const std::vector<Sph> &sc, int row_step = 1, bool rays = true) {
    static const std::vector<double> lp = lens_points();
    Tally t;
    const int wtx = (g.W + kWaveTileW - 1) / kWaveTileW, wty = (g.rows + kWaveTileH - 1) / kWaveTileH;
    const bool lens = g.lens_radius > 0;
    const Vec3d cam = vec3d(g.cam[0], g.cam[1], g.cam[2]);
    std::vector<char> missed(sc.size());
    for (int wy = 0; wy < wty; wy += row_step)
        for (int wx = 0; wx < wtx; wx++) {
            const TileRays tr = wave_tile_rays(g, wx, wy);
            t.wave_tiles++;
            int cls = 3, cand = 0;
            for (size_t i = 0; i < sc.size(); i++) {
                const Vec3d c = vec3d(sc[i].c[0], sc[i].c[1], sc[i].c[2]);
                missed[i] = sphere_surely_missed(g, tr, c, sc[i].r * sc[i].r);
                if (sc[i].special && !cone_clear_of(g, tr.cone, c, sc[i].r)) cls = 1;
                cand += missed[i] ? 0 : 1;
                t.dropped += missed[i] ? 1 : 0;
            }
            if (cls == 3) {
                t.class3++;
                t.class3_candidates += cand;
                for (size_t i = 0; i < sc.size(); i++) CHECK(!sc[i].special || missed[i], "%s: special sphere %zu is a candidate of class-3 wave tile (%d, %d)", name, i, wx, wy);
            }
            if (!rays) continue;
            for (int ly = 0; ly < kWaveTileH; ly++)
                for (int lx = 0; lx < kWaveTileW; lx++) {
                    const int w = wx * kWaveTileW + lx, j = wy * kWaveTileH + ly, h = global_row(g, j);
                    if (!(w < g.W && j < g.rows && h < g.H)) continue;  // not a live lane
                    const Vec3d pdir = pixel_dir(g, cam, w, j);
                    const double s = (g.focus_plane - cam.z) / pdir.z;
                    const Vec3d pof = vec3d(pdir.x * s + cam.x, pdir.y * s + cam.y, pdir.z * s + cam.z);
                    for (size_t k = 0; k < (lens ? lp.size() / 2 : 1); k++) {
                        Vec3d o = cam, d = pdir;
                        if (lens) {
                            o = vec3d(cam.x + lp[2 * k] * g.lens_radius, cam.y + lp[2 * k + 1] * g.lens_radius, cam.z + 0.0 * g.lens_radius);
                            d = normalized3d(vec3d(pof.x - o.x, pof.y - o.y, pof.z - o.z));
                        }
                        t.rays++;
                        for (size_t i = 0; i < sc.size(); i++)
                            if (missed[i])
                                CHECK(!sphere_len_finite(sc[i], o, d), "%s: sphere %zu dropped from wave tile (%d, %d) but pixel (%d, %d) lens point %zu meets it",
                                      name, i, wx, wy, w, j, k);
                    }
                }
        }
    std::printf("%-44s wave tiles %6lld  class 3 %6lld  candidates/class-3 tile %.3f  dropped/tile %.2f  rays %lld\n", name, t.wave_tiles, t.class3,
                t.class3 ? (double)t.class3_candidates / t.class3 : 0.0, (double)t.dropped / t.wave_tiles, t.rays);
    return t;
}

int main() {
    const std::vector<Sph> c2 = c2_scene();
    const cgrt_camera dof = camera(0, 0, -10, 1.5), pin = camera(0, 0, -10, 0);

    // not vacuous: every wave tile of the C2 frame (no rays), then the rays of every 7th wave-tile row
    const Tally all = run("c2 1920x1080 (masks only)", frame(dof, 1920, 1080), c2, 1, false);
    CHECK(all.class3 > 20000, "class-3 wave tiles %lld", all.class3);
    CHECK((double)all.class3_candidates <= 3.5 * (double)all.class3, "mean candidates %.3f", (double)all.class3_candidates / (double)all.class3);
    run("c2 1920x1080 every 7th row", frame(dof, 1920, 1080), c2, 7);
    run("c2 200x52", frame(dof, 200, 52), c2);
    run("c2 pinhole 200x52", frame(pin, 200, 52), c2);
    run("c2 pinhole 1920x1080 every 31st row", frame(pin, 1920, 1080), c2, 31);
    run("c2 lens 0.01 192x108", frame(camera(0, 0, -10, 0.01), 192, 108), c2);
    run("c2 lens 6 192x108", frame(camera(0, 0, -10, 6), 192, 108), c2);
    run("c2 camera (12, 9, -10) lens", frame(camera(12, 9, -10, 1.5), 192, 108), c2);
    run("c2 camera (12, 9, -10) pinhole", frame(camera(12, 9, -10, 0), 192, 108), c2);
    run("c2 camera in the room z = 5, lens", frame(camera(0, 0, 5, 1.5), 192, 108), c2);
    run("c2 camera in the room z = 5, pinhole", frame(camera(0, 0, 5, 0), 192, 108), c2);
    run("c2 camera inside the floor sphere, lens", frame(camera(0, -25, -10, 1.5), 192, 108), c2);
    run("c2 camera inside the floor sphere, pinhole", frame(camera(0, -25, -10, 0), 192, 108), c2);
    run("c2 focus plane behind the camera", frame(camera(0, 0, -10, 1.5, -30.0), 96, 54), c2);
    run("c2 stripe (8, 1, 4)", frame(dof, 192, 108, 32, 8, 1, 4), c2);
    run("c2 stripe (16, 3, 8)", frame(dof, 200, 300, 48, 16, 3, 8), c2);
    run("c2 stripe (16, 3, 8) pinhole", frame(pin, 200, 300, 48, 16, 3, 8), c2);

    // spheres around and behind the camera
    std::vector<Sph> more = c2;
    more.push_back({{3.0, 2.0, -10.0}, 2, false, false});   // straddles the lens plane
    more.push_back({{0.0, 0.0, -30.0}, 5, false, false});   // wholly behind the camera
    more.push_back({{1.0, 0.5, -10.5}, 3, false, false});   // holds the camera and the lens
    for (const cgrt_camera &cam : {dof, pin, camera(0, 0, -10, 6)}) {
        const Tally t = run("c2 + spheres at the lens plane and behind", frame(cam, 192, 108), more);
        CHECK(t.dropped > 0, "nothing dropped");
    }

    // a diffuse sphere tangent to a tile's outermost ray to within 1e-9, on either side of tangency: the lower-left pixel of wave
    // tile (3, 5) of a 192x108 frame, pinhole and the lens point at the rim
    for (int lensed = 0; lensed < 2; lensed++) {
        const cgrt_camera cam = lensed ? dof : pin;
        const GridParams g = frame(cam, 192, 108);
        const Vec3d cm = vec3d(g.cam[0], g.cam[1], g.cam[2]);
        const Vec3d pdir = pixel_dir(g, cm, 3 * kWaveTileW, 5 * kWaveTileH);
        Vec3d o = cm, d = pdir;
        if (lensed) {
            const double s = (g.focus_plane - cm.z) / pdir.z, rim = 1.0 - 0x1p-40;
            o = vec3d(cm.x + rim * g.lens_radius, cm.y, cm.z);
            d = normalized3d(vec3d(pdir.x * s + cm.x - o.x, pdir.y * s + cm.y - o.y, pdir.z * s + cm.z - o.z));
        }
        Vec3d n = vec3d(-1 - d.x * (-d.x - d.y), -1 - d.y * (-d.x - d.y), 0 - d.z * (-d.x - d.y));  // (-1, -1, 0) less its part along d
        n = normalized3d(n);
        for (double r : {0.5, 3.0})
            for (double gap : {1e-9, -1e-9, 1e-12, -1e-12, 0.0}) {
                std::vector<Sph> sc = c2;
                const double t = 25.0, off = r + gap;
                sc.push_back({{o.x + d.x * t + n.x * off, o.y + d.y * t + n.y * off, o.z + d.z * t + n.z * off}, r, false, false});
                run(lensed ? "tangent sphere, lens" : "tangent sphere, pinhole", g, sc);
            }
    }
    std::printf("ok: %d failed checks\n", failed);
    return failed ? 1 : 0;
}
