// CPU test of the proven first hit behind the terminal-diffuse body's sure tiles (cgraytracing_amd/csrc/cgrt_sure_first.h), built
// with ASan + UBSan and -ffp-contract=off by tests/test_sure_first_host.py.
//
// SOUND (may never fail): for a set of frames, cameras and scenes every pixel of every wave tile that sphere_sure_first() names a
// winner for is enumerated with the 33 lens points of sphere_mask.cpp -- the centre, 16 on the rim at radius 1 - 2^-40, 16
// pseudo-random -- and the device's sphere loop (sphere_len in its operation order, strict < over ALL spheres) must end on that
// winner for every one of those rays.  The mask handed to the proof is the one tile_order_kernel computes (sphere_surely_missed).
// REFUSALS: scenes and cameras where whole frames, or named tiles, must have no winner.
// NOT VACUOUS: on the C2 frame at 1920x1080 under the thin lens at least 80 % of the wave tiles of class-3 tiles have a winner.
// argv[1], optional: a text file of spheres "x y z r special" (tests/scenes.py many_spheres), run as one more scene.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cgrt_sure_first.h"

static int failed = 0;
#define CHECK(c, ...)                                                  \
    do {                                                               \
        if (!(c)) {                                                    \
            if (failed++ < 20) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                              \
    } while (0)

struct Sph {
    double c[3], r;
    bool special;
};
static std::vector<Sph> walls() {  // tests/scenes.py wall_spheres
    return {{{0.0, -10020, 0}, 10000, false}, {{10020, 0.0, 0}, 10000, false}, {{-10020, 0.0, 0}, 10000, false},
            {{0.0, 0.0, 10040}, 10000, false}, {{0.0, 10020, 0}, 10000, false}};
}
static std::vector<Sph> c1_scene() {
    std::vector<Sph> s = walls();
    s.push_back({{-15.0, -20.0, 60}, 10, false});
    return s;
}
static std::vector<Sph> c2_scene() {
    std::vector<Sph> s = c1_scene();
    s.push_back({{10.0, -13.0, 30}, 7, true});
    s.push_back({{-8.0, -13.0, 25}, 7, true});
    return s;
}
static cgrt_camera camera(double x, double y, double z, double lens, double focus = 20.0) {
    cgrt_camera c{};
    c.cam[0] = x; c.cam[1] = y; c.cam[2] = z;
    c.half_width = 10.0;
    c.focus_plane = focus;
    c.lens_radius = lens;
    return c;
}
static GridParams frame(const cgrt_camera &cam, int W, int H, int rows = 0, int row_offset = 0, int stripe_rows = 0, int rank = 0, int nranks = 1) {
    cgrt_grid gr{};
    gr.width = W; gr.height = H; gr.rows = rows ? rows : H; gr.row_offset = row_offset;
    gr.stripe_rows = stripe_rows; gr.stripe_rank = rank; gr.stripe_nranks = nranks;
    gr.spp = 1; gr.spp_total = 1; gr.max_depth = 5;
    return grid_params(&cam, &gr);
}

// sphere_len (cgrt_scene_walk.hpp) in the device's operation order; sqrt is correctly rounded here as sqrt_cr is there
static const double kInf = 1e308;
static double sphere_len(const Sph &s, Vec3d o, Vec3d d) {
    const double r2 = s.r * s.r;  // what the scene stores (ObjRec::s0)
    const Vec3d l = vec3d(s.c[0] - o.x, s.c[1] - o.y, s.c[2] - o.z);
    const double tca = dot3d(l, d), l2 = dot3d(l, l);
    double len = kInf;
    if (!(tca < 0 && l2 > r2)) {
        const double d2 = l2 - tca * tca;
        if (!(d2 > r2)) {
            const double thc = std::sqrt(r2 - d2);
            const double t0 = tca - thc, t1 = tca + thc;
            len = (t0 < 0) ? t1 : t0;
        }
    }
    return len;
}
static int first_hit(const std::vector<Sph> &sc, Vec3d o, Vec3d d) {  // intersect_scene's sphere loop
    double best = kInf;
    int id = -1;
    for (size_t i = 0; i < sc.size(); i++) {
        const double len = sphere_len(sc[i], o, d);
        if (len < best) {
            best = len;
            id = (int)i;
        }
    }
    return id;
}

static std::vector<double> lens_points() {  // 33 (sx, sy) with sx^2 + sy^2 < 1: sphere_mask.cpp's
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
    long long wave_tiles = 0, class3 = 0, class3_sure = 0, sure = 0, rays = 0, missing = 0, missing_sure = 0;
    std::vector<int> win;  // per wave tile
    int wtx = 0;
};
// class3: wave tiles of class-3 TILES (all the 2x2 wave tiles of the 32x8 tile are clear of every special sphere), as
// tile_order_kernel folds them.  all_rays: also trace the wave tiles without a winner, to count the rays that hit nothing.
static Tally run(const char *name, const GridParams &g, const std::vector<Sph> &sc, bool all_rays = false) {
    static const std::vector<double> lp = lens_points();
    Tally t;
    const int wtx = (g.W + kWaveTileW - 1) / kWaveTileW, wty = (g.rows + kWaveTileH - 1) / kWaveTileH;
    t.wtx = wtx;
    t.win.assign((size_t)wtx * wty, -1);
    const bool lens = g.lens_radius > 0;
    const Vec3d cam = vec3d(g.cam[0], g.cam[1], g.cam[2]);
    const auto get = [&sc](int i) { return SureSphere{vec3d(sc[i].c[0], sc[i].c[1], sc[i].c[2]), sc[i].r * sc[i].r}; };
    std::vector<char> wcls3((size_t)wtx * wty);
    for (int wy = 0; wy < wty; wy++)
        for (int wx = 0; wx < wtx; wx++) {
            const TileCone tc = wave_tile_cone(g, wx, wy);
            bool c3 = true;
            for (const Sph &s : sc)
                if (s.special && !cone_clear_of(g, tc, vec3d(s.c[0], s.c[1], s.c[2]), s.r)) c3 = false;
            wcls3[(size_t)wy * wtx + wx] = c3;
        }
    for (int wy = 0; wy < wty; wy++)
        for (int wx = 0; wx < wtx; wx++) {
            const TileRays tr = wave_tile_rays(g, wx, wy);
            uint32_t mask = 0;
            for (size_t i = 0; i < sc.size() && i < 32; i++)
                if (!sphere_surely_missed(g, tr, vec3d(sc[i].c[0], sc[i].c[1], sc[i].c[2]), sc[i].r * sc[i].r)) mask |= 1u << i;
            const int win = sphere_sure_first(g, tr, (int)sc.size(), get, mask);
            CHECK(win >= -1 && win < (int)sc.size() && (win < 0 || ((mask >> win) & 1u)), "%s: winner %d of wave tile (%d, %d) is no bit of its mask %x", name, win, wx, wy, mask);
            t.win[(size_t)wy * wtx + wx] = win;
            t.wave_tiles++;
            t.sure += win >= 0;
            bool c3 = true;
            for (int b = 0; b < 2; b++)
                for (int a = 0; a < 2; a++) {
                    const int x = (wx & ~1) + a, y = (wy & ~1) + b;
                    if (x < wtx && y < wty && !wcls3[(size_t)y * wtx + x]) c3 = false;
                }
            if (c3) {
                t.class3++;
                t.class3_sure += win >= 0;
                CHECK(win < 0 || !sc[win].special, "%s: the winner %d of class-3 wave tile (%d, %d) reflects or refracts", name, win, wx, wy);
            }
            if (win < 0 && !all_rays) continue;
            bool miss = false;
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
                        const int id = first_hit(sc, o, d);
                        miss = miss || id < 0;
                        if (win >= 0)
                            CHECK(id == win, "%s: wave tile (%d, %d) is sure of sphere %d but pixel (%d, %d) lens point %zu hits %d first", name, wx, wy, win, w, j, k, id);
                    }
                }
            t.missing += miss;
            t.missing_sure += miss && win >= 0;
        }
    std::printf("%-46s wave tiles %6lld  sure %6lld  of class-3 tiles' %6lld: %6lld (%.1f %%)  rays %lld\n", name, t.wave_tiles, t.sure, t.class3,
                t.class3_sure, t.class3 ? 100.0 * (double)t.class3_sure / (double)t.class3 : 0.0, t.rays);
    return t;
}
// the wave tile whose pinhole rays cover the scene point p
static size_t wave_tile_of(const GridParams &g, const Tally &t, Vec3d p) {
    const double s = (0 - g.cam[2]) / (p.z - g.cam[2]);
    const double px = g.cam[0] + (p.x - g.cam[0]) * s, py = g.cam[1] + (p.y - g.cam[1]) * s;
    const int w = (int)std::floor((px / g.half_width + 1) / 2 * g.W), h = (int)std::floor((py / (g.half_width * g.H / g.W) + 1) / 2 * g.H);
    return (size_t)(h / kWaveTileH) * t.wtx + (size_t)(w / kWaveTileW);
}

int main(int argc, char **argv) {
    const std::vector<Sph> c2 = c2_scene();
    const cgrt_camera dof = camera(0, 0, -10, 1.5), pin = camera(0, 0, -10, 0);

    // ---- sound, and not vacuous ----
    const Tally full = run("c2 1920x1080", frame(dof, 1920, 1080), c2);
    const double share = full.class3 ? (double)full.class3_sure / (double)full.class3 : 0.0;
    std::printf("share of the class-3 tiles' wave tiles with a winner, c2 1920x1080 thin lens: %.4f (%lld of %lld)\n", share, full.class3_sure, full.class3);
    CHECK(full.class3 > 20000, "class-3 wave tiles %lld", full.class3);
    CHECK(share >= 0.80, "share %.4f", share);
    run("c2 pinhole 1920x1080", frame(pin, 1920, 1080), c2);
    run("c2 192x108", frame(dof, 192, 108), c2);
    run("c2 pinhole 192x108", frame(pin, 192, 108), c2);
    run("c2 200x52", frame(dof, 200, 52), c2);
    run("c2 pinhole 200x52", frame(pin, 200, 52), c2);
    run("c2 stripe (8, 1, 2)", frame(dof, 192, 108, 56, 0, 8, 1, 2), c2);
    run("c2 stripe (8, 1, 2) pinhole", frame(pin, 192, 108, 56, 0, 8, 1, 2), c2);
    run("c2 rows 40 from 24", frame(dof, 192, 108, 40, 24), c2);
    run("c2 rows 30 from 78, pinhole", frame(pin, 200, 108, 30, 78), c2);
    run("c2 lens 0.01 192x108", frame(camera(0, 0, -10, 0.01), 192, 108), c2);
    run("c2 lens 6 192x108", frame(camera(0, 0, -10, 6), 192, 108), c2);
    run("c2 camera (12, 9, -10) lens", frame(camera(12, 9, -10, 1.5), 192, 108), c2);
    run("c2 camera (12, 9, -10) pinhole", frame(camera(12, 9, -10, 0), 192, 108), c2);
    run("c2 camera in the room z = 5, pinhole", frame(camera(0, 0, 5, 0), 192, 108), c2);
    const Tally c1 = run("c1 192x108", frame(dof, 192, 108), c1_scene());
    CHECK(c1.sure > 0, "c1: no winner at all");
    run("c1 pinhole 192x108", frame(pin, 192, 108), c1_scene());
    if (argc > 1) {
        std::vector<Sph> sc;
        if (FILE *f = std::fopen(argv[1], "r")) {
            Sph s;
            int special;
            while (std::fscanf(f, "%lf %lf %lf %lf %d", &s.c[0], &s.c[1], &s.c[2], &s.r, &special) == 5) {
                s.special = special != 0;
                sc.push_back(s);
            }
            std::fclose(f);
        }
        CHECK(sc.size() == 32, "scene file: %zu spheres", sc.size());
        const Tally a = run("scene file, lens", frame(dof, 192, 108), sc), b = run("scene file, pinhole", frame(pin, 192, 108), sc);
        CHECK(a.sure > 0 && b.sure > 0, "scene file: no winner at all");
    }

    // ---- refusals ----
    {   // a room without its back wall: rays can miss.  No tile with such a ray has a winner; the other walls still do.
        std::vector<Sph> open = c2;
        open.erase(open.begin() + 3);
        for (const cgrt_camera &cam : {dof, pin}) {
            const Tally t = run("c2 without the back wall", frame(cam, 192, 108), open, true);
            CHECK(t.missing > 0 && t.missing_sure == 0 && t.sure > 0, "missing %lld, of them sure %lld, sure %lld", t.missing, t.missing_sure, t.sure);
        }
    }
    for (const cgrt_camera &cam : {camera(0, -25, -10, 1.5), camera(0, -25, -10, 0)}) {
        const Tally t = run("c2 camera inside the floor sphere", frame(cam, 192, 108), c2);
        CHECK(t.sure == 0, "sure %lld", t.sure);
    }
    for (const cgrt_camera &cam : {camera(0, 0, 5, 1.5), camera(0, 0, 0, 1.5)}) {
        const Tally t = run("c2 lens camera at z >= 0", frame(cam, 192, 108), c2);
        CHECK(t.sure == 0, "sure %lld", t.sure);
    }
    {   // a small diffuse sphere poking 0.01 out of the back wall (surface z = 40 - (x^2 + y^2) / 2e4 there), inside a tile
        for (const cgrt_camera &cam : {dof, pin}) {
            const double x = 3.3, y = 2.1, r = 0.5, wall_z = 10040 - std::sqrt(1e8 - x * x - y * y);
            std::vector<Sph> sc = c2;
            sc.push_back({{x, y, wall_z + r - 0.01}, r, false});
            const GridParams g = frame(cam, 192, 108);
            const Tally t = run("c2 + a sphere poking 0.01 out of the back wall", g, sc);
            const size_t wt = wave_tile_of(g, t, vec3d(x, y, wall_z - 0.01));
            CHECK(t.win[wt] < 0, "the wave tile %zu over the poking sphere is sure of %d", wt, t.win[wt]);
            CHECK(t.sure > 0, "no winner at all");
        }
    }
    // a diffuse sphere tangent to a tile's outermost ray to within 1e-9, on either side of tangency: the lower-left pixel of a wave
    // tile that HAS a winner without the sphere -- (0, 5) on the left wall, (5, 14) on the back wall of the 192x108 frame -- pinhole
    // and the lens point at the rim.  The tile must lose its winner; with the same sphere moved 8 away from the ray -- farther from the beam's axis than the beam's far end is wide, so
    // that (b)'s second direction separates it -- it keeps it.
    for (int lensed = 0; lensed < 2; lensed++) {
        const cgrt_camera cam = lensed ? dof : pin;
        const GridParams g = frame(cam, 192, 108);
        const Tally base = run(lensed ? "tangent sphere: c2 without it, lens" : "tangent sphere: c2 without it, pinhole", g, c2);
        const Vec3d cm = vec3d(g.cam[0], g.cam[1], g.cam[2]);
        const int tiles[2][2] = {{0, 5}, {5, 14}};
        for (const auto &tile : tiles) {
            const int tx = tile[0], ty = tile[1];
            const size_t wt = (size_t)ty * base.wtx + tx;
            const int base_win = base.win[wt];
            CHECK(base_win >= 0, "wave tile (%d, %d) has no winner in the plain scene: the case would check nothing", tx, ty);
            const Vec3d pdir = pixel_dir(g, cm, tx * kWaveTileW, ty * kWaveTileH);
            Vec3d o = cm, d = pdir;
            if (lensed) {
                const double s = (g.focus_plane - cm.z) / pdir.z, rim = 1.0 - 0x1p-40;
                o = vec3d(cm.x + rim * g.lens_radius, cm.y, cm.z);
                d = normalized3d(vec3d(pdir.x * s + cm.x - o.x, pdir.y * s + cm.y - o.y, pdir.z * s + cm.z - o.z));
            }
            Vec3d n = vec3d(-1 - d.x * (-d.x - d.y), -1 - d.y * (-d.x - d.y), 0 - d.z * (-d.x - d.y));  // (-1, -1, 0) less its part along d
            n = normalized3d(n);
            for (double r : {0.5, 1.5})
                for (double gap : {1e-9, -1e-9, 1e-12, -1e-12, 0.0, 8.0}) {
                    std::vector<Sph> sc = c2;
                    const double t = 15.0, off = r + gap;
                    sc.push_back({{o.x + d.x * t + n.x * off, o.y + d.y * t + n.y * off, o.z + d.z * t + n.z * off}, r, false});
                    const Tally ta = run(lensed ? "tangent sphere, lens" : "tangent sphere, pinhole", g, sc);
                    if (gap < 1)
                        CHECK(ta.win[wt] < 0, "wave tile (%d, %d), r %g gap %g: the tile the sphere is tangent to is sure of %d", tx, ty, r, gap, ta.win[wt]);
                    else
                        CHECK(ta.win[wt] == base_win, "wave tile (%d, %d), r %g: a sphere 8 clear of the beam took the winner %d (now %d)", tx, ty, r, base_win, ta.win[wt]);
                }
        }
    }
    {   // condition (b)'s margin, on the function itself: a unit ball whose nearest point lies `gap` from the hull of A = [-1, 1]^2 at
        // z = 0 and P = [-2, 2]^2 at z = 10 is clear only when the gap exceeds r * 1e-9 + 1e-6 -- behind A on the axis (the first
        // direction separates) and beside P's edge at its depth (only the direction without the axial part does)
        const SureBox A{{{-1, 1}, {-1, 1}, {0, 0}}}, P{{{-2, 2}, {-2, 2}, {10, 10}}};
        const struct { double gap; bool clear; } cases[] = {{1e-3, true}, {1e-5, true}, {2e-6, true}, {5e-7, false}, {1e-9, false},
                                                            {0.0, false}, {-1e-9, false}, {-1e-6, false}, {-1e-3, false}, {-0.5, false}};
        for (const auto &c : cases) {
            CHECK(sure_hull_clear_of(A, P, vec3d(0, 0, -(1 + c.gap)), 1.0) == c.clear, "ball behind A, gap %g", c.gap);
            CHECK(sure_hull_clear_of(A, P, vec3d(2 + 1 + c.gap, 0, 10), 1.0) == c.clear, "ball beside P, gap %g", c.gap);
            CHECK(sure_hull_clear_of(A, P, vec3d(0, -(2 + 1 + c.gap), 10), 1.0) == c.clear, "ball below P, gap %g", c.gap);
        }
        CHECK(!sure_hull_clear_of(A, P, vec3d(0, 0, 5), 1.0), "ball inside the hull");
        CHECK(!sure_hull_clear_of(A, P, vec3d(0.5, 0.5, 5), 100.0), "ball around the hull");
    }
    {   // an exact duplicate of the back wall behind it in the list, and in front of it: neither copy is ever a winner
        for (int before = 0; before < 2; before++)
            for (const cgrt_camera &cam : {dof, pin}) {
                std::vector<Sph> sc = c2;
                if (before) sc.insert(sc.begin(), c2[3]);
                else sc.push_back(c2[3]);
                const int a = before ? 0 : 3, b = before ? 4 : 8;
                const Tally t = run(before ? "c2 + the back wall again, in front" : "c2 + the back wall again, behind", frame(cam, 192, 108), sc);
                long long on_copy = 0;
                for (int w : t.win) on_copy += w == a || w == b;
                CHECK(on_copy == 0 && t.sure > 0, "%lld wave tiles are sure of a duplicated wall; sure %lld", on_copy, t.sure);
            }
    }
    {   // 33 spheres: beyond the mask word
        std::vector<Sph> sc = c2;
        for (int i = 0; sc.size() < 33; i++) sc.push_back({{-12.0 + i, 5.0, 30.0}, 0.4, false});
        const Tally t = run("33 spheres", frame(dof, 192, 108), sc);
        CHECK(t.sure == 0, "sure %lld", t.sure);
    }
    {   // the order buffer's part for the bytes: behind the masks, on 256 bytes, read a word at a time; absent unless asked for
        for (size_t n_wt : {(size_t)1, (size_t)60, (size_t)32400}) {
            const TileOrderLayout off = tile_order_layout((n_wt + 3) / 4, n_wt), on = tile_order_layout((n_wt + 3) / 4, n_wt, true);
            CHECK(off.wsure.bytes == 0 && off.total == off.wmask.at + align256(off.wmask.bytes), "layout without sure tiles: total %zu", off.total);
            CHECK(on.wmask.at == off.wmask.at && on.wsure.at == off.total && on.wsure.at % 256 == 0 && on.wsure.bytes == n_wt &&
                      on.total == on.wsure.at + align256(n_wt),
                  "layout with sure tiles: wsure at %zu, %zu bytes, total %zu", on.wsure.at, on.wsure.bytes, on.total);
        }
    }
    {   // the frame plan: sure tiles wherever there are masks, unless the flag or the knob switches them off; the relay's form is not theirs
        FrameInputs in{};
        in.grid.width = 1920;
        in.grid.height = in.grid.rows = 1080;
        in.grid.spp = in.grid.spp_total = 64;
        in.grid.max_depth = 5;
        in.glass = true;
        in.nt = 256;
        in.prim_obj = -1;
        in.mem_total = 288000000000ull;
        in.n_cu = 256;
        in.waves_per_simd = 4;
        in.image = in.sph = in.pair = in.order_ok = in.aux_stream = in.all_spheres = true;
        in.n_objs = in.n_lds = 8;
        const FramePlan on = frame_plan(in, 0);
        CHECK(on.order.on && on.order.masks && on.order.sure, "default: masks %d sure %d", (int)on.order.masks, (int)on.order.sure);
        FrameInputs off = in;
        off.grid.flags = CGRT_GRID_NO_SURE_TILES;
        CHECK(frame_plan(off, 0).order.masks && !frame_plan(off, 0).order.sure, "CGRT_GRID_NO_SURE_TILES");
        CHECK(frame_plan(off, 0).relay.base.k == on.relay.base.k && frame_plan(off, 0).relay.order == on.relay.order, "the flag changed the relay");
        off.grid.flags = CGRT_GRID_NO_SPHERE_MASKS;
        CHECK(!frame_plan(off, 0).order.masks && !frame_plan(off, 0).order.sure, "CGRT_GRID_NO_SPHERE_MASKS implies it");
        off.grid.flags = CGRT_GRID_DIFFUSE_TILES;
        CHECK(frame_plan(off, 0).order.class3 == TileOrderPlan::SecondLaunch && frame_plan(off, 0).order.sure, "the second launch has them too");
        off = in;
        off.knobs.no_sure_tiles = true;
        CHECK(frame_plan(off, 0).order.masks && !frame_plan(off, 0).order.sure, "CGRT_NO_SURE_TILES");
        off = in;
        off.n_objs = off.n_lds = 33;
        CHECK(!frame_plan(off, 0).order.sure, "33 spheres");
        off = in;
        off.all_special = true;
        CHECK(!frame_plan(off, 0).order.sure, "no class-3 tile at all");
    }
    std::printf("ok: %d failed checks\n", failed);
    return failed ? 1 : 0;
}
