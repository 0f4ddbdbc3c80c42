// CPU test of the inside trips' rule (cgraytracing_amd/csrc/cgrt_inside_sphere.h), built with ASan + UBSan and -ffp-contract=off by
// tests/test_inside_sphere_host.py.
//
// SOUND (may never fail): for a set of scenes and every refracting sphere i of each, rays whose origin passes starts_inside -- on
// the shell r - kEps where the body's own origins lie, on the shell just inside r_in, at the centre, anywhere inside -- in
// directions drawn at random, aimed at the nearest point of every other sphere, tangential to sphere i and along the line through
// both centres: the device's sphere loop (sphere_len in its operation order, strict <) over ALL spheres and over inside_mask(i)
// alone must end on the same (len, id).
// REFUSALS: spheres that are not finite, a candidate too small for r_in, too many refracting spheres, too many spheres, an object
// that is no sphere.
// NOT VACUOUS: C2's glass sphere keeps nobody but itself; the body's loop, simulated for the wave tile over the glass sphere's
// centre on the 1920x1080 thin-lens frame, has every active lane inside in at least a third of its trips.
// argv[1], optional: a text file of spheres "x y z r refl transp" (tests/scenes.py many_spheres), run as one more scene.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cgrt_inside_sphere.h"
#include "cgrt_sphere_mask.h"

static int failed = 0;
#define CHECK(c, ...)                                                  \
    do {                                                               \
        if (!(c)) {                                                    \
            if (failed++ < 20) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                              \
    } while (0)

struct Sph {
    double c[3], r, refl, transp;
};
static const double kEpsRef = 1e-4, kInfDev = 1e10;  // cgrt_types.h: kEps, kInf
static std::vector<Sph> c2_scene() {  // tests/scenes.py scene_c2
    return {{{0.0, -10020, 0}, 10000, 0, 0}, {{10020, 0.0, 0}, 10000, 0, 0}, {{-10020, 0.0, 0}, 10000, 0, 0},
            {{0.0, 0.0, 10040}, 10000, 0, 0}, {{0.0, 10020, 0}, 10000, 0, 0}, {{-15.0, -20.0, 60}, 10, 0, 0},
            {{10.0, -13.0, 30}, 7, 0.8, 0}, {{-8.0, -13.0, 25}, 7, 0.8, 0.5}};
}
static const int kGlass = 7, kMirror = 6;

// sphere_len (cgrt_scene_walk.hpp) in the device's operation order; sqrt is correctly rounded here as sqrt_cr is there
static double sphere_len(const Sph &s, Vec3d o, Vec3d d) {
    const double r2 = s.r * s.r;  // what the scene stores (ObjRec::s0)
    const Vec3d l = vec3d(s.c[0] - o.x, s.c[1] - o.y, s.c[2] - o.z);
    const double tca = dot3d(l, d), l2 = dot3d(l, l);
    double len = kInfDev;
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
struct Hit {
    double t;
    int id;
};
static Hit loop_over(const std::vector<Sph> &sc, uint32_t mask, Vec3d o, Vec3d d) {  // intersect_scene's sphere loop over the mask's bits
    Hit h{kInfDev, -1};
    for (size_t i = 0; i < sc.size(); i++) {
        if (!((mask >> i) & 1u)) continue;
        const double len = sphere_len(sc[i], o, d);
        if (len < h.t) {
            h.t = len;
            h.id = (int)i;
        }
    }
    return h;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform01() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * 0x1p-53;
}
static Vec3d random_unit() {
    while (true) {
        const Vec3d v = vec3d(2 * uniform01() - 1, 2 * uniform01() - 1, 2 * uniform01() - 1);
        const double n2 = dot3d(v, v);
        if (n2 > 1e-3 && n2 < 1) return normalized3d(v);
    }
}
static std::vector<InsideBall> balls_of(const std::vector<Sph> &sc) {
    std::vector<InsideBall> b;
    for (const Sph &s : sc) b.push_back(InsideBall{{s.c[0], s.c[1], s.c[2]}, s.r * s.r});
    return b;
}
static InsideTrait trait_of(const std::vector<Sph> &sc, bool all_spheres = true) {
    const std::vector<InsideBall> b = balls_of(sc);
    std::vector<double> tr;
    for (const Sph &s : sc) tr.push_back(s.transp);
    return inside_trait(b.data(), tr.data(), (int)sc.size(), all_spheres);
}

// SOUND for one scene: every refracting sphere, whatever the trait's capacity.  Returns the rays compared.
static long long sound(const char *name, const std::vector<Sph> &sc) {
    const std::vector<InsideBall> b = balls_of(sc);
    const int n = (int)sc.size();
    const uint32_t full = inside_full_mask(n);
    long long rays = 0;
    for (int i = 0; i < n; i++) {
        if (sc[i].transp < kEpsRef) continue;
        const uint32_t mask = inside_mask(b.data(), n, i);
        CHECK((mask >> i) & 1u, "%s: sphere %d is not in its own mask %x", name, i, mask);
        CHECK((mask & ~full) == 0u, "%s: mask %x has bits beyond %d spheres", name, mask, n);
        const double rin2 = inside_rin2(b[i].r2), r_in = std::sqrt(rin2), r = sc[i].r;
        const Vec3d c = vec3d(sc[i].c[0], sc[i].c[1], sc[i].c[2]);
        std::vector<Vec3d> origins;
        for (int k = 0; k < 200; k++) {
            const Vec3d u = random_unit();
            origins.push_back(vec3d(c.x + u.x * (r - kEpsRef), c.y + u.y * (r - kEpsRef), c.z + u.z * (r - kEpsRef)));
            double f = r_in;  // the largest radius along u that still passes
            Vec3d p = vec3d(c.x + u.x * f, c.y + u.y * f, c.z + u.z * f);
            for (int it = 0; it < 64 && !starts_inside(p, c, rin2); it++) {
                f = f * (1 - 0x1p-50);
                p = vec3d(c.x + u.x * f, c.y + u.y * f, c.z + u.z * f);
            }
            origins.push_back(p);
            const double q = r_in * std::cbrt(uniform01()) * 0.999;
            origins.push_back(vec3d(c.x + u.x * q, c.y + u.y * q, c.z + u.z * q));
        }
        origins.push_back(c);
        long long passing = 0;
        for (const Vec3d &o : origins) {
            if (!starts_inside(o, c, rin2)) continue;  // (r - kEps of a sphere beyond 1e5: not an inside ray)
            passing++;
            std::vector<Vec3d> dirs;
            for (int k = 0; k < 16; k++) dirs.push_back(random_unit());
            const Vec3d radial = vec3d(o.x - c.x, o.y - c.y, o.z - c.z);
            for (int k = 0; k < 8; k++) {  // tangential to sphere i at o (any direction at the centre)
                const Vec3d v = random_unit();
                const double rr = dot3d(radial, radial), s = rr > 0 ? dot3d(v, radial) / rr : 0.0;
                dirs.push_back(normalized3d(vec3d(v.x - s * radial.x, v.y - s * radial.y, v.z - s * radial.z)));
            }
            for (int j = 0; j < n; j++) {
                if (j == i) continue;
                const Vec3d cj = vec3d(sc[j].c[0], sc[j].c[1], sc[j].c[2]);
                dirs.push_back(normalized3d(vec3d(cj.x - o.x, cj.y - o.y, cj.z - o.z)));  // at sphere j's nearest point
                const Vec3d axis = normalized3d(vec3d(cj.x - c.x, cj.y - c.y, cj.z - c.z));
                dirs.push_back(axis);
                dirs.push_back(vec3d(-axis.x, -axis.y, -axis.z));
                // grazing sphere j: at a point of its outline as seen from o, a little inside and a little outside
                const Vec3d v = random_unit();
                const double dist = std::sqrt(dot3d(vec3d(cj.x - o.x, cj.y - o.y, cj.z - o.z), vec3d(cj.x - o.x, cj.y - o.y, cj.z - o.z)));
                if (dist > sc[j].r) {
                    const Vec3d to = normalized3d(vec3d(cj.x - o.x, cj.y - o.y, cj.z - o.z));
                    const double s = dot3d(v, to);
                    const Vec3d side = normalized3d(vec3d(v.x - s * to.x, v.y - s * to.y, v.z - s * to.z));
                    for (double k : {1 - 1e-9, 1.0, 1 + 1e-9}) {
                        const double sn = sc[j].r / dist * k, cs = std::sqrt(std::fmax(0.0, 1 - sn * sn));
                        dirs.push_back(normalized3d(vec3d(to.x * cs + side.x * sn, to.y * cs + side.y * sn, to.z * cs + side.z * sn)));
                    }
                }
            }
            for (const Vec3d &d : dirs) {
                const Hit a = loop_over(sc, full, o, d), m = loop_over(sc, mask, o, d);
                rays++;
                CHECK(a.id == m.id && a.t == m.t, "%s: sphere %d mask %x: origin (%.17g, %.17g, %.17g) direction (%.17g, %.17g, %.17g): all spheres %d at %.17g, the mask %d at %.17g",
                      name, i, mask, o.x, o.y, o.z, d.x, d.y, d.z, a.id, a.t, m.id, m.t);
                CHECK(m.id >= 0 && m.t < 2 * r + 1e-6 * (1 + r), "%s: sphere %d: an inside ray leaves at %.17g, radius %g", name, i, m.t, r);
            }
        }
        CHECK(passing > 400 || r > 9e4, "%s: sphere %d: only %lld origins pass starts_inside", name, i, passing);
        std::printf("%-52s sphere %2d  mask %08x (%2d of %2d)  rin2 %.9g\n", name, i, mask, __builtin_popcount(mask), n, rin2);
    }
    return rays;
}

// The body's loop (trace_grid_body with shade_step's order) for one wave tile: one lane per pixel, a lane without a ray starts
// its next sample, every lane with a ray enters the sphere loop, mirror continues, glass continues with the reflection and
// pushes the refraction, pop when idle.  Counts the trips and those in which every lane that has a ray starts it inside sphere i.
struct Lane {
    bool have = false;
    Vec3d o, d;
    int depth_left = 0, s = 0;
    std::vector<Vec3d> stack_o, stack_d;
    std::vector<int> stack_depth;
};
static void simulate(const std::vector<Sph> &sc, const GridParams &g, int wx, int wy, int spp, int max_depth, int i, uint32_t mask, double rin2,
                     long long &trips, long long &inside_trips) {
    const Vec3d cam = vec3d(g.cam[0], g.cam[1], g.cam[2]), ci = vec3d(sc[i].c[0], sc[i].c[1], sc[i].c[2]);
    const uint32_t full = inside_full_mask((int)sc.size());
    std::vector<Lane> lanes(64);
    std::vector<Vec3d> pof(64);
    for (int l = 0; l < 64; l++) {
        const Vec3d pdir = pixel_dir(g, cam, wx * kWaveTileW + (l & 15), wy * kWaveTileH + (l >> 4));
        const double s = (g.focus_plane - cam.z) / pdir.z;
        pof[l] = vec3d(pdir.x * s + cam.x, pdir.y * s + cam.y, pdir.z * s + cam.z);
    }
    trips = inside_trips = 0;
    while (true) {
        bool any = false;
        for (int l = 0; l < 64; l++) {
            Lane &L = lanes[l];
            if (!L.have && L.s < spp) {
                double sx, sy;
                do {
                    sx = 2 * uniform01() - 1;
                    sy = 2 * uniform01() - 1;
                } while (!(sx * sx + sy * sy < 1));
                L.o = vec3d(cam.x + sx * g.lens_radius, cam.y + sy * g.lens_radius, cam.z);
                L.d = normalized3d(vec3d(pof[l].x - L.o.x, pof[l].y - L.o.y, pof[l].z - L.o.z));
                L.depth_left = max_depth;
                L.have = true;
                L.s++;
            }
            any = any || L.have;
        }
        if (!any) break;
        trips++;
        bool all_inside = true;
        for (const Lane &L : lanes)
            if (L.have && !starts_inside(L.o, ci, rin2)) all_inside = false;
        inside_trips += all_inside;
        for (Lane &L : lanes) {
            if (!L.have) continue;
            const Hit hit = loop_over(sc, full, L.o, L.d);
            if (all_inside) {
                const Hit m = loop_over(sc, mask, L.o, L.d);
                CHECK(m.id == hit.id && m.t == hit.t, "simulated body: an inside trip's ray ends on %d at %.17g, the mask's loop on %d at %.17g", hit.id, hit.t, m.id, m.t);
            }
            L.have = false;
            if (hit.id >= 0) {
                const Sph &ob = sc[hit.id];
                const bool diffuse = ob.refl < kEpsRef && ob.transp < kEpsRef;
                if (!diffuse && L.depth_left > 1) {
                    const Vec3d P = vec3d(L.o.x + L.d.x * hit.t, L.o.y + L.d.y * hit.t, L.o.z + L.d.z * hit.t);
                    const Vec3d n_old = normalized3d(vec3d(P.x - ob.c[0], P.y - ob.c[1], P.z - ob.c[2]));
                    Vec3d n = n_old;
                    bool into = true;
                    if (dot3d(n, L.d) > 0) {
                        n = vec3d(-n.x, -n.y, -n.z);
                        into = false;
                    }
                    const Vec3d out_o = vec3d(P.x + n.x * kEpsRef, P.y + n.y * kEpsRef, P.z + n.z * kEpsRef);
                    if (ob.transp < kEpsRef) {  // mirror
                        const double k = 2.0 * dot3d(n, L.d);
                        L.d = vec3d(L.d.x - n.x * k, L.d.y - n.y * k, L.d.z - n.z * k);
                        L.o = out_o;
                    } else {  // glass
                        const double nnt = into ? 1.0 / 1.33 : 1.33 / 1.0, ddn = dot3d(L.d, n), k = 2.0 * dot3d(n_old, L.d);
                        const Vec3d refl_dir = vec3d(L.d.x - n_old.x * k, L.d.y - n_old.y * k, L.d.z - n_old.z * k);
                        const double cos2t = 1 - nnt * nnt * (1 - ddn * ddn);
                        if (!(cos2t < 0)) {
                            const double f = (into ? 1 : -1) * (ddn * nnt + std::sqrt(cos2t));
                            L.stack_o.push_back(vec3d(P.x - n.x * kEpsRef, P.y - n.y * kEpsRef, P.z - n.z * kEpsRef));
                            L.stack_d.push_back(normalized3d(vec3d(L.d.x * nnt - n_old.x * f, L.d.y * nnt - n_old.y * f, L.d.z * nnt - n_old.z * f)));
                            L.stack_depth.push_back(L.depth_left - 1);
                        }
                        L.o = out_o;
                        L.d = refl_dir;
                    }
                    L.depth_left--;
                    L.have = true;
                }
            }
            if (!L.have && !L.stack_o.empty()) {
                L.o = L.stack_o.back();
                L.d = L.stack_d.back();
                L.depth_left = L.stack_depth.back();
                L.stack_o.pop_back();
                L.stack_d.pop_back();
                L.stack_depth.pop_back();
                L.have = true;
            }
        }
    }
}

int main(int argc, char **argv) {
    const std::vector<Sph> c2 = c2_scene();
    long long rays = 0;

    // ---- not vacuous: C2's mask ----
    {
        const InsideTrait t = trait_of(c2);
        CHECK(t.n == 1 && t.idx[0] == kGlass, "C2: %d candidates, the first sphere %d", t.n, t.idx[0]);
        CHECK(t.mask[0] == (1u << kGlass), "C2: the glass sphere's mask is %x", t.mask[0]);
        CHECK(inside_pays(t, 0, (int)c2.size()), "C2: the guarded loop does not pay");
        const double r_in = 7 * (1 - 1e-9) - 1e-6;
        CHECK(t.rin2[0] == r_in * r_in, "C2: rin2 %.17g", t.rin2[0]);
        for (size_t j = 0; j < c2.size(); j++) {
            if ((int)j == kGlass) continue;
            const double dx = c2[j].c[0] - c2[kGlass].c[0], dy = c2[j].c[1] - c2[kGlass].c[1], dz = c2[j].c[2] - c2[kGlass].c[2];
            const double D = std::sqrt(dx * dx + dy * dy + dz * dz);
            std::printf("C2: glass to sphere %zu: gap %.6g, margin %.3g\n", j, D - 7 - c2[j].r, inside_margin(D, 7, c2[j].r));
        }
    }
    // ---- sound ----
    rays += sound("c2", c2);
    {   // the glass sphere lowered until it touches the floor sphere, then until it overlaps it
        const double y_touch = -10020 + std::sqrt(10007.0 * 10007.0 - 64 - 625);
        for (double extra : {0.0, 1e-4, 0.5}) {
            std::vector<Sph> sc = c2;
            sc[kGlass].c[1] = y_touch - extra;
            rays += sound(extra == 0 ? "c2, glass touching the floor" : "c2, glass overlapping the floor", sc);
            CHECK(trait_of(sc).mask[0] == ((1u << kGlass) | 1u), "glass on the floor (%g): mask %x", extra, trait_of(sc).mask[0]);
        }
    }
    for (double gap : {1e-3, 0.1}) {  // beside the right wall: kept at 1e-3, left out at 0.1
        std::vector<Sph> sc = c2;
        sc[kGlass].c[0] = 10020 - std::sqrt((10007 + gap) * (10007 + gap) - 25 - 625);
        sc[kGlass].c[1] = -5;
        rays += sound(gap < 0.01 ? "c2, glass 1e-3 from the right wall" : "c2, glass 0.1 from the right wall", sc);
        const uint32_t m = trait_of(sc).mask[0];
        CHECK(((m >> 1) & 1u) == (gap < 0.01 ? 1u : 0u), "glass %g from the right wall: mask %x", gap, m);
    }
    {   // overlapping the mirror
        std::vector<Sph> sc = c2;
        sc[kGlass].c[0] = 0;
        sc[kGlass].c[2] = 28;
        rays += sound("c2, glass overlapping the mirror", sc);
        CHECK(trait_of(sc).mask[0] == ((1u << kGlass) | (1u << kMirror)), "glass over the mirror: mask %x", trait_of(sc).mask[0]);
    }
    {   // a small diffuse sphere nested in the glass sphere, concentric and off-centre
        for (double off : {0.0, 3.0}) {
            std::vector<Sph> sc = c2;
            sc.push_back({{-8.0 + off, -13.0, 25}, 2, 0, 0});
            rays += sound("c2 + a diffuse sphere inside the glass sphere", sc);
            CHECK(trait_of(sc).mask[0] == ((1u << kGlass) | (1u << 8)), "nested diffuse sphere: mask %x", trait_of(sc).mask[0]);
        }
    }
    {   // the glass sphere nested in a larger glass sphere: two refracting spheres, each in the other's mask
        std::vector<Sph> sc = c2;
        sc.insert(sc.begin() + 5, {{-8.0, -12.0, 25}, 12, 0.8, 0.5});
        rays += sound("c2 + a glass sphere around the glass sphere", sc);
        const std::vector<InsideBall> b = balls_of(sc);
        CHECK((inside_mask(b.data(), 9, 5) >> 8) & 1u, "the outer sphere's mask leaves the inner one out");
        CHECK((inside_mask(b.data(), 9, 8) >> 5) & 1u, "the inner sphere's mask leaves the outer one out");
        CHECK(trait_of(sc).n == (kInsideMax >= 2 ? 2 : 0), "two nested glass spheres: %d candidates", trait_of(sc).n);
    }
    {   // two disjoint glass spheres
        std::vector<Sph> sc = c2;
        sc[kMirror].transp = 0.5;
        rays += sound("c2 with two glass spheres", sc);
        CHECK(trait_of(sc).n == (kInsideMax >= 2 ? 2 : 0), "two glass spheres: %d candidates", trait_of(sc).n);
    }
    {   // kInsideMax + 1 glass spheres: the feature is off
        std::vector<Sph> sc = c2;
        for (int k = 0; k < kInsideMax; k++) sc.push_back({{-12.0 + 3 * k, 5.0, 30.0}, 1.0, 0.8, 0.5});
        rays += sound("c2 + kInsideMax glass spheres", sc);
        const InsideTrait t = trait_of(sc);
        CHECK(t.n == 0, "kInsideMax + 1 glass spheres: %d candidates", t.n);
    }
    if (argc > 1) {
        std::vector<Sph> sc;
        if (FILE *f = std::fopen(argv[1], "r")) {
            Sph s;
            while (std::fscanf(f, "%lf %lf %lf %lf %lf %lf", &s.c[0], &s.c[1], &s.c[2], &s.r, &s.refl, &s.transp) == 6) sc.push_back(s);
            std::fclose(f);
        }
        CHECK(sc.size() == 32, "scene file: %zu spheres", sc.size());
        int glass = 0;
        for (const Sph &s : sc) glass += !(s.transp < kEpsRef);
        CHECK(glass > 0, "scene file: no refracting sphere");
        rays += sound("scene file", sc);
    }
    std::printf("sound: %lld rays compared\n", rays);
    CHECK(rays > 500000, "only %lld rays", rays);

    // ---- refusals ----
    {
        const uint32_t full = inside_full_mask(8);
        for (int bad : {0, 5, kGlass})
            for (int what = 0; what < 4; what++) {
                std::vector<Sph> sc = c2;
                if (what == 0) sc[bad].c[1] = NAN;
                if (what == 1) sc[bad].c[2] = INFINITY;
                if (what == 2) sc[bad].r = INFINITY;
                if (what == 3) sc[bad].c[0] = 1e160;
                const InsideTrait t = trait_of(sc);
                CHECK(t.n == 1 && t.mask[0] == full && t.rin2[0] == 0 && !inside_pays(t, 0, 8), "sphere %d not finite (%d): mask %x rin2 %g", bad, what, t.mask[0], t.rin2[0]);
            }
        for (double r : {0.0, 1e-7, 9.9e-7}) {  // the rounding bound: no positive r_in
            std::vector<Sph> sc = c2;
            sc[kGlass].r = r;
            const InsideTrait t = trait_of(sc);
            CHECK(t.n == 1 && t.mask[0] == full && t.rin2[0] == 0 && !inside_pays(t, 0, 8), "glass radius %g: mask %x rin2 %g", r, t.mask[0], t.rin2[0]);
            CHECK(!starts_inside(vec3d(-8.0, -13.0, 25), vec3d(-8.0, -13.0, 25), t.rin2[0]), "glass radius %g: its centre counts as inside", r);
        }
        {   // a full mask never pays; a mask of 7 of 8 does not either, one of 6 of 8 does
            InsideTrait t{};
            t.n = 1;
            t.rin2[0] = 1;
            t.mask[0] = 0x7f;
            CHECK(!inside_pays(t, 0, 8), "7 of 8 pays");
            t.mask[0] = 0x3f;
            CHECK(inside_pays(t, 0, 8), "6 of 8 does not pay");
        }
        std::vector<Sph> many = c2;
        for (int k = 0; many.size() < 33; k++) many.push_back({{-12.0 + k, 5.0, 30.0}, 0.4, 0, 0});
        CHECK(trait_of(many).n == 0, "33 spheres: %d candidates", trait_of(many).n);
        CHECK(trait_of(c2, false).n == 0, "an object that is no sphere: %d candidates", trait_of(c2, false).n);
        CHECK(trait_of(std::vector<Sph>(c2.begin(), c2.begin() + 6)).n == 0, "no glass: candidates");
        CHECK(trait_of(std::vector<Sph>()).n == 0, "empty scene: candidates");
        // starts_inside at the bound itself: strict
        const double rin2 = inside_rin2(49.0);
        CHECK(!starts_inside(vec3d(std::sqrt(rin2) * (1 + 1e-15), 0, 0), vec3d(0, 0, 0), rin2), "an origin beyond r_in passes");
        CHECK(starts_inside(vec3d(7 - kEpsRef, 0, 0), vec3d(0, 0, 0), rin2), "the body's own origin, kEps inside, fails");
        CHECK(!starts_inside(vec3d(7 + kEpsRef, 0, 0), vec3d(0, 0, 0), rin2), "an origin kEps outside passes");
        CHECK(!starts_inside(vec3d(NAN, 0, 0), vec3d(0, 0, 0), rin2), "a NaN origin passes");
    }

    // ---- not vacuous: the body's loop over the glass sphere's centre ----
    {
        cgrt_camera cam{};
        cam.cam[2] = -10;
        cam.half_width = 10.0;
        cam.focus_plane = 20.0;
        cam.lens_radius = 1.5;
        cgrt_grid gr{};
        gr.width = 1920; gr.height = gr.rows = 1080;
        gr.stripe_nranks = 1;
        gr.spp = gr.spp_total = 16; gr.max_depth = 5;
        const GridParams g = grid_params(&cam, &gr);
        // the pixel whose pinhole ray passes through the glass sphere's centre
        const double s = (0 - cam.cam[2]) / (c2[kGlass].c[2] - cam.cam[2]);
        const double px = c2[kGlass].c[0] * s, py = c2[kGlass].c[1] * s;
        const int w = (int)std::floor((px / g.half_width + 1) / 2 * g.W), h = (int)std::floor((py / (g.half_width * g.H / g.W) + 1) / 2 * g.H);
        const InsideTrait t = trait_of(c2);
        long long trips = 0, inside = 0;
        simulate(c2, g, w / kWaveTileW, h / kWaveTileH, 16, 5, kGlass, t.mask[0], t.rin2[0], trips, inside);
        std::printf("simulated body, wave tile (%d, %d) over the glass sphere's centre, 16 samples: %lld trips, %lld with every active lane inside (%.3f)\n",
                    w / kWaveTileW, h / kWaveTileH, trips, inside, trips ? (double)inside / (double)trips : 0.0);
        CHECK(trips >= 16 * 5 && 3 * inside >= trips, "inside trips %lld of %lld", inside, trips);
    }
    std::printf("ok: %d failed checks\n", failed);
    return failed ? 1 : 0;
}
