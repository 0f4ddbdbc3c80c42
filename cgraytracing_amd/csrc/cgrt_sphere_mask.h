// Which spheres a wave tile's primary rays can meet, in plain C++ (no HIP): the cone around a wave tile's directions and its
// test (tile_order_kernel's and classify_kernel's), and the candidate test of the terminal-diffuse body's sphere masks.
// tile_order_kernel (cgrt_eye.hpp) runs it on the device, one thread per wave tile; tests/native/sphere_mask.cpp runs the same
// functions on the CPU against every ray of a frame.
//
// sphere_surely_missed(g, tile, c, r2) == true promises: sphere_len (cgrt_scene_walk.hpp) returns kInf for EVERY primary ray of
// the wave tile -- any pixel of it, any lens point -- so the sphere loop of a class-3 wave may pass the sphere over and keep its
// bits.  Two arms, either suffices; everything doubtful is a candidate.
//
// BEHIND.  sphere_len's first test, `tca < 0 && l2 > r2` with l = c - o, tca = l . d, l2 = l . l, holds for a ray when the
// sphere's centre lies behind its origin and the origin outside the sphere.  The tile's rays are bounded by two boxes:
//   * origins: o = cam + (sx, sy, 0) * lens_radius with sx^2 + sy^2 < 1, so o.x, o.y lie within lens_radius of cam.x, cam.y and
//     o.z == cam.z exactly (the box is the point cam for a pinhole);
//   * directions: d = normalized(v), v = pof - o (thin lens; pof = the pixel's point on the focal plane) or v = p - cam (pinhole;
//     p = the pixel's point on the image plane z = 0).  pof and p are affine in the pixel's (w, h), so over the tile's pixels they
//     lie in the rectangle spanned by the four corner pixels one pixel beyond the tile (the margin wave_tile_cone takes); v's
//     components then lie in intervals, and d_k = v_k / |v| rises with v_k and, for a given v_k, moves towards 0 as the other two
//     components grow: the ends of d_k's interval come from the ends of v_k's with the other components at their smallest or
//     largest magnitude, by the sign of v_k.
// tca <= sum_k max(l_k d_k) over the intervals' ends, l2 >= sum_k min(l_k^2).  The sphere is surely missed when
//     tca_hi < -(1e-9 * T + 1e-6)   and   l2_lo > r2 + 1e-9 * (r2 + l2_lo) + 1e-6,      T = sum_k max|l_k| max|d_k|.
// Slack: the device forms o (2 roundings), v and d (3 products, 2 sums, one root, one reciprocal, 3 products: each component
// within 8 ulp), l (1), tca and l2 (3 products, 2 sums each), and this header forms the boxes in about as many operations; every
// one of them is correctly rounded, relative error <= 2^-53 of a term whose magnitude T (resp. l2) bounds.  All of it stays below
// 64 x 2^-53 x T < 1e-14 T -- five orders of magnitude inside the relative term; the absolute term covers T, l2 near zero.  They
// are cone_clear_of's margins.
//
// CLEAR CONE.  cone_clear_of below: no primary ray of the tile touches the sphere grown by its margins; such a ray has
// d2 > r2 or the sphere behind it, so sphere_len returns kInf.
//
// A candidate in any doubtful case: a non-finite value anywhere, f = focus_plane - cam.z <= 0 with a lens, an origin box that
// touches the sphere or lies in it.
#ifndef CGRT_SPHERE_MASK_H
#define CGRT_SPHERE_MASK_H
#include <cmath>

#include "cgrt_frame.h"
#include "cgrt_rng.hpp"  // CGRT_HD

struct Vec3d {
    double x, y, z;
};
CGRT_HD Vec3d vec3d(double x, double y, double z) { return Vec3d{x, y, z}; }
CGRT_HD double dot3d(Vec3d a, Vec3d b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// vec3.h:36-44 in IEEE double (what the device's normalized() returns, bit for bit: tests/test_gpu_device_math.py)
CGRT_HD Vec3d normalized3d(Vec3d a) {
    const double len = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    if (len > 0) {
        const double r = 1 / len;
        a.x *= r;
        a.y *= r;
        a.z *= r;
    }
    return a;
}

// local row -> global row (cgrt.h: block-cyclic stripes)
CGRT_HD int global_row(const GridParams &g, int j) {
    if (g.stripe_nranks > 1) {
        int S = g.stripe_rows;
        return ((j / S) * g.stripe_nranks + g.stripe_rank) * S + (j % S);
    }
    return g.row_offset + j;
}

// the image-plane point of pixel (w, local row j), main.cpp:188-189
CGRT_HD Vec3d pixel_point(const GridParams &g, int w, int j) {
    const int h = global_row(g, j);
    const double px = (2.0 * ((double)w / g.W) - 1) * g.half_width;
    const double py = (2.0 * ((double)h / g.H) - 1) * g.half_width * g.H / g.W;
    return vec3d(px, py, 0);
}
// its pinhole direction
CGRT_HD Vec3d pixel_dir(const GridParams &g, Vec3d cam, int w, int j) {
    const Vec3d p = pixel_point(g, w, j);
    return normalized3d(vec3d(p.x - cam.x, p.y - cam.y, p.z - cam.z));
}

struct TileCone {  // the cone around a wave tile's pinhole directions: axis dc, half-angle alpha
    Vec3d cam, dc;
    double alpha;
};
CGRT_HD TileCone wave_tile_cone(const GridParams &g, int wx, int wy) {
    TileCone tc;
    tc.cam = vec3d(g.cam[0], g.cam[1], g.cam[2]);
    const int w0 = wx * kWaveTileW, j0 = wy * kWaveTileH;
    // corners one pixel beyond the tile on every side (pixels are sampled at their lower-left corner; the margin also covers
    // the curvature of the angle function along the edges)
    const Vec3d c00 = pixel_dir(g, tc.cam, w0 - 1, j0 - 1), c10 = pixel_dir(g, tc.cam, w0 + kWaveTileW, j0 - 1),
                c01 = pixel_dir(g, tc.cam, w0 - 1, j0 + kWaveTileH), c11 = pixel_dir(g, tc.cam, w0 + kWaveTileW, j0 + kWaveTileH);
    tc.dc = normalized3d(vec3d((c00.x + c10.x) + (c01.x + c11.x), (c00.y + c10.y) + (c01.y + c11.y), (c00.z + c10.z) + (c01.z + c11.z)));
    double cmin = fmin(fmin(dot3d(tc.dc, c00), dot3d(tc.dc, c10)), fmin(dot3d(tc.dc, c01), dot3d(tc.dc, c11)));
    cmin = fmin(1.0, fmax(-1.0, cmin));
    tc.alpha = 1.5 * acos(cmin) + 1e-6;
    return tc;
}
// the stripe mapping keeps a wave tile's four rows adjacent (stripes are multiples of 8 rows), so the corners bound it
// false: the sphere (c, r) may be touched by a primary ray of the tile
CGRT_HD bool cone_clear_of(const GridParams &g, const TileCone &tc, Vec3d c, double r) {
    r = r * (1 + 1e-9) + 1e-6;
    if (g.lens_radius > 0) {
        const double f = g.focus_plane - tc.cam.z;
        const double s_lo = (c.z - r - tc.cam.z) / f, s_hi = (c.z + r - tc.cam.z) / f;
        if (!(f > 0) || !(s_lo > 0)) return false;  // object reaches the lens plane or behind it
        // a camera at z >= 0 looks at the image plane z = 0 backwards: its lens rays, which leave through the focal plane in front,
        // are nowhere near the cone of its pinhole directions
        if (!(tc.cam.z < 0)) return false;
        r += g.lens_radius * fmax(fabs(1 - s_lo), fabs(1 - s_hi));
    }
    const Vec3d v = vec3d(c.x - tc.cam.x, c.y - tc.cam.y, c.z - tc.cam.z);
    const double dist = sqrt(dot3d(v, v));
    if (!(dist > r)) return false;
    double ct = dot3d(tc.dc, v) / dist;
    ct = fmin(1.0, fmax(-1.0, ct));
    return !(acos(ct) <= tc.alpha + asin(r / dist) + 1e-6);
}

// ---- the candidate test ----
struct Interval {
    double lo, hi;
};
CGRT_HD double sq_min(Interval a) { return (a.lo <= 0 && a.hi >= 0) ? 0.0 : fmin(a.lo * a.lo, a.hi * a.hi); }
CGRT_HD double sq_max(Interval a) { return fmax(a.lo * a.lo, a.hi * a.hi); }
// the interval of v_k / |v| for v_k in k and the other two components in a, b
CGRT_HD Interval unit_component(Interval k, Interval a, Interval b) {
    const double near = sq_min(a) + sq_min(b), far = sq_max(a) + sq_max(b);
    Interval d;
    d.lo = k.lo / sqrt(k.lo * k.lo + (k.lo < 0 ? near : far));
    d.hi = k.hi / sqrt(k.hi * k.hi + (k.hi < 0 ? far : near));
    return d;
}
struct TileRays {   // the boxes around a wave tile's primary rays
    Interval o[3];  // origins
    Interval d[3];  // directions
    Interval q[3];  // targets: the focal-plane points (lens) or image-plane points (pinhole) every ray of the tile passes through
    bool ok;        // false: no bound (f <= 0 with a lens, something not finite): every sphere is a candidate
    TileCone cone;
};
CGRT_HD TileRays wave_tile_rays(const GridParams &g, int wx, int wy) {
    TileRays t;
    t.cone = wave_tile_cone(g, wx, wy);
    const Vec3d cam = t.cone.cam;
    const bool lens = g.lens_radius > 0;
    const double R = lens ? g.lens_radius : 0.0;
    t.o[0] = Interval{cam.x - R, cam.x + R};
    t.o[1] = Interval{cam.y - R, cam.y + R};
    t.o[2] = Interval{cam.z, cam.z};
    const int w0 = wx * kWaveTileW, j0 = wy * kWaveTileH;
    // the target rectangle: the four corner pixels' image-plane points (pinhole) or focal-plane points (lens)
    Interval q[3] = {{INFINITY, -INFINITY}, {INFINITY, -INFINITY}, {INFINITY, -INFINITY}};
    const double f = g.focus_plane - cam.z;
    t.ok = !lens || f > 0;
    for (int c = 0; c < 4; c++) {
        const int w = (c & 1) ? w0 + kWaveTileW : w0 - 1, j = (c & 2) ? j0 + kWaveTileH : j0 - 1;
        Vec3d p = pixel_point(g, w, j);
        if (lens) {  // main.cpp:198: pof = pdir * ((focus_plane - cam.z) / pdir.z) + cam
            const Vec3d pd = normalized3d(vec3d(p.x - cam.x, p.y - cam.y, p.z - cam.z));
            const double s = f / pd.z;
            p = vec3d(pd.x * s + cam.x, pd.y * s + cam.y, pd.z * s + cam.z);
        }
        q[0].lo = fmin(q[0].lo, p.x); q[0].hi = fmax(q[0].hi, p.x);
        q[1].lo = fmin(q[1].lo, p.y); q[1].hi = fmax(q[1].hi, p.y);
        q[2].lo = fmin(q[2].lo, p.z); q[2].hi = fmax(q[2].hi, p.z);
    }
    Interval v[3];
    for (int k = 0; k < 3; k++) t.q[k] = q[k];
    for (int k = 0; k < 3; k++) v[k] = Interval{q[k].lo - t.o[k].hi, q[k].hi - t.o[k].lo};
    t.d[0] = unit_component(v[0], v[1], v[2]);
    t.d[1] = unit_component(v[1], v[0], v[2]);
    t.d[2] = unit_component(v[2], v[0], v[1]);
    for (int k = 0; k < 3; k++)  // (a NaN fails every comparison)
        if (!(t.d[k].lo >= -1 && t.d[k].hi <= 1 && t.d[k].lo <= t.d[k].hi && fabs(t.o[k].lo) < 1e300 && fabs(t.o[k].hi) < 1e300)) t.ok = false;
    return t;
}
// the BEHIND arm (header comment): centre c, squared radius r2
CGRT_HD bool sphere_behind_tile(const TileRays &t, Vec3d c, double r2) {
    if (!t.ok) return false;
    const double cc[3] = {c.x, c.y, c.z};
    double tca_hi = 0, l2_lo = 0, T = 0;
    for (int k = 0; k < 3; k++) {
        const Interval l{cc[k] - t.o[k].hi, cc[k] - t.o[k].lo};
        tca_hi += fmax(fmax(l.lo * t.d[k].lo, l.lo * t.d[k].hi), fmax(l.hi * t.d[k].lo, l.hi * t.d[k].hi));
        l2_lo += sq_min(l);
        T += fmax(fabs(l.lo), fabs(l.hi)) * fmax(fabs(t.d[k].lo), fabs(t.d[k].hi));
    }
    if (!(T < 1e300 && l2_lo < 1e300 && r2 >= 0 && r2 < 1e300)) return false;
    return tca_hi < -(1e-9 * T + 1e-6) && l2_lo > r2 + 1e-9 * (r2 + l2_lo) + 1e-6;
}
// true: sphere_len returns kInf for every primary ray of the wave tile
CGRT_HD bool sphere_surely_missed(const GridParams &g, const TileRays &t, Vec3d c, double r2) {
    return sphere_behind_tile(t, c, r2) || cone_clear_of(g, t.cone, c, sqrt(r2));
}

#endif
