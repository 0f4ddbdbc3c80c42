// The sphere every primary ray of a wave tile hits first, proven from the tile's boxes, in plain C++ (no HIP).  sure_first_kernel
// (cgrt_eye.hpp) runs it on the device, one thread per wave tile of a class-3 tile; tests/native/sure_first.cpp runs the same
// function on the CPU against every ray of a set of frames.
//
// sphere_sure_first(g, tile, n, get, mask) == i >= 0 promises: for EVERY primary ray of the wave tile -- any pixel of it, any
// lens point -- the device's sphere loop (sphere_len over all n spheres, strict <, cgrt_scene_walk.hpp) ends with id == i.  A
// terminal-diffuse ray contributes nothing but that sphere's colour, so a wave whose tile has a winner adds the colour once per
// sample and traces nothing (trace_grid_body<..., DIFF>).  -1: no promise.
//
// The rays.  A primary ray is p(u) = a + u (b - a), u >= 0: a its origin, in the rectangle A = TileRays::o (the lens, z = cam.z;
// the point cam for a pinhole), b the point it aims at, in the box B = TileRays::q (the focal-plane points of the tile's
// corner pixels one pixel beyond it; the image-plane points for a pinhole), a and b independent.  At a fixed u the ray's point
// lies in the box P(u) = (1 - u) A + u B (interval arithmetic: 1 - u < 0 flips A beyond the focal plane).
//
// The candidate i is the first sphere, among the tile's mask, that the ray from A's centre to B's centre meets, at u_c (the
// conjugate root C / (B + sqrt(B^2 - A C)), which does not cancel for a wall of radius 1e4).  It is only a guess; the proof is:
//  (o) A lies outside ball i (box-to-centre distance), like every other ball by (b);
//  (a) for some u_hi on a short ladder above u_c, P(u_hi) lies inside ball i (its farthest corner does).  A ray that is outside
//      ball i at u = 0 and inside at u_hi has entered it at some u_i < u_hi;
//  (b) for every OTHER sphere j of the scene -- not only the mask's -- a plane separates ball j from the convex hull of A and
//      P(u_hi): n . (v - c_j) > r_j for the hull's vertices v (the boxes' support function in direction n).  A ray's point at
//      u <= u_hi is a convex combination of a and p(u_hi), both in the hull, so the ray does not touch ball j before u_hi.  Two
//      directions are tried: from c_j to the hull's midpoint (tight for the walls, nearly planes at this scale), and that vector
//      without its component along the beam's axis (tight for a small sphere beside a long beam).
// Then every ray meets i first.  An exact duplicate of the winner fails (b): P(u_hi) lies inside it.
//
// Margins and the device's arithmetic.  Radii are taken as cone_clear_of takes them: delta = r * 1e-9 + 1e-6 outward for (o) and
// (b), inward for (a).  Along a ray, with t the distance from its origin: the point at t_hi lies delta_i deep in ball i, so i is
// entered at t_i <= t_hi - delta_i / 2 (thc - sqrt(thc^2 - r delta) >= delta / 2 for thc <= r); a ray that meets j at all meets
// it at t_j >= t_hi + delta_j (its points up to t_hi are farther than r_j + delta_j from c_j).  sphere_len forms l = c - o,
// tca = l . d, l2 = l . l, d2 = l2 - tca^2, thc = sqrt_cr(r2 - d2), len = tca - thc from a direction d that is within 8 ulp a
// component (cgrt_sphere_mask.h): with L = |l|, d2 is off by at most E = 8e-15 L^2 (5 roundings of L^2-sized terms and
// 2 tca err(tca), err(tca) <= 2.4e-15 L), and len by err(tca) + E / (2 thc).  For the winner r2 - d2 >= r delta, for a loser that is
// hit (tca - t_hi)^2 >= thc^2 + 2 r delta, so the computed lens keep the order whenever E <= r delta / 2 -- which is required
// of EVERY sphere (kSureRound below) and holds with five orders to spare in a room of radius-1e4 walls (E = 8e-7, r delta / 2 =
// 5e-2; len itself is good to 1e-11 there, thc being thousands).  The same bound keeps the winner's two tests in sphere_len true
// (d2 <= r2 by r delta - E; tca > 0) and a loser that the ray misses by delta missed (d2 - r2 >= 2 r delta - E).  This header's own
// roundings -- the boxes, P(u), the dot products: a few ulp of coordinates of the size of L -- vanish in the same margins.
//
// Refused (-1): !tile.ok, more than 32 spheres, an empty mask, a lens with cam.z >= 0 (order_all_special's case: the lens rays are
// nowhere near the pinhole cone), targets in the lens plane, a centre ray that starts inside a candidate or meets none, an
// origin box that touches the winner (or any other ball: (b)), anything not finite, a sphere that fails the rounding bound.
#ifndef CGRT_SURE_FIRST_H
#define CGRT_SURE_FIRST_H
#include "cgrt_sphere_mask.h"

static constexpr int kSureNone = 0xff;  // wsure[wave tile]: no winner
static constexpr double kSureRound = 8e-15;

struct SureSphere {
    Vec3d c;
    double r2;
};
struct SureBox {
    Interval k[3];
};
CGRT_HD SureBox sure_beam_at(const TileRays &t, double u) {  // P(u), u >= 0
    const double w = 1 - u;
    SureBox b;
    for (int k = 0; k < 3; k++) {
        const double a0 = w * t.o[k].lo, a1 = w * t.o[k].hi;
        b.k[k] = Interval{fmin(a0, a1) + u * t.q[k].lo, fmax(a0, a1) + u * t.q[k].hi};
    }
    return b;
}
// the smallest n . (v - c) over the box
CGRT_HD double sure_support(const SureBox &b, Vec3d n, Vec3d c) {
    const double nn[3] = {n.x, n.y, n.z}, cc[3] = {c.x, c.y, c.z};
    double s = 0;
    for (int k = 0; k < 3; k++) s += fmin(nn[k] * (b.k[k].lo - cc[k]), nn[k] * (b.k[k].hi - cc[k]));
    return s;
}
CGRT_HD Vec3d sure_mid(const SureBox &b) {
    return vec3d(0.5 * (b.k[0].lo + b.k[0].hi), 0.5 * (b.k[1].lo + b.k[1].hi), 0.5 * (b.k[2].lo + b.k[2].hi));
}
// (b): a plane separates the ball (c, r grown by its margin) from the hull of the boxes A and P
CGRT_HD bool sure_hull_clear_of(const SureBox &A, const SureBox &P, Vec3d c, double r) {
    const double ro = r * (1 + 1e-9) + 1e-6;
    const Vec3d ma = sure_mid(A), mp = sure_mid(P);
    const Vec3d m = vec3d(0.5 * (ma.x + mp.x) - c.x, 0.5 * (ma.y + mp.y) - c.y, 0.5 * (ma.z + mp.z) - c.z);
    const Vec3d ax = vec3d(mp.x - ma.x, mp.y - ma.y, mp.z - ma.z);
    const double aa = dot3d(ax, ax);
    for (int pass = 0; pass < 2; pass++) {
        Vec3d n = m;
        if (pass == 1) {
            if (!(aa > 0)) break;
            const double s = dot3d(m, ax) / aa;
            n = vec3d(m.x - s * ax.x, m.y - s * ax.y, m.z - s * ax.z);
        }
        const double len = sqrt(dot3d(n, n));
        if (!(len > 1e-12 && len < 1e300)) continue;
        n = vec3d(n.x / len, n.y / len, n.z / len);
        if (sure_support(A, n, c) > ro && sure_support(P, n, c) > ro) return true;
    }
    return false;
}

// get(i) -> SureSphere: sphere i of the scene's n, in the object list's order
template <class Get> CGRT_HD int sphere_sure_first(const GridParams &g, const TileRays &t, int n, Get get, uint32_t mask) {
    if (!t.ok || n < 1 || n > 32 || mask == 0u) return -1;
    if (n < 32) mask &= (1u << n) - 1u;
    const bool lens = g.lens_radius > 0;
    if (lens && !(g.cam[2] < 0)) return -1;
    SureBox A;
    for (int k = 0; k < 3; k++) {
        A.k[k] = t.o[k];
        if (!(fabs(t.q[k].lo) < 1e300 && fabs(t.q[k].hi) < 1e300 && t.q[k].lo <= t.q[k].hi)) return -1;
    }
    // the targets lie strictly on one side of the lens plane
    if (!((t.q[2].lo - t.o[2].hi) * (t.q[2].hi - t.o[2].lo) > 0 && fabs(t.q[2].lo - t.o[2].lo) > 1e-9)) return -1;
    // the rounding bound, for every sphere: E = kSureRound L^2 <= r delta / 2, L the largest |c - o| over the origin box
    for (int j = 0; j < n; j++) {
        const SureSphere s = get(j);
        const double cc[3] = {s.c.x, s.c.y, s.c.z};
        double L2 = 0;
        for (int k = 0; k < 3; k++) L2 += sq_max(Interval{cc[k] - A.k[k].hi, cc[k] - A.k[k].lo});
        const double r = sqrt(s.r2);
        if (!(s.r2 > 0 && s.r2 < 1e300 && L2 < 1e300 && kSureRound * L2 <= 0.5 * r * (r * 1e-9 + 1e-6))) return -1;
    }
    // the candidate: the centre ray's first hit among the mask's spheres
    const Vec3d a0 = sure_mid(A), b0 = vec3d(0.5 * (t.q[0].lo + t.q[0].hi), 0.5 * (t.q[1].lo + t.q[1].hi), 0.5 * (t.q[2].lo + t.q[2].hi));
    const Vec3d v = vec3d(b0.x - a0.x, b0.y - a0.y, b0.z - a0.z);
    const double qa = dot3d(v, v);
    if (!(qa > 0 && qa < 1e300)) return -1;
    int win = -1;
    double u_c = INFINITY;
    for (uint32_t m = mask; m != 0u; m &= m - 1u) {
        const int i = __builtin_ctz(m);
        const SureSphere s = get(i);
        const Vec3d l = vec3d(s.c.x - a0.x, s.c.y - a0.y, s.c.z - a0.z);
        const double qb = dot3d(v, l), qc = dot3d(l, l) - s.r2;
        if (!(qc > 0)) return -1;  // the centre of the lens inside a candidate, or on it
        const double disc = qb * qb - qa * qc;
        if (!(qb > 0 && disc >= 0)) continue;
        const double u = qc / (qb + sqrt(disc));
        if (u < u_c) {
            u_c = u;
            win = i;
        }
    }
    if (win < 0 || !(u_c > 0 && u_c < 1e300)) return -1;
    const SureSphere wi = get(win);
    const double r = sqrt(wi.r2), r_in = r * (1 - 1e-9) - 1e-6, r_out = r * (1 + 1e-9) + 1e-6;
    if (!(r_in > 0)) return -1;
    const double wc[3] = {wi.c.x, wi.c.y, wi.c.z};
    // (o): the origin box outside the winner
    double near2 = 0;
    for (int k = 0; k < 3; k++) {
        const double gap = fmax(fmax(A.k[k].lo - wc[k], wc[k] - A.k[k].hi), 0.0);
        near2 += gap * gap;
    }
    if (!(near2 > r_out * r_out)) return -1;
    // (a): the first rung whose box lies inside the winner
    SureBox P = A;
    bool inside = false;
    for (int rung = 0; rung < 4 && !inside; rung++) {
        const double u_hi = u_c * (1 + (rung == 0 ? 0.002 : rung == 1 ? 0.01 : rung == 2 ? 0.04 : 0.16)) + 1e-3;
        P = sure_beam_at(t, u_hi);
        double far2 = 0;
        for (int k = 0; k < 3; k++) {
            const double f = fmax(fabs(P.k[k].lo - wc[k]), fabs(P.k[k].hi - wc[k]));
            far2 += f * f;
        }
        inside = far2 < r_in * r_in;
    }
    if (!inside) return -1;
    // (b): every other sphere clear of the hull
    for (int j = 0; j < n; j++) {
        if (j == win) continue;
        const SureSphere s = get(j);
        if (!sure_hull_clear_of(A, P, s.c, sqrt(s.r2))) return -1;
    }
    return win;
}

#endif
