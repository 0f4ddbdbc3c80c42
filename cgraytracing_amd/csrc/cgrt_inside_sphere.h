// The spheres a ray that starts inside a refracting sphere can hit first, in plain C++ (no HIP).  cgrt_scene_commit computes the
// trait on the host (scene_traits, cgrt_build.cpp), the PAIR variants' sphere loop reads it (intersect_scene, cgrt_scene_walk.hpp)
// and tests/native/inside_sphere.cpp runs the same functions on the CPU against the device's loop in its operation order.
//
// inside_mask(s, n, i) promises: for EVERY ray (o, d) with starts_inside(o, c_i, rin2_i) and d a unit vector to within 8 ulp a
// component (what normalized() and the shade step produce), the device's sphere loop over all n spheres (sphere_len, strict <,
// ascending) and the same loop over the mask's bits alone end on the same (t, id).  A glass scene's waves spend 28 % of their
// trips on such rays -- the refracted child of an entering ray, the reflected child of a ray inside -- and the spheres the mask
// leaves out are distances that cannot win.
//
// The argument.  Ball i has centre c_i and radius r_i; r_in = r_i (1 - 1e-9) - 1e-6 as cgrt_sure_first.h takes its inward margin,
// rin2 = r_in^2.  Sphere j is left out only when D = |c_i - c_j| > r_i + r_j + m_ij, so with gap = D - r_i - r_j > m_ij every
// point of ball j is farther than gap from ball i.  Take a ray with l = c_i - o, l . l < rin2, and let T be the parameter at
// which it leaves ball i exactly (T <= 2 r_i; the ray's points up to T lie in ball i, which is convex).
//  (i)  sphere_len for i.  The computed l2 is below rin2 < r2 (starts_inside forms it by sphere_len's own operations), so the
//       first test passes; d2 = l2 - tca^2 <= l2 and its rounding E_i (below) is far below r2 - rin2 = 2 r_i delta - delta^2,
//       delta = r_i 1e-9 + 1e-6, so the second passes; the result is tca -+ thc, at most the computed tca + thc.  With
//       |sqrt(a + e) - sqrt(a)| <= sqrt(|e|):  len_i <= T + err(tca_i) + sqrt(E_i) + 2 ulp(2 r_i).
//  (j)  sphere_len for a left-out j, L_j = |c_j - o| <= D + r_i.  A computed hit needs the computed r2 - d2 >= 0, so the line
//       passes c_j within sqrt(r_j^2 + E_j) <= r_j + sqrt(E_j), E_j = kSureRound L_j^2 (the bound cgrt_sure_first.h derives for d2:
//       five roundings of L^2-sized terms and 2 tca err(tca), err(tca) <= 2.4e-15 L, the direction's 8 ulp included).
//       - The line meets ball j exactly, first at t_j = tca - thc: that point is in ball j, hence gap outside ball i, hence --
//         the ray moves at unit speed and is inside ball i up to T -- t_j >= T + gap.  The computed thc exceeds the exact one by
//         at most sqrt(E_j):  len_j >= T + gap - sqrt(E_j) - err(tca_j) - 2 ulp(L_j + r_j).
//       - It misses exactly and hits as computed: its closest point p(tca) lies within r_j + sqrt(E_j) of c_j, so at least
//         gap - sqrt(E_j) outside ball i, and the computed thc is at most sqrt(E_j):  len_j >= T + gap - 2 sqrt(E_j) - err(tca_j) - ...
//       - A hit behind the origin is none: sphere_len's first test refuses tca < 0 with l2 > r2; a computed tca >= 0 whose exact
//         value is negative is within err(tca_j) of 0, a point of ball i, which the line does not share with ball j grown by
//         sqrt(E_j) < gap.  (l2 > r2 as computed: l2 >= (r_j + gap)^2 and gap^2 > 1e-13 L_j^2, against l2's 1e-15 L_j^2.)
//       The other root, where the computed t0 < 0, is larger still.
//  So len_j > len_i -- j cannot take the place of the mask's winner, whose len is at most len_i, nor tie with it -- whenever
//       gap > 2 sqrt(E_j) + sqrt(E_i) + err(tca_i) + err(tca_j) + a few ulp of (D + r_i + r_j),
//  and m_ij is twice the square-root terms plus the margin this project takes everywhere, on the scale S = D + r_i + r_j:
//       m_ij = 2 (2 sqrt(E_j) + sqrt(E_i)) + S 1e-9 + 1e-6,      E_j = kSureRound (D + r_i)^2,  E_i = kSureRound r_i^2.
//  The linear terms (2.4e-15 (L_j + r_i), the ulps, this header's own roundings of D and the radii) are below 1e-13 S.  For a wall
//  of radius 1e4 beside a sphere of radius 7: sqrt(E_j) = 9.0e-4, m_ij = 3.6e-3 -- C2's floor, 0.034 clear of the glass ball, is
//  left out; a wall 1e-3 away is kept.  In general m_ij is about 3.6e-7 (D + r_i).
//
// Kept in the mask (bit set): i itself; every sphere that touches, overlaps, lies inside or encloses ball i (D <= r_i + r_j + m_ij
// covers all four); a pair with anything not finite or beyond 1e150.  A scene with ANY sphere not finite has every mask full, and so
// has a candidate whose r_in is not positive (radius below 1e-6: the rounding bound's only way to fail -- E_i <= r_i delta / 2 holds
// for every positive radius); its rin2 is 0 and no origin passes.  A full mask is the unchanged loop.
//
// The candidates are the scene's refracting spheres (transp >= kEps, main.cpp:129's `!(transparency < eps)`), at most kInsideMax; a
// scene with more, with more than 32 spheres, or with an object that is no sphere has none (n == 0): the feature is off.
#ifndef CGRT_INSIDE_SPHERE_H
#define CGRT_INSIDE_SPHERE_H
#include <stdint.h>
#include <cmath>

// (cgrt_types.h includes this header ahead of any HIP header: the attributes are spelt out, not taken from one)
#if defined(__HIPCC__)
#define CGRT_INSIDE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CGRT_INSIDE_HD inline
#endif

static constexpr int kInsideMax = 1;           // candidates a scene may have (C2 has one); each costs every trip a test
static constexpr int kInsideSpheresMax = 32;   // the mask is one word
static constexpr double kInsideRound = 8e-15;  // kSureRound (cgrt_sure_first.h): d2's rounding is at most this times L^2

struct InsideBall {  // a sphere as the scene stores it: ObjRec::a and ObjRec::s0
    double c[3], r2;
};
struct InsideTrait {
    int32_t n;                  // candidates; 0: none
    int32_t idx[kInsideMax];    // the candidate's place in the object list
    uint32_t mask[kInsideMax];  // inside_mask of it
    double rin2[kInsideMax];    // starts_inside's bound; 0: no origin passes
};

CGRT_INSIDE_HD bool inside_finite(const InsideBall &b) {
    return fabs(b.c[0]) < 1e150 && fabs(b.c[1]) < 1e150 && fabs(b.c[2]) < 1e150 && b.r2 > 0 && b.r2 < 1e300;
}
// r_in^2, or 0 where r_in is not positive
CGRT_INSIDE_HD double inside_rin2(double r2) {
    const double r = sqrt(r2), r_in = r * (1 - 1e-9) - 1e-6;
    return (r2 > 0 && r2 < 1e300 && r_in > 0) ? r_in * r_in : 0.0;
}
// m_ij: what the gap between balls i and j must exceed (see above); D the distance of their centres
CGRT_INSIDE_HD double inside_margin(double D, double ri, double rj) {
    const double Lj = D + ri, S = D + ri + rj;
    return 2 * (2 * sqrt(kInsideRound * Lj * Lj) + sqrt(kInsideRound * ri * ri)) + (S * 1e-9 + 1e-6);
}
CGRT_INSIDE_HD uint32_t inside_full_mask(int n) { return n >= 32 ? 0xffffffffu : (1u << n) - 1u; }

// Bit i, and bit j of every sphere whose ball is not provably disjoint from ball i.  n <= kInsideSpheresMax.
CGRT_INSIDE_HD uint32_t inside_mask(const InsideBall *s, int n, int i) {
    const uint32_t full = inside_full_mask(n);
    if (n < 1 || n > kInsideSpheresMax || i < 0 || i >= n) return full;
    for (int j = 0; j < n; j++)
        if (!inside_finite(s[j])) return full;
    if (!(inside_rin2(s[i].r2) > 0)) return full;
    const double ri = sqrt(s[i].r2);
    uint32_t mask = 1u << i;
    for (int j = 0; j < n; j++) {
        if (j == i) continue;
        const double dx = s[j].c[0] - s[i].c[0], dy = s[j].c[1] - s[i].c[1], dz = s[j].c[2] - s[i].c[2];
        const double D = sqrt(dx * dx + dy * dy + dz * dz), rj = sqrt(s[j].r2);
        if (!(D > ri + rj + inside_margin(D, ri, rj))) mask |= 1u << j;
    }
    return mask;
}

// The ray's origin lies inside ball (c, r_in): l = c - o and l . l as sphere_len forms them.  V: any vector type with x, y, z
// (the kernels' V3, the host's Vec3d).
template <class V> CGRT_INSIDE_HD bool starts_inside(V o, V c, double rin2) {
    const double lx = c.x - o.x, ly = c.y - o.y, lz = c.z - o.z;
    return lx * lx + ly * ly + lz * lz < rin2;
}

// The scene's trait: its refracting spheres with their masks.  transp[j]: sphere j's transparency; all_spheres: the object list
// holds nothing but these n spheres.
inline InsideTrait inside_trait(const InsideBall *s, const double *transp, int n, bool all_spheres) {
    InsideTrait t{};
    if (!all_spheres || n < 1 || n > kInsideSpheresMax) return t;
    int count = 0;
    for (int j = 0; j < n; j++)
        if (!(transp[j] < 1e-4)) count++;  // kEps (cgrt_types.h)
    if (count > kInsideMax) return t;
    for (int j = 0; j < n; j++)
        if (!(transp[j] < 1e-4)) {
            t.idx[t.n] = j;
            t.mask[t.n] = inside_mask(s, n, j);
            t.rin2[t.n] = t.mask[t.n] == inside_full_mask(n) ? 0.0 : inside_rin2(s[j].r2);
            t.n++;
        }
    return t;
}
// Whether the guarded loop pays for candidate k: sphere_len alone is about 0.6 of a sphere_len_pair trip, so a mask of m of the
// n spheres costs 0.6 m against n / 2 -- taken where 5 m <= 4 n; a fuller mask, the full one included, leaves the pair loop alone.
inline bool inside_pays(const InsideTrait &t, int k, int n) {
    return k < t.n && t.rin2[k] > 0 && 5 * (int)__builtin_popcount(t.mask[k]) <= 4 * n;
}

#endif
