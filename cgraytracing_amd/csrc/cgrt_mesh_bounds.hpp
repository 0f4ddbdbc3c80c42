// Device helpers shared by everything that writes a committed mesh's records: the commit's device build (cgrt_devbuild.hpp), the
// refit (cgrt_refit.hpp), the rebuild (cgrt_rebuild.hpp, through the commit's builder) and the tree cost (cgrt_tree_cost.hpp).
// Included by cgrt_hip.hip before cgrt_devbuild.hpp.  The formulas that the host evaluates too -- tree_bmax, cover_radius,
// sphere_s0 -- are cgrt_build.h's.
#ifndef CGRT_MESH_BOUNDS_HPP
#define CGRT_MESH_BOUNDS_HPP

namespace mesh_bounds {

static constexpr int kReduceThreads = 256;  // the workgroup of every kernel that calls block_reduce

__device__ inline double neg_inf() { return -__builtin_huge_val(); }

// objects.h:98-99: e1 = pa - pb, e2 = pa - pc
__device__ inline TriRec make_tri_rec(const double *pa, const double *pb, const double *pc) {
    TriRec tr;
    for (int k = 0; k < 3; k++) {
        tr.pa[k] = pa[k];
        tr.e1[k] = pa[k] - pb[k];
        tr.e2[k] = pa[k] - pc[k];
    }
    return tr;
}

// the box of one triangle's three vertices (t: 9 doubles)
__device__ inline void tri_box(const double *t, double lo[3], double hi[3]) {
    for (int k = 0; k < 3; k++) {
        lo[k] = fmin(t[k], fmin(t[3 + k], t[6 + k]));
        hi[k] = fmax(t[k], fmax(t[3 + k], t[6 + k]));
    }
}
// ... folded into a vertex box kept as MAXIMA: v[0..2] = max(-lo), v[3..5] = max(hi), so that one max reduction, and for keys in
// memory one memset, serve both ends.  Negation is exact: -v[k] is the minimum itself.
__device__ inline void fold_box(const double *t, double *v) {
    double lo[3], hi[3];
    tri_box(t, lo, hi);
    for (int k = 0; k < 3; k++) {
        v[k] = fmax(v[k], -lo[k]);
        v[3 + k] = fmax(v[3 + k], hi[k]);
    }
}

__device__ inline double dist2(const double *p, const double *c) {
    const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
    return dx * dx + dy * dy + dz * dz;
}

struct Max { __device__ double operator()(double a, double b) const { return fmax(a, b); } };
struct Sum { __device__ double operator()(double a, double b) const { return a + b; } };

// v[k] = op over the workgroup's kReduceThreads values of v[k], in every thread.  All threads call it; part: 4 * NV doubles of
// LDS, free again on return.  The order is fixed: xor-shuffles 32, 16, ..., 1 inside each wave, then op(op(p0, p1), op(p2, p3)) of
// the four waves' results -- immaterial for Max, and what makes a Sum the same double in every launch.
template <int NV, class Op>
__device__ inline void block_reduce(double (&v)[NV], double *part, Op op) {
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < NV; k++) v[k] = op(v[k], __shfl_xor(v[k], off));
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < NV; k++) part[(threadIdx.x >> 6) * NV + k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; k++) v[k] = op(op(part[k], part[NV + k]), op(part[2 * NV + k], part[3 * NV + k]));
    __syncthreads();
}

// The cover sphere of positions [b, e) of a triangle order -- order[stride * j] is the index in tri9 of position j's triangle
// (stride 1: MeshArgs::idx_out, 2: the refit plan's {src, rec} pairs): c = the centre of the range's vertex box, r2[0] = the
// largest squared vertex distance from c and, where a mesh centre mc is given, r2[1] = that from mc (0 without).  All threads of
// the workgroup call it and get the results; part: 24 doubles of LDS.  An empty range leaves c undefined and r2 zero.
__device__ inline void range_sphere(const double *tri9, const int *order, int stride, int b, int e, const double *mc, double *part,
                                    double c[3], double (&r2)[2]) {
    double v[6];
    for (int k = 0; k < 6; k++) v[k] = neg_inf();
    for (int j = b + (int)threadIdx.x; j < e; j += kReduceThreads) fold_box(tri9 + 9 * (size_t)order[(size_t)stride * j], v);
    block_reduce<6>(v, part, Max());
    for (int k = 0; k < 3; k++) c[k] = 0.5 * (-v[k] + v[3 + k]);
    r2[0] = r2[1] = 0.0;
    for (int j = b + (int)threadIdx.x; j < e; j += kReduceThreads) {
        const double *t = tri9 + 9 * (size_t)order[(size_t)stride * j];
        for (int q = 0; q < 3; q++) {
            r2[0] = fmax(r2[0], dist2(t + 3 * q, c));
            if (mc) r2[1] = fmax(r2[1], dist2(t + 3 * q, mc));
        }
    }
    block_reduce<2>(r2, part, Max());
}
// ... stored as (cx, cy, cz, r); an empty range (any = false) becomes a point at `empty_at`
__device__ inline void store_cover(double *o, const double c[3], double r2, bool any, const double *empty_at) {
    for (int k = 0; k < 3; k++) o[k] = any ? c[k] : empty_at[k];
    o[3] = cover_radius(any ? r2 : 0.0);
}

}  // namespace mesh_bounds

#endif
