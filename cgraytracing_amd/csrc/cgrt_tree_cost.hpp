// cgrt_scene_mesh_cost: the surface-area cost of the 4-wide hierarchy the device walks for an opaque mesh,
// read from the device's records -- whichever builder, refit or rebuild wrote them.  Included by cgrt_hip.hip.
//
//   S(b)       2 (x y + y z + z x), the extents x, y, z taken as (double)hi - (double)lo of a slot's fp32 box (kBoxPad keeps them
//              positive); each operation rounded on its own, so the host can compute the same double
//   root_area  S of the union of the root node's used slots
//   node_cost  1 + the sum over inner slots of S / root_area
//   tri_cost   the sum over leaf slots of count * S / root_area
//
// Two launches, so that no sum is handed from workgroup to workgroup inside one: tree_cost_kernel, a thread per wide node, sums
// in fp64 (mesh_bounds::block_reduce) and writes one partial pair per workgroup; tree_cost_sum_kernel, one
// workgroup, adds the partials in workgroup order and divides by root_area.  The result does not depend on the launch.
#ifndef CGRT_TREE_COST_HPP
#define CGRT_TREE_COST_HPP

namespace tree_cost {

using namespace mesh_bounds;
static constexpr int kThreadsCost = kReduceThreads;

__device__ inline double slot_area(float lox, float loy, float loz, float hix, float hiy, float hiz) {
    const double x = (double)hix - (double)lox, y = (double)hiy - (double)loy, z = (double)hiz - (double)loz;
    return 2.0 * __dadd_rn(__dadd_rn(__dmul_rn(x, y), __dmul_rn(y, z)), __dmul_rn(z, x));  // (no contraction: the host's double)
}

// partial[2 b] = the sum of S over workgroup b's inner slots, partial[2 b + 1] = of count * S over its leaf slots
__global__ __launch_bounds__(kThreadsCost) void tree_cost_kernel(const WideNodeRec *wnodes, int nwide, double *partial) {
    __shared__ double part[4 * 2];
    const int i = blockIdx.x * kThreadsCost + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (i < nwide) {
        const WideNodeRec w = wnodes[i];
        for (int k = 0; k < 4; k++) {
            const int32_t r = w.ref[k];
            if (r == kWideNone) continue;
            const double S = slot_area(w.lox[k], w.loy[k], w.loz[k], w.hix[k], w.hiy[k], w.hiz[k]);
            if (r < 0) v[0] += S;
            else v[1] += (double)(r & 15) * S;
        }
    }
    block_reduce<2>(v, part, Sum());  // (its fixed order: the same doubles in every launch)
    if (threadIdx.x == 0)
        for (int k = 0; k < 2; k++) partial[2 * (size_t)blockIdx.x + k] = v[k];
}

// cost3 = {node_cost, tri_cost, root_area}
__global__ void tree_cost_sum_kernel(const WideNodeRec *wnodes, const double *partial, int nblocks, double *cost3) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const WideNodeRec w = wnodes[0];
    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    for (int k = 0; k < 4; k++) {
        if (w.ref[k] == kWideNone) continue;
        lo[0] = fminf(lo[0], w.lox[k]);
        lo[1] = fminf(lo[1], w.loy[k]);
        lo[2] = fminf(lo[2], w.loz[k]);
        hi[0] = fmaxf(hi[0], w.hix[k]);
        hi[1] = fmaxf(hi[1], w.hiy[k]);
        hi[2] = fmaxf(hi[2], w.hiz[k]);
    }
    const double root = slot_area(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    double node = 0.0, tri = 0.0;
    for (int b = 0; b < nblocks; b++) {
        node += partial[2 * (size_t)b];
        tri += partial[2 * (size_t)b + 1];
    }
    cost3[0] = 1.0 + node / root;
    cost3[1] = tri / root;
    cost3[2] = root;
}

}  // namespace tree_cost

// cost3: DEVICE room for three doubles.  Everything is enqueued on st.
static int mesh_cost_launch(const cgrt_scene *s, int t, double *cost3, hipStream_t st) {
    const TreeRec &tr = s->tree_recs[(size_t)t];
    const int T = tree_cost::kThreadsCost, nblocks = (tr.nwide + T - 1) / T;
    HIP_TRY(s->cost_partials.need((size_t)nblocks * 2 * sizeof(double)));
    const WideNodeRec *w = s->dev.wnodes + tr.wnode_begin;
    double *partial = reinterpret_cast<double *>(s->cost_partials.p);
    hipLaunchKernelGGL(tree_cost::tree_cost_kernel, dim3((unsigned)nblocks), dim3(T), 0, st, w, tr.nwide, partial);
    hipLaunchKernelGGL(tree_cost::tree_cost_sum_kernel, dim3(1), dim3(64), 0, st, w, (const double *)partial, nblocks, cost3);
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

extern "C" {

int cgrt_scene_mesh_cost(const cgrt_scene *s, int obj, double *cost3_dev, void *stream) {
    MeshTarget m;
    if (const int rc = walk_target(s, obj, "cost", m)) return rc;
    if (!cost3_dev) return fail(CGRT_ERR_INVALID, "cost: null cost3");
    ON_DEVICE(s->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (m.empty) {  // zeros
        HIP_TRY(hipMemsetAsync(cost3_dev, 0, 3 * sizeof(double), st));
        return CGRT_OK;
    }
    return mesh_cost_launch(s, m.tree, cost3_dev, st);
}

int cgrt_scene_mesh_cost_host(const cgrt_scene *s, int obj, cgrt_tree_cost *out) {
    MeshTarget m;
    if (const int rc = walk_target(s, obj, "cost", m)) return rc;
    if (!out) return fail(CGRT_ERR_INVALID, "cost: null out");
    out->node_cost = out->tri_cost = out->root_area = 0.0;
    if (m.empty) return CGRT_OK;
    ON_DEVICE(s->device);
    HostStage hs;
    double c[3];
    double *d = hs.out(c, sizeof(c));
    if (hs.error()) return hs.error();
    if (const int rc = hs.finish(mesh_cost_launch(s, m.tree, d, 0))) return rc;
    out->node_cost = c[0];
    out->tri_cost = c[1];
    out->root_area = c[2];
    return CGRT_OK;
}

}  // extern "C"

#endif
