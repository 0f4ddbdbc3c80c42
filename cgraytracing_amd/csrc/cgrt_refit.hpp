// cgrt_scene_refit_mesh: new vertices for a committed OPAQUE mesh, on the device.  Included by
// cgrt_hip.hip.  The topology of the 4-wide triangle-level hierarchy stays -- which triangles share a leaf, which node hangs in
// which slot -- and every box is recomputed bottom-up by the builders' own rule: the fp64 extent, grown by kBoxPad, rounded
// outward to fp32 (cgrt_build.cpp emit_wide, cgrt_devbuild.hpp wide_level_kernel).  Four kernels on the caller's stream behind
// one memset, no host read-back:
//
//   refit_tris_kernel    one thread per position of the hierarchy's triangle order: the TriRec into otris[] and into its record
//                        of tris[]; the vertex box and the largest |coordinate|, reduced per workgroup, then one ordered-key
//                        atomic per value and workgroup.
//   refit_nodes_kernel   one thread per wide node: fits the node's leaf slots, then arrives at the node; the arrival that
//                        completes a node writes the union of the node's four boxes into the parent's slot and arrives there
//                        (lbvh_fit_kernel's scheme with a count per node, RefitPlan::arrivals).  No thread waits for another.
//   refit_bounds_kernel  one workgroup per cover sphere: a contiguous range of the triangle order -> (centre of its vertex box,
//                        largest vertex distance + 1e-3) into cover[]; the same pass takes the largest squared distance from
//                        the centre of the MESH's vertex box, complete by now.
//   refit_finish_kernel  ObjRec::a / s0 (add_mesh_triangles' formulas) and TreeRec::bmax (tree_bmax's) into the device arrays.
//
// Parity class: that of CGRT_BUILD_DEVICE (cgrt.h).  Boxes are supersets and the triangle test is the same code, so every ray
// with a unique nearest hit gets the hit of a scene freshly committed with the new vertices, bit for bit; exact ties keep the
// tie order the tree had (OTriRec::k and ::leaf are not touched).
#ifndef CGRT_REFIT_HPP
#define CGRT_REFIT_HPP

namespace refit {

using devbuild::dkey;
using devbuild::dunkey;
using devbuild::f_down;
using devbuild::f_up;

static constexpr int kThreadsRefit = 256;
// keys[]: every value is kept as the key of a MAXIMUM (a lower bound as the maximum of its negation), so one memset clears them
enum { KEY_NEG_LO = 0, KEY_HI = 3, KEY_MAX_ABS = 6, KEY_R2 = 7, N_KEYS = 8 };

struct Args {
    const double *tri9;  // n x 9, construction order (the caller's)
    int n, nwide;
    const int2 *srcrec;        // per position: {construction index, record of tris[]}
    const RefitNode *nodes;    // per wide node
    TriRec *tris;              // the tree's first record of each array
    OTriRec *otris;
    WideNodeRec *wnodes;
    unsigned long long *keys;  // N_KEYS
    int *arrive;               // nwide arrival counters, cleared on the stream by every refit
    ObjRec *obj;
    TreeRec *tree;
    double *cover;  // the mesh's first cover sphere (4 doubles each), or nullptr
    int n_cover;
};

__device__ inline double neg_inf() { return -__builtin_huge_val(); }

// v[k] = the workgroup's maximum of v[k], in every thread.  All kThreadsRefit threads call it.
template <int NV>
__device__ inline void block_max(double (&v)[NV], double (*part)[NV]) {
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < NV; k++) v[k] = fmax(v[k], __shfl_xor(v[k], off));
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < NV; k++) part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; k++) v[k] = fmax(fmax(part[0][k], part[1][k]), fmax(part[2][k], part[3][k]));
    __syncthreads();  // (part is free again)
}

// max(-lo), max(hi) of a triangle's three vertices into v[0..2], v[3..5]
__device__ inline void fold_box(const double *t, double *v) {
    for (int k = 0; k < 3; k++) {
        v[k] = fmax(v[k], -fmin(t[k], fmin(t[3 + k], t[6 + k])));
        v[3 + k] = fmax(v[3 + k], fmax(t[k], fmax(t[3 + k], t[6 + k])));
    }
}

__global__ __launch_bounds__(kThreadsRefit) void refit_tris_kernel(Args a) {
    __shared__ double part[4][7];
    const int j = blockIdx.x * kThreadsRefit + threadIdx.x;
    double v[7];
    for (int k = 0; k < 7; k++) v[k] = neg_inf();
    if (j < a.n) {
        const int2 sr = a.srcrec[j];
        const double *t = a.tri9 + 9 * (size_t)sr.x;
        double p[9];
        for (int k = 0; k < 9; k++) p[k] = t[k];
        TriRec tr;  // objects.h:98-99, as mesh_prep_kernel
        for (int k = 0; k < 3; k++) {
            tr.pa[k] = p[k];
            tr.e1[k] = p[k] - p[3 + k];
            tr.e2[k] = p[k] - p[6 + k];
        }
        a.otris[j].t = tr;  // (k and leaf stay: ties go on as before)
        a.tris[sr.y] = tr;
        fold_box(p, v);
        for (int k = 0; k < 3; k++) v[6] = fmax(v[6], fmax(fabs(v[k]), fabs(v[3 + k])));
    }
    block_max<7>(v, part);
    if (threadIdx.x == 0)
        for (int k = 0; k < 7; k++) atomicMax(a.keys + k, dkey(v[k]));
}

// The boxes of wide nodes are handed from thread to thread INSIDE the launch, between workgroups on any XCD: every box word is
// written and read as an agent-scope atomic (write-through stores, loads past the L1), the writer drains its stores and
// releases before it arrives, and the completing arrival acquires before it reads.
__device__ inline void st_box(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline float ld_box(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_slot(WideNodeRec *w, int k, const float lo[3], const float hi[3]) {
    st_box(&w->lox[k], lo[0]);
    st_box(&w->loy[k], lo[1]);
    st_box(&w->loz[k], lo[2]);
    st_box(&w->hix[k], hi[0]);
    st_box(&w->hiy[k], hi[1]);
    st_box(&w->hiz[k], hi[2]);
}

__global__ __launch_bounds__(kThreadsRefit) void refit_nodes_kernel(Args a) {
    const int i = blockIdx.x * kThreadsRefit + threadIdx.x;
    if (i >= a.nwide) return;
    {   // this node's leaf slots, each fitted to its triangles
        WideNodeRec *w = a.wnodes + i;
        for (int k = 0; k < 4; k++) {
            const int32_t r = w->ref[k];  // (references are never written by a refit)
            if (r < 0) continue;          // an inner child or an empty slot
            const int first = r >> 4, cnt = r & 15;
            double v[6];
            for (int q = 0; q < 6; q++) v[q] = neg_inf();
            for (int q = 0; q < cnt; q++) fold_box(a.tri9 + 9 * (size_t)a.srcrec[first + q].x, v);
            const float lo[3] = {f_down(-v[0] - kBoxPad), f_down(-v[1] - kBoxPad), f_down(-v[2] - kBoxPad)};
            const float hi[3] = {f_up(v[3] + kBoxPad), f_up(v[4] + kBoxPad), f_up(v[5] + kBoxPad)};
            st_slot(w, k, lo, hi);
        }
    }
    int node = i;
    while (true) {
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const RefitNode rn = a.nodes[node];
        if (atomicAdd(&a.arrive[node], 1) + 1 < rn.need) return;  // another arrival will complete this node
        __threadfence();
        if (rn.parent < 0) return;  // the root is complete
        // The union of already grown and rounded boxes, not padded again: rounding is monotone, so this equals "round the fp64
        // union", which is what both builders store.
        const WideNodeRec *c = a.wnodes + node;
        float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
        float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
        for (int k = 0; k < 4; k++) {
            if (c->ref[k] == kWideNone) continue;
            lo[0] = fminf(lo[0], ld_box(&c->lox[k]));
            lo[1] = fminf(lo[1], ld_box(&c->loy[k]));
            lo[2] = fminf(lo[2], ld_box(&c->loz[k]));
            hi[0] = fmaxf(hi[0], ld_box(&c->hix[k]));
            hi[1] = fmaxf(hi[1], ld_box(&c->hiy[k]));
            hi[2] = fmaxf(hi[2], ld_box(&c->hiz[k]));
        }
        st_slot(a.wnodes + rn.parent, rn.slot, lo, hi);
        node = rn.parent;
    }
}

// One workgroup per cover sphere g: positions [g n / G, (g + 1) n / G) of the triangle order (cover_kernel's ranges; contiguous
// in either builder's order, hence compact).  Any spheres that together contain every triangle serve classify_kernel.
__global__ __launch_bounds__(kThreadsRefit) void refit_bounds_kernel(Args a) {
    __shared__ double part6[4][6];
    __shared__ double part2[4][2];
    const int G = a.n_cover > 0 ? a.n_cover : 1, g = blockIdx.x, n = a.n;
    const int b = (int)((long long)g * n / G), e = (int)((long long)(g + 1) * n / G);
    double v[6];
    for (int k = 0; k < 6; k++) v[k] = neg_inf();
    for (int j = b + (int)threadIdx.x; j < e; j += kThreadsRefit) fold_box(a.tri9 + 9 * (size_t)a.srcrec[j].x, v);
    block_max<6>(v, part6);
    double c[3], mc[3];  // the range's centre, the mesh's (its vertex box is complete: refit_tris_kernel ran before)
    for (int k = 0; k < 3; k++) {
        c[k] = 0.5 * (-v[k] + v[3 + k]);
        mc[k] = 0.5 * (-dunkey(a.keys[KEY_NEG_LO + k]) + dunkey(a.keys[KEY_HI + k]));
    }
    double r2[2] = {0.0, 0.0};
    for (int j = b + (int)threadIdx.x; j < e; j += kThreadsRefit) {
        const double *t = a.tri9 + 9 * (size_t)a.srcrec[j].x;
        for (int q = 0; q < 3; q++) {
            const double dx = t[3 * q] - c[0], dy = t[3 * q + 1] - c[1], dz = t[3 * q + 2] - c[2];
            r2[0] = fmax(r2[0], dx * dx + dy * dy + dz * dz);
            const double mx = t[3 * q] - mc[0], my = t[3 * q + 1] - mc[1], mz = t[3 * q + 2] - mc[2];
            r2[1] = fmax(r2[1], mx * mx + my * my + mz * mz);
        }
    }
    block_max<2>(r2, part2);
    if (threadIdx.x != 0) return;
    if (a.cover && g < a.n_cover) {
        double *o = a.cover + 4 * (size_t)g;
        const bool any = e > b;  // (an empty range: a point at the mesh's centre)
        o[0] = any ? c[0] : mc[0];
        o[1] = any ? c[1] : mc[1];
        o[2] = any ? c[2] : mc[2];
        o[3] = (any ? sqrt(r2[0]) : 0.0) + 1e-3;
    }
    atomicMax(a.keys + KEY_R2, dkey(r2[1]));
}

// HostScene::add_mesh_triangles' bounding sphere and tree_bmax's bound (cgrt_build.cpp), written where the kernels read them
__global__ void refit_finish_kernel(Args a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int k = 0; k < 3; k++) a.obj->a[k] = 0.5 * (-dunkey(a.keys[KEY_NEG_LO + k]) + dunkey(a.keys[KEY_HI + k]));
    const double r = sqrt(dunkey(a.keys[KEY_R2])) + 1e-3;
    a.obj->s0 = r * r * (1 + 1e-9);
    const double max_abs = dunkey(a.keys[KEY_MAX_ABS]);
    a.tree->bmax = (float)((max_abs + 2 * kBoxPad) * (1 + 1e-6)) * (1.f + 1e-6f);
}

}  // namespace refit

// ---- host side ---------------------------------------------------------------------------------------------------------

static const char *const kRefitStale = "the scene was refitted after this session was created";

// Which tree a refit of object `obj` works on, after every check that needs no device.  *tree = -1: an empty mesh, nothing to do.
// The rebuild (what = "rebuild") and the tree cost (what = "cost", which takes no vertices: cost = true) refuse the same.
static int refit_check(const cgrt_scene *s, int obj, const double *tri9, int ntri, int *tree, const char *what = "refit", bool cost = false) {
    const std::string who = what;
    *tree = -1;
    if (!s) return fail(CGRT_ERR_INVALID, who + ": null scene");
    if (!s->committed) return fail(CGRT_ERR_INVALID, who + ": scene not committed");
    if (obj < 0 || obj >= (int)s->host.objs.size()) return fail(CGRT_ERR_INVALID, who + ": no such object");
    const ObjRec &o = s->host.objs[(size_t)obj];
    if (o.kind == KIND_SPHERE) return fail(CGRT_ERR_INVALID, who + ": the object is a sphere, not a mesh");
    if (o.kind == KIND_BEZIER) return fail(CGRT_ERR_INVALID, who + ": the object is a Bezier surface, not a mesh");
    if (o.kind == KIND_PLANE)
        return fail(CGRT_ERR_INVALID, o.tree >= 0 ? who + ": the object is a bump floor, not a mesh" : who + ": the object is a plane, not a mesh");
    if (o.kind != KIND_MESH || o.tree < 0 || o.tree >= (int)s->tree_recs.size()) return fail(CGRT_ERR_INVALID, who + ": the object is no mesh");
    if (!(o.transp < kEps) && cost) return fail(CGRT_ERR_INVALID, who + ": the mesh is transparent: its tree has no 4-wide hierarchy");
    if (!(o.transp < kEps))
        return fail(CGRT_ERR_INVALID, who + ": the mesh is transparent (its improvement counter makes the leaf order observable, quirk Q5)");
    const TreeRec &tr = s->tree_recs[(size_t)o.tree];
    if (cost) ntri = tr.ntris;
    if (ntri != tr.ntris) return fail(CGRT_ERR_INVALID, who + ": ntri is not the mesh's triangle count (" + std::to_string(tr.ntris) + ")");
    if (ntri == 0) return CGRT_OK;
    if (!tr.tri_level || tr.nwide <= 0) return fail(CGRT_ERR_INVALID, who + ": the tree has no 4-wide hierarchy (CGRT_TREE=ref)");
    if (!tri9 && !cost) return fail(CGRT_ERR_INVALID, who + ": null tri9");
    *tree = o.tree;
    return CGRT_OK;
}

// The plan of tree t: from the host's records (a host-built tree, committed or not) or from the device's (a device-built one)
static int tree_refit_plan(const cgrt_scene *s, int t, RefitPlan &plan) {
    const HostTree &T = s->host.trees[(size_t)t];
    std::vector<WideNodeRec> wide_dev;
    std::vector<int32_t> k;
    const WideNodeRec *wide = T.wide.data();
    int32_t nwide = (int32_t)T.wide.size(), ntri = (int32_t)T.otris.size();
    if (T.dev_kind == 1) {
        if (!s->committed) return fail(CGRT_ERR_INVALID, "refit plan: a device-built tree exists only after the commit");
        ON_DEVICE(s->device);
        const TreeRec &tr = s->tree_recs[(size_t)t];
        nwide = tr.nwide;
        ntri = tr.ntris;
        wide_dev.resize((size_t)std::max(nwide, 0));
        std::vector<OTriRec> ot((size_t)std::max(ntri, 0));
        if (!wide_dev.empty()) HIP_TRY(hipMemcpy(wide_dev.data(), s->dev.wnodes + tr.wnode_begin, wide_dev.size() * sizeof(WideNodeRec), hipMemcpyDeviceToHost));
        if (!ot.empty()) HIP_TRY(hipMemcpy(ot.data(), s->dev.otris + tr.otri_begin, ot.size() * sizeof(OTriRec), hipMemcpyDeviceToHost));
        wide = wide_dev.data();
        for (const OTriRec &o : ot) k.push_back(o.k);
    } else {
        for (const OTriRec &o : T.otris) k.push_back(o.k);
        if ((size_t)ntri != T.leaf_ids.size()) return fail(CGRT_ERR_INVALID, "refit plan: the tree has no triangle-level hierarchy");
    }
    try {
        if (const char *bad = refit_plan(wide, nwide, k.data(), ntri, T.dev_kind == 1 ? nullptr : T.leaf_ids.data(), plan)) return fail(CGRT_ERR_INVALID, bad);
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string("refit plan: ") + e.what());
    }
    plan.cover_first = (int32_t)T.cover_first;
    plan.n_cover = T.cover_n;
    return CGRT_OK;
}

// The first refit of a mesh: its plan, and the plan's device copy in front of the words every refit clears
static int refit_prepare(cgrt_scene *s, int obj, int t, RefitState **out) {
    auto it = s->refit.find(obj);
    int64_t refits_so_far = 0;
    if (it != s->refit.end()) {
        if (!it->second->stale) {
            *out = it->second.get();
            return CGRT_OK;
        }
        refits_so_far = it->second->refits;  // (a rebuild dropped the plan: built again here, the count goes on)
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<RefitState> st(new (std::nothrow) RefitState());
    if (!st) return fail(CGRT_ERR_LIMIT, "out of host memory");
    if (const int rc = tree_refit_plan(s, t, st->plan)) return rc;
    const RefitPlan &p = st->plan;
    const size_t nwide = p.parent.size(), ntri = p.src.size();
    if ((size_t)p.cover_first + (size_t)p.n_cover > (size_t)s->dev.n_cover || p.n_cover < 0)
        return fail(CGRT_ERR_INVALID, "refit plan: the mesh's cover spheres lie outside the scene's");
    // [keys | arrival counters] (cleared by one memset, from the allocation's start) [nodes] [src, rec]
    auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    st->clear_bytes = round16(refit::N_KEYS * sizeof(unsigned long long) + nwide * sizeof(int));
    const size_t nodes_at = st->clear_bytes, srcrec_at = nodes_at + round16(nwide * sizeof(RefitNode));
    st->bytes = srcrec_at + round16(ntri * sizeof(int2));
    HIP_TRY(st->mem.alloc(st->bytes));
    std::vector<RefitNode> nodes(nwide);
    for (size_t i = 0; i < nwide; i++) nodes[i] = RefitNode{p.parent[i], p.slot[i], p.arrivals[i], 0};
    std::vector<int2> srcrec(ntri);
    for (size_t j = 0; j < ntri; j++) srcrec[j] = make_int2(p.src[j], p.rec[j]);
    unsigned char *base = st->mem.as<unsigned char>();
    HIP_TRY(hipMemcpy(base + nodes_at, nodes.data(), nwide * sizeof(RefitNode), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + srcrec_at, srcrec.data(), ntri * sizeof(int2), hipMemcpyHostToDevice));
    st->keys = reinterpret_cast<unsigned long long *>(base);
    st->arrive = reinterpret_cast<int *>(base + refit::N_KEYS * sizeof(unsigned long long));
    st->nodes = reinterpret_cast<const RefitNode *>(base + nodes_at);
    st->srcrec = reinterpret_cast<const int2 *>(base + srcrec_at);
    st->ms_plan = ms_since(t0);
    st->refits = refits_so_far;
    *out = st.get();
    s->refit[obj] = std::move(st);
    return CGRT_OK;
}

// tri9: DEVICE pointer.  Everything behind the first call's plan is enqueued on st.
static int refit_launch(cgrt_scene *s, int obj, int t, const double *tri9, hipStream_t st) {
    RefitState *rs = nullptr;
    if (const int rc = refit_prepare(s, obj, t, &rs)) return rc;
    const TreeRec &tr = s->tree_recs[(size_t)t];
    refit::Args a;
    a.tri9 = tri9;
    a.n = tr.ntris;
    a.nwide = tr.nwide;
    a.srcrec = rs->srcrec;
    a.nodes = rs->nodes;
    a.tris = const_cast<TriRec *>(s->dev.tris) + tr.tri_begin;
    a.otris = const_cast<OTriRec *>(s->dev.otris) + tr.otri_begin;
    a.wnodes = const_cast<WideNodeRec *>(s->dev.wnodes) + tr.wnode_begin;
    a.keys = rs->keys;
    a.arrive = rs->arrive;
    a.obj = const_cast<ObjRec *>(s->dev.objs) + obj;
    a.tree = const_cast<TreeRec *>(s->dev.trees) + t;
    a.n_cover = rs->plan.n_cover;
    a.cover = a.n_cover > 0 ? const_cast<double *>(s->dev.cover) + 4 * (size_t)rs->plan.cover_first : nullptr;
    const int T = refit::kThreadsRefit;
    HIP_TRY(hipMemsetAsync(rs->mem.p, 0, rs->clear_bytes, st));
    hipLaunchKernelGGL(refit::refit_tris_kernel, dim3((unsigned)((a.n + T - 1) / T)), dim3(T), 0, st, a);
    hipLaunchKernelGGL(refit::refit_nodes_kernel, dim3((unsigned)((a.nwide + T - 1) / T)), dim3(T), 0, st, a);
    hipLaunchKernelGGL(refit::refit_bounds_kernel, dim3((unsigned)std::max(a.n_cover, 1)), dim3(T), 0, st, a);
    hipLaunchKernelGGL(refit::refit_finish_kernel, dim3(1), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    rs->refits++;
    s->geometry_gen++;
    s->host.trees[(size_t)t].refitted = true;  // the reference's tree over the old vertices describes nothing any more
    return CGRT_OK;
}

extern "C" {

int cgrt_scene_refit_mesh(cgrt_scene *s, int obj, const double *tri9, int ntri, void *stream) {
    int t = -1;
    if (const int rc = refit_check(s, obj, tri9, ntri, &t)) return rc;
    if (t < 0) return CGRT_OK;
    ON_DEVICE(s->device);
    return refit_launch(s, obj, t, tri9, reinterpret_cast<hipStream_t>(stream));
}

int cgrt_scene_refit_mesh_host(cgrt_scene *s, int obj, const double *tri9, int ntri) {
    int t = -1;
    if (const int rc = refit_check(s, obj, tri9, ntri, &t)) return rc;
    if (t < 0) return CGRT_OK;
    ON_DEVICE(s->device);
    const size_t bytes = (size_t)ntri * 9 * sizeof(double);
    DevBuf d;
    HIP_TRY(d.alloc(bytes));
    HIP_TRY(hipMemcpy(d.p, tri9, bytes, hipMemcpyHostToDevice));
    if (const int rc = refit_launch(s, obj, t, d.as<double>(), 0)) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    // the host mirrors of what the device now owns
    HostScene &H = s->host;
    ObjRec o;
    HIP_TRY(hipMemcpy(&o, s->dev.objs + obj, sizeof(o), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) H.objs[(size_t)obj].a[k] = o.a[k];
    H.objs[(size_t)obj].s0 = o.s0;
    TreeRec tr;
    HIP_TRY(hipMemcpy(&tr, s->dev.trees + t, sizeof(tr), hipMemcpyDeviceToHost));
    s->tree_recs[(size_t)t].bmax = tr.bmax;
    const RefitPlan &p = s->refit[obj]->plan;
    if (p.n_cover > 0)
        HIP_TRY(hipMemcpy(H.cover.data() + 4 * (size_t)p.cover_first, s->dev.cover + 4 * (size_t)p.cover_first,
                          (size_t)p.n_cover * 4 * sizeof(double), hipMemcpyDeviceToHost));
    try {
        H.trees[(size_t)t].tri9.assign(tri9, tri9 + (size_t)ntri * 9);
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string("refit: ") + e.what());
    }
    return CGRT_OK;
}

int cgrt_scene_refit_info(const cgrt_scene *s, int obj, cgrt_refit_info *out) {
    if (!s || !out) return fail(CGRT_ERR_INVALID, "null argument");
    if (obj < 0 || obj >= (int)s->host.objs.size() || s->host.objs[(size_t)obj].kind != KIND_MESH || s->host.objs[(size_t)obj].tree < 0)
        return fail(CGRT_ERR_INVALID, "refit info: the object is no mesh");
    const int t = s->host.objs[(size_t)obj].tree;
    const HostTree &T = s->host.trees[(size_t)t];
    std::memset(out, 0, sizeof(*out));
    if (s->committed) {
        out->nwide = s->tree_recs[(size_t)t].nwide;
        out->ntris = s->tree_recs[(size_t)t].ntris;
    } else {
        out->nwide = (int32_t)T.wide.size();
        out->ntris = T.dev_kind ? (int32_t)T.dev_ntri : (int32_t)(T.tri9.size() / 9);
    }
    const auto it = s->refit.find(obj);
    if (it != s->refit.end()) {
        out->refits = it->second->refits;
        out->plan_built = it->second->stale ? 0 : 1;
        out->ms_plan = it->second->ms_plan;
    }
    out->geometry_gen = s->geometry_gen;
    return CGRT_OK;
}

int cgrt_scene_refit_plan_host(const cgrt_scene *s, int tree, int32_t *nwide, int32_t *ntris, int32_t *parent, int32_t *slot,
                               int32_t *arrivals, int32_t *src) {
    if (!s || tree < 0 || tree >= (int)s->host.trees.size()) return fail(CGRT_ERR_INVALID, "bad tree index");
    const HostTree &T = s->host.trees[(size_t)tree];
    const bool wide = T.dev_kind == 1 ? (s->committed && s->tree_recs[(size_t)tree].nwide > 0) : (T.tri_level && !T.wide.empty());
    if (!wide) {  // no 4-wide hierarchy: nothing to plan (as cgrt_scene_wide_dump reports no node)
        if (nwide) *nwide = 0;
        if (ntris) *ntris = 0;
        return CGRT_OK;
    }
    if (!parent && !slot && !arrivals && !src) {  // the sizing call
        if (nwide) *nwide = T.dev_kind == 1 ? s->tree_recs[(size_t)tree].nwide : (int32_t)T.wide.size();
        if (ntris) *ntris = T.dev_kind == 1 ? s->tree_recs[(size_t)tree].ntris : (int32_t)T.otris.size();
        return CGRT_OK;
    }
    RefitPlan plan;
    if (const int rc = tree_refit_plan(s, tree, plan)) return rc;
    if (nwide) *nwide = (int32_t)plan.parent.size();
    if (ntris) *ntris = (int32_t)plan.src.size();
    if (parent) std::memcpy(parent, plan.parent.data(), plan.parent.size() * sizeof(int32_t));
    if (slot) std::memcpy(slot, plan.slot.data(), plan.slot.size() * sizeof(int32_t));
    if (arrivals) std::memcpy(arrivals, plan.arrivals.data(), plan.arrivals.size() * sizeof(int32_t));
    if (src) std::memcpy(src, plan.src.data(), plan.src.size() * sizeof(int32_t));
    return CGRT_OK;
}

}  // extern "C"

#endif
