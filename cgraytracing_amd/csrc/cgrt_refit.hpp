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
//   refit_finish_kernel  ObjRec::a / s0 and TreeRec::bmax (cgrt_build.h's formulas) into the device arrays.
//
// Parity class: that of CGRT_BUILD_DEVICE (cgrt.h).  Boxes are supersets and the triangle test is the same code, so every ray
// with a unique nearest hit gets the hit of a scene freshly committed with the new vertices, bit for bit; exact ties keep the
// tie order the tree had (OTriRec::k and ::leaf are not touched).
#ifndef CGRT_REFIT_HPP
#define CGRT_REFIT_HPP

namespace refit {

using namespace devbuild;  // (dkey, dunkey, f_down, f_up; mesh_bounds)

static constexpr int kThreadsRefit = kReduceThreads;
// keys[]: every value is kept as the key of a MAXIMUM (a lower bound as the maximum of its negation), so one memset clears them
enum { KEY_NEG_LO = 0, KEY_HI = 3, KEY_MAX_ABS = 6, KEY_R2 = 7, N_KEYS = 8 };

struct Args {
    const double *tri9;  // n x 9, construction order (the caller's)
    int n, nwide;
    const int2 *srcrec;        // per position: {construction index, record of tris[]}
    const RefitNode *nodes;    // per wide node
    MeshSlots at;              // where the mesh's records are
    unsigned long long *keys;  // N_KEYS
    int *arrive;               // nwide arrival counters, cleared on the stream by every refit
    int n_cover;               // cover spheres of the mesh at at.cover
};

__global__ __launch_bounds__(kThreadsRefit) void refit_tris_kernel(Args a) {
    __shared__ double part[4 * 7];
    const int j = blockIdx.x * kThreadsRefit + threadIdx.x;
    double v[7];
    for (int k = 0; k < 7; k++) v[k] = neg_inf();
    if (j < a.n) {
        const int2 sr = a.srcrec[j];
        const double *t = a.tri9 + 9 * (size_t)sr.x;
        double p[9];
        for (int k = 0; k < 9; k++) p[k] = t[k];
        const TriRec tr = make_tri_rec(p, p + 3, p + 6);
        a.at.otris[j].t = tr;  // (k and leaf stay: ties go on as before)
        a.at.tris[sr.y] = tr;
        fold_box(p, v);
        for (int k = 0; k < 3; k++) v[6] = fmax(v[6], fmax(fabs(v[k]), fabs(v[3 + k])));
    }
    block_reduce<7>(v, part, Max());
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
        WideNodeRec *w = a.at.wnodes + i;
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
        const WideNodeRec *c = a.at.wnodes + node;
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
        st_slot(a.at.wnodes + rn.parent, rn.slot, lo, hi);
        node = rn.parent;
    }
}

// One workgroup per cover sphere g: positions [g n / G, (g + 1) n / G) of the triangle order (cover_kernel's ranges; contiguous
// in either builder's order, hence compact).  Any spheres that together contain every triangle serve classify_kernel.
__global__ __launch_bounds__(kThreadsRefit) void refit_bounds_kernel(Args a) {
    __shared__ double part[4 * 6];
    const int G = a.n_cover > 0 ? a.n_cover : 1, g = blockIdx.x, n = a.n;
    const int b = (int)((long long)g * n / G), e = (int)((long long)(g + 1) * n / G);
    double mc[3];  // the centre of the mesh's vertex box, complete by now: refit_tris_kernel ran before
    for (int k = 0; k < 3; k++) mc[k] = 0.5 * (-dunkey(a.keys[KEY_NEG_LO + k]) + dunkey(a.keys[KEY_HI + k]));
    double c[3], r2[2];
    range_sphere(a.tri9, reinterpret_cast<const int *>(a.srcrec), 2, b, e, mc, part, c, r2);
    if (threadIdx.x != 0) return;
    if (g < a.n_cover) store_cover(a.at.cover + 4 * (size_t)g, c, r2[0], e > b, mc);
    atomicMax(a.keys + KEY_R2, dkey(r2[1]));
}

// the bounding sphere and the coordinate bound by the builders' formulas (cgrt_build.h), written where the kernels read them
__global__ void refit_finish_kernel(Args a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int k = 0; k < 3; k++) a.at.obj->a[k] = 0.5 * (-dunkey(a.keys[KEY_NEG_LO + k]) + dunkey(a.keys[KEY_HI + k]));
    a.at.obj->s0 = sphere_s0(cover_radius(dunkey(a.keys[KEY_R2])));
    a.at.tree->bmax = tree_bmax(dunkey(a.keys[KEY_MAX_ABS]));
}

}  // namespace refit

// ---- host side ---------------------------------------------------------------------------------------------------------

// The plan of tree t: from the host's records (a host-built tree, committed or not) or from the device's
static int tree_refit_plan(const cgrt_scene *s, int t, RefitPlan &plan) {
    const HostTree &T = s->host.trees[(size_t)t];
    std::vector<WideNodeRec> wide_dev;
    std::vector<OTriRec> ot_dev;
    if (T.dev_kind == 1 && !s->committed) return fail(CGRT_ERR_INVALID, "refit plan: a device-built tree exists only after the commit");
    const bool dev = tree_lives_on_device(s, t);
    if (dev)
        if (const int rc = read_device_tree(s, t, &wide_dev, &ot_dev)) return rc;
    const std::vector<WideNodeRec> &wide = dev ? wide_dev : T.wide;
    std::vector<int32_t> k;
    for (const OTriRec &o : dev ? ot_dev : T.otris) k.push_back(o.k);
    if (T.dev_kind != 1 && k.size() != T.leaf_ids.size()) return fail(CGRT_ERR_INVALID, "refit plan: the tree has no triangle-level hierarchy");
    try {
        if (const char *bad = refit_plan(wide.data(), (int32_t)wide.size(), k.data(), (int32_t)k.size(), T.dev_kind == 1 ? nullptr : T.leaf_ids.data(), plan))
            return fail(CGRT_ERR_INVALID, bad);
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string("refit plan: ") + e.what());
    }
    plan.cover_first = (int32_t)T.cover_first;
    plan.n_cover = T.cover_n;
    return CGRT_OK;
}

// The first refit of a mesh, or the first after a rebuild: its plan, and the plan's device copy in front of the words every
// refit clears
static int refit_prepare(cgrt_scene *s, MeshEdit &ed, int t) {
    if (ed.plan) return CGRT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<RefitPlanDev> st(new (std::nothrow) RefitPlanDev());
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
    ed.ms_plan = ms_since(t0);
    ed.plan = std::move(st);
    return CGRT_OK;
}

// tri9: DEVICE pointer.  Everything behind the first call's plan is enqueued on st.
static int refit_launch(cgrt_scene *s, const MeshTarget &m, const double *tri9, hipStream_t st) {
    MeshEdit &ed = s->edits[m.obj];
    if (const int rc = refit_prepare(s, ed, m.tree)) return rc;
    const RefitPlanDev &rs = *ed.plan;
    const TreeRec &tr = s->tree_recs[(size_t)m.tree];
    refit::Args a;
    a.tri9 = tri9;
    a.n = tr.ntris;
    a.nwide = tr.nwide;
    a.srcrec = rs.srcrec;
    a.nodes = rs.nodes;
    a.at = m.at;
    a.keys = rs.keys;
    a.arrive = rs.arrive;
    a.n_cover = rs.plan.n_cover;
    const int T = refit::kThreadsRefit;
    HIP_TRY(hipMemsetAsync(rs.mem.p, 0, rs.clear_bytes, st));
    hipLaunchKernelGGL(refit::refit_tris_kernel, dim3((unsigned)((a.n + T - 1) / T)), dim3(T), 0, st, a);
    hipLaunchKernelGGL(refit::refit_nodes_kernel, dim3((unsigned)((a.nwide + T - 1) / T)), dim3(T), 0, st, a);
    hipLaunchKernelGGL(refit::refit_bounds_kernel, dim3((unsigned)std::max(a.n_cover, 1)), dim3(T), 0, st, a);
    hipLaunchKernelGGL(refit::refit_finish_kernel, dim3(1), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    ed.refits++;
    s->geometry_gen++;
    s->host.trees[(size_t)m.tree].refitted = true;  // the reference's tree over the old vertices describes nothing any more
    return CGRT_OK;
}

// The bounds the device holds for the mesh now, as a build's result: what the topology fixes comes from the handle
static int read_mesh_bounds(const cgrt_scene *s, const MeshTarget &m, devbuild::MeshResult &mr) {
    const HostTree &T = s->host.trees[(size_t)m.tree];
    ObjRec o;
    TreeRec tr;
    HIP_TRY(hipMemcpy(&o, m.at.obj, sizeof(o), hipMemcpyDeviceToHost));  // synchronises
    HIP_TRY(hipMemcpy(&tr, m.at.tree, sizeof(tr), hipMemcpyDeviceToHost));
    mr.nwide = tr.nwide;
    mr.stack_need = T.wide_stack;
    mr.balanced = T.dev_balanced;
    for (int k = 0; k < 3; k++) mr.centre[k] = o.a[k];
    mr.r2 = o.s0;
    mr.bmax = tr.bmax;
    mr.cover.resize((size_t)T.cover_n * 4);
    if (T.cover_n > 0) HIP_TRY(hipMemcpy(mr.cover.data(), m.at.cover, mr.cover.size() * sizeof(double), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

extern "C" {

int cgrt_scene_refit_mesh(cgrt_scene *s, int obj, const double *tri9, int ntri, void *stream) {
    MeshTarget m;
    if (const int rc = vertex_target(s, obj, tri9, ntri, "refit", m)) return rc;
    if (m.empty) return CGRT_OK;
    ON_DEVICE(s->device);
    return refit_launch(s, m, tri9, reinterpret_cast<hipStream_t>(stream));
}

int cgrt_scene_refit_mesh_host(cgrt_scene *s, int obj, const double *tri9, int ntri) {
    MeshTarget m;
    if (const int rc = vertex_target(s, obj, tri9, ntri, "refit", m)) return rc;
    if (m.empty) return CGRT_OK;
    ON_DEVICE(s->device);
    HostStage hs;
    const double *d = hs.in(tri9, (size_t)ntri * 9 * sizeof(double));
    if (hs.error()) return hs.error();
    if (const int rc = hs.finish(refit_launch(s, m, d, 0))) return rc;
    devbuild::MeshResult mr;  // the host mirrors of what the device now owns
    if (const int rc = read_mesh_bounds(s, m, mr)) return rc;
    HostTree &T = s->host.trees[(size_t)m.tree];
    apply_mesh_result(s->host, T, s->tree_recs[(size_t)m.tree], obj, mr);
    return keep_vertices(T, tri9, ntri, "refit");
}

int cgrt_scene_refit_info(const cgrt_scene *s, int obj, cgrt_refit_info *out) {
    if (!s || !out) return fail(CGRT_ERR_INVALID, "null argument");
    const int t = info_tree(s, obj);
    if (t < 0) return fail(CGRT_ERR_INVALID, "refit info: the object is no mesh");
    const HostTree &T = s->host.trees[(size_t)t];
    std::memset(out, 0, sizeof(*out));
    if (s->committed) {
        out->nwide = s->tree_recs[(size_t)t].nwide;
        out->ntris = s->tree_recs[(size_t)t].ntris;
    } else {
        out->nwide = (int32_t)T.wide.size();
        out->ntris = T.dev_kind ? (int32_t)T.dev_ntri : (int32_t)(T.tri9.size() / 9);
    }
    const auto it = s->edits.find(obj);
    if (it != s->edits.end()) {
        out->refits = it->second.refits;
        out->plan_built = it->second.plan ? 1 : 0;
        out->ms_plan = it->second.ms_plan;
    }
    out->geometry_gen = s->geometry_gen;
    return CGRT_OK;
}

int cgrt_scene_mesh_bounds_host(const cgrt_scene *s, int obj, double centre3[3], double *s0, float *bmax, double *cover4, int32_t cap,
                                int32_t *n_cover) {
    MeshTarget m;
    if (const int rc = walk_target(s, obj, "bounds", m)) return rc;
    const int n = s->host.trees[(size_t)m.tree].cover_n;
    if (n_cover) *n_cover = n;
    if (cover4 && cap < n) return fail(CGRT_ERR_INVALID, "bounds: room for fewer cover spheres than the mesh has (" + std::to_string(n) + ")");
    ON_DEVICE(s->device);
    devbuild::MeshResult mr;
    if (const int rc = read_mesh_bounds(s, m, mr)) return rc;
    if (centre3) std::copy(mr.centre, mr.centre + 3, centre3);
    if (s0) *s0 = mr.r2;
    if (bmax) *bmax = mr.bmax;
    if (cover4) std::copy(mr.cover.begin(), mr.cover.end(), cover4);
    return CGRT_OK;
}

int cgrt_scene_refit_plan_host(const cgrt_scene *s, int tree, int32_t *nwide, int32_t *ntris, int32_t *parent, int32_t *slot,
                               int32_t *arrivals, int32_t *src) {
    if (!s || tree < 0 || tree >= (int)s->host.trees.size()) return fail(CGRT_ERR_INVALID, "bad tree index");
    const HostTree &T = s->host.trees[(size_t)tree];
    const bool dev = T.dev_kind == 1, sizing = !parent && !slot && !arrivals && !src;
    const bool wide = dev ? (s->committed && s->tree_recs[(size_t)tree].nwide > 0) : (T.tri_level && !T.wide.empty());
    if (!wide || sizing) {  // no 4-wide hierarchy: nothing to plan (as cgrt_scene_wide_dump reports no node); or the sizing call
        if (nwide) *nwide = !wide ? 0 : dev ? s->tree_recs[(size_t)tree].nwide : (int32_t)T.wide.size();
        if (ntris) *ntris = !wide ? 0 : dev ? s->tree_recs[(size_t)tree].ntris : (int32_t)T.otris.size();
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
