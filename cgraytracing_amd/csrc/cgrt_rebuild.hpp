// cgrt_scene_rebuild_mesh: a new hierarchy for a committed, device-built OPAQUE mesh, in place.
// Included by cgrt_hip.hip.  The builder is the commit's (cgrt_devbuild.hpp build_mesh_core), run on the caller's stream with a
// scratch the handle keeps: it writes triangle records, hierarchy-order records and wide nodes into STAGING arrays of that
// scratch; only once the host has seen the node count and a stack bound below kWideStack are they put in place --
// device-to-device copies on the stream and rebuild_finish_kernel, which writes ObjRec::a / s0 and TreeRec::bmax / nwide with
// the values the commit would have uploaded.  An error return before that leaves the committed scene as it was.
//
// Parity class: that of CGRT_BUILD_DEVICE (cgrt.h): the tree is the one a fresh device-build commit of these vertices gets, up
// to the numbering of wide nodes inside a level.
#ifndef CGRT_REBUILD_HPP
#define CGRT_REBUILD_HPP

namespace rebuild {

struct Finish {
    ObjRec *obj;
    TreeRec *tree;
    double centre[3], s0;
    float bmax;
    int32_t nwide;
};
// the host's own doubles (MeshResult), so the records equal a fresh commit's bit for bit
__global__ void rebuild_finish_kernel(Finish f) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int k = 0; k < 3; k++) f.obj->a[k] = f.centre[k];
    f.obj->s0 = f.s0;
    f.tree->bmax = f.bmax;
    f.tree->nwide = f.nwide;
}

}  // namespace rebuild

// refit_check's refusals, then the rebuild's own: all before any device is touched
static int rebuild_check(const cgrt_scene *s, int obj, const double *tri9, int ntri, int *tree) {
    if (const int rc = refit_check(s, obj, tri9, ntri, tree, "rebuild")) return rc;
    if (*tree < 0) return CGRT_OK;
    const HostTree &T = s->host.trees[(size_t)*tree];
    if (T.dev_kind != 1)
        return fail(CGRT_ERR_INVALID, "rebuild: the mesh's tree was built on the host (its arrays have room for that topology only): commit the scene "
                                      "under CGRT_BUILD_DEVICE");
    // the cover spheres' count depends on ntri alone: the mesh's slice of cover[] keeps its size
    if (T.cover_n != devbuild::cover_groups(ntri) || (size_t)T.cover_first + (size_t)T.cover_n > (size_t)s->dev.n_cover)
        return fail(CGRT_ERR_INVALID, "rebuild: the mesh's cover spheres are not the " + std::to_string(devbuild::cover_groups(ntri)) + " its triangle count gives");
    return CGRT_OK;
}

// tri9: DEVICE pointer.  Enqueues on st and synchronises it.
static int rebuild_launch(cgrt_scene *s, int obj, int t, const double *tri9, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    HostScene &H = s->host;
    HostTree &T = H.trees[(size_t)t];
    TreeRec &tr = s->tree_recs[(size_t)t];
    const int n = tr.ntris;
    RebuildState *rs = nullptr;
    auto it = s->rebuild.find(obj);
    if (it != s->rebuild.end()) {
        rs = it->second.get();
    } else {  // the mesh's first rebuild: its scratch
        std::unique_ptr<RebuildState> fresh(new (std::nothrow) RebuildState());
        if (!fresh) return fail(CGRT_ERR_LIMIT, "out of host memory");
        if (const int rc = fresh->scratch.alloc(n, false, true)) return rc;
        rs = fresh.get();
        s->rebuild[obj] = std::move(fresh);
    }
    devbuild::MeshScratch &S = rs->scratch;
    devbuild::MeshResult mr;
    if (const int rc = devbuild::build_mesh_core(tri9, n, st, S, S.tris, S.otris, S.wnodes, mr)) return rc;  // (the scene is untouched)
    if (mr.nwide < 1 || mr.nwide > n || (int)(mr.cover.size() / 4) != T.cover_n) return fail(CGRT_ERR_DEVICE, "rebuild: the builder's counts are out of range");
    // in place
    const size_t N = (size_t)n;
    HIP_TRY(hipMemcpyAsync(const_cast<TriRec *>(s->dev.tris) + tr.tri_begin, S.tris, N * sizeof(TriRec), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(const_cast<OTriRec *>(s->dev.otris) + tr.otri_begin, S.otris, N * sizeof(OTriRec), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(const_cast<WideNodeRec *>(s->dev.wnodes) + tr.wnode_begin, S.wnodes, (size_t)mr.nwide * sizeof(WideNodeRec),
                           hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(s->dev.cover) + 4 * T.cover_first, S.cover, mr.cover.size() * sizeof(double), hipMemcpyDeviceToDevice, st));
    rebuild::Finish f;
    f.obj = const_cast<ObjRec *>(s->dev.objs) + obj;
    f.tree = const_cast<TreeRec *>(s->dev.trees) + t;
    for (int k = 0; k < 3; k++) f.centre[k] = mr.centre[k];
    f.s0 = mr.r2;
    f.bmax = tree_bmax(mr.bmax);
    f.nwide = mr.nwide;
    hipLaunchKernelGGL(rebuild::rebuild_finish_kernel, dim3(1), dim3(64), 0, st, f);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    // the handle's state
    tr.nwide = mr.nwide;
    tr.bmax = f.bmax;
    T.dev_nwide = mr.nwide;
    T.wide_stack = mr.stack_need;
    T.dev_balanced = mr.balanced;
    ObjRec &ob = H.objs[(size_t)obj];
    for (int k = 0; k < 3; k++) ob.a[k] = mr.centre[k];
    ob.s0 = mr.r2;
    std::copy(mr.cover.begin(), mr.cover.end(), H.cover.begin() + (std::ptrdiff_t)(4 * T.cover_first));
    auto rf = s->refit.find(obj);
    if (rf != s->refit.end() && !rf->second->stale) {  // the plan describes the old topology
        RefitState &old = *rf->second;
        if (void *p = old.mem.release()) (void)hipFree(p);
        old.bytes = old.clear_bytes = 0;
        old.keys = nullptr;
        old.arrive = nullptr;
        old.nodes = nullptr;
        old.srcrec = nullptr;
        old.plan = RefitPlan();
        old.stale = true;
    }
    s->geometry_gen++;
    rs->rebuilds++;
    rs->balanced = mr.balanced ? 1 : 0;
    rs->levels = mr.levels;
    rs->readbacks = mr.readbacks;
    rs->ms_last = ms_since(t0);
    return CGRT_OK;
}

extern "C" {

int cgrt_scene_rebuild_mesh(cgrt_scene *s, int obj, const double *tri9_dev, int ntri, void *stream) {
    int t = -1;
    if (const int rc = rebuild_check(s, obj, tri9_dev, ntri, &t)) return rc;
    if (t < 0) return CGRT_OK;
    ON_DEVICE(s->device);
    return rebuild_launch(s, obj, t, tri9_dev, reinterpret_cast<hipStream_t>(stream));
}

int cgrt_scene_rebuild_mesh_host(cgrt_scene *s, int obj, const double *tri9, int ntri) {
    int t = -1;
    if (const int rc = rebuild_check(s, obj, tri9, ntri, &t)) return rc;
    if (t < 0) return CGRT_OK;
    ON_DEVICE(s->device);
    const size_t bytes = (size_t)ntri * 9 * sizeof(double);
    DevBuf d;
    HIP_TRY(d.alloc(bytes));
    HIP_TRY(hipMemcpy(d.p, tri9, bytes, hipMemcpyHostToDevice));
    if (const int rc = rebuild_launch(s, obj, t, d.as<double>(), 0)) return rc;
    try {
        s->host.trees[(size_t)t].tri9.assign(tri9, tri9 + (size_t)ntri * 9);
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string("rebuild: ") + e.what());
    }
    return CGRT_OK;
}

int cgrt_scene_rebuild_info(const cgrt_scene *s, int obj, cgrt_rebuild_info *out) {
    if (!s || !out) return fail(CGRT_ERR_INVALID, "null argument");
    if (obj < 0 || obj >= (int)s->host.objs.size() || s->host.objs[(size_t)obj].kind != KIND_MESH || s->host.objs[(size_t)obj].tree < 0)
        return fail(CGRT_ERR_INVALID, "rebuild info: the object is no mesh");
    const int t = s->host.objs[(size_t)obj].tree;
    const HostTree &T = s->host.trees[(size_t)t];
    std::memset(out, 0, sizeof(*out));
    out->nwide = s->committed ? s->tree_recs[(size_t)t].nwide : (int32_t)T.wide.size();
    out->stack_need = T.wide_stack;
    out->balanced = T.dev_balanced ? 1 : 0;
    const auto it = s->rebuild.find(obj);
    if (it != s->rebuild.end()) {
        const RebuildState &r = *it->second;
        out->rebuilds = r.rebuilds;
        out->balanced = r.balanced;
        out->levels = r.levels;
        out->readbacks = r.readbacks;
        out->ms_last = r.ms_last;
        out->scratch_bytes = (int64_t)r.scratch.bytes;
    }
    return CGRT_OK;
}

}  // extern "C"

#endif
