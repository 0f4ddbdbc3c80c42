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

// the builder's own values (MeshResult), so the records equal a fresh commit's bit for bit
__global__ void rebuild_finish_kernel(MeshSlots at, double cx, double cy, double cz, double s0, float bmax, int32_t nwide) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    at.obj->a[0] = cx;
    at.obj->a[1] = cy;
    at.obj->a[2] = cz;
    at.obj->s0 = s0;
    at.tree->bmax = bmax;
    at.tree->nwide = nwide;
}

}  // namespace rebuild

// vertex_target's refusals, then the rebuild's own: all before any device is touched
static int rebuild_target(const cgrt_scene *s, int obj, const double *tri9, int ntri, MeshTarget &m) {
    if (const int rc = vertex_target(s, obj, tri9, ntri, "rebuild", m)) return rc;
    if (m.empty) return CGRT_OK;
    const HostTree &T = s->host.trees[(size_t)m.tree];
    if (T.dev_kind != 1)
        return fail(CGRT_ERR_INVALID, "rebuild: the mesh's tree was built on the host (its arrays have room for that topology only): commit the scene "
                                      "under CGRT_BUILD_DEVICE");
    // the cover spheres' count depends on ntri alone: the mesh's slice of cover[] keeps its size
    if (T.cover_n != devbuild::cover_groups(ntri) || (size_t)T.cover_first + (size_t)T.cover_n > (size_t)s->dev.n_cover)
        return fail(CGRT_ERR_INVALID, "rebuild: the mesh's cover spheres are not the " + std::to_string(devbuild::cover_groups(ntri)) + " its triangle count gives");
    return CGRT_OK;
}

// tri9: DEVICE pointer.  Enqueues on st and synchronises it.
static int rebuild_launch(cgrt_scene *s, const MeshTarget &m, const double *tri9, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    HostTree &T = s->host.trees[(size_t)m.tree];
    TreeRec &tr = s->tree_recs[(size_t)m.tree];
    const int n = tr.ntris;
    MeshEdit &ed = s->edits[m.obj];
    devbuild::MeshScratch &S = ed.scratch;
    if (!S.bytes)  // the mesh's first rebuild: its scratch
        if (const int rc = S.alloc(n, false, true)) return rc;
    devbuild::MeshResult mr;
    if (const int rc = devbuild::build_mesh_core(tri9, n, st, S, S.tris, S.otris, S.wnodes, mr)) return rc;  // (the scene is untouched)
    if (mr.nwide < 1 || mr.nwide > n || (int)(mr.cover.size() / 4) != T.cover_n) return fail(CGRT_ERR_DEVICE, "rebuild: the builder's counts are out of range");
    // in place
    const size_t N = (size_t)n;
    HIP_TRY(hipMemcpyAsync(m.at.tris, S.tris, N * sizeof(TriRec), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(m.at.otris, S.otris, N * sizeof(OTriRec), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(m.at.wnodes, S.wnodes, (size_t)mr.nwide * sizeof(WideNodeRec), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(m.at.cover, S.cover, mr.cover.size() * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(rebuild::rebuild_finish_kernel, dim3(1), dim3(64), 0, st, m.at, mr.centre[0], mr.centre[1], mr.centre[2], mr.r2, mr.bmax,
                       (int32_t)mr.nwide);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    apply_mesh_result(s->host, T, tr, m.obj, mr);
    ed.plan.reset();  // it describes the old topology: the next refit builds it again
    s->geometry_gen++;
    ed.rebuilds++;
    ed.balanced = mr.balanced ? 1 : 0;
    ed.levels = mr.levels;
    ed.readbacks = mr.readbacks;
    ed.ms_last = ms_since(t0);
    return CGRT_OK;
}

extern "C" {

int cgrt_scene_rebuild_mesh(cgrt_scene *s, int obj, const double *tri9_dev, int ntri, void *stream) {
    MeshTarget m;
    if (const int rc = rebuild_target(s, obj, tri9_dev, ntri, m)) return rc;
    if (m.empty) return CGRT_OK;
    ON_DEVICE(s->device);
    return rebuild_launch(s, m, tri9_dev, reinterpret_cast<hipStream_t>(stream));
}

int cgrt_scene_rebuild_mesh_host(cgrt_scene *s, int obj, const double *tri9, int ntri) {
    MeshTarget m;
    if (const int rc = rebuild_target(s, obj, tri9, ntri, m)) return rc;
    if (m.empty) return CGRT_OK;
    ON_DEVICE(s->device);
    HostStage hs;
    const double *d = hs.in(tri9, (size_t)ntri * 9 * sizeof(double));
    if (hs.error()) return hs.error();
    if (const int rc = rebuild_launch(s, m, d, 0)) return rc;
    return keep_vertices(s->host.trees[(size_t)m.tree], tri9, ntri, "rebuild");
}

int cgrt_scene_rebuild_info(const cgrt_scene *s, int obj, cgrt_rebuild_info *out) {
    if (!s || !out) return fail(CGRT_ERR_INVALID, "null argument");
    const int t = info_tree(s, obj);
    if (t < 0) return fail(CGRT_ERR_INVALID, "rebuild info: the object is no mesh");
    const HostTree &T = s->host.trees[(size_t)t];
    std::memset(out, 0, sizeof(*out));
    out->nwide = s->committed ? s->tree_recs[(size_t)t].nwide : (int32_t)T.wide.size();
    out->stack_need = T.wide_stack;
    out->balanced = T.dev_balanced ? 1 : 0;
    const auto it = s->edits.find(obj);
    if (it != s->edits.end() && it->second.scratch.bytes) {  // (it has been rebuilt, or tried)
        const MeshEdit &r = it->second;
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
