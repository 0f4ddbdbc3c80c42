// The one host path of everything that writes, or reads back, a committed mesh's device records (DESIGN.md sections 16, 17): the
// commit's device build (cgrt_hip.hip device_builds), the refit (cgrt_refit.hpp), the rebuild (cgrt_rebuild.hpp), the tree cost
// (cgrt_tree_cost.hpp) and the verification dumps.  Included by cgrt_hip.hip behind cgrt_scene.
#ifndef CGRT_MESH_EDIT_HPP
#define CGRT_MESH_EDIT_HPP

static const char *const kRefitStale = "the scene was refitted after this session was created";

struct MeshSlots {
    TriRec *tris = nullptr;  // the tree's first record of each array
    OTriRec *otris = nullptr;
    WideNodeRec *wnodes = nullptr;
    ObjRec *obj = nullptr;  // the records themselves (null until the commit has uploaded them)
    TreeRec *tree = nullptr;
    double *cover = nullptr;  // the mesh's first cover sphere (4 doubles each)
};
static MeshSlots mesh_slots(const DeviceScene &d, const TreeRec &tr, int obj, int t, size_t cover_first) {
    MeshSlots m;
    m.tris = const_cast<TriRec *>(d.tris) + tr.tri_begin;
    m.otris = const_cast<OTriRec *>(d.otris) + tr.otri_begin;
    m.wnodes = const_cast<WideNodeRec *>(d.wnodes) + tr.wnode_begin;
    if (d.objs) m.obj = const_cast<ObjRec *>(d.objs) + obj;
    if (d.trees) m.tree = const_cast<TreeRec *>(d.trees) + t;
    if (d.cover) m.cover = const_cast<double *>(d.cover) + 4 * cover_first;
    return m;
}

struct MeshTarget {
    int obj = -1, tree = -1;
    bool empty = false;  // a mesh without a triangle: accepted, nothing to do
    MeshSlots at;
};

// `who` names the entry in every message ("refit", "rebuild", "cost", "bounds"); all of this before any device is touched
static int mesh_target(const cgrt_scene *s, int obj, const std::string &who, MeshTarget &out) {
    out = MeshTarget();
    if (!s) return fail(CGRT_ERR_INVALID, who + ": null scene");
    if (!s->committed) return fail(CGRT_ERR_INVALID, who + ": scene not committed");
    if (obj < 0 || obj >= (int)s->host.objs.size()) return fail(CGRT_ERR_INVALID, who + ": no such object");
    const ObjRec &o = s->host.objs[(size_t)obj];
    if (o.kind == KIND_SPHERE) return fail(CGRT_ERR_INVALID, who + ": the object is a sphere, not a mesh");
    if (o.kind == KIND_BEZIER) return fail(CGRT_ERR_INVALID, who + ": the object is a Bezier surface, not a mesh");
    if (o.kind == KIND_PLANE)
        return fail(CGRT_ERR_INVALID, o.tree >= 0 ? who + ": the object is a bump floor, not a mesh" : who + ": the object is a plane, not a mesh");
    if (o.kind != KIND_MESH || o.tree < 0 || o.tree >= (int)s->tree_recs.size()) return fail(CGRT_ERR_INVALID, who + ": the object is no mesh");
    out.obj = obj;
    out.tree = o.tree;
    out.empty = s->tree_recs[(size_t)o.tree].ntris == 0;
    out.at = mesh_slots(s->dev, s->tree_recs[(size_t)o.tree], obj, o.tree, s->host.trees[(size_t)o.tree].cover_first);
    return CGRT_OK;
}
// the refusals only some entries have: each names what the entry cannot do with a transparent mesh itself
static int need_opaque(const cgrt_scene *s, const MeshTarget &m, const std::string &why) {
    return s->host.objs[(size_t)m.obj].transp < kEps ? CGRT_OK : fail(CGRT_ERR_INVALID, why);
}
static int need_ntri(const cgrt_scene *s, const MeshTarget &m, const std::string &who, int ntri) {
    const int have = s->tree_recs[(size_t)m.tree].ntris;
    return ntri == have ? CGRT_OK : fail(CGRT_ERR_INVALID, who + ": ntri is not the mesh's triangle count (" + std::to_string(have) + ")");
}
static int need_wide(const cgrt_scene *s, const MeshTarget &m, const std::string &who) {
    const TreeRec &tr = s->tree_recs[(size_t)m.tree];
    return tr.tri_level && tr.nwide > 0 ? CGRT_OK : fail(CGRT_ERR_INVALID, who + ": the tree has no 4-wide hierarchy (CGRT_TREE=ref)");
}
// an entry that takes new vertices (refit, rebuild) ...
static int vertex_target(const cgrt_scene *s, int obj, const double *tri9, int ntri, const std::string &who, MeshTarget &m) {
    if (const int rc = mesh_target(s, obj, who, m)) return rc;
    if (const int rc = need_opaque(s, m, who + ": the mesh is transparent (its improvement counter makes the leaf order observable, quirk Q5)")) return rc;
    if (const int rc = need_ntri(s, m, who, ntri)) return rc;
    if (m.empty) return CGRT_OK;
    if (const int rc = need_wide(s, m, who)) return rc;
    return tri9 ? CGRT_OK : fail(CGRT_ERR_INVALID, who + ": null tri9");
}
// ... and one that reads what the device walks (cost, bounds)
static int walk_target(const cgrt_scene *s, int obj, const std::string &who, MeshTarget &m) {
    if (const int rc = mesh_target(s, obj, who, m)) return rc;
    if (const int rc = need_opaque(s, m, who + ": the mesh is transparent: its tree has no 4-wide hierarchy")) return rc;
    return m.empty ? CGRT_OK : need_wide(s, m, who);
}

// What a build of tree T (owned by object obj, records tr) left on the device, into the handle's mirrors; the mesh's slice of
// H.cover has its room already.
static void apply_mesh_result(HostScene &H, HostTree &T, TreeRec &tr, int obj, const devbuild::MeshResult &mr) {
    tr.nwide = mr.nwide;
    tr.bmax = mr.bmax;
    T.dev_nwide = mr.nwide;
    T.wide_stack = mr.stack_need;
    T.dev_balanced = mr.balanced;
    ObjRec &ob = H.objs[(size_t)obj];
    for (int k = 0; k < 3; k++) ob.a[k] = mr.centre[k];
    ob.s0 = mr.r2;
    std::copy(mr.cover.begin(), mr.cover.end(), H.cover.begin() + (std::ptrdiff_t)(4 * T.cover_first));
}

// The device owns tree t's hierarchy: built there (row f3) or refitted there
static bool tree_lives_on_device(const cgrt_scene *s, int t) {
    return s->committed && (s->host.trees[(size_t)t].dev_kind == 1 || s->host.trees[(size_t)t].refitted);
}
// ... its wide nodes and / or hierarchy-order records, read back (synchronises)
static int read_device_tree(const cgrt_scene *s, int t, std::vector<WideNodeRec> *wide, std::vector<OTriRec> *otris) {
    ON_DEVICE(s->device);
    const TreeRec &tr = s->tree_recs[(size_t)t];
    if (wide) wide->resize((size_t)std::max(tr.nwide, 0));
    if (wide && !wide->empty()) HIP_TRY(hipMemcpy(wide->data(), s->dev.wnodes + tr.wnode_begin, wide->size() * sizeof(WideNodeRec), hipMemcpyDeviceToHost));
    if (otris) otris->resize((size_t)std::max(tr.ntris, 0));
    if (otris && !otris->empty()) HIP_TRY(hipMemcpy(otris->data(), s->dev.otris + tr.otri_begin, otris->size() * sizeof(OTriRec), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

static int keep_vertices(HostTree &T, const double *tri9, int ntri, const char *who) {
    try {
        T.tri9.assign(tri9, tri9 + (size_t)ntri * 9);
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string(who) + ": " + e.what());
    }
    return CGRT_OK;
}

// the "is this object a mesh" of the two *_info entries, which also serve an uncommitted scene: its tree, or -1
static int info_tree(const cgrt_scene *s, int obj) {
    if (obj < 0 || obj >= (int)s->host.objs.size() || s->host.objs[(size_t)obj].kind != KIND_MESH) return -1;
    return s->host.objs[(size_t)obj].tree < 0 ? -1 : s->host.objs[(size_t)obj].tree;
}

#endif
