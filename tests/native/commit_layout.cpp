// The host side of cgrt_scene_commit (cgrt_build.cpp: commit_knobs, scene_layout, scene_traits) on scenes built through
// HostScene::add_*: record placement and the DeviceScene fields that select kernel variants, against values written out by
// hand from the rules.  CPU build under ASan + UBSan, driven by tests/test_commit_layout_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cgrt_build.h"

using namespace cgrt;

static int g_failed = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        if (a_ != b_) {                                                                                         \
            std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)

static const double kGrey[3] = {0.5, 0.5, 0.5};

static int sphere(HostScene &H, double x, double refl = 0, double transp = 0) {
    const double c[3] = {x, 0, 20};
    return H.add_sphere(c, 1.0, kGrey, refl, transp);
}
// floor, ceiling, left, right and back wall: exactly axis-aligned, diffuse, no texture
static void room(HostScene &H, int n = 5) {
    const double p[5][3] = {{0, -4, 0}, {0, 6, 0}, {-8, 0, 0}, {8, 0, 0}, {0, 0, 40}};
    const double nrm[5][3] = {{0, 1, 0}, {0, -1, 0}, {1, 0, 0}, {-1, 0, 0}, {0, 0, -1}};
    for (int i = 0; i < n; i++) H.add_plane(p[i], nrm[i], kGrey, 0, 0, -1);
}
// a bump-mapped floor over a 12 x 15 texture: 4 x 3 grid cells, 24 triangles
static constexpr int kFloorCells = 12, kFloorTris = 24;
static int bump_floor(HostScene &H) {
    std::vector<uint8_t> rgb(12 * 15 * 3);
    for (size_t k = 0; k < rgb.size(); k++) rgb[k] = (uint8_t)(k * 37u & 255u);
    const double n[3] = {0, 1, 0}, p[3] = {-21, 0, 0}, at[3] = {0, -5, 0};
    const int t = H.add_texture(rgb.data(), 12, 15, n, p, 42, 40, 1);
    return H.add_plane(at, n, kGrey, 0, 0, t);
}
// a 6 x 6 quad patch in the plane z = 30 (72 triangles, largest |coordinate| 30)
static constexpr int kMeshTris = 72;
static int mesh(HostScene &H, double transp) {
    std::vector<double> t9;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            const double a[3] = {i - 3.0, j - 3.0, 30}, b[3] = {i - 2.0, j - 3.0, 30}, c[3] = {i - 3.0, j - 2.0, 30},
                         d[3] = {i - 2.0, j - 2.0, 30};
            for (const double *v : {a, b, c, d, b, c}) t9.insert(t9.end(), v, v + 3);
        }
    return H.add_mesh_triangles(t9.data(), kMeshTris, kGrey, 0.0, transp, 0);
}
static int bezier(HostScene &H) {
    const double cp[4 * 3] = {0, 0, 0.5, 0, 0.5, 1.0, 0, 1.0, 0.8, 0, 1.5, 0.2}, pos[3] = {3, -4, 25};
    return H.add_bezier(cp, 4, pos, kGrey, 0, 0);
}

static DeviceScene traits(const HostScene &H, const SceneLayout &L, const CommitKnobs &k = CommitKnobs()) {
    DeviceScene d{};
    scene_traits(H, L.trees, k, d);
    return d;
}

static void diffuse_spheres() {
    HostScene H;
    for (int i = 0; i < 4; i++) sphere(H, 3.0 * i);
    const SceneLayout L = scene_layout(H, CommitKnobs());
    CHECK_EQ(L.trees.size(), 0);
    const DeviceScene d = traits(H, L);
    CHECK_EQ(d.n_objs, 4);
    CHECK_EQ(d.n_lds, 4);
    CHECK_EQ(d.all_spheres, 1);
    CHECK_EQ(d.single_ray, 1);
    CHECK_EQ(d.light_ok, 0);
    CHECK_EQ(d.has_glass, 0);
    CHECK_EQ(d.has_mesh, 0);
    CHECK_EQ(d.has_wide, 0);
    CHECK_EQ(d.prim_obj, -1);
    CHECK_EQ(d.cached_tree, -1);
    CHECK_EQ(d.prun_end, 0);
}

static void plane_run() {
    {   // planes first: the run is all five
        HostScene H;
        room(H);
        sphere(H, 0);
        const DeviceScene d = traits(H, scene_layout(H, CommitKnobs()));
        CHECK_EQ(d.all_spheres, 0);
        CHECK_EQ(d.single_ray, 1);
        CHECK_EQ(d.prun_begin, 0);
        CHECK_EQ(d.prun_end, 5);
        CommitKnobs off;
        off.no_plane_run = true;
        CHECK_EQ(traits(H, scene_layout(H, off), off).prun_end, 0);
    }
    {   // a bump floor in front of the run; a sphere in front: no run
        HostScene H;
        bump_floor(H);
        room(H, 3);
        sphere(H, 0);
        const SceneLayout L = scene_layout(H, CommitKnobs());
        const DeviceScene d = traits(H, L);
        CHECK_EQ(d.prun_begin, 1);
        CHECK_EQ(d.prun_end, 4);
        CHECK_EQ(d.single_ray, 1);
        CHECK_EQ(d.light_trees, 1);
        CHECK_EQ(d.light_hf_only, 1);
        CHECK_EQ(L.trees[0].hfield, 0);  // an opaque floor is walked as a grid: no node array
        CHECK_EQ(L.trees[0].nnodes, 0);
        CHECK_EQ(L.hcells.size(), kFloorCells);
        CHECK_EQ(L.hcell_y.size(), kFloorCells);
        CHECK_EQ(L.texels.size(), 12 * 15 * 3);
        CHECK_EQ(L.texs[0].isbump, 1);
        HostScene S;
        sphere(S, 0);
        room(S);
        CHECK_EQ(traits(S, scene_layout(S, CommitKnobs())).prun_end, 0);
    }
}

static void opaque_mesh(bool with_floor) {
    HostScene H;
    if (with_floor) bump_floor(H);
    room(H);
    const int m = mesh(H, 0.0);
    sphere(H, 4.0, 0.9, 0.0);  // mirror
    const SceneLayout L = scene_layout(H, CommitKnobs());
    const int mt = with_floor ? 1 : 0;
    const HostTree &T = H.trees[(size_t)mt];
    const TreeRec &tr = L.trees[(size_t)mt];
    CHECK_EQ(T.wide.size() > 0, 1);
    CHECK_EQ(tr.tri_level, 1);
    CHECK_EQ(tr.nwide, T.wide.size());
    CHECK_EQ(tr.nnodes, 0);  // the wide form is walked: its one-box-per-node copies stay on the host
    CHECK_EQ(tr.noct, 1);
    CHECK_EQ(tr.ntris, kMeshTris);
    CHECK_EQ(tr.bmax == tree_bmax(30.0), 1);
    CHECK_EQ(tr.bmax > 30.0f, 1);
    CHECK_EQ(L.nodes.size(), 0);
    CHECK_EQ(L.tris.size(), kMeshTris + (with_floor ? kFloorTris : 0));
    CHECK_EQ(tr.tri_begin, with_floor ? kFloorTris : 0);
    CHECK_EQ(tr.tbox_begin, with_floor ? kFloorTris : 0);
    CHECK_EQ(L.otris.size(), kMeshTris);
    CHECK_EQ(L.wnodes.size(), T.wide.size());
    const DeviceScene d = traits(H, L);
    CHECK_EQ(d.prim_obj, m);
    CHECK_EQ(d.has_wide, 1);
    CHECK_EQ(d.light_ok, 1);
    CHECK_EQ(d.single_ray, 0);
    CHECK_EQ(d.n_cover, 1);  // fewer than 128 triangles: one cover sphere
    CHECK_EQ(d.prim_finish, with_floor ? 0 : 1);
    CHECK_EQ(d.light_trees, with_floor ? 1 : 0);
    CHECK_EQ(d.light_hf_only, with_floor ? 1 : 0);
    CHECK_EQ(d.prun_begin, with_floor ? 1 : 0);
    CHECK_EQ(d.prun_end, with_floor ? 6 : 5);
}

static void glass_bezier_cached_tree() {
    HostScene H;
    room(H);
    const int g = mesh(H, 0.5);
    bezier(H);
    const SceneLayout L = scene_layout(H, CommitKnobs());
    const HostTree &T = H.trees[0];
    CHECK_EQ(L.trees[0].tri_level, 0);
    CHECK_EQ(L.trees[0].noct, 8);  // one SAH copy per ray-direction octant
    CHECK_EQ(L.trees[0].nnodes, T.bvh_nodes);
    CHECK_EQ(L.nodes.size(), 8 * (size_t)T.bvh_nodes);
    CHECK_EQ(L.otris.size(), 0);
    CHECK_EQ(T.bvh_nodes > 0 && T.bvh_nodes <= kNodeCache, 1);
    const DeviceScene d = traits(H, L);
    CHECK_EQ(g, 5);
    CHECK_EQ(d.has_glass, 1);
    CHECK_EQ(d.has_bezier, 1);
    CHECK_EQ(d.n_beziers, 1);
    CHECK_EQ(d.prim_obj, -1);
    CHECK_EQ(d.cached_tree, 0);
    CHECK_EQ(d.cached_nodes, T.bvh_nodes);
    CHECK_EQ(d.light_ok, 1);
    HostScene B;  // an opaque mesh beside a Bezier object: no primary walk kernel
    mesh(B, 0.0);
    bezier(B);
    CHECK_EQ(traits(B, scene_layout(B, CommitKnobs())).prim_obj, -1);
}

static void many_objects() {
    HostScene H;
    room(H);
    const int early = mesh(H, 0.0);
    for (int i = 0; i < 800; i++) sphere(H, 0.01 * i);
    const SceneLayout L = scene_layout(H, CommitKnobs());
    DeviceScene d = traits(H, L);
    CHECK_EQ(d.n_objs, 806);
    CHECK_EQ(d.n_lds, kLdsObjsMax);
    CHECK_EQ(d.prim_obj, early);
    CommitKnobs k;
    k.lds_objs = 7;
    d = traits(H, L, k);
    CHECK_EQ(d.n_lds, 7);
    CHECK_EQ(d.prim_obj, early);
    CHECK_EQ(d.prun_end, 5);
    k.lds_objs = 5;
    d = traits(H, L, k);
    CHECK_EQ(d.prim_obj, -1);  // the mesh is no longer resident
    k.lds_objs = 4;
    CHECK_EQ(traits(H, L, k).prun_end, 4);  // the run ends with the LDS list
    k.lds_objs = 2;
    CHECK_EQ(traits(H, L, k).prun_end, 0);
    k.lds_objs = -3;
    CHECK_EQ(traits(H, L, k).n_lds, 0);
    HostScene F;  // the mesh beyond the LDS list
    room(F);
    for (int i = 0; i < 800; i++) sphere(F, 0.01 * i);
    mesh(F, 0.0);
    d = traits(F, scene_layout(F, CommitKnobs()));
    CHECK_EQ(d.n_lds, kLdsObjsMax);
    CHECK_EQ(d.prim_obj, -1);
    CHECK_EQ(d.has_wide, 1);
}

static void reference_tree_order() {
    HostScene H;
    room(H);
    mesh(H, 0.0);
    mesh(H, 0.5);
    CommitKnobs k;
    k.ref_tree = true;
    const SceneLayout L = scene_layout(H, k);
    for (int t = 0; t < 2; t++) {
        CHECK_EQ(L.trees[(size_t)t].noct, 1);
        CHECK_EQ(L.trees[(size_t)t].tri_level, 0);
        CHECK_EQ(L.trees[(size_t)t].nwide, 0);
        CHECK_EQ(L.trees[(size_t)t].nnodes, H.trees[(size_t)t].nodes.size());
    }
    CHECK_EQ(L.trees[1].node_begin, H.trees[0].nodes.size());
    CHECK_EQ(L.nodes.size(), H.trees[0].nodes.size() + H.trees[1].nodes.size());
    CHECK_EQ(L.otris.size(), 0);
    CHECK_EQ(L.wnodes.size(), 0);
    const DeviceScene d = traits(H, L, k);
    CHECK_EQ(d.has_wide, 0);
    CHECK_EQ(d.prim_obj, -1);
}

static void device_builds() {
    HostScene H;
    H.build_mode = 1;  // CGRT_BUILD_DEVICE
    room(H);
    const int m = mesh(H, 0.0);  // tree 0: device
    mesh(H, 0.5);                // tree 1: glass, host
    bump_floor(H);               // tree 2: device
    CHECK_EQ(H.trees[0].dev_kind, 1);
    CHECK_EQ(H.trees[1].dev_kind, 0);
    CHECK_EQ(H.trees[2].dev_kind, 2);
    SceneLayout L = scene_layout(H, CommitKnobs());
    const int glass_nodes = H.trees[1].bvh_nodes;
    CHECK_EQ(L.n_dev_trees, 2);
    CHECK_EQ(L.nodes.size(), 8 * glass_nodes);
    CHECK_EQ(L.tris.size(), kMeshTris);
    CHECK_EQ(L.tboxes.size(), kMeshTris);
    CHECK_EQ(L.otris.size() + L.wnodes.size() + L.hcells.size() + L.hcell_y.size(), 0);
    CHECK_EQ(L.room_tris, kMeshTris + kFloorTris);
    CHECK_EQ(L.room_otris, kMeshTris);
    CHECK_EQ(L.room_wnodes, kMeshTris);
    CHECK_EQ(L.room_hcells, kFloorCells);
    const TreeRec &dm = L.trees[0], &gl = L.trees[1], &fl = L.trees[2];
    CHECK_EQ(gl.node_begin, 0);
    CHECK_EQ(gl.tri_begin, 0);
    CHECK_EQ(gl.nnodes, glass_nodes);
    CHECK_EQ(dm.node_begin, 8 * glass_nodes);
    CHECK_EQ(dm.tbox_begin, kMeshTris);
    CHECK_EQ(dm.tri_begin, kMeshTris);
    CHECK_EQ(dm.otri_begin, 0);
    CHECK_EQ(dm.wnode_begin, 0);
    CHECK_EQ(dm.ntris, kMeshTris);
    CHECK_EQ(dm.tri_level, 1);
    CHECK_EQ(dm.noct, 1);
    CHECK_EQ(dm.nnodes, 0);
    CHECK_EQ(dm.nwide, 0);  // until the build
    CHECK_EQ(dm.hfield, -1);
    CHECK_EQ(fl.tri_begin, 2 * kMeshTris);
    CHECK_EQ(fl.otri_begin, kMeshTris);
    CHECK_EQ(fl.wnode_begin, kMeshTris);
    CHECK_EQ(fl.ntris, kFloorTris);
    CHECK_EQ(fl.tri_level, 0);
    CHECK_EQ(fl.hfield, 0);
    CHECK_EQ(L.hfields.size(), 1);
    CHECK_EQ(L.hfields[0].cell_begin, 0);
    CHECK_EQ(L.hfields[0].nx, 4);
    CHECK_EQ(L.hfields[0].nz, 3);
    L.trees[0].nwide = 9;  // what the mesh build reports
    const DeviceScene d = traits(H, L);
    CHECK_EQ(m, 5);
    CHECK_EQ(d.has_wide, 1);
    CHECK_EQ(d.has_glass, 1);
    CHECK_EQ(d.prim_obj, -1);  // two meshes
    CHECK_EQ(d.cached_tree, 1);
    CHECK_EQ(d.light_hf_only, 1);
    CHECK_EQ(d.prim_finish, 0);
    CHECK_EQ(d.n_trees, 3);
    CHECK_EQ(d.n_texs, 1);
}

static void knobs() {
    const char *names[] = {"CGRT_TREE", "CGRT_LDS_OBJS", "CGRT_NO_PLANE_RUN", "CGRT_NO_BEZIER_CULL", "CGRT_AUX_PRIORITY"};
    for (const char *n : names) unsetenv(n);
    CommitKnobs k = commit_knobs();
    CHECK_EQ(k.ref_tree, 0);
    CHECK_EQ(k.lds_objs, kLdsObjsMax);
    CHECK_EQ(k.no_plane_run, 0);
    CHECK_EQ(k.no_bezier_cull, 0);
    CHECK_EQ(k.aux_priority, AUX_LOWEST);
    setenv("CGRT_TREE", "ref", 1);
    setenv("CGRT_LDS_OBJS", "40", 1);
    setenv("CGRT_NO_PLANE_RUN", "1", 1);
    setenv("CGRT_NO_BEZIER_CULL", "1", 1);
    setenv("CGRT_AUX_PRIORITY", "high", 1);
    k = commit_knobs();  // read again at every commit
    CHECK_EQ(k.ref_tree, 1);
    CHECK_EQ(k.lds_objs, 40);
    CHECK_EQ(k.no_plane_run, 1);
    CHECK_EQ(k.no_bezier_cull, 1);
    CHECK_EQ(k.aux_priority, AUX_HIGH);
    setenv("CGRT_TREE", "sah", 1);
    setenv("CGRT_NO_PLANE_RUN", "0", 1);
    setenv("CGRT_NO_BEZIER_CULL", "", 1);
    setenv("CGRT_AUX_PRIORITY", "same", 1);
    k = commit_knobs();
    CHECK_EQ(k.ref_tree, 0);
    CHECK_EQ(k.no_plane_run, 0);
    CHECK_EQ(k.no_bezier_cull, 0);
    CHECK_EQ(k.aux_priority, AUX_SAME);
    for (const char *n : names) unsetenv(n);
}

int main() {
    diffuse_spheres();
    plane_run();
    opaque_mesh(false);
    opaque_mesh(true);
    glass_bezier_cached_tree();
    many_objects();
    reference_tree_order();
    device_builds();
    knobs();
    std::printf("%s: %d failed checks\n", g_failed ? "FAILED" : "ok", g_failed);
    return g_failed ? 1 : 0;
}
