// Host-side scene assembly: mesh loaders, bump-mesh construction, tree build, flattening, scene traits.
// These are the reference's pre-pass (objects.h:217-267,338-403,480-504; texture.h:19-38), run once per
// scene on the CPU; the per-ray work is all in cgrt_hip.hip.
#ifndef CGRT_BUILD_H
#define CGRT_BUILD_H
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "cgrt_types.h"

namespace cgrt {

struct HostTree {
    std::vector<double> tri9;        // construction order, 9 doubles per triangle
    // reference-numbered view (for verification dumps)
    std::vector<int32_t> node_lr_size;  // left, right, count
    std::vector<double> bbox;           // xmin,xmax,ymin,ymax,zmin,zmax (unpadded)
    std::vector<int32_t> leaf_ids;      // triangle ids of leaves, node order
    // device view: the reference's leaves (tris, in leaf order) and two hierarchies over them --
    // `nodes`: the reference's own tree in preorder with skip links;
    // `bvh`  : a surface-area-heuristic hierarchy over the SAME leaves, stored once per ray-direction octant
    //          (8 x bvh_nodes records, each a preorder with skip links whose children are ordered near-to-far
    //          for rays of that octant), see build_bvh()
    std::vector<NodeRec> nodes;
    std::vector<TriRec> tris;
    std::vector<NodeRec> tboxes;  // one grown, outward-rounded fp32 box per triangle of tris[] (the leaf scan's cheap pre-test)
    std::vector<NodeRec> bvh;
    int32_t bvh_nodes = 0;
    // opaque owner (transparency < eps): only the nearest hit matters, so the hierarchy goes down to small groups of
    // TRIANGLES (<= 4) instead of stopping at the reference's leaves; its leaves index otris
    bool tri_level = false;
    std::vector<OTriRec> otris;
    std::vector<WideNodeRec> wide;  // tri_level: the same hierarchy four children to a node (device walk); root = wide[0]
    int32_t wide_stack = 0;         // deepest the walk's stack can get on it (< kWideStack, or `wide` is left empty)
    void build_bvh(bool opaque);
    // bump floors only: the same triangles in grid order (construction order is cell-major: quad (i,j) = triangles
    // 2*(i*nx+j) and +1), see HCellRec
    bool is_hfield = false;
    HFieldRec hfield{};
    std::vector<HCellRec> hcells;
    std::vector<HCellY> hcell_y;  // per cell: its vertices' height range, rounded outward
    void build(bool opaque = false, bool with_bvh = true);
    void build_hfield(int nx, int nz, double x0, double z0, double hx, double hz);
    // Row f3 (cgrt_devbuild.hpp): an opaque owner's structure is built on the device at commit; nothing above is filled on the
    // host then except tri9 (a mesh's input triangles).  dev_kind: 0 = host build, 1 = mesh (4-wide triangle-level hierarchy),
    // 2 = bump floor (grid cells generated from the texture bytes).
    int dev_kind = 0;
    int64_t dev_ntri = 0;       // triangles the device build will produce / was given
    int dev_tex = -1;           // bump floor: texture index
    double dev_plane_y = 0;     // bump floor: the plane's y (objects.h:489-492)
    int dev_obj = -1;           // mesh: the owning object (its bounding sphere is computed by the device build)
    // filled by the commit for the verification dumps (cgrt_scene_wide_dump on a device-built tree reads the device arrays)
    int32_t dev_nwide = 0;
    bool dev_balanced = false;
    // a mesh's cover spheres in HostScene::cover, whichever build made them: spheres [cover_first, cover_first + cover_n)
    // (a refit writes new ones into the same places, cgrt_refit.hpp)
    size_t cover_first = 0;
    int cover_n = 0;
    // cgrt_scene_refit_mesh has moved the vertices: the device's records are the tree now, and what above describes the
    // reference's tree over the old vertices is reported empty (leaf_ids stays: it maps tris[] to construction order)
    bool refitted = false;
};
// nodes of the reference's tree over n triangles (objects.h:217-267: leaf below 10, halves n/2 and n - n/2): what
// cgrt_scene_stats reports for a tree that was never built on the host
int64_t ref_node_count(int64_t n);

struct HostTexture {
    std::vector<uint8_t> rgb;
    int rows = 0, cols = 0;
    double n[3], p[3], lenx = 0, leny = 0;
    bool isbump = false;
};

struct HostScene {
    std::vector<ObjRec> objs;
    std::vector<HostTree> trees;
    std::vector<HostTexture> textures;
    std::vector<BezierRec> beziers;
    std::vector<BezSlabRec> bez_slabs;  // kBezSlabs per Bezier object (see BezSlabRec)
    std::vector<double> cover;  // (cx, cy, cz, r) spheres that together contain every mesh triangle (classify_kernel)
    std::string error;
    int build_mode = 0;      // CGRT_BUILD_HOST / CGRT_BUILD_DEVICE (cgrt.h): where opaque owners' structures are built
    double host_build_ms = 0;  // wall-clock spent in HostTree::build* by the add_* calls

    int add_sphere(const double c[3], double r, const double sc[3], double refl, double transp);
    int add_texture(const uint8_t *rgb, int rows, int cols, const double n[3], const double p[3], double lx,
                    double ly, int isbump);
    int add_plane(const double p[3], const double n[3], const double sc[3], double refl, double transp, int tex);
    int add_mesh_file(const char *file, double a, const double b[3], const double sc[3], double refl,
                      double transp, int type);
    int add_mesh_triangles(const double *tri9, int ntri, const double sc[3], double refl, double transp, int type);
    int add_bezier(const double *cp3, int ncp, const double pos[3], const double sc[3], double refl, double transp);
};

// returns false and sets err on malformed input; a missing file gives an empty list and true
bool load_mesh_file(const char *file, double a, const double b[3], int type, std::vector<double> &tri9,
                    std::string &err);

// ---- the host side of cgrt_scene_commit: knobs -> layout -> (uploads, device builds) -> traits ----------------------------

// The commit's switches (measurement and test aids), read from the environment once per commit.
enum AuxPriority { AUX_LOWEST, AUX_SAME, AUX_HIGH };
struct CommitKnobs {
    bool ref_tree = false;        // CGRT_TREE=ref: the device walks the reference's own inner nodes instead of the SAH hierarchy
    int lds_objs = kLdsObjsMax;   // CGRT_LDS_OBJS=n: at most n objects resident in LDS (drives the SPILL variants)
    bool no_plane_run = false;    // CGRT_NO_PLANE_RUN=1: the leading planes are tested one by one
    bool no_bezier_cull = false;  // CGRT_NO_BEZIER_CULL=1: every solve of every ray that enters a Bezier object's box is run
    AuxPriority aux_priority = AUX_LOWEST;  // CGRT_AUX_PRIORITY=same|high: priority of the light launch's stream
};
CommitKnobs commit_knobs();

#if defined(__HIPCC__)
#define CGRT_BOUNDS_HD __host__ __device__ inline
#else
#define CGRT_BOUNDS_HD inline
#endif
// The bounds formulas, written once for the host builder, the device builder's host tail and the refit's kernels:
// TreeRec::bmax from the largest |coordinate| of a tree's vertices -- a bound on |coordinate| of every box face (the fp32 box
// test's error term, cgrt_traverse.hpp Ray32): the growth of the boxes and a little more;
CGRT_BOUNDS_HD float tree_bmax(double max_abs) { return (float)((max_abs + 2 * kBoxPad) * (1 + 1e-6)) * (1.f + 1e-6f); }
// the radius of a sphere around vertices whose largest squared distance from its centre is r2 (1e-3: far above the triangle
// test's rounding), and ObjRec::s0 of a mesh's bounding sphere of that radius
CGRT_BOUNDS_HD double cover_radius(double r2) { return std::sqrt(r2) + 1e-3; }
CGRT_BOUNDS_HD double sphere_s0(double r) { return r * r * (1 + 1e-9); }

// Where every record of the device arrays goes.  Host-built records come first, in tree order.  Behind them each array keeps
// room for what the device builds (HostTree::dev_kind) write at commit, again in tree order; that room has no host copy.
struct SceneLayout {
    std::vector<NodeRec> nodes;
    std::vector<TriRec> tris;
    std::vector<OTriRec> otris;
    std::vector<NodeRec> tboxes;
    std::vector<WideNodeRec> wnodes;
    std::vector<HCellRec> hcells;
    std::vector<HCellY> hcell_y;  // parallel to hcells
    std::vector<uint8_t> texels;
    std::vector<TexRec> texs;
    std::vector<HFieldRec> hfields;
    std::vector<TreeRec> trees;   // one per HostTree, device-built ones included (their nwide, a mesh's bmax and a floor's
                                  // height range are filled by the build)
    size_t room_tris = 0, room_otris = 0, room_wnodes = 0, room_hcells = 0;  // records behind the host-built ones (hcells: and hcell_y)
    int n_dev_trees = 0;
};
SceneLayout scene_layout(const HostScene &H, const CommitKnobs &k);

// Every scalar field of d -- the inputs of kernel-variant selection -- from the scene (objects, cover spheres), its final tree
// records (after the device builds) and the knobs.  The pointers are left as they are.
void scene_traits(const HostScene &H, const std::vector<TreeRec> &trees, const CommitKnobs &k, DeviceScene &d);

}  // namespace cgrt
#endif
