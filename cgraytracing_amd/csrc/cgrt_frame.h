// The host side of an eye-pass launch in plain C++ (no HIP): the kernel parameters, the workgroup / tile constants, the
// environment switches and the frame plan -- sample chunks, tile counts, heavy-tile capacity, scheduling, the tile order of a
// sphere scene (whether it runs, who renders its class-3 tiles, the sphere masks, the lens stage, the lens table), its sample relay (RelayPlan:
// the one decision of its form, its two areas and everything derived from them) and where each array lies in the handle's
// launch scratch and in its order buffer.  cgrt_trace_grid (cgrt_hip.hip) launches what frame_plan decides;
// tests/native/frame_plan.cpp checks it on the CPU.
#ifndef CGRT_FRAME_H
#define CGRT_FRAME_H
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/cgrt.h"
#include "cgrt_lens_stage.h"
#include "cgrt_relay.h"

// =====================================================================================================
// kernel parameters
// =====================================================================================================
struct GridParams {
    int32_t W, H, rows, row_offset, stripe_rows, stripe_rank, stripe_nranks;
    int32_t spp, sample_offset, max_depth;
    int32_t accumulate;  // CGRT_GRID_ACCUMULATE: rgb += this pass (nhit is overwritten)
    int32_t xcd_tiles;   // block -> tile mapping: 1 = XCD-aware super-tiles, 0 = row-major (see tile_of_block)
    // CGRT_GRID_SPLIT_SAMPLES: chunks > 1 workgroups per tile, workgroup c of a tile takes samples [c*chunk_spp, ...) and
    // leaves its raw fp64 sums in partial[c][local pixel][3] (and its hit count in partial_nhit[c][local pixel])
    int32_t chunks, chunk_spp;
    double *partial;
    uint32_t *partial_nhit;
    // Cost-aware scheduling (cgrt_hip.hip, "classify -> probe -> plan -> render -> ordered sum").  The unit of
    // bookkeeping is a WAVE TILE of 16x4 pixels, numbered wy * ceil(W/16) + wx over the local rows.
    //   probe != 0 : trace this launch's first sample only to measure it -- nothing is stored except cost[wave tile] =
    //                shader-clock ticks the wave spent on it.  probe == 2 (the relay's cost start, cgrt_relay.h): cost[wave tile] =
    //                the wave's iterations over the launch's samples -- a count, the same in every run.
    //   render     : order[0..K) = the HEAVY wave tiles (plan_kernel), plan[0] = K, hidx[wave tile] = rank among them or -1.
    //                The first heavy_blocks workgroups of the render launch (the unit-form body; they loop until the queue
    //                is empty) serve the heavy tiles through a queue of ITEMS (plan[2] = next item; item = heavy tile rank *
    //                items_per_tile + part): an item is units_per_item (pixel, sample) UNITS of one heavy tile, which the
    //                lanes of the wave take one after another as they become free, so a heavy tile is spread over many waves
    //                on many CUs and no lane idles while units remain.  Every Hitpoint value of a unit goes to
    //                dvals[rank][sample][emission index][pixel] (dcnt = how many), and deferred_sum_kernel adds them per
    //                pixel in the reference's order -- sample by sample, emission order within a sample -- so the fp64 sum
    //                is bit for bit the sequential one.  The other tiles are rendered in the tile form (waves whose tile is
    //                heavy stand down): through the tile queue below, or one workgroup per tile.
    // Light tiles (classify_kernel): light[wave tile] != 0 -- no primary ray of the tile can come near a mesh, a Bezier
    // object or a mirror / glass sphere, so it is rendered by the kernel variant without tree, Bezier and pending-ray code
    // (fewer registers, more waves per SIMD; with bump-mapped diffuse planes: the tree-capable variant without Bezier and
    // pending-ray code), launched beside the full variant on a second stream.  light_mode: 0 = this
    // launch leaves the light tiles alone, 1 = this launch renders only them; light == nullptr: no split.
    const unsigned char *light;
    // tile_order != 0 (set only by the image-order launch of a sphere scene that ran tile_order_kernel, never by a probe, a
    // light or a scheduled launch): trace_grid_kernel's workgroup b renders tile border[b] (ty * tiles_x + tx), the tiles that
    // may see a refracting or reflecting sphere first; plan[c] = workgroups of classes < c (kOrderSpheresMax below).  kOrderAll:
    // every entry of the list; kOrderFull / kOrderDiffuse: one of a pair of launches over the list -- the entries of classes
    // 0-2, resp. workgroup b renders entry plan[3] + b (class 3: the terminal-diffuse variant, on the handle's second stream);
    // kOrderAllDiffuse: every entry, the workgroups from plan[3] on by the terminal-diffuse body inside the same kernel
    int32_t light_mode, tile_order;
    // wmask != nullptr (tile-order launches of a scene of at most 32 spheres and nothing else): wmask[wave tile] = the spheres some
    // primary ray of the wave tile may meet, bit i = object i (tile_order_kernel, cgrt_sphere_mask.h); the terminal-diffuse body
    // tests only those.  nullptr: every sphere.
    const uint32_t *wmask;
    const uint32_t *order;
    // Tile queue of the scheduled launch (chunks == 1): border[0..plan[3]) = the tiles (ty * tiles_x + tx) with at least one
    // wave tile that is neither heavy nor light, costliest first (plan_kernel); plan[4] = next entry.  The launch is then
    // heavy_blocks + a chip's worth of workgroups, each serving one queue until it is empty and then the other, so neither
    // empty tiles nor a late expensive tile cost anything at the end of the frame.  nullptr: one workgroup per tile.
    const uint32_t *border;
    uint32_t *cost;
    const int32_t *hidx;
    uint32_t *plan;
    double *dvals;
    unsigned char *dcnt;
    double *pconst;  // heavy tiles: per pixel {pdir(3), pof(3), bits of k_pix}, layout [rank][7][64], filled by pixel_const_kernel
    int32_t probe, heavy_blocks, items_per_tile, units_per_item, maxhp;
    // Primary-ray mesh hits of the heavy tiles' units, computed by primary_walk_kernel before the render launch
    // (cgrt_primwalk.hpp): [rank][sample][pixel] distance (kInf: none) and triangle (-1: none) in object prim_obj; nullptr: off
    const double *prim_len;
    const int32_t *prim_tri;
    int32_t prim_obj;
    int32_t prim_done;  // primary_walk_kernel also completes units (dcnt != 255: done there, the unit-queue body skips them)
    int32_t pw_refill, pw_rounds;  // primary_walk_kernel: idle lanes that trigger a refill; inner-node rounds between leaf phases
    // development aid (env CGRT_TIMELINE_FILE, cgrt_hip.hip): per workgroup {start, end (wall_clock64, 100 MHz), HW_ID | XCC_ID << 32,
    // tile_x | tile_y << 16 | rays << 32}; nullptr in normal operation
    unsigned long long *timeline;
    double inv_spp_total;
    uint64_t seed;
    double cam[3], half_width, focus_plane, lens_radius;
    // The sample relay (cgrt_relay.h; tile-order launches of the PAIR variants only): relay_k > 1 -- the first
    // min(plan[2], relay_cap) entries of the list (relay_extent == kRelayMirror: min(plan[3], relay_cap), the class-2 tiles too)
    // are rendered by relay_k workgroups each, chunk c taking relay_chunk_spp samples from c * relay_chunk_spp on, the workgroups
    // in the order relay_order names (relay_block_ordered); `relay` is the handle's relay area, laid out for (relay_cap,
    // relay_k, relay_slots).  relay_k <= 1: every entry by one workgroup.
    unsigned char *relay;
    int32_t relay_k, relay_chunk_spp, relay_cap, relay_slots;
    int32_t relay_extent, relay_order;
    // lens_batch != 0 (the PAIR variants' kOrderAllDiffuse launch of a thin-lens camera): a wave of the terminal-diffuse body inside
    // that launch stages the lens draws of its next kLensBatch samples per lane in LDS (cgrt_lens_stage.h); 0: lens_disc per sample
    int32_t lens_batch;
    // relay_start_at != 0 (a relaying launch with a start table, cgrt_relay.h): plan[relay_start_at + b] = entry << 2 | chunk of
    // workgroup b < t (relay_items_total), in place of relay_block_ordered; the table is a part of the order buffer like plan
    uint32_t relay_start_at;
    // wsure != nullptr (tile-order launches that have masks, unless switched off): wsure[wave tile] = the sphere that EVERY primary
    // ray of the wave tile hits first (sure_first_kernel, cgrt_sure_first.h), or kSureNone; set only for wave tiles of class-3
    // tiles.  A wave of the terminal-diffuse body whose tile has one adds that sphere's colour per sample and traces nothing.
    const unsigned char *wsure;
    // relay_boost_at != 0 (a launch with a start table that promotes its heaviest tiles to boost_k chunks, cgrt_relay.h):
    // plan[relay_boost_at + kBoostItems] = the table's items, plan[relay_boost_at + kBoostHead + e] = bslot[e] of split entry e.
    // A promoted tile's chunks have boost_chunk_spp samples and boost_slots slots a stream, and its slot lies in the boost area,
    // laid out for (boost_cap, boost_k, boost_slots) at relay + relay_boost_off.
    uint64_t relay_boost_off;
    uint32_t relay_boost_at;
    int32_t boost_k, boost_chunk_spp, boost_cap, boost_slots, pad_boost_;
    // lens_table != nullptr (the one-launch tile-order PAIR variants under a thin lens, their table-reading twins; cgrt_lens_stage.h):
    // the full and the parking body of the workgroups of list entries < lens_table_cap take their samples' lens draws from
    // table[entry][sample][thread], lens_table_spp samples an entry, written by lens_table_kernel ahead of the frame
    const uint64_t *lens_table;
    int32_t lens_table_cap, lens_table_spp;
    // posed != 0 (CGRT_GRID_POSED; the POSE kernels, camera_ray): the camera's frame in the world -- `cam`, half_width, focus_plane
    // and lens_radius above are the camera in that frame, and the primary rays start from pose_point's images of its points.
    // posed == 0: the identity frame (origin 0, the unit axes), which no kernel reads.
    double pose_origin[3], pose_right[3], pose_up[3], pose_forward[3];
    int32_t posed, pad_pose_;
};
static_assert(sizeof(GridParams) == 488, "GridParams is a kernel argument: its layout is fixed");
static_assert(offsetof(GridParams, pose_origin) == 384, "the pose is appended: no earlier field moves");

#if defined(__HIPCC__)
#define CGRT_HD __host__ __device__ __forceinline__
#else
#define CGRT_HD inline
#endif
// ---- the posed camera (cgrt_posed_camera, cgrt.h) ----
// M(p) = ((origin + right * p.x) + up * p.y) + forward * p.z, per component in exactly this order; the library is built without
// contraction, so host and device give the same bits.  For the identity frame every product is p's component or a zero and
// every sum adds zeros: M(p) == p (a component of -0 comes out as +0, the same value).
// The one definition of a posed primary ray, used by trace_grid_body and pixel_const_kernel (cgrt_eye.hpp) and by camera_ray
// (cgrt_rays.hpp): in the camera's own frame nothing changes -- the pixel point pix = (px, py, 0), the eye cam, the focus point
// pof = pdir * ((focus_plane - cam.z) / pdir.z) + cam with pdir = normalized(pix - cam), the lens point o = cam + (sx, sy, 0) *
// lens_radius -- and the ray is made of the images of those points:
//     pinhole:   origin M(cam), direction normalized(M(pix) - M(cam))
//     thin lens: origin M(o),   direction normalized(M(pof) - M(o))       (M(pof) once per pixel, M(o) once per sample)
// The direction is normalised from world points: unit to the standard of the built-in camera's, whatever the basis's last bits.
CGRT_HD void pose_point(const GridParams &g, double x, double y, double z, double &wx, double &wy, double &wz) {
    wx = ((g.pose_origin[0] + g.pose_right[0] * x) + g.pose_up[0] * y) + g.pose_forward[0] * z;
    wy = ((g.pose_origin[1] + g.pose_right[1] * x) + g.pose_up[1] * y) + g.pose_forward[1] * z;
    wz = ((g.pose_origin[2] + g.pose_right[2] * x) + g.pose_up[2] * y) + g.pose_forward[2] * z;
}

// What is wrong with the camera of (cam, grid), or nullptr: with CGRT_GRID_POSED `cam` is the base of a cgrt_posed_camera whose
// 12 numbers must be finite, its axes of length 1 within kPoseTol and orthogonal within kPoseTol (no handedness is asked: a
// mirrored basis mirrors the image).  The one validation of a pose, asked by every entry before grid_params reads it.
static constexpr double kPoseTol = 1e-9;
inline const char *pose_error(const cgrt_camera *cam, const cgrt_grid *grid) {
    if (!(grid->flags & CGRT_GRID_POSED)) return nullptr;
    const cgrt_posed_camera *pc = reinterpret_cast<const cgrt_posed_camera *>(cam);
    const double *ax[3] = {pc->right, pc->up, pc->forward};
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(pc->origin[k])) return "posed camera: origin is not finite";
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(ax[a][k])) return "posed camera: a basis vector is not finite";
    }
    const auto dot3 = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    for (int a = 0; a < 3; a++)
        if (!(std::fabs(std::sqrt(dot3(ax[a], ax[a])) - 1.0) <= kPoseTol)) return "posed camera: right, up and forward must have length 1 (within 1e-9)";
    for (int a = 0; a < 3; a++)
        if (!(std::fabs(dot3(ax[a], ax[(a + 1) % 3])) <= kPoseTol)) return "posed camera: right, up and forward must be orthogonal (dot products within 1e-9)";
    return nullptr;
}

// cgrt_look_at (cgrt.h) in plain fp64; nullptr, or what is wrong with the arguments
inline const char *look_at_camera(const double eye[3], const double target[3], const double up_hint[3], double fov_x_deg,
                                  double focus_distance, double lens_radius, cgrt_posed_camera *out) {
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(eye[k]) || !std::isfinite(target[k]) || !std::isfinite(up_hint[k])) return "cgrt_look_at: eye, target and up_hint must be finite";
    if (!(fov_x_deg > 0 && fov_x_deg < 180)) return "cgrt_look_at: fov_x_deg must lie in (0, 180)";
    if (!(focus_distance > 0) || !std::isfinite(focus_distance)) return "cgrt_look_at: focus_distance must be positive";
    if (!(lens_radius >= 0) || !std::isfinite(lens_radius)) return "cgrt_look_at: lens_radius must be >= 0";
    const auto norm3 = [](const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    const auto cross3 = [](const double *a, const double *b, double *c) {
        c[0] = a[1] * b[2] - a[2] * b[1];
        c[1] = a[2] * b[0] - a[0] * b[2];
        c[2] = a[0] * b[1] - a[1] * b[0];
    };
    double f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]}, r[3], u[3];
    const double D = norm3(f);
    if (!(D > 0) || !std::isfinite(D)) return "cgrt_look_at: eye and target coincide";
    for (int k = 0; k < 3; k++) f[k] /= D;
    cross3(up_hint, f, r);
    const double rl = norm3(r), ul = norm3(up_hint);
    // (parallel: the sine of the angle between hint and view below 1e-12)
    if (!(ul > 0) || !(rl > 1e-12 * ul)) return "cgrt_look_at: up_hint is zero or parallel to the view";
    for (int k = 0; k < 3; k++) r[k] /= rl;
    cross3(f, r, u);
    cgrt_posed_camera pc;
    pc.base.cam[0] = pc.base.cam[1] = 0.0;
    pc.base.cam[2] = -D;
    pc.base.half_width = D * std::tan(fov_x_deg * (3.14159265358979323846 / 360.0));
    pc.base.focus_plane = focus_distance - D;
    pc.base.lens_radius = lens_radius;
    for (int k = 0; k < 3; k++) {
        pc.origin[k] = target[k];
        pc.right[k] = r[k];
        pc.up[k] = u[k];
        pc.forward[k] = f[k];
    }
    *out = pc;
    return nullptr;
}
// the head of the order buffer's boost part, in words: S (two words), the promoted entries, the table's items; bslot follows
static constexpr int kBoostS = 0, kBoostPromoted = 2, kBoostItems = 3, kBoostHead = 4;

static constexpr int kTileW = 32, kTileH = 8, kThreads = 256;
// Tile order of image-order launches (tile_order_kernel, cgrt_eye.hpp): the special spheres -- those that reflect or refract --
// travel as a kernel argument; a scene with more of them than this is left in row-major order.  The handle's order buffer (TileOrderLayout) is
// plan[kOrderPlanWords] | list[n_tiles] | tile class[n_tiles] (bytes) | wave-tile class[n_wt] (bytes) | wave-tile sphere mask[n_wt]
// (words; GridParams::wmask) | wave-tile sure sphere[n_wt] (bytes; GridParams::wsure; only where asked for), each part padded to 256 bytes; plan[c], c = 0..4 = tiles of classes < c, plan[kOrderArrived] = the
// workgroups of tile_order_kernel that are through (0 between launches).
static constexpr int kOrderSpheresMax = 16, kOrderClasses = 4, kOrderPlanWords = 8, kOrderArrived = 5;
static constexpr int kOrderAll = 1, kOrderFull = 2, kOrderDiffuse = 3, kOrderAllDiffuse = 4;  // GridParams::tile_order
struct OrderSpheres {
    double s[kOrderSpheresMax][4];  // centre, radius
    uint32_t n, transp;             // transp: bit i set = sphere i refracts (transp >= kEps), else it only reflects
};
static constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// A part of a launch buffer of the handle; bytes == 0: not used by this frame (its pointer is nullptr)
struct Region {
    size_t at, bytes;
    template <class T> T *in(unsigned char *base) const { return bytes ? reinterpret_cast<T *>(base + at) : nullptr; }
};
// Where the parts of the order buffer lie, in bytes from its start
struct TileOrderLayout {
    Region plan{}, list{}, tile_cls{}, wave_cls{}, wmask{}, wsure{};
    // start_words > 0 (the relay's cost start, cgrt_relay.h), behind everything else: the wave tiles' probe costs, the items'
    // weights (8 bytes each) and the start table, start_words each of the two
    Region wcost{}, weight{}, start{};
    // boost_words > 0 (a start table with promoted tiles, cgrt_relay.h), behind those: head and bslot (kBoostHead + split_cap words;
    // `bslot` names the words behind the head), the entries' costs, the virtual items' weights (n_tiles * boost_k) and the table
    // the launch reads instead of `start` (start_words + boost_words)
    Region boost{}, bslot{}, ecost{}, bweight{}, bstart{};
    uint32_t word(const Region &r) const { return (uint32_t)((r.at - plan.at) / sizeof(uint32_t)); }  // where a part begins, in words of plan[]
    size_t total = 0;  // bytes to allocate
};
inline TileOrderLayout tile_order_layout(size_t n_tiles, size_t n_wt, bool sure = false, size_t start_words = 0, size_t boost_words = 0,
                                         size_t split_cap = 0, int boost_k = 0) {
    TileOrderLayout L;
    size_t end = 0;  // the list follows the plan at once; every other part starts on 256 bytes
    const auto take = [&end](size_t bytes) { end += bytes; return Region{end - bytes, bytes}; };
    L.plan = take(kOrderPlanWords * sizeof(uint32_t));
    L.list = take(n_tiles * sizeof(uint32_t));
    end = align256(end);
    L.tile_cls = take(n_tiles);
    end = align256(end);
    L.wave_cls = take(n_wt);
    end = align256(end);
    L.wmask = take(n_wt * sizeof(uint32_t));
    if (sure) {  // (read a word at a time: the part ends on 256 bytes like the others)
        end = align256(end);
        L.wsure = take(n_wt);
    }
    if (start_words) {
        end = align256(end);
        L.wcost = take(n_wt * sizeof(uint32_t));
        end = align256(end);
        L.weight = take(start_words * sizeof(uint64_t));
        end = align256(end);
        L.start = take(start_words * sizeof(uint32_t));
    }
    if (start_words && boost_words) {
        end = align256(end);
        L.boost = take((kBoostHead + split_cap) * sizeof(uint32_t));
        L.bslot = Region{L.boost.at + kBoostHead * sizeof(uint32_t), split_cap * sizeof(uint32_t)};
        end = align256(end);
        L.ecost = take(n_tiles * sizeof(uint32_t));
        end = align256(end);
        L.bweight = take(n_tiles * (size_t)boost_k * sizeof(uint64_t));
        end = align256(end);
        L.bstart = take((start_words + boost_words) * sizeof(uint32_t));
    }
    L.total = align256(end);
    return L;
}
static constexpr int kSphereMaskMax = 32;  // spheres a wave tile's mask word holds
// True when no tile of any grid seen from `cam` can be of class 3: some special sphere fails cone_clear_of (cgrt_eye.hpp) by
// one of its tests that do not look at the tile -- it reaches the lens plane, or its bound, grown by the lens blur, holds the
// camera.  The same expressions as on the device; a last-bit difference would only cost an idle launch or leave class-3 tiles
// to the full variant.
inline bool order_all_special(const OrderSpheres &sp, const cgrt_camera &cam) {
    for (uint32_t i = 0; i < sp.n; i++) {
        double r = sp.s[i][3] * (1 + 1e-9) + 1e-6;
        if (cam.lens_radius > 0) {
            const double f = cam.focus_plane - cam.cam[2];
            const double s_lo = (sp.s[i][2] - r - cam.cam[2]) / f, s_hi = (sp.s[i][2] + r - cam.cam[2]) / f;
            if (!(f > 0) || !(s_lo > 0) || !(cam.cam[2] < 0)) return true;
            r += cam.lens_radius * std::max(std::fabs(1 - s_lo), std::fabs(1 - s_hi));
        }
        const double vx = sp.s[i][0] - cam.cam[0], vy = sp.s[i][1] - cam.cam[1], vz = sp.s[i][2] - cam.cam[2];
        if (!(std::sqrt(vx * vx + vy * vy + vz * vz) > r)) return true;
    }
    return false;
}
static constexpr int kWaveTileW = 16, kWaveTileH = 4;  // one pixel per lane
// blockIdx -> tile, XCD-aware (tile_of_block, cgrt_grid.hpp): super-tiles of kSuperW x kSuperH tiles dealt to kXcds L2 groups
static constexpr int kXcds = 8, kSuperW = 4, kSuperH = 4, kSuperTiles = kSuperW * kSuperH;

inline int tile_grid_blocks(int W, int rows, bool xcd_tiles, int tile_w = kTileW, int tile_h = kTileH) {
    const int tiles_x = (W + tile_w - 1) / tile_w, tiles_y = (rows + tile_h - 1) / tile_h;
    if (!xcd_tiles) return tiles_x * tiles_y;
    const int sx = (tiles_x + kSuperW - 1) / kSuperW, sy = (tiles_y + kSuperH - 1) / kSuperH;
    const int nsuper = sx * sy;
    return ((nsuper + kXcds - 1) / kXcds) * kXcds * kSuperTiles;
}

// The GridParams of a launch over `grid` seen from `cam`, every scheduling, chunk and primary-walk field at its default:
// row-major tiles, one workgroup per tile with all its samples, no probe, no light split, nothing deferred or walked ahead
// (fields not named here are 0 / nullptr).  With CGRT_GRID_POSED `cam` is the base of a cgrt_posed_camera that pose_error has
// passed; without it no byte behind the cgrt_camera is read and the frame is the identity.
inline GridParams grid_params(const cgrt_camera *cam, const cgrt_grid *grid) {
    GridParams g{};
    g.W = grid->width;
    g.H = grid->height;
    g.rows = grid->rows;
    g.row_offset = grid->row_offset;
    g.stripe_rows = grid->stripe_rows;
    g.stripe_rank = grid->stripe_rank;
    g.stripe_nranks = grid->stripe_nranks;
    g.spp = grid->spp;
    g.sample_offset = grid->sample_offset;
    g.max_depth = grid->max_depth;
    g.accumulate = (grid->flags & CGRT_GRID_ACCUMULATE) ? 1 : 0;
    g.inv_spp_total = 1.0 / (double)grid->spp_total;
    g.seed = grid->seed;
    for (int k = 0; k < 3; k++) g.cam[k] = cam->cam[k];
    g.half_width = cam->half_width;
    g.focus_plane = cam->focus_plane;
    g.lens_radius = cam->lens_radius;
    g.chunks = 1;
    g.chunk_spp = grid->spp;
    g.items_per_tile = 1;
    g.units_per_item = 256;
    g.maxhp = 16;
    g.prim_obj = -1;
    g.pw_refill = 16;
    g.pw_rounds = 8;
    g.pose_right[0] = g.pose_up[1] = g.pose_forward[2] = 1.0;
    if (grid->flags & CGRT_GRID_POSED) {
        const cgrt_posed_camera *pc = reinterpret_cast<const cgrt_posed_camera *>(cam);
        for (int k = 0; k < 3; k++) {
            g.pose_origin[k] = pc->origin[k];
            g.pose_right[k] = pc->right[k];
            g.pose_up[k] = pc->up[k];
            g.pose_forward[k] = pc->forward[k];
        }
        g.posed = 1;
    }
    return g;
}

// ---- the eye pass's environment switches CGRT_* (measurement and development aids) ----
struct EyeKnobs {
    bool force_reorder = false;  // FORCE_REORDER: schedule sphere-only scenes too
    long long defer_bytes = 0;   // DEFER_BYTES: <= 0: the default
    int heavy_div = 32, units_per_item = 256;  // HEAVY_DIV, UNITS_PER_ITEM (whole waves)
    bool no_primwalk = false, pw_no_finish = false;
    int pw_refill = 16, pw_rounds = 8;
    int lds_pad = 0;  // LDS_PAD: extra dynamic LDS bytes of the main launch
    bool no_hfonly = false, no_tile_queue = false, plan_dump = false;
    bool no_sure_tiles = false;   // NO_SURE_TILES: as CGRT_GRID_NO_SURE_TILES on every launch (a measurement aid)
    bool no_order_reuse = false;  // NO_ORDER_REUSE: tile_order_kernel in front of every tile-order launch (order_tiles)
    int relay_chunks = kRelayDefaultChunks;  // RELAY_CHUNKS: most workgroups a relayed tile's samples are cut into (2..4)
    long long relay_tiles = 0;           // RELAY_TILES: > 0: at most this many tiles are relayed (the relay area's capacity)
    int relay_mirror = -1;  // RELAY_MIRROR: 0 / 1: the relay's extent where the launch's flags name none (-1: unset)
    int relay_order = -1;   // RELAY_ORDER: chunks_first / mirror_first / interleaved (or 0 / 1 / 2), likewise
    int relay_start = -1;   // RELAY_START: list / cost (kRelayStartList / kRelayStartCost), where the launch's flags name neither (-1: unset)
    int relay_probe_spp = kRelayProbeSpp;  // RELAY_PROBE_SPP: samples of the cost probe (1, 2 or 4; a measurement aid)
    // RELAY_BOOST: off, or num/den -- the promotion threshold (cgrt_relay.h; a measurement aid); RELAY_BOOST_TILES: >= 0: at most
    // this many tiles are promoted (the boost area's capacity)
    bool relay_boost_off = false;
    uint32_t relay_boost_num = kRelayBoostNum, relay_boost_den = kRelayBoostDen;
    long long relay_boost_tiles = -1;
    int lens_stage = -1;    // LENS_STAGE: off / lds (kLensStageOff / kLensStageLds), where the launch's flags do not switch it off (-1: unset)
    int lens_table = -1;    // LENS_TABLE: off / on (on: written by every launch that needs it), where the launch's flags say neither (-1: unset)
    long long lens_table_bytes = 0;  // LENS_TABLE_BYTES: >= 0 where set: the lens table's byte budget (default kLensTableBudget)
    bool lens_table_bytes_set = false;
    bool no_inside_trips = false;  // INSIDE_TRIPS=off: as CGRT_GRID_NO_INSIDE_TRIPS on every launch (a measurement aid)
    const char *timeline_file = nullptr;  // TIMELINE_FILE (nullptr: off)
};
inline const char *env_str(const char *name) { const char *e = std::getenv(name); return e ? e : ""; }
inline bool env_on(const char *name) { const char *e = env_str(name); return *e && *e != '0'; }
inline int env_positive(const char *name, int def) { const int v = std::atoi(env_str(name)); return v > 0 ? v : def; }
// CGRT_RELAY_ORDER's value: a name or its number; -1: none of them
inline int relay_order_named(const char *e) {
    const std::string v(e);
    if (v == "chunks_first" || v == "0") return kRelayChunksFirst;
    if (v == "mirror_first" || v == "1") return kRelayMirrorFirst;
    if (v == "interleaved" || v == "2") return kRelayInterleaved;
    return -1;
}
// CGRT_RELAY_START's value; -1: none of them
inline int relay_start_named(const char *e) {
    const std::string v(e);
    if (v == "list" || v == "0") return kRelayStartList;
    if (v == "cost" || v == "1") return kRelayStartCost;
    return -1;
}
// CGRT_RELAY_BOOST's value: "" (nothing set), off / 0, or num/den; false: none of them (nothing is changed)
inline bool relay_boost_named(const char *e, bool &off, uint32_t &num, uint32_t &den) {
    const std::string v(e);
    if (v.empty()) return true;
    if (v == "off" || v == "0") {
        off = true;
        return true;
    }
    const size_t slash = v.find('/');
    if (slash == std::string::npos || slash == 0 || slash + 1 >= v.size()) return false;
    for (size_t i = 0; i < v.size(); i++)
        if (i != slash && (v[i] < '0' || v[i] > '9')) return false;
    if (slash > 6 || v.size() - slash - 1 > 6) return false;
    const unsigned long n = std::strtoul(v.c_str(), nullptr, 10), d = std::strtoul(v.c_str() + slash + 1, nullptr, 10);
    if (n > kRelayBoostMaxTerm || d < 1 || d > kRelayBoostMaxTerm) return false;
    num = (uint32_t)n;
    den = (uint32_t)d;
    return true;
}
// Lens points staged ahead of the sample loop (cgrt_lens_stage.h; TileOrderPlan::lens_stage): per-lane batches in LDS
static constexpr int kLensStageOff = 0, kLensStageLds = 1;
static constexpr int kLensStageDefault = kLensStageLds;  // the measured form
// CGRT_LENS_STAGE's value; -1: none of them
inline int lens_stage_named(const char *e) {
    const std::string v(e);
    if (v == "off" || v == "0") return kLensStageOff;
    if (v == "lds" || v == "1") return kLensStageLds;
    return -1;
}
// The lens table of classes 0-2 (cgrt_lens_stage.h; TileOrderPlan::lens_table_cap).  CGRT_LENS_TABLE's value; -1: none of them
// Unset, a launch reads the table where it holds its draws and writes it only where the cost probe hides the writing: written
// with nothing beside it, the table costs a frame more than it saves (the measured form)
static constexpr bool kLensTableAlways = false;
inline int lens_table_named(const char *e) {
    const std::string v(e);
    if (v == "off" || v == "0") return 0;
    if (v == "on" || v == "1") return 1;
    return -1;
}
// Read once per process, at the first launch, except CGRT_TIMELINE_FILE, CGRT_RELAY_BOOST and CGRT_RELAY_BOOST_TILES, which every
// launch reads.
inline EyeKnobs eye_knobs() {
    static const EyeKnobs once = [] {
        EyeKnobs k;
        k.force_reorder = env_on("CGRT_FORCE_REORDER");
        k.defer_bytes = std::atoll(env_str("CGRT_DEFER_BYTES"));
        k.heavy_div = env_positive("CGRT_HEAVY_DIV", 32);
        k.units_per_item = (env_positive("CGRT_UNITS_PER_ITEM", 256) + 63) / 64 * 64;
        k.no_primwalk = env_on("CGRT_NO_PRIMWALK");
        k.pw_no_finish = env_on("CGRT_PW_NO_FINISH");
        k.pw_refill = env_positive("CGRT_PW_REFILL", 16);
        k.pw_rounds = env_positive("CGRT_PW_ROUNDS", 8);
        k.lds_pad = std::atoi(env_str("CGRT_LDS_PAD"));
        k.no_hfonly = env_on("CGRT_NO_HFONLY");
        k.no_tile_queue = env_on("CGRT_NO_TILE_QUEUE");
        k.plan_dump = env_on("CGRT_PLAN_DUMP");
        k.no_order_reuse = env_on("CGRT_NO_ORDER_REUSE");
        k.no_sure_tiles = env_on("CGRT_NO_SURE_TILES");
        k.relay_chunks = std::min(std::max(env_positive("CGRT_RELAY_CHUNKS", kRelayDefaultChunks), 2), kRelayMaxChunks);
        k.relay_tiles = std::atoll(env_str("CGRT_RELAY_TILES"));
        if (*env_str("CGRT_RELAY_MIRROR")) k.relay_mirror = env_on("CGRT_RELAY_MIRROR") ? 1 : 0;
        k.relay_order = relay_order_named(env_str("CGRT_RELAY_ORDER"));
        k.relay_start = relay_start_named(env_str("CGRT_RELAY_START"));
        if (k.relay_start < 0 && *env_str("CGRT_RELAY_START"))
            std::fprintf(stderr, "cgrt: CGRT_RELAY_START=%s names no start order of this library (list, cost): the default is used\n", env_str("CGRT_RELAY_START"));
        {
            const int ps = std::atoi(env_str("CGRT_RELAY_PROBE_SPP"));
            if (ps == 1 || ps == 2 || ps == 4) k.relay_probe_spp = ps;
        }
        k.lens_stage = lens_stage_named(env_str("CGRT_LENS_STAGE"));
        // (`area` and `both` name forms that exist only as profiles/experiments/lens_stage_area.patch: said aloud, so that no
        // A/B run takes the default for them)
        if (k.lens_stage < 0 && *env_str("CGRT_LENS_STAGE"))
            std::fprintf(stderr, "cgrt: CGRT_LENS_STAGE=%s names no form of this library (off, lds): the default is used\n", env_str("CGRT_LENS_STAGE"));
        k.lens_table = lens_table_named(env_str("CGRT_LENS_TABLE"));
        if (k.lens_table < 0 && *env_str("CGRT_LENS_TABLE"))
            std::fprintf(stderr, "cgrt: CGRT_LENS_TABLE=%s is neither off nor on: the default is used\n", env_str("CGRT_LENS_TABLE"));
        if (*env_str("CGRT_LENS_TABLE_BYTES")) {
            k.lens_table_bytes = std::max(std::atoll(env_str("CGRT_LENS_TABLE_BYTES")), 0ll);
            k.lens_table_bytes_set = true;
        }
        {
            const std::string v(env_str("CGRT_INSIDE_TRIPS"));
            k.no_inside_trips = v == "off" || v == "0";
            if (!v.empty() && !k.no_inside_trips && v != "on" && v != "1")
                std::fprintf(stderr, "cgrt: CGRT_INSIDE_TRIPS=%s is neither off nor on: the default is used\n", v.c_str());
        }
        return k;
    }();
    EyeKnobs k = once;
    k.timeline_file = *env_str("CGRT_TIMELINE_FILE") ? env_str("CGRT_TIMELINE_FILE") : nullptr;
    // (the promotion knobs too: a threshold sweep or a test sets them between the launches of one process)
    if (!relay_boost_named(env_str("CGRT_RELAY_BOOST"), k.relay_boost_off, k.relay_boost_num, k.relay_boost_den)) {
        static bool said = false;
        if (!said)
            std::fprintf(stderr, "cgrt: CGRT_RELAY_BOOST=%s is neither off nor a threshold num/den (integers, num <= %u, 1 <= den <= %u): the default is used\n",
                         env_str("CGRT_RELAY_BOOST"), kRelayBoostMaxTerm, kRelayBoostMaxTerm);
        said = true;
    }
    if (*env_str("CGRT_RELAY_BOOST_TILES")) k.relay_boost_tiles = std::max(std::atoll(env_str("CGRT_RELAY_BOOST_TILES")), 0ll);
    return k;
}

// =====================================================================================================
// the frame plan
// =====================================================================================================
// What the plan needs of a launch: cgrt_trace_grid's arguments, its eye launch (EyeLaunch), the scene (DeviceScene) and
// the device (read at commit)
struct FrameInputs {
    cgrt_grid grid;
    cgrt_camera cam;
    bool sched, spill, stats, glass;  // the eye launch: form == Sched, and its kernel's flags
    int nt;                           // threads per workgroup: 256, or 64 (one-wave workgroups on 16x4 tiles)
    bool has_mesh, has_bezier, prim_finish, light_ok;
    int prim_obj;
    EyeKnobs knobs;
    size_t mem_total;
    int n_cu, waves_per_simd;  // waves_per_simd: the scheduled kernel's occupancy (kBezWaves, kSchedTreeWaves or 4)
    // What the tile order asks (TileOrderPlan): the eye launch's form == Image and its kernel's flags SPH and PAIR; the scene's
    // order_ok (spheres and planes, 1..kOrderSpheresMax special spheres), whether the handle has its second stream, whether all
    // its objects are spheres, how many there are and how many of them lie in LDS; order_all_special for this camera
    bool image = false, sph = false, pair = false;
    bool order_ok = false, aux_stream = false, all_spheres = false;
    int n_objs = 0, n_lds = 0;
    bool all_special = false;
    // CGRT_GRID_POSED: the launch runs the POSE kernels; the tile order and what hangs on it, the light-tile split and the
    // primary walk reason about rays in the built-in frame and are left out (cgrt.h).  posed_cam: the whole camera of such a
    // launch (its base is `cam` above), which frame_params reads; unposed launches leave it alone
    bool posed = false;
    cgrt_posed_camera posed_cam{};
};

// Where each array of a launch lies in the handle's scratch, in bytes from its start: the chunk sums, then (scheduled
// launches) the schedule arrays and the deferred arrays of kmax heavy tiles, one array after another.
struct ScratchLayout {
    Region partial{}, partial_nhit{}, cost{}, order{}, hidx{}, border{}, plan{}, light{}, dvals{}, dcnt{}, pconst{}, prim_len{}, prim_tri{};
    size_t total = 0;  // bytes to allocate
    void place(GridParams &g, unsigned char *base, bool nhit) const {
        g.partial = partial.in<double>(base);
        g.partial_nhit = nhit ? partial_nhit.in<uint32_t>(base) : nullptr;
        g.cost = cost.in<uint32_t>(base);
        g.order = order.in<uint32_t>(base);
        g.hidx = hidx.in<int32_t>(base);
        g.border = border.in<uint32_t>(base);
        g.plan = plan.in<uint32_t>(base);
        g.light = light.in<unsigned char>(base);
        g.dvals = dvals.in<double>(base);
        g.dcnt = dcnt.in<unsigned char>(base);
        g.pconst = pconst.in<double>(base);
        g.prim_len = prim_len.in<double>(base);
        g.prim_tri = prim_tri.in<int32_t>(base);
    }
};

// The tile order of an image-order launch of a sphere scene (tile_order_kernel; GridParams::tile_order)
struct TileOrderPlan {
    bool on = false;  // the launch runs through the ordered list (order_tiles)
    // who renders the list's class-3 tiles, those that see no mirror or glass: the eye launch's own body like every other tile
    // (kOrderAll), the terminal-diffuse variant in a launch of its own on the second stream (kOrderFull + kOrderDiffuse), or the
    // terminal-diffuse body inside the PAIR variant (kOrderAllDiffuse)
    enum Class3 { None, SecondLaunch, InKernel } class3 = None;
    bool masks = false;  // tile_order_kernel writes the wave tiles' sphere masks (GridParams::wmask)
    // sure_first_kernel writes the sphere every ray of a class-3 wave tile hits first (GridParams::wsure): wherever there are masks,
    // unless CGRT_GRID_NO_SURE_TILES or the knob CGRT_NO_SURE_TILES switches it off
    bool sure = false;
    // kLensStageLds: the terminal-diffuse body inside the launch stages its lens draws in batches (GridParams::lens_batch)
    int lens_stage = kLensStageOff;
    // lens_table_cap > 0: lens_table_kernel writes the lens draws of the list's first lens_table_cap entries, as far as they are of
    // classes 0-2, into a table of lens_table_bytes on the handle, and the launch runs the table-reading twin of its kernel
    // (GridParams::lens_table; a launch that cannot have the table goes without).  lens_table_always: a launch that does not find
    // its draws in the table writes them wherever it stands; false: only beside its cost probe, and otherwise it goes without
    size_t lens_table_cap = 0, lens_table_bytes = 0;
    bool lens_table_always = false;
};

// Whether a launch of n_tiles tiles relays samples by default: at 32 samples or more (two chunks of 16), and with every workgroup
// slot of the device -- four 256-thread workgroups a CU -- taken at least once, so that the extra workgroups find the chip full
// of other work; CGRT_GRID_SAMPLE_RELAY lifts the second condition, CGRT_GRID_NO_SAMPLE_RELAY switches the relay off.
inline bool relay_engaged(int32_t flags, int32_t spp, size_t n_tiles, int n_cu) {
    if ((flags & CGRT_GRID_NO_SAMPLE_RELAY) || spp < 2 * kRelayMinChunkSpp) return false;
    return (flags & CGRT_GRID_SAMPLE_RELAY) || n_tiles >= (size_t)4 * (size_t)n_cu;
}

// The form of an engaged relay: relay_block_ordered's extent and order, whether the workgroups start by cost, and whether a launch
// that does promotes.  For each: what the launch's flags name holds (off before on); else the knob (CGRT_RELAY_MIRROR / _ORDER /
// _START / _BOOST=off); else a launch that asked for the relay (CGRT_GRID_SAMPLE_RELAY) relays classes 0 and 1, chunk workgroups
// first, from the list -- what that flag has always meant -- and one that names an order, by flag or knob, gets the list it named;
// only the launch that relays by default and names no order takes the measured form (kRelayDefaultExtent / kRelayDefaultOrder,
// by cost), and it promotes unless it names a start, by flag or knob.
static constexpr int kRelayDefaultExtent = kRelayMirror, kRelayDefaultOrder = kRelayInterleaved;
struct RelayRule { int extent, order, start; bool boost; };
inline RelayRule relay_rule(int32_t f, const EyeKnobs &kn) {
    const bool asked = (f & CGRT_GRID_SAMPLE_RELAY) != 0;  // the launch asked for the relay
    const int32_t order_flag = f & CGRT_GRID_RELAY_ORDER_MASK;
    const bool measured = !asked && !order_flag && kn.relay_order < 0;  // it names no order either
    const bool names_start = (f & (CGRT_GRID_NO_RELAY_COST_START | CGRT_GRID_RELAY_COST_START)) || kn.relay_start >= 0;
    RelayRule r;
    r.extent = (f & CGRT_GRID_RELAY_MIRROR) ? kRelayMirror : (f & CGRT_GRID_RELAY_NO_MIRROR) ? kRelayGlass
               : kn.relay_mirror >= 0 ? (kn.relay_mirror ? kRelayMirror : kRelayGlass) : asked ? kRelayGlass : kRelayDefaultExtent;
    r.order = order_flag ? (order_flag == CGRT_GRID_RELAY_MIRROR_FIRST ? kRelayMirrorFirst : order_flag == CGRT_GRID_RELAY_INTERLEAVED ? kRelayInterleaved : kRelayChunksFirst)
              : kn.relay_order >= 0 ? kn.relay_order : asked ? kRelayChunksFirst : kRelayDefaultOrder;
    r.start = (f & CGRT_GRID_NO_RELAY_COST_START) ? kRelayStartList : (f & CGRT_GRID_RELAY_COST_START) ? kRelayStartCost
              : kn.relay_start >= 0 ? kn.relay_start : measured ? kRelayStartCost : kRelayStartList;
    r.boost = (f & CGRT_GRID_NO_RELAY_BOOST) ? false : (f & CGRT_GRID_RELAY_BOOST) ? true : !kn.relay_boost_off && !names_start && measured;
    return r;
}

// The sample relay of a launch (cgrt_relay.h).  An area of the handle's relay buffer holds `cap` tiles, each rendered by k
// workgroups of chunk_spp samples that park in `slots` slots a stream; `bytes` is relay_layout(cap, k, slots).total.
struct RelayArea {
    int k = 0, chunk_spp = 0, slots = 0;
    size_t cap = 0, bytes = 0;
};
static constexpr int kRelayWgPerCu = 4;  // resident workgroups a compute unit of the START variants (256 threads, 4 waves a SIMD)
struct RelayPlan {
    // base.k > 1: the launch relays (the buffer lives on the handle; a launch that cannot have it goes without the relay).
    // boost.k > base.k: it promotes -- its heaviest split tiles by boost.k workgroups, parked in an area of their own behind the base area
    RelayArea base{1, 0, 0, 0, 0}, boost;
    int spp = 0, extent = kRelayGlass, order = kRelayChunksFirst;  // the launch's samples; relay_block_ordered's extent and order
    // kRelayStartCost: the workgroups of classes 0-2 start by probed cost, through a table of start_words words in the order
    // buffer, probed with probe_spp samples; `order` stays the order of a launch that has to go without the table
    int start = kRelayStartList, probe_spp = 0;
    // promotion: the words the table may have more, which are also the workgroups the launch has more; the threshold is num / den
    // of a workgroup slot's even share, over wg_slots slots
    size_t start_words = 0, boost_words = 0;
    uint32_t num = 0, den = 1;
    int wg_slots = 0;
    bool relays() const { return base.k > 1; }
    bool boosts() const { return boost.k > base.k; }
    // the handle's relay buffer: the base area, then (boosts()) the boost area
    size_t boost_at() const { return align256(base.bytes); }
    size_t bytes() const { return boosts() ? boost_at() + boost.bytes : base.bytes; }
    // workgroups of a launch over n_tiles tiles; `boosted`: it has the promoted form's table
    size_t grid(size_t n_tiles, bool boosted) const { return relay_grid(n_tiles, base.k, base.cap) + (boosted ? boost_words : 0); }
    RelayBoost boost_rule() const {
        return boosts() ? RelayBoost{(uint32_t)boost.k, (uint32_t)boost.cap, boost.chunk_spp, num, den, (uint32_t)wg_slots} : RelayBoost{};
    }
    RelayItems items(uint32_t n01, uint32_t n012, uint32_t n_tiles) const {
        return RelayItems{(uint32_t)base.k, n01, n012, n_tiles, (uint32_t)base.cap, extent, base.chunk_spp, spp};
    }
    TileOrderLayout order_layout(size_t n_tiles, size_t n_wt, bool sure) const {
        return tile_order_layout(n_tiles, n_wt, sure, start_words, boost_words, base.cap, boost.k);
    }
    // g's relay fields, for the buffer at `buf`
    void place(GridParams &g, unsigned char *buf) const {
        g.relay = buf;
        g.relay_k = base.k;
        g.relay_chunk_spp = base.chunk_spp;
        g.relay_cap = (int32_t)base.cap;
        g.relay_slots = base.slots;
        g.relay_extent = extent;
        g.relay_order = order;
        if (!boosts()) return;
        g.relay_boost_off = boost_at();
        g.boost_k = boost.k;
        g.boost_chunk_spp = boost.chunk_spp;
        g.boost_cap = (int32_t)boost.cap;
        g.boost_slots = boost.slots;
    }
};
// The relay of a launch that may have one (frame_plan: the PAIR variant's one-launch tile order) over n_tiles tiles
inline RelayPlan relay_plan(const cgrt_grid &gr, const EyeKnobs &kn, size_t n_tiles, int n_cu, size_t mem_total) {
    RelayPlan r;
    if (!relay_engaged(gr.flags, gr.spp, n_tiles, n_cu)) return r;
    const auto area = [&gr](const RelayChunks &c, size_t tiles, size_t budget, long long bound) {
        RelayArea a{c.k, c.chunk_spp, relay_slots(c.chunk_spp, gr.max_depth), 0, 0};
        a.cap = relay_cap(tiles, a.k, a.slots, budget, bound);
        a.bytes = relay_layout(a.cap, a.k, a.slots).total;
        return a;
    };
    const RelayChunks rc = relay_chunks(gr.spp, (gr.flags & CGRT_GRID_SAMPLE_RELAY_4) ? kRelayMaxChunks : kn.relay_chunks);
    const RelayArea base = rc.k > 1 ? area(rc, n_tiles, relay_budget(mem_total), kn.relay_tiles) : RelayArea{};
    if (base.cap == 0) return r;  // (fewer than 32 samples, or no room for a tile)
    const RelayRule f = relay_rule(gr.flags, kn);
    r.base = base;
    r.spp = gr.spp, r.extent = f.extent, r.order = f.order;
    r.start = n_tiles < kRelayStartMaxTiles ? f.start : kRelayStartList;
    if (r.start != kRelayStartCost) return r;
    r.probe_spp = std::min(kn.relay_probe_spp, (int)gr.spp);
    r.start_words = relay_start_words(n_tiles, base.k, base.cap);
    const RelayChunks rb = relay_chunks(gr.spp, kRelayMaxChunks);
    if (rb.k <= rc.k || !f.boost || kn.relay_boost_tiles == 0) return r;
    const RelayArea boost = area(rb, base.cap, relay_boost_budget(mem_total, r.boost_at()), kn.relay_boost_tiles);
    if (boost.cap == 0) return r;
    r.boost = boost;
    r.boost_words = relay_boost_extra(base.k, boost.k, boost.cap);
    r.num = kn.relay_boost_num, r.den = kn.relay_boost_den;
    r.wg_slots = n_cu * kRelayWgPerCu;
    return r;
}

struct FramePlan {
    int chunks = 1, chunk_spp = 0;  // CGRT_GRID_SPLIT_SAMPLES: workgroups per tile, samples per workgroup
    bool xcd_tiles = false;         // XCD-aware super-tiles, else row-major (tile_of_block)
    int maxhp = 1;                  // Hitpoints per sample: a mirror chain ends in one, a glass tree of depth 5 in <= 16
    int tile_blocks = 0;            // workgroups over the tiles of one chunk
    size_t grid_dim = 0;            // the launch's tile workgroups (behind heavy_blocks unit-form ones)
    int wtiles_x = 0, wtiles_y = 0;
    size_t n_wt = 0, tile_bytes = 0, kmax = 0;  // wave tiles; deferred bytes per heavy tile; heavy tiles they hold (0: image order)
    bool use_prim = false;                      // the primary walk's distances and triangles (in tile_bytes)
    // kmax > 0 only (off / 0 otherwise)
    bool split_light = false, tile_queue = false, prim_done = false;
    int wave_slots = 0, items_per_tile = 1, heavy_blocks = 0;
    unsigned long long plan_div = 0;  // plan_kernel: heavy when cost x spp > total x spp / plan_div
    ScratchLayout scratch;
    TileOrderPlan order;
    RelayPlan relay;  // the sample relay of the launch (relay.relays()), decided by relay_plan
};

// The launch at capacity kmax (0 when it is not scheduled): a function of the inputs and kmax only
inline FramePlan frame_plan(const FrameInputs &in, size_t kmax) {
    const cgrt_grid &gr = in.grid;
    const EyeKnobs &kn = in.knobs;
    FramePlan p;
    p.chunk_spp = gr.spp;
    p.xcd_tiles = !in.spill && in.has_mesh && !in.has_bezier;
    p.maxhp = in.glass ? 16 : 1;
    // Split a tile's samples over several workgroups (CGRT_GRID_SPLIT_SAMPLES, opt-in for every scene since the cost
    // scheduler balances Bezier scenes too): chunks of >= 16 samples, at most 16 chunks, at most 4 GiB of chunk sums.
    const size_t npx = (size_t)gr.rows * gr.width;
    if ((gr.flags & CGRT_GRID_SPLIT_SAMPLES) && gr.spp >= 32 && !in.spill) {
        int chunks = std::min(gr.spp / 16, 16);
        while (chunks > 1 && (size_t)chunks * npx * 28 > ((size_t)4 << 30)) chunks--;
        if (chunks > 1) {
            p.chunk_spp = (gr.spp + chunks - 1) / chunks;
            p.chunks = (gr.spp + p.chunk_spp - 1) / p.chunk_spp;
        }
    }
    // Bezier scenes run one-wave workgroups on 16x4 tiles (TileGeom<64>): waves over the vase outlast their neighbours ~100x
    const bool one_wave = in.nt == 64;
    const int waves_per_block = in.nt / 64;
    p.tile_blocks = one_wave ? tile_grid_blocks(gr.width, gr.rows, false, kWaveTileW, kWaveTileH)
                             : tile_grid_blocks(gr.width, gr.rows, p.xcd_tiles);
    p.grid_dim = (size_t)p.tile_blocks * p.chunks;
    // The tile order: image order, one workgroup per tile with all its samples, row-major, 256 threads.  The second launch for
    // class 3 is for the plain sphere variant (no SPILL, no STATS; not a timeline launch, which is one launch) where the caller
    // asks for it and the handle has the stream; otherwise the PAIR variant renders class 3 by the body it carries.  Neither
    // where no tile can be of class 3 at all (all_special).  Sphere masks: where a terminal-diffuse body runs, in either form,
    // over a list of at most 32 spheres, all of them in LDS.  The relay is the PAIR variant's, in its one-launch forms.  A launch
    // that asks for split samples and gets one chunk (fewer than 32 samples, or sums beyond 4 GiB) keeps the tile order, without
    // the second launch and without the relay.  (For a committed scene `on` takes nothing from what the second launch asks by
    // itself: order_ok means no mesh, hence row-major tiles, and without split_asked there is one chunk.)
    TileOrderPlan &o = p.order;
    const bool split_asked = (gr.flags & CGRT_GRID_SPLIT_SAMPLES) != 0;
    o.on = in.image && p.chunks == 1 && !p.xcd_tiles && in.nt == kThreads && in.order_ok && !(gr.flags & CGRT_GRID_NO_TILE_ORDER) && !in.posed;
    if (o.on && !in.all_special) {
        if (in.sph && !in.spill && !in.stats && in.aux_stream && (gr.flags & CGRT_GRID_DIFFUSE_TILES) && !split_asked && !kn.timeline_file)
            o.class3 = TileOrderPlan::SecondLaunch;
        else if (in.pair)
            o.class3 = TileOrderPlan::InKernel;
    }
    o.masks = o.class3 != TileOrderPlan::None && in.all_spheres && in.n_objs <= kSphereMaskMax && in.n_objs == in.n_lds &&
              !(gr.flags & CGRT_GRID_NO_SPHERE_MASKS);
    o.sure = o.masks && !(gr.flags & CGRT_GRID_NO_SURE_TILES) && !kn.no_sure_tiles;
    // Lens stage: the thin-lens terminal-diffuse body INSIDE the launch, whose batches lie in the launch's pending-ray levels;
    // the second launch's variant asks for no such LDS and draws sample by sample.  CGRT_GRID_NO_LENS_STAGE switches it off;
    // otherwise the knob CGRT_LENS_STAGE holds, and the default where it names nothing.
    if (o.class3 == TileOrderPlan::InKernel && in.cam.lens_radius > 0 && !(gr.flags & CGRT_GRID_NO_LENS_STAGE))
        o.lens_stage = kn.lens_stage >= 0 ? kn.lens_stage : kLensStageDefault;
    if (o.on && in.pair && o.class3 != TileOrderPlan::SecondLaunch && !split_asked)
        p.relay = relay_plan(gr, kn, (size_t)p.tile_blocks, in.n_cu, in.mem_total);
    // Lens table: the same launches as the relay's, whether or not they relay, under a thin lens -- the full and the parking body
    // read their draws from the handle's table.  CGRT_GRID_NO_LENS_TABLE switches it off and CGRT_GRID_LENS_TABLE has every
    // launch write what it does not find; otherwise the knob CGRT_LENS_TABLE holds (off, on: the same two), and where it names
    // nothing a launch writes the table only beside its cost probe (kLensTableAlways).  None of them touches the LDS stage of
    // class 3 above, nor does that one's flag touch the table.
    const int lens_table = (gr.flags & CGRT_GRID_NO_LENS_TABLE) ? 0 : (gr.flags & CGRT_GRID_LENS_TABLE) ? 1 : kn.lens_table;
    if (o.on && in.pair && o.class3 != TileOrderPlan::SecondLaunch && !split_asked && in.cam.lens_radius > 0 && lens_table != 0) {
        const size_t budget = kn.lens_table_bytes_set ? (size_t)kn.lens_table_bytes : kLensTableBudget;
        o.lens_table_cap = lens_table_cap((size_t)p.tile_blocks, gr.spp, kThreads, budget);
        o.lens_table_bytes = lens_table_bytes(o.lens_table_cap, gr.spp, kThreads);
        o.lens_table_always = o.lens_table_cap > 0 && (lens_table > 0 || kLensTableAlways);
    }
    p.wtiles_x = (gr.width + kWaveTileW - 1) / kWaveTileW;
    p.wtiles_y = (gr.rows + kWaveTileH - 1) / kWaveTileH;
    p.n_wt = (size_t)p.wtiles_x * p.wtiles_y;
    // primary-ray mesh hits of the heavy tiles' units (cgrt_primwalk.hpp): a double and an int per unit
    p.use_prim = in.sched && in.prim_obj >= 0 && !kn.no_primwalk && !(gr.flags & CGRT_GRID_STATS) && !in.posed;
    // per heavy tile: its Hitpoint values [spp][maxhp][64 px][3], their counts [spp][64 px] (padded to 8 bytes), the pixel
    // constants [7][64] and, with the primary walk, its distances and triangles [spp][64]
    const size_t units = (size_t)gr.spp * 64;
    const size_t vals = units * (size_t)p.maxhp * 3 * sizeof(double), cnt = (units + 7) & ~(size_t)7, pconst = 7 * 64 * sizeof(double),
                 plen = p.use_prim ? units * sizeof(double) : 0, ptri = p.use_prim ? units * sizeof(int32_t) : 0;
    p.tile_bytes = vals + cnt + pconst + plen + ptri;
    p.kmax = in.sched ? kmax : 0;

    ScratchLayout &L = p.scratch;
    size_t end = 0;  // the arrays one after another; used == false: room kept, nothing placed
    const auto take = [&end](size_t bytes, bool used = true) { end += bytes; return Region{end - bytes, used ? bytes : 0}; };
    if (p.chunks > 1) {
        L.partial = take((size_t)p.chunks * npx * 3 * sizeof(double));
        L.partial_nhit = take((size_t)p.chunks * npx * sizeof(uint32_t));
    }
    L.total = end = align256(end);
    if (!in.sched) return p;
    // cost, order, hidx, border (8 entries of slack each), plan[64], light: reserved even when no heavy tile fits
    const size_t np = (p.n_wt + 8) * sizeof(uint32_t), sched_bytes = align256(4 * np + 64 * sizeof(uint32_t) + align256(p.n_wt));
    L.total += sched_bytes + (p.kmax ? p.kmax * p.tile_bytes + 256 : 0);
    if (p.kmax == 0) return p;
    p.split_light = in.light_ok && p.chunks == 1 && !in.stats && !in.posed;
    // tiles through a queue too (GridParams::border) unless their samples are split over workgroups or the workgroups are
    // single waves (trace_grid_sched_kernel)
    p.tile_queue = p.chunks == 1 && !one_wave && !kn.no_tile_queue;
    p.prim_done = p.use_prim && in.prim_finish && !kn.pw_no_finish;
    // heavy: cost x spp > (total cost x spp / wave slots) / heavy_div
    p.wave_slots = in.n_cu * 4 * in.waves_per_simd;
    p.plan_div = (unsigned long long)p.wave_slots * (unsigned long long)kn.heavy_div;
    p.items_per_tile = (int)((units + kn.units_per_item - 1) / kn.units_per_item);
    // enough heavy workgroups to fill the chip once: they loop over the item queue until it is empty
    const size_t fill = (size_t)p.wave_slots / waves_per_block;
    p.heavy_blocks = (int)std::min((p.kmax * (size_t)p.items_per_tile + waves_per_block - 1) / waves_per_block, fill);
    if (p.tile_queue) p.grid_dim = fill;  // tile workgroups: a chip's worth, each loops over the tile queue
    const size_t sched_at = end;
    L.cost = take(np);
    L.order = take(np);
    L.hidx = take(np);
    L.border = take(np, p.tile_queue);
    L.plan = take(64 * sizeof(uint32_t));
    L.light = take(p.n_wt, p.split_light);
    end = sched_at + sched_bytes;
    L.dvals = take(p.kmax * vals);
    L.dcnt = take(p.kmax * cnt);
    L.pconst = take(p.kmax * pconst);
    L.prim_len = take(p.kmax * plen);
    L.prim_tri = take(p.kmax * ptri);
    return p;
}

// Heavy tiles the deferred arrays may hold before the device is asked: up to 12 GiB, at most an eighth of the scene's
// device (MI355X: 288 GB; read at commit -- a process may drive devices of different sizes), or CGRT_DEFER_BYTES
inline size_t max_heavy_tiles(const FrameInputs &in) {
    if (!in.sched) return 0;
    const FramePlan p = frame_plan(in, 0);
    const size_t budget = in.knobs.defer_bytes > 0 ? (size_t)in.knobs.defer_bytes : std::min((size_t)12 << 30, in.mem_total / 8);
    return std::min(budget / p.tile_bytes, p.n_wt);
}

// A size the device has refused before (refused; 0: none) is not asked for again -- every attempt is a synchronous hipFree
// plus failing hipMallocs: the deferred arrays shrink, fewer heavy tiles and the same image, until the need lies below it
inline size_t fit_heavy_tiles(const FrameInputs &in, size_t kmax, size_t refused) {
    while (refused && kmax > 0 && frame_plan(in, kmax).scratch.total >= refused) kmax /= 2;
    return kmax;
}

// The launch's GridParams, scratch not yet placed
inline GridParams frame_params(const FrameInputs &in, const FramePlan &p) {
    GridParams g = grid_params(in.posed ? &in.posed_cam.base : &in.cam, &in.grid);
    g.xcd_tiles = p.xcd_tiles ? 1 : 0;
    g.chunks = p.chunks;
    g.chunk_spp = p.chunk_spp;
    g.maxhp = p.maxhp;
    g.units_per_item = in.knobs.units_per_item;
    g.pw_refill = in.knobs.pw_refill;
    g.pw_rounds = in.knobs.pw_rounds;
    g.items_per_tile = p.items_per_tile;
    g.heavy_blocks = p.heavy_blocks;
    g.lens_batch = p.order.lens_stage == kLensStageLds ? 1 : 0;
    g.lens_table_cap = (int32_t)p.order.lens_table_cap;  // (the table itself: lens_table_prepare, which clears this where there is none)
    g.lens_table_spp = p.order.lens_table_cap ? in.grid.spp : 0;
    if (p.heavy_blocks > 0 && p.use_prim) {
        g.prim_obj = in.prim_obj;
        g.prim_done = p.prim_done ? 1 : 0;
    }
    return g;
}

#endif
