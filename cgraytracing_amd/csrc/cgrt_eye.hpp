// The eye pass: trace_grid_kernel and the function-level probe kernel.  Part of libcgrt.so (cgrt_hip.hip).
#ifndef CGRT_EYE_HPP
#define CGRT_EYE_HPP
#include "cgrt_lens_stage.h"
#include "cgrt_scene_walk.hpp"
#include "cgrt_sphere_mask.h"
#include "cgrt_sure_first.h"
#include "cgrt_variants.h"

// =====================================================================================================
// the eye pass
// =====================================================================================================
struct Pending {  // a refracted child waiting for its turn (main.cpp:157)
    V3 o, d, adj;
    int32_t depth_left;
    uint32_t path;
};

// GLASS: the scene contains a transparent object, so refracted children can be pending; without it the
// pending-ray storage (LDS levels, sibling registers) is compiled out and occupancy goes up.
// SPH: every object is a sphere (C1/C2-type scenes): specialised object loop.
// HPS: additionally append every Hitpoint {f, pos, normal} (hitpoints.h:6-20, main.cpp:87-98) to a global stream.
// PAIR (SPH with GLASS, the variants the tile order serves): the sphere loop takes two spheres a trip as two independent
// instruction chains (sphere_len_pair) -- the frame ends with a few waves over the glass sphere, each alone on its SIMD and bound
// by its own dependent fp64 chain.
// DIFF (SPH without GLASS): the terminal-diffuse body for tiles none of whose rays can meet a reflecting or refracting sphere
// (class 3 of tile_order_kernel): every ray ends at its first hit with adj == (1, 1, 1), so neither the hit point, the normal,
// the material dispatch nor any pending-ray state exists in it.
#ifndef CGRT_DIFF_WAVES
#define CGRT_DIFF_WAVES 8
#endif
#ifndef CGRT_DIFF_DOF_WAVES
#define CGRT_DIFF_DOF_WAVES 6
#endif
// waves per SIMD the DIFF variants are compiled for: the pinhole one fits 8 (52 VGPRs); the thin-lens one spills 4 VGPRs at 8
// (64) and is compiled for 6
static constexpr int kDiffWaves = CGRT_DIFF_WAVES, kDiffDofWaves = CGRT_DIFF_DOF_WAVES;
// (kBezWaves, kTreeWaves and kSchedTreeWaves, the other variants' occupancies, stand in cgrt_variants.h: the launch plans read them)

// uniform_sampling_circle (sampling.h:35-43) on a sample's lens stream (cgrt_rng.hpp): attempt j takes the two draws of the
// splitmix output z_j = fin64(key + (j + 1) G) -- what Stream::pair returns at position 2j, with the 64-bit multiply of the
// counter replaced by a running addition (the same integers mod 2^64).  Shared by every kernel that starts a primary ray.
__host__ __device__ __forceinline__ void lens_disc(uint64_t k_smp, double &sx, double &sy) {  // (host: cgrt_camera_rays_host)
    uint64_t ctr = k_smp;
    while (true) {
        ctr += kGolden;
        const uint64_t z = fin64(ctr);
        const double ux = div_rand_max((uint32_t)(z >> 33)), uy = div_rand_max((uint32_t)((z >> 2) & 0x7fffffffu));
        sx = ux * 2.0 - 1;
        sy = uy * 2.0 - 1;
        if (sx * sx + sy * sy < 1) break;
    }
}

// A point of the camera's frame in the world (pose_point, cgrt_frame.h): the POSE kernels' primary rays start from these
__device__ __forceinline__ V3 pose_v(const GridParams &g, const V3 &p) {
    V3 w;
    pose_point(g, p.x, p.y, p.z, w.x, w.y, w.z);
    return w;
}

struct HitpointSink {
    double *rec;                // cap x 10 doubles: f(3) pos(3) normal(3) label
    unsigned long long *count;  // appended so far (may exceed cap: then the tail was dropped)
    unsigned long long cap;
};

// Whether this wave of a tile workgroup has a wave tile to render in this launch -- the decisions trace_grid_body makes below,
// ahead of everything else: a workgroup none of whose waves has one (tiles of the other launch of a light / full pair, heavy
// tiles, tiles outside the image: three quarters of a probe launch's workgroups on C3) leaves before it stages the object list
// and the node cache in LDS.
template <int NT>
__device__ __forceinline__ bool wave_has_tile(const GridParams &g, int tile_block, int tile_grid) {
    using TG = TileGeom<NT>;
    const int wave = threadIdx.x >> 6;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW, wtiles_y = (g.rows + kWaveTileH - 1) / kWaveTileH;
    int tile_x, tile_y;
    if (tile_grid < 0) {
        const int tiles_x = (g.W + TG::W - 1) / TG::W;
        tile_x = tile_block % tiles_x;
        tile_y = tile_block / tiles_x;
    } else {
        const int tile_blocks = tile_grid / g.chunks;
        if (!tile_of_block(g, tile_block % tile_blocks, tile_x, tile_y, TG::W, TG::H)) return false;
    }
    const int wx = tile_x * (TG::W / kWaveTileW) + (NT == 256 ? (wave & 1) : 0);
    const int wy = tile_y * (TG::H / kWaveTileH) + (NT == 256 ? (wave >> 1) : 0);
    if (!(wx < wtiles_x && wy < wtiles_y)) return false;
    if (g.hidx && g.hidx[wy * wtiles_x + wx] >= 0) return false;
    if (g.light && (g.light[wy * wtiles_x + wx] != 0) != (g.light_mode != 0)) return false;
    return true;
}

// A workgroup's part in the sample relay (cgrt_relay.h), workgroup-uniform: slot >= 0 -- it renders chunk `chunk` of the
// relayed tile in slot `slot` of the relay area, samples [s0, s1); slot < 0: not relayed, all the launch's samples.
// boost (the START variants only): the tile is promoted -- slot is its slot of the boost area, whose form relay_form gives.
struct RelayWg {
    int slot = -1, chunk = 0, s0 = 0, s1 = 0, boost = 0;
};
// The area a relayed workgroup's tile lies in and its form (workgroup-uniform; asked for at each point of use, so that nothing
// of it lives across the ray loop): the launch's base form, or for a promoted tile the boost area's.  Without COST -- the
// variants that read no table -- the expressions are the base form's, as they stood.
struct RelayForm {
    unsigned char *area;
    size_t cap;
    int k, slots;
};
template <bool COST>
__device__ __forceinline__ RelayForm relay_form(const GridParams &g, const RelayWg &rw) {
    if (COST && rw.boost) return RelayForm{g.relay + g.relay_boost_off, (size_t)g.boost_cap, g.boost_k, g.boost_slots};
    return RelayForm{g.relay, (size_t)g.relay_cap, g.relay_k, g.relay_slots};
}

// The body of the eye pass for one workgroup.  HEAVY selects how the waves get their work (see GridParams): false -- each
// wave owns one wave tile (16x4 pixels, one per lane) and every lane runs its pixel's samples; true -- the waves serve the
// queue of heavy-tile items, lanes drawing (pixel, sample) units.  tile_block / tile_grid: this workgroup's index among the
// tile workgroups and their number (the launch may put heavy workgroups in front of them).
// PARK (PAIR variants, chunks >= 1 of a relayed tile): a Hitpoint value is not added but stored, slot after slot, in the lane's
// stream of the relay area; the body keeps no sums.  A relayed workgroup (rw.slot >= 0; PAIR with or without PARK) leaves its
// sums or counts in the area, and the last of the tile's workgroups to arrive adds them up in chunk order and stores the pixels.
// COST (the PAIR variants with a start table, trace_grid_kernel's START): the body also serves as the relay's cost probe
// (g.probe == 2) and leaves the wave's iteration count; every other variant is spared the test.
// LSTAGE (DIFF with DOF, the body inside the PAIR variants' launch only): with g.lens_batch the wave stages its lens draws in
// batches (cgrt_lens_stage.h), in the part of the launch's LDS that holds the PAIR body's pending-ray levels.
// LTAB (the full and the parking body of the thin-lens PAIR variants' table-reading twins): the lens draws of this workgroup's
// samples lie in the lens table (cgrt_lens_stage.h), lens_row = table[entry][0][0] of its list entry (workgroup-uniform); the body
// computes no sample key and runs no rejection loop.
// POSE (the kernels of a launch with CGRT_GRID_POSED, cgrt.h): the camera's frame stands in the world (g.pose_*); a pixel's
// direction and focus point, the eye and every lens point are the images of the frame's points under pose_point, the direction
// normalised from those (cgrt_frame.h has the definition).  Without POSE none of it is compiled.
template <bool TREES, bool BEZ, bool DOF, bool GLASS, bool SPH, bool STATS, bool HPS, int NT, bool HEAVY, bool SPILL = false, bool HFONLY = false,
          bool DIFF = false, bool PAIR = false, bool PARK = false, bool LSTAGE = false, bool COST = false, bool LTAB = false, bool POSE = false>
__device__ __forceinline__ void trace_grid_body(const DeviceScene &sc, const GridParams &g, float *__restrict__ rgb,
                                                uint32_t *__restrict__ nhit_out, unsigned long long *__restrict__ counters,
                                                const HitpointSink &hps, int tile_block, int tile_grid, const RelayWg rw = RelayWg{},
                                                const uint64_t *__restrict__ lens_row = nullptr) {
    using TG = TileGeom<NT>;
    static_assert(!LTAB || (PAIR && DOF && !LSTAGE), "LTAB: the thin-lens PAIR variants' full and parking bodies");
    static_assert(!PARK || (PAIR && NT == kRelayThreads), "PARK: a relayed tile's later chunks");
    static_assert(!DIFF || (SPH && !GLASS && !HPS && !HEAVY && !STATS && !SPILL), "DIFF: the sphere loop, first hits only");
    static_assert(!PAIR || (SPH && GLASS && !HPS && !HEAVY && !STATS && !SPILL), "PAIR: the glass sphere variants of the tile order");
    static_assert(!LSTAGE || (DIFF && DOF && !PAIR), "LSTAGE: the thin-lens terminal-diffuse body inside a PAIR launch");
    static_assert(!COST || PAIR, "COST: the PAIR variants with a start table");
    static_assert(!POSE || (!DIFF && !PAIR && !LSTAGE && !LTAB), "POSE: no body of the tile order, whose tests stand in the built-in frame");
    // (the launch asked for the PAIR body's LDS -- pending-ray levels, then the object list; this body's object list lies at the
    // start and its batches behind it: they fit where the levels are, so the request and the occupancy stay what they were)
    static_assert(!LSTAGE || lens_batch_lds(NT) <= (size_t)kLdsLevels * pending_level_bytes(NT), "the lens batches fit the PAIR launch's pending-ray levels");
    const long long tl_t0 = g.timeline ? wall_clock64() : 0;
    if (!HEAVY && !g.timeline) {  // (the timeline, a development aid, wants a record from every workgroup)
        if (!__syncthreads_or((int)wave_has_tile<NT>(g, tile_block, tile_grid))) return;
    }
    // LDS carve-up, written out here: wg_lds()'s regions for wg_ask_trace(NT, TREES, BEZ, GLASS, SPILL, HFONLY) (cgrt_wg_lds.h, whose
    // total the launch requested; the static_assert below holds the two together) -- this body's code generation is measured to
    // the percent and did not keep its speed through the shared wg_lds_carve.
    // WALK: HFONLY walks height fields only and has neither node cache nor wide-walk stack.
    constexpr size_t level_bytes = pending_level_bytes(NT), stack_bytes = (size_t)kLdsLevels * level_bytes;
    constexpr bool WALK = TREES && !HFONLY;
    {   // the header's layout for 3 objects, 5 cached nodes and a wide tree has the regions and sizes written out below
        constexpr WgLds chk = wg_lds(wg_ask_trace(NT, TREES, BEZ, GLASS, SPILL, HFONLY), 3, 5, true);
        static_assert(chk.pending == 0 && chk.objs == (GLASS ? stack_bytes : 0) && chk.staging - chk.objs == 3 * sizeof(ObjRec) &&
                          chk.bez - chk.staging == (SPILL ? (NT / 64) * sizeof(ObjRec) : 0) &&
                          chk.nodes - chk.bez == (BEZ ? (NT / 64) * sizeof(BezLds) : 0) &&
                          chk.wstack - chk.nodes == (WALK ? 5 * sizeof(NodeRec) : 0) && chk.has.nodes == WALK &&
                          chk.has.wstack == (WALK && !GLASS && !BEZ),
                      "trace_grid_body's carve-up and cgrt_wg_lds.h");
    }
    extern __shared__ __align__(16) unsigned char lds_raw[];
    ObjRec *lobjs = reinterpret_cast<ObjRec *>(lds_raw + (GLASS ? stack_bytes : 0));  // n_objs records
    // BEZ: one BezLds per wave behind the object list (16-byte aligned: ObjRec is 128 B)
    unsigned char *lrest = reinterpret_cast<unsigned char *>(lobjs + sc.n_lds);
    LdsAux aux;
    if (SPILL) {  // one staging record per wave for the objects beyond the LDS list
        aux.spill = reinterpret_cast<ObjRec *>(lrest) + (threadIdx.x >> 6);
        lrest += (NT / 64) * sizeof(ObjRec);
    }
    aux.bl = BEZ ? reinterpret_cast<volatile BezLds *>(lrest) + (threadIdx.x >> 6) : nullptr;
    if (BEZ) lrest += (NT / 64) * sizeof(BezLds);
    // TREES: node cache behind that (32-byte records, region is 16-byte aligned)
    NodeRec *lnodes = reinterpret_cast<NodeRec *>(lrest);
    aux.lnodes = (WALK && sc.cached_tree >= 0) ? lnodes : nullptr;
    // TREES without glass or Bezier (their LDS is spoken for): the first entries of the wide walk's stack, behind the node cache
    aux.wstack = (WALK && !GLASS && !BEZ && sc.has_wide)
                     ? reinterpret_cast<uint2 *>(lrest + ((sc.cached_tree >= 0 ? (size_t)sc.cached_nodes * sizeof(NodeRec) : 0)))
                     : nullptr;
    if (WALK && sc.cached_tree >= 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(sc.nodes + sc.trees[sc.cached_tree].node_begin);
        uint4 *dst = reinterpret_cast<uint4 *>(lnodes);
        const int n16 = sc.cached_nodes * (int)(sizeof(NodeRec) / 16);
        for (int k = threadIdx.x; k < n16; k += NT) dst[k] = src[k];
    }

    // stage the primitive list in LDS (128 B records, copied as 16-byte pieces)
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(sc.objs);
        uint4 *dst = reinterpret_cast<uint4 *>(lobjs);
        const int n16 = sc.n_lds * (int)(sizeof(ObjRec) / 16);
        for (int k = threadIdx.x; k < n16; k += NT) dst[k] = src[k];
    }
    __syncthreads();
    const long long cost_t0 = g.probe ? (long long)clock64() : 0;

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW, wtiles_y = (g.rows + kWaveTileH - 1) / kWaveTileH;
    const V3 camorg = mk(g.cam[0], g.cam[1], g.cam[2]);
    const V3 camw = POSE ? pose_v(g, camorg) : camorg;  // the eye in the world
    // HEAVY: this launch's waves serve the queue of heavy-tile items instead of owning a tile each (its own kernel variant:
    // the per-unit pixel state costs registers the tile variant does not have to spare).
    constexpr bool heavy = HEAVY;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;

    // ---- the pixel a lane is working on: fixed for a tile's wave, set per unit for a heavy wave ----
    int wx = 0, wy = 0, chunk = 0, s_end = 0;
    bool have_tile = false;
    int w = 0, j = 0, h = 0;
    bool live = false;
    V3 pdir = mk(0, 0, 1), pof = mk(0, 0, 0);
    uint64_t k_pix = 0;
    auto set_pixel = [&](int lx, int ly) {  // lane-local pixel (lx, ly) of wave tile (wx, wy); main.cpp:188-189,198,203
        w = wx * kWaveTileW + lx;
        j = wy * kWaveTileH + ly;  // local row
        h = global_row(g, j);
        live = have_tile && (w < g.W) && (j < g.rows) && (h < g.H);
        const double px = (2.0 * ((double)w / g.W) - 1) * g.half_width;
        const double py = (2.0 * ((double)h / g.H) - 1) * g.half_width * g.H / g.W;
        pdir = normalized(mk(px, py, 0) - camorg);
        pof = pdir * ((g.focus_plane - camorg.z) / pdir.z) + camorg;
        if (POSE) {  // both from here on in the world
            pof = pose_v(g, pof);
            pdir = normalized(pose_v(g, mk(px, py, 0)) - camw);
        }
        k_pix = pixel_key(g.seed, (uint64_t)h * (uint64_t)g.W + (uint64_t)w);
    };
    if (!heavy) {
        // Natural order: a workgroup's waves are the 2x2 wave tiles of a 32x8 tile (tile_of_block: XCD-aware or row-major);
        // 8x8 per wave measured: meshes equal, C2 7 % slower.  When a tile's samples are split over several workgroups
        // (chunks > 1) the chunk index comes from the block index too.
        const int nb = tile_block;
        int tile_x, tile_y;
        if (tile_grid < 0) {  // an entry of the tile queue: the tile's number itself
            const int tiles_x = (g.W + TG::W - 1) / TG::W;
            tile_x = nb % tiles_x;
            tile_y = nb / tiles_x;
        } else {
            const int tile_blocks = tile_grid / g.chunks;
            chunk = nb / tile_blocks;
            if (!tile_of_block(g, nb % tile_blocks, tile_x, tile_y, TG::W, TG::H)) return;  // whole workgroup (no later barrier is missed)
        }
        wx = tile_x * (TG::W / kWaveTileW) + (NT == 256 ? (wave & 1) : 0);
        wy = tile_y * (TG::H / kWaveTileH) + (NT == 256 ? (wave >> 1) : 0);
        have_tile = wx < wtiles_x && wy < wtiles_y;
        // a heavy tile is rendered by the heavy workgroups: its wave stands down here; so does the wave of a tile that
        // belongs to the other launch of a light / full pair (the probe leaves the light tiles out: they are never heavy)
        if (have_tile && g.hidx && g.hidx[wy * wtiles_x + wx] >= 0) have_tile = false;
        if (have_tile && g.light && (g.light[wy * wtiles_x + wx] != 0) != (g.light_mode != 0)) have_tile = false;
        s_end = (g.chunks > 1) ? ((chunk + 1) * g.chunk_spp < g.spp ? (chunk + 1) * g.chunk_spp : g.spp) : (PAIR && rw.slot >= 0 ? rw.s1 : g.spp);
        set_pixel(lane & 15, lane >> 4);
    }
    // DIFF: the spheres a primary ray of this wave tile can meet at all (GridParams::wmask, tile_order_kernel): wave-uniform, read
    // once through the scalar cache
    const bool masked = DIFF && g.wmask != nullptr;
    uint32_t smask = 0u;
    if (masked) {
        smask = load_uniform(g.wmask + __builtin_amdgcn_readfirstlane(have_tile ? wy * wtiles_x + wx : 0));
        if (sc.n_lds < 32) smask &= (1u << sc.n_lds) - 1u;
    }
    // DIFF: the sphere every primary ray of this wave tile hits first, where sure_first_kernel has proven one (GridParams::wsure;
    // wave-uniform, the byte's word read through the scalar cache): kSureNone -- trace
    uint32_t sure = (uint32_t)kSureNone;
    if (DIFF && g.wsure != nullptr && have_tile) {
        const uint32_t wt = (uint32_t)__builtin_amdgcn_readfirstlane(wy * wtiles_x + wx);
        sure = (load_uniform(reinterpret_cast<const uint32_t *>(g.wsure) + (wt >> 2)) >> ((wt & 3u) * 8u)) & 0xffu;
        if (sure >= (uint32_t)sc.n_lds) sure = (uint32_t)kSureNone;
    }
    uint64_t k_smp = 0;  // key of the sample whose ray tree this lane is tracing

    double acc_r = 0, acc_g = 0, acc_b = 0;
    uint32_t my_hits = 0, my_rays = 0, my_nodes = 0, my_tris = 0, wave_iters = 0;
    uint32_t hp_seq = 0;  // index of the next Hitpoint within the current sample's ray tree (emission order)

    Pending deep[2];   // third stack level (scratch; indexed dynamically so that it stays out of registers)
    Pending sib;       // refracted sibling of a leaf-level glass hit (registers)
    bool sib_valid = false;
    unsigned char *lslot = lds_raw;  // level L, field f of this thread: lslot + L*level_bytes + (f*NT + tid)*8
    int sp = 0;
    int s = (g.chunks > 1) ? chunk * g.chunk_spp : (PAIR && rw.slot >= 0 ? rw.s0 : 0);  // next sample to start
    // PARK: the lane's stream -- value i at park[i * 3 * NT + {0, NT, 2 NT}] -- and the values it holds
    double *park = nullptr;
    uint32_t park_n = 0;
    if (PARK) {
        const RelayForm rf = relay_form<COST>(g, rw);
        park = reinterpret_cast<double *>(rf.area + relay_layout(rf.cap, rf.k, rf.slots).rvals) +
               ((size_t)rw.slot * (size_t)(rf.k - 1) + (size_t)(rw.chunk - 1)) * (size_t)rf.slots * (3 * NT) + threadIdx.x;
    }
    bool have = false;
    V3 o = camorg, d = pdir, adj = mk(1, 1, 1);
    int depth_left = 0;
    uint32_t path = 1;
    // heavy waves: the item units are being drawn from (wave-uniform) and the lane's own unit
    int unit_next = 0, unit_end = 0, hrank = 0;
    int unit_pix = 0, unit_smp = 0, unit_rank = 0;
    bool unit_open = false;
    // PRE: the primary ray of a fresh unit finds its mesh hit in the table primary_walk_kernel filled (cgrt_primwalk.hpp)
    constexpr bool PRE = HEAVY && TREES && !BEZ && !STATS && !SPILL;
    bool pre_valid = false;
    double pre_len = 0;
    int32_t pre_tri = -1;

    // Lens stage (cgrt_lens_stage.h).  A wave of this body starts the same sample in all its lanes every iteration, so its lanes
    // run out of staged draws together: samples [batch_first, batch_end) of the pixel are in the lane's slots, slot b of this
    // thread at lens_slot[b * NT].  A lane reads only its own slots: no barrier.
    const bool staging = LSTAGE && g.lens_batch != 0;
    uint64_t *const lens_slot = reinterpret_cast<uint64_t *>(lrest) + threadIdx.x;
    static_assert(lens_slot_at(1, 0, NT) == NT * sizeof(uint64_t) && lens_slot_at(0, 1, NT) == sizeof(uint64_t), "lens_slot's strides");
    int batch_first = 0, batch_end = 0;
    auto stage_lens = [&](int first, int count) {  // wave-uniform: samples first .. first + count - 1, count <= kLensBatch
        uint32_t rejected = 0u;
        for (int b = 0; b < count; b++) {  // phase A: attempt 1 of every sample, no divergence (a lane without a pixel included)
            const LensSlot a = lens_stage_first(k_pix, (uint64_t)(g.sample_offset + first + b));
            lens_slot[b * NT] = a.v;
            rejected |= a.done ? 0u : (1u << b);
        }
        if (!live) rejected = 0u;
        while (__ballot(rejected != 0u) != 0ull) {  // phase B: every lane with rejects retries its lowest rejected sample
            if (rejected != 0u) {
                const int b = __ffs((int)rejected) - 1;
                const LensSlot a = lens_stage_retry(lens_slot[b * NT]);
                lens_slot[b * NT] = a.v;
                if (a.done) rejected &= rejected - 1u;
            }
        }
        batch_first = first;
        batch_end = first + count;
    };
    // LTAB: the draw of the next sample this thread starts, row `smp` of the table entry at lens_row[smp * NT + thread] -- a
    // workgroup-uniform base and a 32-bit index; loaded here and again at each start, a sample ahead of its use
    uint64_t z_next = 0;
    if (LTAB && s < s_end) z_next = lens_row[(uint32_t)s * (uint32_t)NT + threadIdx.x];
    auto start_sample = [&](int smp) {  // main.cpp:204-209
        if (LTAB) {
            double sx, sy;
            lens_point(z_next, sx, sy);
            o = camorg + mk(sx, sy, 0) * g.lens_radius;
            d = normalized(pof - o);
            k_smp = 0;  // (a sphere scene draws nothing else from the sample's streams)
            if (smp + 1 < s_end) z_next = lens_row[(uint32_t)(smp + 1) * (uint32_t)NT + threadIdx.x];
        } else if (LSTAGE && staging) {
            double sx, sy;
            lens_point(lens_slot[(smp - batch_first) * NT], sx, sy);
            o = camorg + mk(sx, sy, 0) * g.lens_radius;
            d = normalized(pof - o);
            k_smp = 0;  // (a sphere scene draws nothing else from the sample's streams)
        } else if (DOF) {
            k_smp = sample_key(k_pix, (uint64_t)(g.sample_offset + smp));
            double sx, sy;
            lens_disc(k_smp, sx, sy);  // purpose 0: the lens stream's key is the sample key
            o = camorg + mk(sx, sy, 0) * g.lens_radius;
            if (POSE) o = pose_v(g, o);
            d = normalized(pof - o);
        } else {
            k_smp = sample_key(k_pix, (uint64_t)(g.sample_offset + smp));
            o = POSE ? camw : camorg;
            d = pdir;
        }
        adj = mk(1, 1, 1);
        depth_left = g.max_depth;
        path = 1;
        hp_seq = 0;
        have = true;
    };

    // heavy waves: `hrank`, wx, wy and [unit_next, unit_end) describe the item the wave is currently drawing units from
    // (wave-uniform); a lane remembers the item of the unit it is tracing in unit_rank (the wave may have moved on)
    bool queue_empty = false;
    unsigned item_ahead = 0, n_items_total = 0;
    if (DIFF && sure != (uint32_t)kSureNone) {
        // A sure wave tile: every ray of every sample of every live lane ends on sphere `sure` and contributes its colour, so the
        // sample loop below has nothing to decide.  What it would have done is done here -- hf added once per sample, one
        // addition after the other (the sums' bits are the loop's), a ray and a Hitpoint counted per lane and sample, an iteration
        // per sample while any lane is live -- and with s at s_end the loop is left at its first test: no lens draw, no staging.
        const V3 hf = load_mat<false>(lobjs, sc.n_lds, sc.objs, (int)sure).col;
        if (__ballot(live && s < s_end) != 0ull) wave_iters += (uint32_t)(s_end - s);
        if (live) {
            for (int k = s; k < s_end; k++) {
                acc_r += hf.x;
                acc_g += hf.y;
                acc_b += hf.z;
            }
            if (s < s_end) my_hits = my_rays = (uint32_t)(s_end - s);
        }
        s = s_end;
    }
    if (heavy) {
        n_items_total = load_uniform(g.plan) * (unsigned)g.items_per_tile;
        if (lane == 0) item_ahead = atomicAdd(&g.plan[2], 1u);
    }
    while (true) {
        if (heavy) {
            // A lane without a ray closes its unit (how many Hitpoints it produced) and takes the next one: unit u of an item
            // is sample u / 64 of pixel u % 64 of the item's tile, so the lanes of a wave keep working on neighbouring pixels
            // of one sample.  When the item runs dry the wave takes the next item from the queue at once -- lanes still
            // tracing units of the old item carry on -- so lanes idle only when the whole queue is empty.
            const bool want = !have;
            const unsigned long long m = __ballot(want);
            if (m != 0ull) {
                if (want && unit_open) {
                    g.dcnt[((size_t)unit_rank * g.spp + unit_smp) * 64 + unit_pix] = (unsigned char)hp_seq;
                    unit_open = false;
                }
                if (unit_next >= unit_end && !queue_empty) {
                    // the item fetched ahead (its atomic has been in flight while the previous item was traced) ...
                    const unsigned item = (unsigned)__builtin_amdgcn_readfirstlane((int)item_ahead);
                    // ... and the one after it is requested now
                    if (lane == 0) item_ahead = atomicAdd(&g.plan[2], 1u);
                    if (item >= n_items_total) {
                        queue_empty = true;
                    } else {
                        hrank = (int)(item / (unsigned)g.items_per_tile);
                        const uint32_t wt = load_uniform(g.order + hrank);
                        wx = (int)(wt % (uint32_t)wtiles_x);
                        wy = (int)(wt / (uint32_t)wtiles_x);
                        have_tile = true;
                        unit_next = (int)(item % (unsigned)g.items_per_tile) * g.units_per_item;
                        unit_end = unit_next + g.units_per_item;
                        if (unit_end > 64 * g.spp) unit_end = 64 * g.spp;
                    }
                }
                const int u = unit_next + (int)__popcll(m & lanes_below);
                unit_next += (int)__popcll(m);  // lanes that drew beyond unit_end draw again from the next item
                if (want && u < unit_end) {
                    unit_pix = u & 63;
                    unit_smp = u >> 6;
                    unit_rank = hrank;
                    // the pixel's camera constants come from the table pixel_const_kernel filled (five fp64 divisions, a square
                    // root and two hash rounds per pixel: a third of a sphere-scene sample if redone for every unit)
                    w = wx * kWaveTileW + (unit_pix & 15);
                    j = wy * kWaveTileH + (unit_pix >> 4);
                    h = global_row(g, j);
                    live = (w < g.W) && (j < g.rows) && (h < g.H);
                    // PRE: a unit primary_walk_kernel has already completed (its nearest object was diffuse) is not opened
                    if (PRE && live && g.prim_len && g.prim_done &&
                        g.dcnt[((size_t)unit_rank * g.spp + unit_smp) * 64 + unit_pix] != 255)
                        live = false;
                    if (live) {
                        const double *pc = g.pconst + (size_t)unit_rank * (7 * 64) + unit_pix;
                        pdir = mk(pc[0 * 64], pc[1 * 64], pc[2 * 64]);
                        pof = mk(pc[3 * 64], pc[4 * 64], pc[5 * 64]);
                        k_pix = (uint64_t)__double_as_longlong(pc[6 * 64]);
                        start_sample(unit_smp);
                        unit_open = true;
                        if (PRE && g.prim_len) {
                            const size_t us = ((size_t)unit_rank * g.spp + unit_smp) * 64 + unit_pix;
                            pre_len = g.prim_len[us];
                            pre_tri = g.prim_tri[us];
                            pre_valid = true;
                        }
                    }
                }
            }
            if (__ballot(have) == 0ull) {
                if (queue_empty && unit_next >= unit_end) break;  // nothing left anywhere
                continue;                                         // drew nothing traceable (item boundary, pixels outside the image)
            }
        } else {
            if (LSTAGE && staging) {
                // the lanes that start a sample are all at the same one; when it lies beyond the batch, the wave stages the next
                const unsigned long long starting = __ballot(!have && live && s < s_end);
                if (starting != 0ull) {
                    const int first = __builtin_amdgcn_readlane(s, (int)__ffsll((long long)starting) - 1);
                    // (wave-uniform: `first` is a scalar and batch_end is set in stage_lens alone, by every lane alike -- the
                    // ballot loop in there needs the whole wave)
                    if (first >= batch_end) stage_lens(first, min(kLensBatch, s_end - first));
                }
            }
            if (!have && live && s < s_end) {
                // start the next sample of this lane's pixel
                start_sample(s);
                s++;
            }
            if (__ballot(have) == 0ull) break;  // every lane of the wave has drained its pixel
        }
        wave_iters++;
        UTILP(heavy ? 0 : 11, have);
        // All 64 lanes enter the scene walk together (lanes without a ray carry on == false): the object list
        // is wave-uniform, so its control flow stays scalar.
        RayKey rk{k_smp, path, false, 0u};
        if (PRE) {
            rk.pre_valid = have && pre_valid;  // only the ray a unit starts with
            rk.pre_obj = g.prim_obj;
            rk.pre_len = pre_len;
            rk.pre_tri = pre_tri;
            rk.pre_counter = pre_tri >= 0 ? 1 : 0;
            pre_valid = false;
        }
        const SceneHit hit =
            intersect_scene<TREES, BEZ, SPH, STATS, SPILL, PRE, HFONLY, !SPH, PAIR, DIFF>(lobjs, sc.n_lds, sc.n_objs, sc, o, d, rk, have, aux, my_nodes, my_tris,
                                                                                          masked, smask);
        if (have) {
            my_rays++;
            have = false;
            if (hit.id >= 0) {
                const ObjMat ob = load_mat<SPILL>(lobjs, sc.n_lds, sc.objs, hit.id);
                // hit point, normal and side.  SPH: the walk leaves the sphere's normal to the branches that use it -- the ray
                // that ends on a diffuse sphere needs none of this (normalized and sqrt_cr ballot over the lanes that are there)
                V3 P = o, n = d, n_old = d;
                bool into = true;
                auto surface = [&]() {
                    P = o + d * hit.t;  // main.cpp:68
                    n = SPH ? normalized(P - load_centre<SPILL>(lobjs, sc.n_lds, sc.objs, hit.id)) : hit.n;  // objects.h:65-66
                    n_old = n;
                    into = true;
                    if (dot(n, d) > 0) {  // main.cpp:73-76
                        n = -n;
                        into = false;
                    }
                };
                if (!SPH) surface();
                V3 f = ob.col;  // getSurfaceColor
                if (!SPH && ob.kind == KIND_PLANE && ob.tex >= 0) {
                    V3 c;
                    if (texture_color(sc.texs[ob.tex], sc.texels, P, c)) f = c;  // objects.h:533-539
                }
                const double refl = ob.refl, transp = ob.transp;
                if (DIFF || (refl < kEps && transp < kEps)) {
                    UTIL(heavy ? 7 : 12);
                    // diffuse: the reference stores Hitpoint{f*adj,...} (main.cpp:85-100); we accumulate it (DIFF: adj is 1)
                    const V3 hf = DIFF ? f : mulv(f, adj);
                    if (heavy) {
                        // deferred: the value is added in deferred_sum_kernel, in this (sample, emission) position
                        double *q = g.dvals + ((((size_t)unit_rank * g.spp + unit_smp) * g.maxhp + hp_seq) * 64 + unit_pix) * 3;
                        q[0] = hf.x;
                        q[1] = hf.y;
                        q[2] = hf.z;
                    } else if (PARK) {
                        if (park_n < (uint32_t)relay_form<COST>(g, rw).slots) {  // (always: the slots bound a chunk's ray trees)
                            double *q = park + (size_t)park_n * (3 * NT);
                            q[0] = hf.x;
                            q[NT] = hf.y;
                            q[2 * NT] = hf.z;
                        }
                        park_n++;
                    } else {
                        acc_r += hf.x;
                        acc_g += hf.y;
                        acc_b += hf.z;
                    }
                    my_hits++;
                    if (HPS && SPH) surface();
                    if (HPS) {
                        // one atomic per wave, not per lane (same-address atomics are served one after the other): the lanes
                        // that are here take consecutive places behind the count their first lane fetched
                        const unsigned long long here = __ballot(true);
                        unsigned long long base = 0ull;
                        if (lane == (int)__ffsll((long long)here) - 1) base = atomicAdd(hps.count, (unsigned long long)__popcll(here));
                        base = (unsigned long long)__shfl((long long)base, (int)__ffsll((long long)here) - 1);
                        const unsigned long long k = base + (unsigned long long)__popcll(here & lanes_below);
                        if (k < hps.cap) {
                            double *q = hps.rec + 10 * k;
                            q[0] = hf.x; q[1] = hf.y; q[2] = hf.z;
                            q[3] = P.x; q[4] = P.y; q[5] = P.z;
                            q[6] = n.x; q[7] = n.y; q[8] = n.z;
                            // label: (sample, local pixel) like Hitpoint::w/h (main.cpp:91-92), times 16, plus the
                            // hitpoint's position in the sample's emission order (<= 16 per tree)
                            q[9] = (double)((((unsigned long long)(s - 1) * (unsigned long long)g.W * g.rows +
                                              (unsigned long long)j * g.W + w) << 4) | (unsigned long long)hp_seq);
                        }
                    }
                    if (HPS || heavy) hp_seq++;
                } else if (depth_left > 1) {
                    if (SPH) surface();
                    if (transp < kEps) {
                        // mirror, main.cpp:129-134
                        const V3 nd = d - n * 2.0 * dot(n, d);
                        adj = mulv(f, adj) * refl;
                        o = P + n * kEps;
                        d = nd;
                        depth_left--;
                        path = path * 2;
                        have = true;
                    } else if (GLASS) {
                        UTIL(heavy ? 8 : 13);
                        // glass, main.cpp:135-157
                        const double nc = 1.0, nt = 1.33;
                        const double nnt = into ? nc / nt : nt / nc;
                        const double ddn = dot(d, n);
                        const V3 refl_dir = d - n_old * 2.0 * dot(n_old, d);
                        const double cos2t = 1 - nnt * nnt * (1 - ddn * ddn);
                        if (cos2t < 0) {
                            // total internal reflection keeps adj (main.cpp:144)
                            o = P + n * kEps;
                            d = refl_dir;
                        } else {
                            const V3 refr_dir =
                                normalized(d * nnt - n_old * ((into ? 1 : -1) * (ddn * nnt + sqrt_cr(cos2t))));
                            const double a = nt - nc, b = nt + nc, R0 = a * a / (b * b);
                            const double c = 1 - (into ? -ddn : dot(refr_dir, n_old));
                            const double Re = R0 + (1 - R0) * c * c * c * c * c;
                            const V3 fa = mulv(f, adj);
                            Pending pe;
                            pe.o = P - n * kEps;
                            pe.d = refr_dir;
                            pe.adj = fa * (1 - Re);
                            pe.depth_left = depth_left - 1;
                            pe.path = path * 2 + 1;
                            if (depth_left == 2) {
                                sib = pe;
                                sib_valid = true;
                            } else {
                                if (sp < kLdsLevels) {
                                    double *q = reinterpret_cast<double *>(lslot + sp * level_bytes) + threadIdx.x;
                                    q[0 * NT] = pe.o.x; q[1 * NT] = pe.o.y; q[2 * NT] = pe.o.z;
                                    q[3 * NT] = pe.d.x; q[4 * NT] = pe.d.y; q[5 * NT] = pe.d.z;
                                    q[6 * NT] = pe.adj.x; q[7 * NT] = pe.adj.y; q[8 * NT] = pe.adj.z;
                                    // depth_left <= 4 and path < 32: one word
                                    reinterpret_cast<uint32_t *>(lslot + sp * level_bytes +
                                                                 kPendDoubles * NT * sizeof(double))[threadIdx.x] =
                                        ((uint32_t)pe.depth_left << 8) | pe.path;
                                } else {
                                    deep[sp - kLdsLevels] = pe;
                                }
                                sp++;
                            }
                            o = P + n * kEps;
                            d = refl_dir;
                            adj = fa * Re;
                        }
                        depth_left--;
                        path = path * 2;
                        have = true;
                    }
                }
            }
            if (GLASS && !have && sib_valid) {
                o = sib.o;
                d = sib.d;
                adj = sib.adj;
                depth_left = sib.depth_left;
                path = sib.path;
                sib_valid = false;
                have = true;
            }
            if (GLASS && !have && sp > 0) {
                UTIL(heavy ? 10 : 14);
                --sp;
                if (sp < kLdsLevels) {
                    const double *q = reinterpret_cast<const double *>(lslot + sp * level_bytes) + threadIdx.x;
                    o = mk(q[0 * NT], q[1 * NT], q[2 * NT]);
                    d = mk(q[3 * NT], q[4 * NT], q[5 * NT]);
                    adj = mk(q[6 * NT], q[7 * NT], q[8 * NT]);
                    const uint32_t meta = reinterpret_cast<const uint32_t *>(
                        lslot + sp * level_bytes + kPendDoubles * NT * sizeof(double))[threadIdx.x];
                    depth_left = (int)(meta >> 8);
                    path = meta & 0xffu;
                } else {
                    const Pending &pe = deep[sp - kLdsLevels];
                    o = pe.o;
                    d = pe.d;
                    adj = pe.adj;
                    depth_left = pe.depth_left;
                    path = pe.path;
                }
                have = true;
            }
        }
    }  // ray loop

    if (g.probe) {
        // cost probe: nothing of the image is stored; the wave leaves what its tile cost and the tile's number
        if (lane == 0 && have_tile) {
            const long long dt = (long long)clock64() - cost_t0;
            const uint32_t wt = (uint32_t)(wy * wtiles_x + wx);
            // (probe == 2, the relay's cost start, COST variants only: the wave's iterations, which no clock enters)
            g.cost[wt] = (COST && g.probe == 2) ? wave_iters : dt > 0 ? (dt < 0xffffffffll ? (uint32_t)dt : 0xffffffffu) : 1u;
        }
        return;  // no counters: the render launch that follows counts these rays
    }
    if (heavy) {
        // nothing to store: deferred_sum_kernel writes the heavy tiles' pixels
    } else if (g.chunks > 1) {
        // split samples: this wave's raw fp64 sums; finalize_chunks_kernel adds the chunks in order
        if (have_tile && (w < g.W) && (j < g.rows)) {  // rows past the image (stripe padding) carry zero sums
            const size_t px = ((size_t)chunk * g.rows + (size_t)j) * g.W + (size_t)w;
            g.partial[3 * px + 0] = acc_r;
            g.partial[3 * px + 1] = acc_g;
            g.partial[3 * px + 2] = acc_b;
            if (g.partial_nhit) g.partial_nhit[px] = my_hits;
        }
    } else {
        uint32_t px_hits = my_hits;  // the pixel's Hitpoints (a relayed tile: of all its chunks)
        bool store = true;
        if (PAIR && rw.slot >= 0) {
            // ---- relay: leave this chunk's results in the tile's slot, publish them, count in; the last workgroup in adds
            // the chunks up.  Nobody waits for anybody (cgrt_relay.h).
            const RelayForm rf = relay_form<COST>(g, rw);  // (here, not across the ray loop; a promoted tile: the boost area's)
            const size_t slot = (size_t)rw.slot, k = (size_t)rf.k;
            const RelayLayout rl = relay_layout(rf.cap, rf.k, rf.slots);
            uint32_t *arrive = reinterpret_cast<uint32_t *>(rf.area) + slot;
            double *racc = reinterpret_cast<double *>(rf.area + rl.racc) + slot * (3 * NT) + threadIdx.x;
            uint32_t *rhits = reinterpret_cast<uint32_t *>(rf.area + rl.rhits) + slot * k * NT + threadIdx.x;
            uint32_t *rcount = reinterpret_cast<uint32_t *>(rf.area + rl.rcount) + slot * (k - 1) * NT + threadIdx.x;
            if (PARK) {
                rcount[(size_t)(rw.chunk - 1) * NT] = park_n;
            } else {
                racc[0] = acc_r;
                racc[NT] = acc_g;
                racc[2 * NT] = acc_b;
            }
            rhits[(size_t)rw.chunk * NT] = my_hits;
            // publish: every wave's stores are out, then one agent-scope release in front of the ticket (the XCDs' L2s are
            // not coherent with one another: nothing narrower makes the values visible to a workgroup on another XCD)
            __shared__ unsigned int relay_last;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const unsigned int ticket = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool last = ticket == (unsigned int)rf.k - 1u;
                if (last) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next launch
                }
                relay_last = last ? 1u : 0u;
            }
            __syncthreads();
            store = relay_last != 0u;
            if (store) {
                // chunk 0's sums, then chunk 1's values in emission order, chunk 2's, ...: acc_r += hf.x; acc_g += hf.y;
                // acc_b += hf.z of the unsplit loop, addition for addition.  A batch of slots is loaded whole (the loop bound is
                // the wave's largest count, the area holds every slot) and added where the lane has a value.
                acc_r = racc[0];
                acc_g = racc[NT];
                acc_b = racc[2 * NT];
                px_hits = rhits[0];
                for (int c = 1; c < rf.k; c++) {
                    px_hits += rhits[(size_t)c * NT];
                    uint32_t n = rcount[(size_t)(c - 1) * NT];
                    if (n > (uint32_t)rf.slots) n = (uint32_t)rf.slots;
                    uint32_t n_max = n;
                    for (int off = 32; off > 0; off >>= 1) {
                        const uint32_t o2 = (uint32_t)__shfl_xor((int)n_max, off);
                        n_max = o2 > n_max ? o2 : n_max;
                    }
                    n_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_max);
                    const double *q = reinterpret_cast<const double *>(rf.area + rl.rvals) +
                                      (slot * (k - 1) + (size_t)(c - 1)) * (size_t)rf.slots * (3 * NT) + threadIdx.x;
                    for (uint32_t i0 = 0; i0 < n_max; i0 += kRelayBatch) {
                        double v[kRelayBatch][3];
#pragma unroll
                        for (int u = 0; u < kRelayBatch; u++) {
                            v[u][0] = q[(size_t)(i0 + u) * (3 * NT)];
                            v[u][1] = q[(size_t)(i0 + u) * (3 * NT) + NT];
                            v[u][2] = q[(size_t)(i0 + u) * (3 * NT) + 2 * NT];
                        }
#pragma unroll
                        for (int u = 0; u < kRelayBatch; u++) {
                            if (i0 + u < n) {
                                acc_r += v[u][0];
                                acc_g += v[u][1];
                                acc_b += v[u][2];
                            }
                        }
                    }
                }
            }
        }
        // ---- store: the wave's 16x4 pixels are 4 rows of 48 contiguous floats; lane l of pass k writes float k*64 + l of
        // the tile, fetched from the lane that owns that pixel (three ds_bpermute shuffles per pass, no LDS, no barrier).
        // A store instruction then covers 256 contiguous bytes of a row (192 + 64 of the next).
        const float v0 = (float)(acc_r * g.inv_spp_total), v1 = (float)(acc_g * g.inv_spp_total),
                    v2 = (float)(acc_b * g.inv_spp_total);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int idx = k * 64 + lane;
            const int row = idx / (kWaveTileW * 3), c = idx % (kWaveTileW * 3);
            const int src = row * kWaveTileW + c / 3, ch = c % 3;
            const float a0 = __shfl(v0, src), a1 = __shfl(v1, src), a2 = __shfl(v2, src);
            const float v = ch == 0 ? a0 : (ch == 1 ? a1 : a2);
            const int jj = wy * kWaveTileH + row, ww = wx * kWaveTileW + c / 3;
            if (store && have_tile && jj < g.rows && ww < g.W) {
                float *dst = rgb + ((size_t)jj * g.W + ww) * 3 + ch;
                *dst = g.accumulate ? *dst + v : v;  // progressive passes add into the fp32 frame
            }
        }
        if (store && nhit_out && have_tile && (w < g.W) && (j < g.rows)) nhit_out[(size_t)j * g.W + w] = px_hits;
    }

    if (g.timeline) {  // development aid: when and where this workgroup ran
        __shared__ unsigned int tl_rays;
        if (threadIdx.x == 0) tl_rays = 0;
        __syncthreads();
        atomicAdd(&tl_rays, my_rays);
        __syncthreads();
        if (threadIdx.x == 0) {  // a workgroup that serves queues passes here once per tile / per queue: first start, last end, all rays
            unsigned long long *q = g.timeline + 4 * (size_t)blockIdx.x;
            const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
            if (q[0] == 0ull) q[0] = (unsigned long long)tl_t0;
            q[1] = (unsigned long long)wall_clock64();
            q[2] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
            q[3] = ((unsigned long long)(wx & 0xffff) | ((unsigned long long)(wy & 0xffff) << 16)) + ((q[3] >> 32) << 32) + ((unsigned long long)tl_rays << 32);
        }
    }
    if (counters) {
        // wave reduction, then one atomic per wave and counter
        unsigned long long r = my_rays, hh = my_hits, nn = my_nodes, tt = my_tris;
        for (int off = 32; off > 0; off >>= 1) {
            r += __shfl_xor(r, off);
            hh += __shfl_xor(hh, off);
            if (STATS) {
                nn += __shfl_xor(nn, off);
                tt += __shfl_xor(tt, off);
            }
        }
        // (`counters` is the workgroup's LDS array, see wg_counters_begin) a wave that traced nothing adds nothing
        if (lane == 0 && (r | (unsigned long long)wave_iters) != 0ull) {
            atomicAdd(&counters[CGRT_CNT_RAYS], r);
            atomicAdd(&counters[CGRT_CNT_HITPOINTS], hh);
            atomicAdd(&counters[CGRT_CNT_WAVE_ITERS], (unsigned long long)wave_iters);
            if (STATS) {
                atomicAdd(&counters[CGRT_CNT_NODE_TESTS], nn);
                atomicAdd(&counters[CGRT_CNT_TRI_TESTS], tt);
            }
        }
    }
}

// Counters.  A wave adds its sums to counters that all waves of the launch share; same-address atomics are served one after the
// other, ~12 ns each, by the memory side -- measured: a 4096x4096 frame of plane-only rays took 9.5 ms whatever its sample count
// (1, 4 or 16), 262 144 waves x 3 atomics.  So a workgroup collects its waves' sums in LDS (wg_counters_begin/end around the
// body or bodies it runs: the body's `counters` IS that LDS array) and adds them to the launch's counters once, when it ends:
// a quarter of the atomics for one-tile workgroups, a few thousand per launch for the persistent ones.
__device__ __forceinline__ unsigned long long *wg_counters_begin(unsigned long long *wg, const unsigned long long *counters) {
    if (!counters) return nullptr;  // (a kernel argument: uniform)
    if (threadIdx.x < CGRT_NCOUNTERS) wg[threadIdx.x] = 0ull;
    __syncthreads();
    return wg;
}
__device__ __forceinline__ void wg_counters_end(const unsigned long long *wg, unsigned long long *counters) {
    if (!counters) return;
    __syncthreads();  // every wave of the workgroup has left its last body
    if (threadIdx.x < CGRT_NCOUNTERS && wg[threadIdx.x] != 0ull) atomicAdd(&counters[threadIdx.x], wg[threadIdx.x]);
}

// One launch = tile workgroups only (probe, image order, Hitpoint capture) ...
template <bool TREES, bool BEZ, bool DOF, bool GLASS, bool SPH, bool STATS, bool HPS = false, int NT = 256, bool SPILL = false, bool HFONLY = false,
          bool DIFF = false, bool PAIR = false, bool START = false, bool LTAB = false, bool POSE = false>
__global__ __launch_bounds__(NT, DIFF ? (DOF ? kDiffDofWaves : kDiffWaves) : BEZ ? kBezWaves : ((TREES && !HFONLY) ? kTreeWaves : 4)) void trace_grid_kernel(DeviceScene sc, GridParams g, float *__restrict__ rgb,
                                                             uint32_t *__restrict__ nhit_out,
                                                             unsigned long long *__restrict__ counters,
                                                             HitpointSink hps = HitpointSink{nullptr, nullptr, 0}) {
    // tile_order: the workgroup's tile comes from tile_order_kernel's list (the body's tile-queue entry: a literal tile number).
    // A pair of launches shares the list (kOrderFull: the entries of classes 0-2, kOrderDiffuse: those of class 3, the DIFF
    // variant); the host does not know where class 3 begins, so both are launched over all tiles and a workgroup beyond its
    // launch's part leaves here, before anything else.
    // The sample relay (PAIR variants, g.relay_k > 1; cgrt_relay.h): the list's first entries -- classes 0 and 1, with
    // g.relay_extent class 2 as well, as many as the relay area holds -- are rendered by relay_k workgroups each, in the order
    // g.relay_order names; the launch spans relay_cap such entries, the host knowing neither plan[2] nor plan[3], and a
    // workgroup whose entry lies beyond the list leaves here.  Index arithmetic on uniform values only.
    int tile_block = (int)blockIdx.x, tile_grid = (int)gridDim.x;
    unsigned entry = blockIdx.x;
    RelayWg rw;
    if (!POSE && g.tile_order) {  // (a posed launch has no tile order, cgrt_frame.h)
        if (g.tile_order == kOrderFull || g.tile_order == kOrderDiffuse) {
            const unsigned first_diffuse = load_uniform(g.plan + 3);
            if (g.tile_order == kOrderDiffuse) entry += first_diffuse;
            if (g.tile_order == kOrderDiffuse ? entry >= load_uniform(g.plan + kOrderClasses) : entry >= first_diffuse) return;
        } else if (PAIR && g.relay_k > 1) {
            const unsigned n_tiles = load_uniform(g.plan + kOrderClasses);
            const unsigned n01 = load_uniform(g.plan + 2), n012 = load_uniform(g.plan + 3);
            RelayBlock rb{n_tiles, 0, false};
            // START (a variant of its own beside each PAIR variant: the launch with a start table and its cost probe, so that the
            // variant without one keeps its code): the workgroups of classes 0-2 in the order the table names (cgrt_relay.h),
            // the others as ever
            bool tabled = false;
            // With promoted tiles (g.relay_boost_at; cgrt_relay.h) the table has `items` workgroups, more than the base form's
            // t0 by the promoted tiles' extra chunks: the workgroups behind it are shifted by the difference, and a split entry's
            // bslot word says whether its tile is promoted and where in the boost area it lies.
            unsigned b = blockIdx.x, bslot = 0u;
            if (START && g.relay_start_at != 0u) {
                const unsigned n_split = relay_split_entries(n01, n012, (unsigned)g.relay_cap, g.relay_extent);
                const unsigned t0 = n012 + ((unsigned)g.relay_k - 1u) * n_split;
                const unsigned items = g.relay_boost_at != 0u ? load_uniform(g.plan + g.relay_boost_at + kBoostItems) : t0;
                tabled = b < items;
                if (tabled) {
                    rb = relay_start_block(load_uniform(g.plan + g.relay_start_at + b), n_split);
                    if (g.relay_boost_at != 0u && rb.split) bslot = load_uniform(g.plan + g.relay_boost_at + kBoostHead + rb.entry);
                    if (rb.chunk >= (bslot != 0u ? g.boost_k : g.relay_k) || bslot > (unsigned)g.boost_cap) return;  // (no table names a chunk or a slot the area has not)
                } else {
                    b -= items - t0;
                }
            }
            if (!tabled) rb = relay_block_ordered(b, (unsigned)g.relay_k, n01, n012, n_tiles, (unsigned)g.relay_cap, g.relay_extent, g.relay_order);
            entry = rb.entry;
            if (entry >= n_tiles) return;
            if (rb.split) {
                const int cs = START && bslot != 0u ? g.boost_chunk_spp : g.relay_chunk_spp;
                rw.slot = START && bslot != 0u ? (int)(bslot - 1u) : (int)entry;
                rw.boost = START && bslot != 0u ? 1 : 0;
                rw.chunk = rb.chunk;
                rw.s0 = relay_first_sample(rb.chunk, cs);
                rw.s1 = relay_end_sample(rb.chunk, cs, g.spp);
            }
        }
        tile_block = (int)load_uniform(g.border + entry);
        tile_grid = -1;
    }
    __shared__ unsigned long long wg_cnt[CGRT_NCOUNTERS];
    unsigned long long *wc = wg_counters_begin(wg_cnt, counters);
    // kOrderAllDiffuse (PAIR variants only): one launch over the whole list whose class-3 workgroups take the terminal-diffuse
    // body here (workgroup-uniform), at this kernel's registers -- 12 % fewer VALU instructions a frame and no second launch
    if (PAIR && g.tile_order == kOrderAllDiffuse && entry >= load_uniform(g.plan + 3))
        trace_grid_body<false, false, DOF, false, true, false, false, NT, false, false, false, true, false, false, DOF>(sc, g, rgb, nhit_out, wc, hps, tile_block, tile_grid);
    // LTAB (a twin of its own beside each thin-lens PAIR variant, so that a launch without a lens table keeps its code): the
    // workgroups of classes 0-2 whose entry the table holds run the bodies that read it (workgroup-uniform); the table's rows have
    // lens_table_spp samples.  The cost probe is given no table (relay_cost_start, cgrt_hip.hip)
    else if (LTAB && g.lens_table != nullptr && entry < (unsigned)g.lens_table_cap && entry < load_uniform(g.plan + 3)) {
        const uint64_t *lens_row = g.lens_table + (size_t)entry * (size_t)g.lens_table_spp * NT;
        if (rw.chunk > 0)
            trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, HPS, NT, false, SPILL, HFONLY, DIFF, PAIR, PAIR, false, START, LTAB>(sc, g, rgb, nhit_out, wc, hps, tile_block, tile_grid, rw, lens_row);
        else
            trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, HPS, NT, false, SPILL, HFONLY, DIFF, PAIR, false, false, START, LTAB>(sc, g, rgb, nhit_out, wc, hps, tile_block, tile_grid, rw, lens_row);
    } else if (PAIR && rw.chunk > 0)  // a relayed tile's later chunks park their values
        trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, HPS, NT, false, SPILL, HFONLY, DIFF, PAIR, PAIR, false, START>(sc, g, rgb, nhit_out, wc, hps, tile_block, tile_grid, rw);
    else
        trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, HPS, NT, false, SPILL, HFONLY, DIFF, PAIR, false, false, START, false, POSE>(sc, g, rgb, nhit_out, wc, hps, tile_block, tile_grid, rw);
    wg_counters_end(wg_cnt, counters);
}
// ... or the scheduled form: the first g.heavy_blocks workgroups serve the heavy tiles' unit queue, the others are the tile
// workgroups.  Two bodies in one kernel: the dispatcher starts workgroups in index order, so the heavy work starts first and
// tile workgroups take over the slots as the heavy waves retire -- no seam between two launches.  Each body keeps its own
// register allocation (the paths are disjoint); the kernel's register and scratch sizes are the larger of the two.
template <bool TREES, bool BEZ, bool DOF, bool GLASS, bool SPH, bool STATS, int NT = 256, bool POSE = false>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kSchedTreeWaves : 4)) void trace_grid_sched_kernel(DeviceScene sc, GridParams g,
                                                                                         float *__restrict__ rgb,
                                                                                         uint32_t *__restrict__ nhit_out,
                                                                                         unsigned long long *__restrict__ counters) {
    const HitpointSink none{nullptr, nullptr, 0};
    const bool heavy_first = (int)blockIdx.x < g.heavy_blocks;
    __shared__ unsigned long long wg_cnt[CGRT_NCOUNTERS];
    unsigned long long *wc = wg_counters_begin(wg_cnt, counters);
    if (NT == 64) {
        // one-wave workgroups (Bezier scenes): one workgroup per 16x4 tile behind the heavy ones -- a slot is handed on the
        // moment its wave ends, and measured on a C5 band the queue form bought nothing (34.6 vs 34.9 ms) while its larger
        // kernel cost 4 %
        if (heavy_first)
            trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, false, NT, true, false, false, false, false, false, false, false, false, POSE>(sc, g, rgb, nhit_out, wc, none, 0, 1);
        else
            trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, false, NT, false, false, false, false, false, false, false, false, false, POSE>(
                sc, g, rgb, nhit_out, wc, none, (int)blockIdx.x - g.heavy_blocks, (int)gridDim.x - g.heavy_blocks);
        wg_counters_end(wg_cnt, counters);
        return;
    }
    // With a tile queue (g.border) both kinds of work come from queues: a workgroup serves its own kind until that queue is
    // empty, then the other.  Without one (split samples) a workgroup behind the heavy ones renders the one tile its index names.
    // Each body appears once in the code: the loop runs them in either order.
    const bool queued = g.border != nullptr;
    __shared__ unsigned tile_entry;
    for (int phase = 0; phase < 2; phase++) {
        if ((phase == 0) == heavy_first) {
            if (queued || heavy_first)
                trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, false, NT, true, false, false, false, false, false, false, false, false, POSE>(sc, g, rgb, nhit_out, wc, none, 0, 1);
        } else {
            const unsigned n_entries = queued ? load_uniform(g.plan + 3) : (heavy_first ? 0u : 1u);
            unsigned served = 0;
            while (true) {
                unsigned e = served++;
                if (queued) {
                    __syncthreads();  // every wave is done with the previous tile (and has read tile_entry)
                    if (threadIdx.x == 0) tile_entry = atomicAdd(&g.plan[4], 1u);
                    __syncthreads();
                    e = tile_entry;
                }
                if (e >= n_entries) break;
                trace_grid_body<TREES, BEZ, DOF, GLASS, SPH, STATS, false, NT, false, false, false, false, false, false, false, false, false, POSE>(
                    sc, g, rgb, nhit_out, wc, none, queued ? (int)g.border[e] : (int)blockIdx.x - g.heavy_blocks,
                    queued ? -1 : (int)gridDim.x - g.heavy_blocks);
            }
        }
    }
    wg_counters_end(wg_cnt, counters);
}

// CGRT_GRID_SPLIT_SAMPLES, second step: chunk sums added in chunk order, scaled, rounded once to fp32.
__global__ void finalize_chunks_kernel(GridParams g, float *__restrict__ rgb, uint32_t *__restrict__ nhit_out) {
    const size_t npx = (size_t)g.rows * g.W;
    const size_t px = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= npx) return;
    if (g.hidx) {  // pixels of heavy tiles are written by deferred_sum_kernel (their chunk sums do not exist)
        const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW;
        if (g.hidx[(int)((px / g.W) / kWaveTileH) * wtiles_x + (int)((px % g.W) / kWaveTileW)] >= 0) return;
    }
    double r = 0, gg = 0, b = 0;
    uint32_t hits = 0;
    for (int c = 0; c < g.chunks; c++) {
        const size_t q = (size_t)c * npx + px;
        r += g.partial[3 * q + 0];
        gg += g.partial[3 * q + 1];
        b += g.partial[3 * q + 2];
        if (g.partial_nhit) hits += g.partial_nhit[q];
    }
    const float fr = (float)(r * g.inv_spp_total), fg = (float)(gg * g.inv_spp_total), fb = (float)(b * g.inv_spp_total);
    float *dst = rgb + 3 * px;
    if (g.accumulate) {
        dst[0] += fr; dst[1] += fg; dst[2] += fb;
    } else {
        dst[0] = fr; dst[1] = fg; dst[2] = fb;
    }
    if (nhit_out) nhit_out[px] = hits;
}

// ---- light tiles -------------------------------------------------------------------------------------------------------
// One thread per wave tile (16x4 pixels).  The tile is LIGHT when no primary ray of it -- any pixel, any lens sample -- can
// touch the bounding sphere of a "special" object: a mesh or Bezier object (trees, Newton) or a sphere that reflects or
// refracts (secondary rays go anywhere).  With every plane diffuse and un-bumped (DeviceScene::light_ok) such a tile's rays
// end on a diffuse sphere or plane after one scene walk, whatever the sample: the variant without tree / Bezier / pending-ray
// code renders it exactly.  Conservative bound: the tile's pinhole directions lie in a cone around its centre direction
// (half-angle = 1.5 x the largest corner deviation + 1e-6); a thin-lens ray deviates from its pinhole ray, at depth z, by
// lens_radius * |1 - (z - cam.z) / (focus_plane - cam.z)| sideways, so the object's sphere is grown by the largest such
// deviation over its depth range.  A mesh is bounded by its cover spheres (DeviceScene::cover: up to 64 spheres over
// median-split groups of its triangles -- a long thin mesh fills little of one sphere around all of it).  Anything doubtful
// (object behind or around the camera, rows beyond the image) is FULL.
// The test itself -- pixel_dir, wave_tile_cone, cone_clear_of -- is shared by classify_kernel, tile_order_kernel and the CPU test
// of the sphere masks: cgrt_sphere_mask.h (plain C++; the stripe mapping keeps a wave tile's four rows adjacent, so the corners
// one pixel beyond the tile bound it).
__device__ __forceinline__ Vec3d vec3d(V3 a) { return vec3d(a.x, a.y, a.z); }

__global__ void classify_kernel(DeviceScene sc, GridParams g, unsigned char *__restrict__ light, int n_wt) {
    const int wt = blockIdx.x * blockDim.x + threadIdx.x;
    if (wt >= n_wt) return;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW;
    const TileCone tc = wave_tile_cone(g, wt % wtiles_x, wt / wtiles_x);
    bool is_light = true;
    auto clear_of = [&](V3 c, double r) { return cone_clear_of(g, tc, vec3d(c), r); };
    for (int i = 0; i < sc.n_objs && is_light; i++) {
        const ObjRec &ob = sc.objs[i];
        if (ob.kind == KIND_SPHERE) {
            if (ob.refl < kEps && ob.transp < kEps) continue;  // diffuse: no secondary rays
            is_light = clear_of(ld3(ob.a), sqrt(ob.s0));
        } else if (ob.kind == KIND_BEZIER) {
            const BezierRec &bz = sc.beziers[ob.aux];
            const V3 hw = mk(0.5 * (bz.box[1] - bz.box[0]), 0.5 * (bz.box[3] - bz.box[2]), 0.5 * (bz.box[5] - bz.box[4]));
            is_light = clear_of(mk(0.5 * (bz.box[0] + bz.box[1]), 0.5 * (bz.box[2] + bz.box[3]), 0.5 * (bz.box[4] + bz.box[5])),
                                sqrt(dot(hw, hw)) + 1e-3);
        }
        // planes: vetted by light_ok; meshes: the cover spheres below
    }
    for (int i = 0; i < sc.n_cover && is_light; i++)
        is_light = clear_of(mk(sc.cover[4 * i], sc.cover[4 * i + 1], sc.cover[4 * i + 2]), sc.cover[4 * i + 3]);
    light[wt] = is_light ? 1 : 0;
}

// ---- tile order of image-order launches (GridParams::tile_order) ----------------------------------------------------------
// A scene of spheres and planes is rendered in image order, one workgroup per 32x8 tile, and the hardware starts workgroups in
// index order.  The tiles that see a refracting sphere carry ray trees of up to 31 rays per sample and run ~10x longer than a
// wall tile: in row-major order the longest of them (C2: the glass sphere's centre) starts only when the first generation of
// wall tiles retires, and that wait is added to the frame.  This kernel, launched in front of trace_grid_kernel on the same
// stream, lists the tiles so that they start first.  Every tile is rendered by the same code on the same lanes: only the
// workgroup index it gets changes, so image, hit counts and counters are bit for bit the row-major launch's.
//   class 0: the tile's centre direction hits a refracting sphere itself     class 2: ... a sphere that only reflects
//   class 1: some primary ray of the tile may touch a refracting sphere      class 3: everything else
// (1 and 2 by the test above over the tile's wave tiles; a doubtful case moves a tile forward, never into class 3).  One thread per wave tile
// classes it; the last workgroup through (plan[kOrderArrived], reset for the next launch) folds the wave tiles into tiles
// and writes list[] = a stable counting sort by class, row-major within a class, plan[c] = tiles of classes < c (c = 0..4).
// The sorting pass reads back only tile-class bytes its own thread wrote, so list[] is a permutation of the tiles in any case.
// Class 3 is more than a place in the order: in a sphere-only scene its tiles are rendered by the terminal-diffuse variant
// (trace_grid_kernel<..., DIFF>), which is exact only where no ray of the tile can meet a special sphere.  So the test must err
// towards classes 1 / 2 alone -- it does: cone 1.5 x the corner angle, the bound grown by the lens blur, anything behind or around
// the camera doubtful -- and the last workgroup must see every other workgroup's wave-tile classes: each workgroup fences its
// wcls[] stores before its thread 0 counts it in at plan[kOrderArrived] (device-scope atomic), and the last one fences again
// before it reads them.
// Sphere masks (wmask != nullptr: a scene of at most 32 spheres and nothing else): the same thread also writes wmask[wave tile],
// bit i set = sphere i of sc.objs is a CANDIDATE -- some primary ray of the wave tile may get a distance from sphere_len
// (sphere_surely_missed, cgrt_sphere_mask.h, says no for the others).  The terminal-diffuse body walks only the set bits; its
// workgroups read masks of their own wave tiles, written by this launch, which has ended when theirs begins.
__global__ __launch_bounds__(1024) void tile_order_kernel(GridParams g, OrderSpheres sp, DeviceScene sc, int tiles_x, int tiles_y,
                                                          uint32_t *__restrict__ plan, uint32_t *__restrict__ list,
                                                          unsigned char *__restrict__ tcls, unsigned char *__restrict__ wcls,
                                                          uint32_t *__restrict__ wmask) {
    constexpr int NT = 1024;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW, wtiles_y = (g.rows + kWaveTileH - 1) / kWaveTileH;
    const int n_wt = wtiles_x * wtiles_y, n = tiles_x * tiles_y, tid = threadIdx.x;
    for (int wt = blockIdx.x * NT + tid; wt < n_wt; wt += gridDim.x * NT) {
        TileRays tr;
        if (wmask) tr = wave_tile_rays(g, wt % wtiles_x, wt / wtiles_x);
        else tr.cone = wave_tile_cone(g, wt % wtiles_x, wt / wtiles_x);
        const TileCone &tc = tr.cone;
        int c = 3;
        for (unsigned i = 0; i < sp.n; i++)
            if (!cone_clear_of(g, tc, vec3d(sp.s[i][0], sp.s[i][1], sp.s[i][2]), sp.s[i][3])) c = min(c, ((sp.transp >> i) & 1u) ? 1 : 2);
        wcls[wt] = (unsigned char)c;
        if (wmask) {
            uint32_t m = 0;
            for (int i = 0; i < sc.n_objs && i < 32; i++)
                if (!sphere_surely_missed(g, tr, vec3d(sc.objs[i].a[0], sc.objs[i].a[1], sc.objs[i].a[2]), sc.objs[i].s0)) m |= 1u << i;
            wmask[wt] = m;
        }
    }
    __shared__ unsigned last_s;
    __shared__ uint32_t pos[kOrderClasses][NT];
    __threadfence();
    __syncthreads();
    if (tid == 0) last_s = atomicAdd(&plan[kOrderArrived], 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    // thread t sorts the tiles [t0, t1): counts per class, a scan over the threads, then the tiles in order
    const int per = (n + NT - 1) / NT, t0 = min(n, tid * per), t1 = min(n, t0 + per);
    const Vec3d cam = vec3d(g.cam[0], g.cam[1], g.cam[2]);
    for (int c = 0; c < kOrderClasses; c++) pos[c][tid] = 0;
    for (int t = t0; t < t1; t++) {
        const int tx = t % tiles_x, ty = t / tiles_x;
        int c = 3;
        for (int b = 0; b < kTileH / kWaveTileH; b++)
            for (int a = 0; a < kTileW / kWaveTileW; a++) {
                const int wx = tx * (kTileW / kWaveTileW) + a, wy = ty * (kTileH / kWaveTileH) + b;
                if (wx < wtiles_x && wy < wtiles_y) c = min(c, (int)wcls[wy * wtiles_x + wx]);
            }
        c = max(c, 1);
        if (c == 1) {
            const Vec3d d = pixel_dir(g, cam, tx * kTileW + kTileW / 2, ty * kTileH + kTileH / 2);
            for (unsigned i = 0; i < sp.n; i++) {
                if (!((sp.transp >> i) & 1u)) continue;
                const Vec3d v = vec3d(sp.s[i][0] - cam.x, sp.s[i][1] - cam.y, sp.s[i][2] - cam.z);
                const double along = dot3d(d, v);
                if (along > 0 && along * along - dot3d(v, v) + sp.s[i][3] * sp.s[i][3] >= 0) c = 0;
            }
        }
        tcls[t] = (unsigned char)c;
        pos[c][tid]++;
    }
    uint32_t own[kOrderClasses], v[kOrderClasses];
    for (int c = 0; c < kOrderClasses; c++) own[c] = pos[c][tid];
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {  // inclusive scan over the threads, all classes at once
        for (int c = 0; c < kOrderClasses; c++) v[c] = tid >= off ? pos[c][tid - off] : 0u;
        __syncthreads();
        for (int c = 0; c < kOrderClasses; c++) pos[c][tid] += v[c];
        __syncthreads();
    }
    uint32_t base = 0;
    for (int c = 0; c < kOrderClasses; c++) {
        v[c] = base + pos[c][tid] - own[c];  // where this thread's first tile of class c goes
        if (tid == 0) plan[c] = base;
        base += pos[c][NT - 1];
    }
    __syncthreads();
    for (int c = 0; c < kOrderClasses; c++) pos[c][tid] = v[c];
    for (int t = t0; t < t1; t++) list[pos[tcls[t]][tid]++] = (uint32_t)t;
    if (tid == 0) {
        plan[kOrderClasses] = (uint32_t)n;
        plan[kOrderArrived] = 0;
    }
}

// The lens table (cgrt_lens_stage.h; behind tile_order_kernel and ahead of the frame -- lens_table_prepare, cgrt_tile_order.hpp, puts it
// on the handle's second stream, beside the cost probe and the ranking kernels, where there is one): one workgroup
// of kThreads threads per list entry below the table's capacity; an entry of class 3 -- the terminal-diffuse body reads no table --
// leaves at once.  Thread t of the workgroup has the pixel thread t of the entry's tile workgroup has in trace_grid_body: the tile
// from the list (a literal tile number, row-major), the 2x2 wave tiles, lane & 15 and lane >> 4, global_row, pixel_key of the global
// pixel.  It writes table[entry][s][t] for every sample s of the launch, a batch of kLensTableBatch at a time: the accepted draw of
// sample sample_offset + s, or 0 where the thread has no live pixel.  Ordinary vector stores; a thread reads back only its own.
__global__ __launch_bounds__(kThreads) void lens_table_kernel(GridParams g, uint64_t *__restrict__ table) {
    constexpr int NT = kThreads;
    const unsigned entry = blockIdx.x;
    if (entry >= (unsigned)g.lens_table_cap || entry >= load_uniform(g.plan + 3)) return;  // workgroup-uniform
    const int tile = (int)load_uniform(g.border + entry), tiles_x = (g.W + kTileW - 1) / kTileW;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW, wtiles_y = (g.rows + kWaveTileH - 1) / kWaveTileH;
    const int wx = (tile % tiles_x) * (kTileW / kWaveTileW) + (wave & 1), wy = (tile / tiles_x) * (kTileH / kWaveTileH) + (wave >> 1);
    const int w = wx * kWaveTileW + (lane & 15), j = wy * kWaveTileH + (lane >> 4), h = global_row(g, j);
    const bool live = wx < wtiles_x && wy < wtiles_y && w < g.W && j < g.rows && h < g.H;
    const uint64_t k_pix = pixel_key(g.seed, (uint64_t)h * (uint64_t)g.W + (uint64_t)w);
    for (int first = 0; first < g.spp; first += kLensTableBatch) {
        const int count = min(kLensTableBatch, g.spp - first);
        uint64_t *row = table + lens_table_at(entry, first, (int)threadIdx.x, g.spp, NT) / sizeof(uint64_t);
        uint32_t rejected = lens_table_first(k_pix, (uint64_t)(g.sample_offset + first), count, live, row, NT);
        while (__ballot(rejected != 0u) != 0ull)
            if (rejected != 0u) rejected = lens_table_retry(rejected, row, NT);
    }
}

// Sure tiles (wsure, GridParams::wsure; behind tile_order_kernel on its stream, where the launch has sphere masks): one thread per wave
// tile.  A wave tile of a class-3 TILE -- the terminal-diffuse body renders no other, and only tile_order_kernel's last workgroup
// knows the tiles' classes, which is why this is a kernel of its own -- gets the sphere that every primary ray of it hits first
// (sphere_sure_first, cgrt_sure_first.h, over the wave tile's mask), every other wave tile kSureNone.
__global__ __launch_bounds__(256) void sure_first_kernel(GridParams g, DeviceScene sc, int tiles_x, const unsigned char *__restrict__ tcls,
                                                         const uint32_t *__restrict__ wmask, unsigned char *__restrict__ wsure) {
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW, wtiles_y = (g.rows + kWaveTileH - 1) / kWaveTileH;
    const int wt = blockIdx.x * blockDim.x + threadIdx.x;
    if (wt >= wtiles_x * wtiles_y) return;
    const int wx = wt % wtiles_x, wy = wt / wtiles_x;
    int win = -1;
    if (tcls[(wy / (kTileH / kWaveTileH)) * tiles_x + wx / (kTileW / kWaveTileW)] == 3) {
        const TileRays tr = wave_tile_rays(g, wx, wy);
        const ObjRec *objs = sc.objs;
        win = sphere_sure_first(g, tr, sc.n_objs, [objs](int i) { return SureSphere{vec3d(objs[i].a[0], objs[i].a[1], objs[i].a[2]), objs[i].s0}; },
                                wmask[wt]);
    }
    wsure[wt] = (unsigned char)(win >= 0 ? win : kSureNone);
}

// The relay's start table by cost (cgrt_relay.h, "The start order by cost"; behind the cost probe on its stream).  Two launches of
// ceil(words / 256) workgroups, `words` being what the host knows to bound t (relay_start_words); threads beyond t store nothing.
// relay_weight_kernel: thread i writes weight[i] of item i.  relay_start_kernel: thread i counts the items that start before
// item i -- all t of them, read a workgroup's worth at a time through LDS -- and writes the item's word at that rank; the order
// is total, so the ranks are a permutation of [0, t) and every word of the table is written once.
struct RelayStartArgs {
    RelayItems r;
    uint32_t tiles_x, wtiles_x, wtiles_y;
};
__device__ __forceinline__ RelayItems relay_items_of(const RelayStartArgs &a, const uint32_t *plan) {
    RelayItems r = a.r;
    r.n01 = plan[2];
    r.n012 = plan[3];
    r.n_tiles = plan[kOrderClasses];
    return r;
}
__global__ __launch_bounds__(kRelayThreads) void relay_weight_kernel(RelayStartArgs a, const uint32_t *__restrict__ plan, const uint32_t *__restrict__ list,
                                                                     const uint32_t *__restrict__ wcost, unsigned long long *__restrict__ weight) {
    const RelayItems r = relay_items_of(a, plan);
    const uint32_t i = blockIdx.x * kRelayThreads + threadIdx.x;
    if (i >= relay_items_total(r)) return;
    const RelayBlock b = relay_item(i, r);
    weight[i] = relay_item_weight(b, relay_tile_cost(wcost, list[b.entry], a.tiles_x, a.wtiles_x, a.wtiles_y), r);
}
__global__ __launch_bounds__(kRelayThreads) void relay_start_kernel(RelayStartArgs a, const uint32_t *__restrict__ plan,
                                                                    const unsigned long long *__restrict__ weight, uint32_t *__restrict__ start) {
    const RelayItems r = relay_items_of(a, plan);
    const uint32_t t = relay_items_total(r), i = blockIdx.x * kRelayThreads + threadIdx.x;
    if (blockIdx.x * kRelayThreads >= t) return;  // the whole workgroup: no barrier is missed
    __shared__ unsigned long long w_s[kRelayThreads];
    const unsigned long long wi = i < t ? weight[i] : 0ull;
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < t; j0 += kRelayThreads) {
        __syncthreads();  // every thread is done with the previous batch
        if (j0 + threadIdx.x < t) w_s[threadIdx.x] = weight[j0 + threadIdx.x];
        __syncthreads();
        const uint32_t n = min((uint32_t)kRelayThreads, t - j0);
        for (uint32_t u = 0; u < n; u++) rank += relay_item_before(w_s[u], j0 + u, wi, i) ? 1u : 0u;
    }
    if (i < t) start[rank] = relay_start_word(relay_item(i, r));
}

// The same table with promoted tiles (cgrt_relay.h, "Four chunks for the heaviest tiles"), four launches in place of the two, `head`
// zeroed in front of them.  relay_boost_cost_kernel: thread e < n012 writes ecost[e], the entry's tile cost, and adds cost x spp to
// S (an integer sum: any order is exact).  relay_boost_promote_kernel: thread e < n_split ranks its entry among the candidates --
// all n_split keys, a workgroup's worth at a time through LDS -- and writes bslot[e]; the promoted are counted.
// relay_boost_weight_kernel: thread v writes weight[v] of virtual item v = entry * k_boost + chunk (kRelayNoItem where the
// entry has no such chunk), and one thread leaves the item count in the head.  relay_boost_start_kernel: relay_start_kernel over
// the virtual items, those that are none skipped.  O(n^2 / 256) a thread as before, n = k_boost * n012.
struct RelayBoostArgs {
    RelayStartArgs a;
    RelayBoost b;
};
__global__ __launch_bounds__(kRelayThreads) void relay_boost_cost_kernel(RelayBoostArgs ba, const uint32_t *__restrict__ plan, const uint32_t *__restrict__ list,
                                                                         const uint32_t *__restrict__ wcost, uint32_t *__restrict__ ecost,
                                                                         uint32_t *__restrict__ head) {
    const RelayItems r = relay_items_of(ba.a, plan);
    const uint32_t e = blockIdx.x * kRelayThreads + threadIdx.x;
    if (e >= r.n012) return;
    const uint32_t c = relay_tile_cost(wcost, list[e], ba.a.tiles_x, ba.a.wtiles_x, ba.a.wtiles_y);
    ecost[e] = c;
    if (c) atomicAdd(reinterpret_cast<unsigned long long *>(head + kBoostS), (unsigned long long)c * (unsigned long long)r.spp);
}
__global__ __launch_bounds__(kRelayThreads) void relay_boost_promote_kernel(RelayBoostArgs ba, const uint32_t *__restrict__ plan,
                                                                            const uint32_t *__restrict__ ecost, uint32_t *__restrict__ head,
                                                                            uint32_t *__restrict__ bslot) {
    const RelayItems r = relay_items_of(ba.a, plan);
    const uint32_t n_split = relay_split_entries(r.n01, r.n012, r.cap, r.extent), e = blockIdx.x * kRelayThreads + threadIdx.x;
    if (blockIdx.x * kRelayThreads >= n_split) return;  // the whole workgroup: no barrier is missed
    const uint64_t S = *reinterpret_cast<const unsigned long long *>(head + kBoostS);
    __shared__ unsigned long long k_s[kRelayThreads];
    const uint32_t ce = e < n_split ? ecost[e] : 0u;
    const uint64_t ke = relay_boost_key(e < n_split && relay_boost_candidate(ce, r, ba.b, S), ce);
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < n_split; j0 += kRelayThreads) {
        __syncthreads();  // every thread is done with the previous batch
        if (j0 + threadIdx.x < n_split) {
            const uint32_t cj = ecost[j0 + threadIdx.x];
            k_s[threadIdx.x] = relay_boost_key(relay_boost_candidate(cj, r, ba.b, S), cj);
        }
        __syncthreads();
        const uint32_t n = min((uint32_t)kRelayThreads, n_split - j0);
        for (uint32_t u = 0; u < n; u++) rank += relay_item_before(k_s[u], j0 + u, ke, e) ? 1u : 0u;
    }
    if (e >= n_split) return;
    const bool promoted = ke != 0 && rank < ba.b.cap;
    bslot[e] = promoted ? rank + 1u : 0u;
    if (promoted) atomicAdd(head + kBoostPromoted, 1u);
}
__global__ __launch_bounds__(kRelayThreads) void relay_boost_weight_kernel(RelayBoostArgs ba, const uint32_t *__restrict__ plan,
                                                                           const uint32_t *__restrict__ ecost, const uint32_t *__restrict__ bslot,
                                                                           uint32_t *__restrict__ head, unsigned long long *__restrict__ weight) {
    const RelayItems r = relay_items_of(ba.a, plan);
    const uint32_t n_split = relay_split_entries(r.n01, r.n012, r.cap, r.extent), v = blockIdx.x * kRelayThreads + threadIdx.x;
    if (v == 0) head[kBoostItems] = relay_boost_items(r, ba.b, head[kBoostPromoted]);
    if (v >= r.n012 * ba.b.k) return;
    const uint32_t e = v / ba.b.k, c = v % ba.b.k;
    const bool promoted = e < n_split && bslot[e] != 0u;
    weight[v] = relay_boost_weight(c, relay_boost_chunks(e, promoted, n_split, r, ba.b), promoted, ecost[e], r, ba.b);
}
__global__ __launch_bounds__(kRelayThreads) void relay_boost_start_kernel(RelayBoostArgs ba, const uint32_t *__restrict__ plan,
                                                                          const unsigned long long *__restrict__ weight, uint32_t *__restrict__ start) {
    const RelayItems r = relay_items_of(ba.a, plan);
    const uint32_t nv = r.n012 * ba.b.k, v = blockIdx.x * kRelayThreads + threadIdx.x;
    if (blockIdx.x * kRelayThreads >= nv) return;  // the whole workgroup: no barrier is missed
    __shared__ unsigned long long w_s[kRelayThreads];
    const unsigned long long wv = v < nv ? weight[v] : kRelayNoItem;
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < nv; j0 += kRelayThreads) {
        __syncthreads();  // every thread is done with the previous batch
        if (j0 + threadIdx.x < nv) w_s[threadIdx.x] = weight[j0 + threadIdx.x];
        __syncthreads();
        const uint32_t n = min((uint32_t)kRelayThreads, nv - j0);
        for (uint32_t u = 0; u < n; u++) rank += relay_boost_before(w_s[u], j0 + u, wv, v) ? 1u : 0u;
    }
    if (wv != kRelayNoItem) start[rank] = relay_start_word(RelayBlock{v / ba.b.k, (int32_t)(v % ba.b.k), false});
}

// ---- cost-aware scheduling: plan and ordered sum (GridParams, "Cost-aware scheduling") ------------------------------------
// One workgroup.  cost[]: the wave tiles' probe costs.  A wave tile is HEAVY when its cost exceeds total / divisor --
// divisor = wave slots of the chip x a constant, i.e. when the tile alone would occupy a wave slot for more than 1/constant
// of the frame's ideal duration.  At most kmax tiles can be heavy (what the deferred buffers hold): if more exceed the
// threshold it is raised, on a quarter-octave histogram of the costs, until the count fits -- the heaviest stay.
// Output: order[0..K) = the heavy wave tiles, heaviest histogram bin first, hidx[wave tile] = rank or -1, plan[0] = K,
// plan[1] = threshold, plan[2] = 0 (the item queue's head); with `border`: the tile queue (GridParams::border), plan[3] = its
// length, plan[4] = 0 (its head).
__global__ __launch_bounds__(1024) void plan_kernel(const uint32_t *__restrict__ cost_in, const unsigned char *__restrict__ light, int n,
                                                    unsigned kmax, unsigned long long divisor, uint32_t *__restrict__ plan,
                                                    uint32_t *__restrict__ order, int32_t *__restrict__ hidx,
                                                    uint32_t *__restrict__ border, int wtiles_x, int wtiles_y, int tw, int th) {
    // a light tile (rendered by the other launch) counts for nothing here
    auto cost = [&](int i) -> uint32_t { return (light && light[i]) ? 0u : cost_in[i]; };
    __shared__ unsigned long long part[1024];
    __shared__ unsigned base_s, hist[128];
    __shared__ unsigned long long thr_s;
    auto bin_of = [](uint32_t c) { return c < 4u ? (int)c : (31 - __clz((int)c)) * 4 + (int)((c >> (29 - __clz((int)c))) & 3u); };
    if (threadIdx.x < 128) hist[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long t = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const uint32_t c = cost(i);
        t += c;
        atomicAdd(&hist[bin_of(c)], 1u);
    }
    part[threadIdx.x] = t;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        unsigned long long thr = part[0] / divisor;
        if (thr < 1) thr = 1;
        // raise the threshold to the lower edge of the lowest histogram bin such that all bins above it hold <= kmax tiles
        unsigned above = 0;
        int b = 127;
        for (; b >= 0; b--) {
            if (above + hist[b] > kmax) break;
            above += hist[b];
        }
        if (b >= 0) {  // bins 0..b must stay out: threshold = the largest cost of bin b
            const unsigned long long edge = b < 4 ? (unsigned long long)b
                                                  : (((4ull + (unsigned long long)(b & 3) + 1ull) << (b / 4)) >> 2) - 1ull;
            if (edge > thr) thr = edge;
        }
        thr_s = thr;
        base_s = 0;
    }
    __syncthreads();
    const unsigned long long thr = thr_s;
    // Counting sort of the heavy tiles by histogram bin, heaviest bin first (longest-processing-time-first at quarter-octave
    // resolution; the order inside a bin is whatever the atomics give -- it affects neither the image nor the counters).
    // hist[] is reused: bins wholly above the threshold get their start offset, the others nothing.
    if (threadIdx.x == 0) {
        unsigned off = 0;
        for (int b = 127; b >= 0; b--) {
            const unsigned long long lo = b < 4 ? (unsigned long long)b : ((4ull + (unsigned long long)(b & 3)) << (b / 4)) >> 2;  // smallest cost of bin b
            const unsigned c = hist[b];
            if (lo > thr) {
                hist[b] = off;
                off += c;
            } else {
                hist[b] = 0xffffffffu;  // the bin holding the threshold (its costs may lie on either side) and all below: not heavy
            }
        }
        base_s = off < kmax ? off : kmax;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
        const uint32_t c = cost(i);
        const int b = bin_of(c);
        int32_t r = -1;
        if (hist[b] != 0xffffffffu) {
            const unsigned slot = atomicAdd(&hist[b], 1u);
            if (slot < kmax) {
                r = (int32_t)slot;
                order[slot] = (uint32_t)i;
            }
        }
        hidx[i] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        plan[0] = base_s;
        plan[1] = (uint32_t)(thr > 0xffffffffull ? 0xffffffffull : thr);
        plan[2] = 0;
        plan[3] = 0;
        plan[4] = 0;
        plan[5] = 0;  // primary_walk_kernel's head of the item queue
    }
    if (!border) return;
    // The tile queue: tiles of tw x th wave tiles (one workgroup's worth) with something left to render -- a wave tile that is
    // neither light nor heavy --, costliest histogram bin first.
    const int tiles_x = (wtiles_x + tw - 1) / tw, tiles_y = (wtiles_y + th - 1) / th, n_tiles = tiles_x * tiles_y;
    auto tile_cost = [&](int t, bool &any) -> uint32_t {
        const int tx = t % tiles_x, ty = t / tiles_x;
        unsigned long long c = 0;
        any = false;
        for (int b = 0; b < th; b++)
            for (int a = 0; a < tw; a++) {
                const int wx = tx * tw + a, wy = ty * th + b;
                if (wx >= wtiles_x || wy >= wtiles_y) continue;
                const int i = wy * wtiles_x + wx;
                if ((light && light[i]) || hidx[i] >= 0) continue;
                any = true;
                c += cost_in[i];
            }
        return c > 0xffffffffull ? 0xffffffffu : (uint32_t)c;
    };
    if (threadIdx.x < 128) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int t2 = threadIdx.x; t2 < n_tiles; t2 += 1024) {
        bool any;
        const uint32_t c = tile_cost(t2, any);
        if (any) atomicAdd(&hist[bin_of(c)], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned off = 0;
        for (int b = 127; b >= 0; b--) {
            const unsigned c = hist[b];
            hist[b] = off;
            off += c;
        }
        plan[3] = off;
    }
    __syncthreads();
    for (int t2 = threadIdx.x; t2 < n_tiles; t2 += 1024) {
        bool any;
        const uint32_t c = tile_cost(t2, any);
        if (any) border[atomicAdd(&hist[bin_of(c)], 1u)] = (uint32_t)t2;
    }
}

// The per-pixel camera constants of the heavy tiles (what set_pixel computes), one 64-thread workgroup per heavy tile.
// POSE: a posed launch's -- direction and focus point in the world, as set_pixel has them there.
template <bool POSE = false>
__global__ __launch_bounds__(64) void pixel_const_kernel(GridParams g) {
    const unsigned hr = blockIdx.x;
    if (hr >= g.plan[0]) return;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW;
    const uint32_t wt = g.order[hr];
    const int p = threadIdx.x;
    const int w = (int)(wt % (uint32_t)wtiles_x) * kWaveTileW + (p & 15), j = (int)(wt / (uint32_t)wtiles_x) * kWaveTileH + (p >> 4);
    const int h = global_row(g, j);
    const V3 camorg = mk(g.cam[0], g.cam[1], g.cam[2]);
    // main.cpp:188-189,198,203 -- the same expressions as set_pixel
    const double px = (2.0 * ((double)w / g.W) - 1) * g.half_width;
    const double py = (2.0 * ((double)h / g.H) - 1) * g.half_width * g.H / g.W;
    V3 pdir = normalized(mk(px, py, 0) - camorg);
    V3 pof = pdir * ((g.focus_plane - camorg.z) / pdir.z) + camorg;
    if (POSE) {
        pof = pose_v(g, pof);
        pdir = normalized(pose_v(g, mk(px, py, 0)) - pose_v(g, camorg));
    }
    const uint64_t k_pix = pixel_key(g.seed, (uint64_t)h * (uint64_t)g.W + (uint64_t)w);
    double *pc = g.pconst + (size_t)hr * (7 * 64) + p;
    pc[0 * 64] = pdir.x; pc[1 * 64] = pdir.y; pc[2 * 64] = pdir.z;
    pc[3 * 64] = pof.x;  pc[4 * 64] = pof.y;  pc[5 * 64] = pof.z;
    pc[6 * 64] = __longlong_as_double((long long)k_pix);
}

// One 64-thread workgroup per heavy tile, one thread per pixel: the pixel's Hitpoint values added sample by sample, in
// emission order within a sample -- the order of the reference's serial loop (main.cpp:204-209 around main.cpp:85-100).
// The additions are a serial chain but the loads are not: the counts and the first value of eight samples are requested
// together (a sample rarely has more than one Hitpoint outside glass), further values of a sample all at once.
__global__ __launch_bounds__(64) void deferred_sum_kernel(GridParams g, float *__restrict__ rgb, uint32_t *__restrict__ nhit_out) {
    const unsigned hr = blockIdx.x;
    if (hr >= g.plan[0]) return;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW;
    const uint32_t wt = g.order[hr];
    const int p = threadIdx.x;
    const int w = (int)(wt % (uint32_t)wtiles_x) * kWaveTileW + (p & 15), j = (int)(wt / (uint32_t)wtiles_x) * kWaveTileH + (p >> 4);
    if (w >= g.W || j >= g.rows) return;
    double r = 0, gg = 0, b = 0;
    uint32_t hits = 0;
    if (global_row(g, j) < g.H) {  // rows past the image (stripe padding) had no units: zero
        constexpr int B = 8;
        for (int s0 = 0; s0 < g.spp; s0 += B) {
            int c[B];
            double v[B][3];
#pragma unroll
            for (int i = 0; i < B; i++) {
                const size_t us = (size_t)hr * g.spp + (s0 + i < g.spp ? s0 + i : g.spp - 1);
                c[i] = s0 + i < g.spp ? (int)g.dcnt[us * 64 + p] : 0;
                const double *q = g.dvals + (us * g.maxhp * 64 + p) * 3;
                v[i][0] = q[0]; v[i][1] = q[1]; v[i][2] = q[2];  // slot 0 always exists (read even when the count is 0)
            }
#pragma unroll
            for (int i = 0; i < B; i++) {
                if (c[i] > 0) {
                    r += v[i][0];
                    gg += v[i][1];
                    b += v[i][2];
                    const size_t us = (size_t)hr * g.spp + s0 + i;
                    for (int q = 1; q < c[i]; q++) {
                        const double *x = g.dvals + ((us * g.maxhp + q) * 64 + p) * 3;
                        r += x[0];
                        gg += x[1];
                        b += x[2];
                    }
                    hits += (uint32_t)c[i];
                }
            }
        }
    }
    const float fr = (float)(r * g.inv_spp_total), fg = (float)(gg * g.inv_spp_total), fb = (float)(b * g.inv_spp_total);
    float *dst = rgb + ((size_t)j * g.W + w) * 3;
    if (g.accumulate) {
        dst[0] += fr; dst[1] += fg; dst[2] += fb;
    } else {
        dst[0] = fr; dst[1] = fg; dst[2] = fb;
    }
    if (nhit_out) nhit_out[(size_t)j * g.W + w] = hits;
}

// function-level probe: one object, n rays (cgrt_intersect_rays)
__global__ void intersect_rays_kernel(DeviceScene sc, int obj, const double *__restrict__ org,
                                      const double *__restrict__ dir, const unsigned long long *__restrict__ keys,
                                      int n, int32_t *__restrict__ hit,
                                      double *__restrict__ len, double *__restrict__ nrm) {
    __shared__ BezLds bl;  // blockDim.x == 64: one wave per block
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    const int ii = on ? i : 0;
    uint32_t a = 0, b = 0;
    const V3 o = ld3(org + 3 * ii), d = ld3(dir + 3 * ii);
    DeviceScene one = sc;
    one.prun_begin = one.prun_end = 0;  // the list handed down is this one object
    RayKey rk{keys ? keys[ii] : 0ull, 1, true, 0u};
    const LdsAux aux{&bl, nullptr};
    SceneHit h = intersect_scene<true, true, false, false>(sc.objs + obj, 1, 1, one, o, d, rk, on, aux, a, b);
    if (!on) return;
    hit[i] = h.id >= 0 ? 1 : 0;
    len[i] = h.t;
    nrm[3 * i] = h.n.x;
    nrm[3 * i + 1] = h.n.y;
    nrm[3 * i + 2] = h.n.z;
}

// ob.getSurfaceColor(P) (objects.h:84-86,533-539 -> Texture::color): the flat colour, except on a textured plane inside the
// texture rectangle.  Shared by surface_colors_kernel and ray_hit_attributes_kernel (cgrt_hit_attr.hpp).
__device__ __forceinline__ V3 surface_color(const DeviceScene &sc, const ObjRec &ob, V3 P) {
    V3 f = ld3(ob.col);
    if (ob.kind == KIND_PLANE && ob.tex >= 0) {
        V3 c;
        if (texture_color(sc.texs[ob.tex], sc.texels, P, c)) f = c;
    }
    return f;
}

// function-level probe: objs[obj]->getSurfaceColor(P) for n points
__global__ void surface_colors_kernel(DeviceScene sc, int obj, const double *__restrict__ pts, int n, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 f = surface_color(sc, sc.objs[obj], ld3(pts + 3 * i));
    out[3 * i] = f.x;
    out[3 * i + 1] = f.y;
    out[3 * i + 2] = f.z;
}

// function-level probe of the device math (cgrt_math_probe): element i runs on thread i % 256 of block i / 256, so elements
// 64k .. 64k+63 are the lanes of one wave; a lane with i >= n returns BEFORE the call, so the ballots of sqrt_cr / normalized see
// the live lanes of the last wave only.  Calls the inlines the render kernels call.
__global__ void math_probe_kernel(int op, const double *__restrict__ in, long long n, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == CGRT_PROBE_SQRT) {  // (wave-uniform branches)
        out[i] = sqrt_cr(in[i]);
    } else if (op == CGRT_PROBE_NORMALIZED) {
        const V3 v = normalized(ld3(in + 3 * i));
        out[3 * i] = v.x;
        out[3 * i + 1] = v.y;
        out[3 * i + 2] = v.z;
    } else if (op == CGRT_PROBE_SPHERE_LEN) {  // centre(3), r2, origin(3), direction(3)
        const double *p = in + 10 * i;
        out[i] = sphere_len(ld3(p), p[3], ld3(p + 4), ld3(p + 7));
    } else {  // CGRT_PROBE_SPHERE_LEN_PAIR: centre A(3), r2 A, centre B(3), r2 B, origin(3), direction(3)
        const double *p = in + 14 * i;
        sphere_len_pair(ld3(p), p[3], ld3(p + 4), p[7], ld3(p + 8), ld3(p + 11), out[2 * i], out[2 * i + 1]);
    }
}

// function-level probe of the inside trips (cgrt_inside_probe, CGRT_PROBE_INSIDE_LOOP): the PAIR variants' sphere loop over a
// committed sphere scene, once without candidates -- the pair loop -- and once with the trait `guarded`, for n rays
// {origin(3), direction(3)} laid out over the waves as math_probe_kernel's elements are.  out[n][5] = t and id of the pair loop,
// t and id of the guarded loop, and 1 where the element's wave took the one-by-one loop.  The object list is read from memory.
__global__ void inside_loop_probe_kernel(DeviceScene sc, InsideTrait guarded, const double *__restrict__ in, long long n, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 o = ld3(in + 6 * i), d = ld3(in + 6 * i + 3);
    RayKey rk{0, 1, false, 0u};
    LdsAux aux;
    aux.bl = nullptr;
    aux.lnodes = nullptr;
    uint32_t nn = 0, nt = 0;
    sc.inside = InsideTrait{};
    const SceneHit a = intersect_scene<false, false, true, false, false, false, false, false, true>(sc.objs, sc.n_lds, sc.n_objs, sc, o, d, rk, true, aux, nn, nt);
    sc.inside = guarded;
    const SceneHit b = intersect_scene<false, false, true, false, false, false, false, false, true>(sc.objs, sc.n_lds, sc.n_objs, sc, o, d, rk, true, aux, nn, nt);
    bool took = false;
    for (int k = 0; k < kInsideMax && k < guarded.n && !took; k++)
        took = __ballot(!starts_inside(o, ld3(sc.objs[guarded.idx[k]].a), guarded.rin2[k])) == 0ull;
    out[5 * i] = a.t;
    out[5 * i + 1] = (double)a.id;
    out[5 * i + 2] = b.t;
    out[5 * i + 3] = (double)b.id;
    out[5 * i + 4] = took ? 1.0 : 0.0;
}

#endif
