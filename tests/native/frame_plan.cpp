// The host side of cgrt_trace_grid (cgrt_frame.h: frame_plan, max_heavy_tiles, fit_heavy_tiles, frame_params,
// ScratchLayout::place, tile_order_layout, eye_knobs): sample chunks, tile counts, heavy-tile capacity, scheduling, the scratch
// layout, the tile order of a sphere scene and its buffer's layout, against values written out by hand from the rules.  CPU build under ASan + UBSan, driven by tests/test_frame_plan_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cgrt_frame.h"

static int g_failed = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        if (a_ != b_) {                                                                                         \
            std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)

static constexpr size_t GiB = (size_t)1 << 30;
static size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// 1920 x 1080 at 64 spp, a scheduled glass mesh scene (no Bezier, no primary walk) on a 288 GB device with 256 CUs
static FrameInputs frame(int W = 1920, int rows = 1080, int spp = 64) {
    FrameInputs in{};
    in.grid.width = W;
    in.grid.height = rows;
    in.grid.rows = rows;
    in.grid.stripe_nranks = 1;
    in.grid.spp = spp;
    in.grid.spp_total = spp;
    in.grid.max_depth = 5;
    in.grid.seed = 7;
    in.cam.cam[2] = -10;
    in.cam.half_width = 10;
    in.cam.focus_plane = 20;
    in.sched = true;
    in.glass = true;
    in.nt = 256;
    in.has_mesh = true;
    in.prim_obj = -1;
    in.mem_total = 288000000000ull;
    in.n_cu = 256;
    in.waves_per_simd = 4;
    return in;
}
static FrameInputs one_wave(FrameInputs in) {  // a Bezier scene: one-wave workgroups on 16x4 tiles
    in.has_bezier = true;
    in.nt = 64;
    in.waves_per_simd = 2;
    return in;
}

static void chunking() {
    FrameInputs in = frame();
    CHECK_EQ(frame_plan(in, 0).chunks, 1);  // no CGRT_GRID_SPLIT_SAMPLES
    CHECK_EQ(frame_plan(in, 0).chunk_spp, 64);
    in.grid.flags = CGRT_GRID_SPLIT_SAMPLES;
    in.grid.spp = 31;
    CHECK_EQ(frame_plan(in, 0).chunks, 1);
    CHECK_EQ(frame_plan(in, 0).chunk_spp, 31);
    in.grid.spp = 32;
    CHECK_EQ(frame_plan(in, 0).chunks, 2);
    CHECK_EQ(frame_plan(in, 0).chunk_spp, 16);
    in.grid.spp = 1024;
    CHECK_EQ(frame_plan(in, 0).chunks, 16);
    CHECK_EQ(frame_plan(in, 0).chunk_spp, 64);
    in.grid.spp = 100;  // 6 chunks of 17 samples, the last one of 15
    CHECK_EQ(frame_plan(in, 0).chunks, 6);
    CHECK_EQ(frame_plan(in, 0).chunk_spp, 17);
    FrameInputs sp = in;
    sp.sched = false;
    sp.spill = true;
    CHECK_EQ(frame_plan(sp, 0).chunks, 1);
    CHECK_EQ(frame_plan(sp, 0).chunk_spp, 100);
    // 10000 x 5000 pixels: 28 bytes of chunk sums per pixel and chunk, at most 4 GiB -> 3 chunks (4 would be 5.6 GB)
    FrameInputs big = frame(10000, 5000, 1000);
    big.grid.flags = CGRT_GRID_SPLIT_SAMPLES;
    const FramePlan p = frame_plan(big, 0);
    CHECK_EQ(p.chunks, 3);
    CHECK_EQ(p.chunk_spp, 334);
    CHECK_EQ(p.scratch.partial.bytes, 3ull * 50000000 * 24);
    CHECK_EQ(p.scratch.partial_nhit.at, 3ull * 50000000 * 24);
    CHECK_EQ(p.scratch.partial_nhit.bytes, 3ull * 50000000 * 4);
}

static void tile_counts() {
    // row-major 32x8 tiles (no mesh): 100 x 20 pixels = 4 x 3 tiles, 7 x 5 wave tiles
    FrameInputs in = frame(100, 20);
    in.has_mesh = false;
    FramePlan p = frame_plan(in, 0);
    CHECK_EQ(p.xcd_tiles, 0);
    CHECK_EQ(p.tile_blocks, 12);
    CHECK_EQ(p.grid_dim, 12);
    CHECK_EQ(p.wtiles_x, 7);
    CHECK_EQ(p.wtiles_y, 5);
    CHECK_EQ(p.n_wt, 35);
    // XCD super-tiles (a mesh, no Bezier): 1000 x 100 pixels = 32 x 13 tiles = 8 x 4 super-tiles of 4 x 4 (the last row of
    // super-tiles is a quarter full) = 4 rounds of 8 XCDs x 16 tiles
    p = frame_plan(frame(1000, 100), 0);
    CHECK_EQ(p.xcd_tiles, 1);
    CHECK_EQ(p.tile_blocks, 512);
    // 1920 x 1080 = 60 x 135 tiles = 15 x 34 super-tiles = 510 -> 64 rounds of 8 x 16
    p = frame_plan(frame(), 0);
    CHECK_EQ(p.tile_blocks, 8192);
    CHECK_EQ(p.n_wt, 32400);
    // one-wave 16x4 tiles: one workgroup per wave tile, row-major
    p = frame_plan(one_wave(frame(100, 20)), 0);
    CHECK_EQ(p.xcd_tiles, 0);
    CHECK_EQ(p.tile_blocks, 35);
    // no XCD order when spilling or with a Bezier object
    FrameInputs sp = frame(1000, 100);
    sp.sched = false;
    sp.spill = true;
    CHECK_EQ(frame_plan(sp, 0).xcd_tiles, 0);
    CHECK_EQ(frame_plan(sp, 0).tile_blocks, 416);
    FrameInputs bz = frame(1000, 100);
    bz.has_bezier = true;
    CHECK_EQ(frame_plan(bz, 0).xcd_tiles, 0);
}

static void capacity() {
    // the worked case: 64 x 64 x 16 x 24 + 4 096 + 3 584 bytes per heavy tile, 12 GiB of budget
    FrameInputs in = frame();
    CHECK_EQ(frame_plan(in, 0).tile_bytes, 1580544);
    CHECK_EQ(max_heavy_tiles(in), 8152);
    in.mem_total = 16 * GiB;  // an eighth of the device: 2 GiB
    CHECK_EQ(max_heavy_tiles(in), 1358);
    in.knobs.defer_bytes = 100 << 20;  // CGRT_DEFER_BYTES
    CHECK_EQ(max_heavy_tiles(in), 66);
    CHECK_EQ(max_heavy_tiles(frame(64, 8)), 8);  // capped at the wave tiles
    FrameInputs im = frame();
    im.sched = false;
    CHECK_EQ(max_heavy_tiles(im), 0);
    // per heavy tile: maxhp 1 against 16, with and without the primary walk's distances and triangles (12 bytes a unit)
    FrameInputs op = frame();
    op.glass = false;
    CHECK_EQ(frame_plan(op, 0).maxhp, 1);
    CHECK_EQ(frame_plan(op, 0).tile_bytes, 98304 + 4096 + 3584);
    op.prim_obj = 0;
    CHECK_EQ(frame_plan(op, 0).use_prim, 1);
    CHECK_EQ(frame_plan(op, 0).tile_bytes, 98304 + 4096 + 3584 + 32768 + 16384);
    // the counts are padded to 8 bytes: spp 1 -> 64 bytes, spp 3 -> 192
    CHECK_EQ(frame_plan(frame(1920, 1080, 3), 0).tile_bytes, 3 * 64 * 16 * 24 + 192 + 3584);
}

// every region inside the total, no two overlapping, the alignments the arrays rely on, and the total of the rule
static void check_layout(const FrameInputs &in, size_t kmax) {
    const FramePlan p = frame_plan(in, kmax);
    const ScratchLayout &L = p.scratch;
    const Region rs[] = {L.partial, L.partial_nhit, L.cost, L.order, L.hidx, L.border, L.plan, L.light, L.dvals, L.dcnt, L.pconst,
                         L.prim_len, L.prim_tri};
    const size_t n = sizeof(rs) / sizeof(rs[0]);
    for (size_t i = 0; i < n; i++) {
        if (!rs[i].bytes) continue;
        CHECK_EQ(rs[i].at + rs[i].bytes <= L.total, 1);
        for (size_t j = i + 1; j < n; j++)
            if (rs[j].bytes) CHECK_EQ(rs[i].at + rs[i].bytes <= rs[j].at || rs[j].at + rs[j].bytes <= rs[i].at, 1);
    }
    const size_t npx = (size_t)in.grid.rows * in.grid.width;
    const size_t chunk = p.chunks > 1 ? al256((size_t)p.chunks * npx * 28) : 0;
    const size_t sched = al256((4 * (p.n_wt + 8) + 64) * 4 + al256(p.n_wt));
    CHECK_EQ(L.total, chunk + (in.sched ? sched + (kmax ? kmax * p.tile_bytes + 256 : 0) : 0));
    if (!kmax) {
        CHECK_EQ(L.cost.bytes + L.dvals.bytes, 0);
        return;
    }
    CHECK_EQ(L.cost.at, chunk);
    CHECK_EQ(L.cost.at % 256, 0);
    CHECK_EQ(L.dvals.at, chunk + sched);
    CHECK_EQ(L.dvals.at % 256, 0);
    CHECK_EQ(L.dcnt.at % 8, 0);
    CHECK_EQ(L.pconst.at % 8, 0);
    CHECK_EQ(L.prim_len.at % 8, 0);
    CHECK_EQ(L.prim_tri.at % 4, 0);
    CHECK_EQ(L.light.at, chunk + (4 * (p.n_wt + 8) + 64) * 4);
    CHECK_EQ(L.dvals.bytes, kmax * (size_t)in.grid.spp * 64 * p.maxhp * 24);
    CHECK_EQ(L.prim_tri.at + L.prim_tri.bytes + 256, L.total);  // the deferred arrays end 256 bytes before the total
}

static void scratch_layout() {
    // the worked case: 551 424 bytes of schedule arrays (32 400 wave tiles), then 8 152 heavy tiles
    FrameInputs in = frame();
    FramePlan p = frame_plan(in, 8152);
    CHECK_EQ(p.scratch.dvals.at, 551424);
    CHECK_EQ(p.scratch.total, 551424 + 8152ull * 1580544 + 256);
    CHECK_EQ(p.items_per_tile, 16);
    for (size_t k : {8152, 1000, 1, 0}) check_layout(in, k);
    // a scheduled launch that holds no heavy tile still reserves the schedule arrays
    CHECK_EQ(frame_plan(in, 0).scratch.total, 551424);
    // chunks, the primary walk, the light split, one-wave tiles, odd sizes; image order
    FrameInputs c = frame(333, 77, 48);
    c.grid.flags = CGRT_GRID_SPLIT_SAMPLES;
    c.prim_obj = 2;
    c.glass = false;
    FrameInputs l = frame(1000, 100, 7);
    l.light_ok = true;
    l.prim_obj = 0;
    for (const FrameInputs &f : {c, l, one_wave(l)}) {
        const size_t kmax = max_heavy_tiles(f);
        for (size_t k = kmax;; k /= 2) {
            check_layout(f, k);
            if (!k) break;
        }
    }
    FrameInputs im = c;
    im.sched = false;
    check_layout(im, 0);
    CHECK_EQ(frame_plan(im, 0).scratch.total, al256(3ull * 333 * 77 * 28));
    // place: pointers only for the arrays this frame uses, the hit counts only when the caller wants them
    static unsigned char base[1];
    GridParams g{};
    frame_plan(c, 4).scratch.place(g, base, false);
    CHECK_EQ(g.partial == (double *)base, 1);
    CHECK_EQ(g.partial_nhit == nullptr, 1);
    CHECK_EQ(g.border == nullptr && g.light == nullptr, 1);  // split samples: no tile queue, no light split
    CHECK_EQ(g.prim_tri != nullptr, 1);
    frame_plan(l, 4).scratch.place(g, base, true);
    CHECK_EQ(g.partial == nullptr && g.partial_nhit == nullptr, 1);
    CHECK_EQ((const unsigned char *)g.light - base, (4 * (frame_plan(l, 4).n_wt + 8) + 64) * 4);
    CHECK_EQ((const unsigned char *)g.border - base, 3 * (frame_plan(l, 4).n_wt + 8) * 4);
}

static void scheduled() {
    FrameInputs in = frame();
    FramePlan p = frame_plan(in, 10);
    CHECK_EQ(p.wave_slots, 4096);  // 256 CUs x 4 SIMDs x 4 waves
    CHECK_EQ(p.plan_div, 4096 * 32);
    CHECK_EQ(p.heavy_blocks, 40);  // 10 tiles x 16 items over 4 waves per workgroup
    p = frame_plan(in, 8152);
    CHECK_EQ(p.heavy_blocks, 1024);  // capped at a chip's worth
    CHECK_EQ(p.tile_queue, 1);
    CHECK_EQ(p.grid_dim, 1024);  // the tile queue's workgroups: the same fill
    in.knobs.units_per_item = 1024;
    CHECK_EQ(frame_plan(in, 10).items_per_tile, 4);
    CHECK_EQ(frame_plan(frame(1920, 1080, 5), 10).items_per_tile, 2);  // 320 units in items of 256
    // one-wave workgroups: one wave each, no tile queue
    p = frame_plan(one_wave(frame()), 10);
    CHECK_EQ(p.wave_slots, 2048);
    CHECK_EQ(p.heavy_blocks, 160);
    CHECK_EQ(p.tile_queue, 0);
    CHECK_EQ(p.grid_dim, 32400);
    CHECK_EQ(frame_plan(one_wave(frame()), 8152).heavy_blocks, 2048);
    // tile queue off with chunks and on request
    FrameInputs ch = frame();
    ch.grid.flags = CGRT_GRID_SPLIT_SAMPLES;
    p = frame_plan(ch, 10);
    CHECK_EQ(p.chunks, 4);
    CHECK_EQ(p.tile_queue, 0);
    CHECK_EQ(p.grid_dim, 8192 * 4);
    FrameInputs nq = frame();
    nq.knobs.no_tile_queue = true;
    CHECK_EQ(frame_plan(nq, 10).tile_queue, 0);
    CHECK_EQ(frame_plan(nq, 10).grid_dim, 8192);
    // light split: needs light_ok, off with STATS or chunks
    FrameInputs lt = frame();
    lt.light_ok = true;
    CHECK_EQ(frame_plan(lt, 10).split_light, 1);
    CHECK_EQ(frame_plan(lt, 10).scratch.light.bytes, 32400);
    lt.stats = true;
    CHECK_EQ(frame_plan(lt, 10).split_light, 0);
    lt.stats = false;
    lt.grid.flags = CGRT_GRID_SPLIT_SAMPLES;
    CHECK_EQ(frame_plan(lt, 10).split_light, 0);
    // primary walk: off with CGRT_GRID_STATS or CGRT_NO_PRIMWALK; it finishes units when the scene lets it and the knob does not
    FrameInputs pw = frame();
    pw.prim_obj = 3;
    pw.prim_finish = true;
    p = frame_plan(pw, 10);
    CHECK_EQ(p.use_prim, 1);
    CHECK_EQ(p.prim_done, 1);
    GridParams g = frame_params(pw, p);
    CHECK_EQ(g.prim_obj, 3);
    CHECK_EQ(g.prim_done, 1);
    CHECK_EQ(g.heavy_blocks, 40);
    CHECK_EQ(g.items_per_tile, 16);
    CHECK_EQ(g.xcd_tiles, 1);
    CHECK_EQ(g.maxhp, 16);
    CHECK_EQ(g.partial == nullptr && g.plan == nullptr, 1);
    pw.knobs.pw_no_finish = true;
    CHECK_EQ(frame_plan(pw, 10).prim_done, 0);
    pw.knobs.pw_no_finish = false;
    pw.prim_finish = false;
    CHECK_EQ(frame_plan(pw, 10).prim_done, 0);
    pw.knobs.no_primwalk = true;
    CHECK_EQ(frame_plan(pw, 10).use_prim, 0);
    pw.knobs.no_primwalk = false;
    pw.grid.flags = CGRT_GRID_STATS;
    CHECK_EQ(frame_plan(pw, 10).use_prim, 0);
    // nothing heavy: image order, the GridParams defaults
    p = frame_plan(lt, 0);
    CHECK_EQ(p.heavy_blocks + p.split_light + p.tile_queue + p.wave_slots, 0);
    g = frame_params(pw, frame_plan(pw, 0));
    CHECK_EQ(g.prim_obj, -1);
    CHECK_EQ(g.items_per_tile, 1);
}

// 200 x 117 at 32 spp, depth 5: the image-order launch of a glass sphere scene -- ten spheres and nothing else, all in LDS, two of
// them special, some tile clear of both -- by the PAIR variant, on a handle with its second stream.  7 x 15 = 105 tiles.
static FrameInputs spheres(int W = 200, int rows = 117, int spp = 32) {
    FrameInputs in = frame(W, rows, spp);
    in.sched = false;
    in.has_mesh = false;
    in.image = in.sph = in.pair = in.order_ok = in.aux_stream = in.all_spheres = true;
    in.n_objs = in.n_lds = 10;
    return in;
}
#define CHECK_ORDER(in_, on_, class3_, masks_, relay_k_)          \
    do {                                                          \
        const FramePlan q_ = frame_plan(in_, 0);                  \
        CHECK_EQ(q_.order.on, on_);                               \
        CHECK_EQ(q_.order.class3, TileOrderPlan::class3_);        \
        CHECK_EQ(q_.order.masks, masks_);                         \
        CHECK_EQ(q_.relay.base.k, relay_k_);                           \
    } while (0)

static void tile_order() {
    FrameInputs in = spheres();
    CHECK_EQ(frame_plan(in, 0).tile_blocks, 105);
    // the pair variant: class 3 inside the kernel, with masks; 105 tiles are fewer than 4 x 256, so the relay only on request
    CHECK_ORDER(in, 1, InKernel, 1, 1);
    in.grid.flags = CGRT_GRID_SAMPLE_RELAY;
    CHECK_ORDER(in, 1, InKernel, 1, 2);
    CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayGlass);
    CHECK_EQ(frame_plan(in, 0).relay.order, kRelayChunksFirst);
    {   // 1920 x 1080: 8100 tiles take every workgroup slot of 256 CUs: relayed by default, in the measured form
        const FramePlan p = frame_plan(spheres(1920, 1080), 0);
        CHECK_EQ(p.tile_blocks, 8100);
        CHECK_EQ(p.order.on, 1);
        CHECK_EQ(p.order.class3, TileOrderPlan::InKernel);
        CHECK_EQ(p.order.masks, 1);
        CHECK_EQ(p.relay.base.k, 2);
        CHECK_EQ(p.relay.base.chunk_spp, 16);
        CHECK_EQ(p.relay.extent, kRelayMirror);
        CHECK_EQ(p.relay.order, kRelayInterleaved);
    }
    // the second launch for class 3, on request: one launch each for the two parts of the list, so nothing is relayed
    in.grid.flags = CGRT_GRID_DIFFUSE_TILES | CGRT_GRID_SAMPLE_RELAY;
    CHECK_ORDER(in, 1, SecondLaunch, 1, 1);
    {
        FrameInputs big = spheres(1920, 1080);
        big.grid.flags = CGRT_GRID_DIFFUSE_TILES;
        CHECK_ORDER(big, 1, SecondLaunch, 1, 1);
    }
    // ... which needs the second stream, and is not taken for a timeline (one launch): the pair variant's own body then
    in.grid.flags = CGRT_GRID_DIFFUSE_TILES;
    in.aux_stream = false;
    CHECK_ORDER(in, 1, InKernel, 1, 1);
    in.aux_stream = true;
    in.knobs.timeline_file = "tl.bin";
    CHECK_ORDER(in, 1, InKernel, 1, 1);
    in.knobs.timeline_file = nullptr;
    CHECK_ORDER(in, 1, SecondLaunch, 1, 1);
    // ... nor by a STATS or a SPILL kernel
    in.stats = true;
    CHECK_ORDER(in, 1, InKernel, 1, 1);
    in.stats = false;
    in.spill = true;
    CHECK_ORDER(in, 1, InKernel, 1, 1);
    in.spill = false;
    // no tile order on request: row-major, nothing for class 3, no masks, no relay -- whatever kernel eye_launch chose
    for (const int32_t f : {0, (int32_t)CGRT_GRID_DIFFUSE_TILES, (int32_t)CGRT_GRID_SAMPLE_RELAY}) {
        in.grid.flags = CGRT_GRID_NO_TILE_ORDER | f;
        CHECK_EQ(in.pair, 1);
        CHECK_ORDER(in, 0, None, 0, 1);
    }
    // split samples: two chunks of 16, which the tile order does not serve
    in.grid.flags = CGRT_GRID_SPLIT_SAMPLES;
    CHECK_EQ(frame_plan(in, 0).chunks, 2);
    CHECK_ORDER(in, 0, None, 0, 1);
    in.grid.flags = CGRT_GRID_SPLIT_SAMPLES | CGRT_GRID_DIFFUSE_TILES | CGRT_GRID_SAMPLE_RELAY;
    CHECK_ORDER(in, 0, None, 0, 1);
    // asked for with fewer than 32 samples: one chunk in tile order, but neither the second launch nor (at any sample count) the relay
    in.grid.spp = 31;
    CHECK_EQ(frame_plan(in, 0).chunks, 1);
    CHECK_ORDER(in, 1, InKernel, 1, 1);
    // a mirror-only sphere scene (no PAIR variant): class 3 by the second launch or like every other tile, then without masks
    FrameInputs mi = spheres();
    mi.glass = mi.pair = false;
    CHECK_ORDER(mi, 1, None, 0, 1);
    mi.grid.flags = CGRT_GRID_SAMPLE_RELAY;  // the relay is the PAIR variant's
    CHECK_ORDER(mi, 1, None, 0, 1);
    mi.grid.flags = CGRT_GRID_DIFFUSE_TILES;
    CHECK_ORDER(mi, 1, SecondLaunch, 1, 1);
    // no tile can be of class 3: no diffuse body in any form, no masks; the relay stays
    for (FrameInputs a : {spheres(), mi}) {
        a.all_special = true;
        for (const int32_t f : {0, (int32_t)CGRT_GRID_DIFFUSE_TILES}) {
            a.grid.flags = f;
            CHECK_ORDER(a, 1, None, 0, 1);
        }
    }
    in = spheres();
    in.all_special = true;
    in.grid.flags = CGRT_GRID_SAMPLE_RELAY;
    CHECK_ORDER(in, 1, None, 0, 2);
    // masks: at most 32 objects, all of them spheres, all of them in LDS, and not switched off
    in = spheres();
    in.n_objs = in.n_lds = 32;
    CHECK_ORDER(in, 1, InKernel, 1, 1);
    in.n_objs = in.n_lds = 33;
    CHECK_ORDER(in, 1, InKernel, 0, 1);
    in.n_objs = 32;
    in.n_lds = 31;
    CHECK_ORDER(in, 1, InKernel, 0, 1);
    in.n_lds = 32;
    in.all_spheres = false;
    CHECK_ORDER(in, 1, InKernel, 0, 1);
    in.all_spheres = true;
    in.grid.flags = CGRT_GRID_NO_SPHERE_MASKS;
    CHECK_ORDER(in, 1, InKernel, 0, 1);
    in.grid.flags = CGRT_GRID_NO_SPHERE_MASKS | CGRT_GRID_DIFFUSE_TILES;
    CHECK_ORDER(in, 1, SecondLaunch, 0, 1);
    // the tile order is for 256-thread workgroups of an image-order launch over row-major tiles of a scene it can order
    in = spheres();
    in.grid.flags = CGRT_GRID_DIFFUSE_TILES | CGRT_GRID_SAMPLE_RELAY;
    FrameInputs off = in;
    off.nt = 64;
    CHECK_ORDER(off, 0, None, 0, 1);
    off = in;
    off.order_ok = false;
    CHECK_ORDER(off, 0, None, 0, 1);
    off = in;
    off.image = false;
    CHECK_ORDER(off, 0, None, 0, 1);
    off = in;
    off.has_mesh = true;  // XCD super-tiles
    CHECK_EQ(frame_plan(off, 0).xcd_tiles, 1);
    CHECK_ORDER(off, 0, None, 0, 1);
}

// plan[8] and the list share the first part; every part starts on 256 bytes
static void order_layout() {
    const struct {
        size_t n, n_wt, tile_cls, wave_cls, wmask, total;
    } cases[] = {
        {1, 1, 256, 512, 768, 1024},      // 36, 1, 1 and 4 bytes: a 256 each
        {28, 60, 256, 512, 768, 1024},    // 144, 28, 60 and 240 bytes
        // 32 672 -> 128 x 256; 8 160 -> 32 x 256; 32 640 -> 128 x 256; 130 560 = 510 x 256
        {8160, 32640, 32768, 32768 + 8192, 32768 + 8192 + 32768, 204288},
    };
    for (const auto &c : cases) {
        const TileOrderLayout L = tile_order_layout(c.n, c.n_wt);
        CHECK_EQ(L.plan.at, 0);
        CHECK_EQ(L.plan.bytes, 32);
        CHECK_EQ(L.list.at, 32);
        CHECK_EQ(L.list.bytes, 4 * c.n);
        CHECK_EQ(L.tile_cls.at, c.tile_cls);
        CHECK_EQ(L.tile_cls.bytes, c.n);
        CHECK_EQ(L.wave_cls.at, c.wave_cls);
        CHECK_EQ(L.wave_cls.bytes, c.n_wt);
        CHECK_EQ(L.wmask.at, c.wmask);
        CHECK_EQ(L.wmask.bytes, 4 * c.n_wt);
        CHECK_EQ(L.wmask.at % 4, 0);
        CHECK_EQ(L.total, c.total);
    }
}

static void fitting() {
    const FrameInputs in = frame();
    const size_t need = frame_plan(in, 8152).scratch.total;
    CHECK_EQ(fit_heavy_tiles(in, 8152, 0), 8152);         // nothing refused yet
    CHECK_EQ(fit_heavy_tiles(in, 8152, need + 1), 8152);  // below the refused size
    CHECK_EQ(fit_heavy_tiles(in, 8152, need), 4076);      // at it: halved once
    CHECK_EQ(fit_heavy_tiles(in, 8152, frame_plan(in, 2038).scratch.total + 1), 2038);
    CHECK_EQ(fit_heavy_tiles(in, 8152, 1), 0);  // down to no heavy tile at all
}

static void knobs() {
    setenv("CGRT_HEAVY_DIV", "0", 1);  // not positive: the default
    setenv("CGRT_UNITS_PER_ITEM", "100", 1);
    setenv("CGRT_NO_PRIMWALK", "0", 1);
    setenv("CGRT_NO_TILE_QUEUE", "1", 1);
    setenv("CGRT_DEFER_BYTES", "12345", 1);
    setenv("CGRT_TIMELINE_FILE", "tl.bin", 1);
    EyeKnobs k = eye_knobs();
    CHECK_EQ(k.heavy_div, 32);
    CHECK_EQ(k.units_per_item, 128);  // whole waves
    CHECK_EQ(k.no_primwalk, 0);
    CHECK_EQ(k.no_tile_queue, 1);
    CHECK_EQ(k.defer_bytes, 12345);
    CHECK_EQ(k.pw_refill, 16);
    CHECK_EQ(k.timeline_file != nullptr, 1);
    // read once per process, except the timeline file
    setenv("CGRT_HEAVY_DIV", "5", 1);
    unsetenv("CGRT_TIMELINE_FILE");
    k = eye_knobs();
    CHECK_EQ(k.heavy_div, 32);
    CHECK_EQ(k.timeline_file == nullptr, 1);
    const EyeKnobs d;
    CHECK_EQ(d.units_per_item, 256);
    CHECK_EQ(d.pw_rounds, 8);
}

int main() {
    chunking();
    tile_counts();
    capacity();
    scratch_layout();
    scheduled();
    fitting();
    tile_order();
    order_layout();
    knobs();
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed != 0;
}
