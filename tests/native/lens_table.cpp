// The lens table of classes 0-2 (cgrt_lens_stage.h): where table[entry][sample][thread] lies and how many entries a budget holds;
// a CPU model of lens_table_kernel's per-thread routine -- lens_table_first over a batch, then lens_table_retry while any lane of
// the wave has a reject left -- against the per-sample rejection loop written on cgrt_rng.hpp's Stream, which is what lens_disc
// computes; and the frame plan's conditions, with and without CGRT_GRID_NO_LENS_TABLE.  CPU build with -ffp-contract=off,
// stand-alone under ASan + UBSan, driven by tests/test_lens_table_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cgrt_frame.h"

static int g_failed = 0;
static long long g_checks = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        g_checks++;                                                  \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_failed++;                                              \
        }                                                            \
    } while (0)
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        g_checks++;                                                                                             \
        if (a_ != b_) {                                                                                         \
            std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)

static constexpr int kLanes = 64, kThreadsWg = 256;

// ---- the table's layout and the capacity rule ----
static void layout() {
    const int spps[] = {1, 17, 64};
    for (const int spp : spps) {
        const size_t entry_bytes = lens_table_entry_bytes(spp, kThreadsWg);
        CHECK_EQ(entry_bytes, (size_t)spp * 2048);
        // budgets: nothing, not one entry, one entry, an exact fit of five, five and a bit, the default
        const size_t budgets[] = {0, entry_bytes - 1, entry_bytes, 5 * entry_bytes, 5 * entry_bytes + 7, kLensTableBudget};
        for (const size_t budget : budgets) {
            const size_t tiles[] = {1, 3, 5, 21, 8100};
            for (const size_t n : tiles) {
                const size_t cap = lens_table_cap(n, spp, kThreadsWg, budget), total = lens_table_bytes(cap, spp, kThreadsWg);
                CHECK_EQ(cap, std::min(n, budget / entry_bytes));
                CHECK(cap <= n && total <= budget);
                CHECK_EQ(total, cap * entry_bytes);
                if (cap == 0 || cap > 5) continue;
                // every (entry, sample, thread) has its own 8 bytes inside the table, and they fill it
                std::vector<unsigned char> seen(total / 8, 0);
                for (size_t e = 0; e < cap; e++)
                    for (int s = 0; s < spp; s++)
                        for (int t = 0; t < kThreadsWg; t++) {
                            const size_t at = lens_table_at(e, s, t, spp, kThreadsWg);
                            CHECK(at % 8 == 0 && at + 8 <= total);
                            if (at + 8 <= total) seen[at / 8]++;
                        }
                for (const unsigned char c : seen) CHECK_EQ(c, 1);
            }
        }
    }
    CHECK_EQ(lens_table_cap(8100, 64, kThreadsWg, 0), 0);
    CHECK_EQ(lens_table_cap(8100, 64, kThreadsWg, 64 * 2048 - 1), 0);  // too small for one entry
    CHECK_EQ(lens_table_cap(8100, 64, kThreadsWg, 64 * 2048), 1);
    CHECK_EQ(lens_table_cap(8100, 64, kThreadsWg, kLensTableBudget), 2048);
    CHECK_EQ(lens_table_at(0, 0, 1, 64, kThreadsWg) - lens_table_at(0, 0, 0, 64, kThreadsWg), 8);         // a workgroup's threads contiguous
    CHECK_EQ(lens_table_at(0, 1, 0, 64, kThreadsWg) - lens_table_at(0, 0, 0, 64, kThreadsWg), 256 * 8);  // then the samples
    CHECK_EQ(lens_table_bytes(1247, 64, kThreadsWg), (size_t)1247 * 64 * 2048);                          // C2: 163 MB
    CHECK(lens_table_bytes(1247, 64, kThreadsWg) <= kLensTableBudget);
    CHECK(kLensTableBatch <= 32);
}

// ---- the draws ----
// The reference: uniform_sampling_circle on the sample's lens stream, one rejection loop per sample (lens_disc's result, through
// the Stream's own counter arithmetic); returns the accepted draw's point
static void lens_reference(uint64_t k_smp, double &sx, double &sy) {
    cgrt::Stream st(k_smp);
    while (true) {
        double ux, uy;
        st.pair(ux, uy);
        sx = ux * 2.0 - 1;
        sy = uy * 2.0 - 1;
        if (sx * sx + sy * sy < 1) return;
    }
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// One wave of lens_table_kernel over `spp` samples of entry `entry`: lanes with key k_pix[l], live[l].  The table is allocated
// exactly (ASan guards its ends) and prefilled, so that a slot nobody wrote shows.
static long long g_draws = 0;
static void run_wave(const uint64_t *k_pix, const bool *live, int spp, int sample_offset, size_t entry, size_t cap, int wave) {
    const uint64_t fill = 0xdeadbeefdeadbeefull;
    std::vector<uint64_t> table(lens_table_bytes(cap, spp, kThreadsWg) / 8, fill);
    for (int first = 0; first < spp; first += kLensTableBatch) {
        const int count = std::min(kLensTableBatch, spp - first);
        uint32_t rejected[kLanes];
        uint64_t *row[kLanes];
        for (int l = 0; l < kLanes; l++) {
            row[l] = table.data() + lens_table_at(entry, first, wave * kLanes + l, spp, kThreadsWg) / 8;
            rejected[l] = lens_table_first(k_pix[l], (uint64_t)(sample_offset + first), count, live[l], row[l], kThreadsWg);
            if (!live[l]) CHECK_EQ(rejected[l], 0);
        }
        while (true) {  // the kernel's ballot loop
            bool left = false;
            for (int l = 0; l < kLanes; l++) left = left || rejected[l] != 0u;
            if (!left) break;
            for (int l = 0; l < kLanes; l++)
                if (rejected[l] != 0u) rejected[l] = lens_table_retry(rejected[l], row[l], kThreadsWg);
        }
    }
    for (int s = 0; s < spp; s++)
        for (int l = 0; l < kLanes; l++) {
            const uint64_t z = table[lens_table_at(entry, s, wave * kLanes + l, spp, kThreadsWg) / 8];
            if (!live[l]) {
                CHECK_EQ(z, 0);  // a lane with no live pixel writes 0
                continue;
            }
            double sx, sy, rx, ry;
            lens_point(z, sx, sy);
            lens_reference(cgrt::sample_key(k_pix[l], (uint64_t)(sample_offset + s)), rx, ry);
            CHECK(same_bits(sx, rx) && same_bits(sy, ry));
            CHECK(lens_accepts(z));
            g_draws++;
        }
    // nothing outside the wave's own slots was written
    size_t written = 0;
    for (const uint64_t v : table) written += v != fill ? 1 : 0;
    CHECK(written <= (size_t)spp * kLanes);
}
static void draws() {
    // a few hundred pixel keys: 5 waves of 64 at each (samples, offset), every fifth lane of the odd waves without a pixel
    const int spps[] = {1, 31, 32, 33, 64};
    const int offsets[] = {0, 3};
    int wave_no = 0;
    for (const int spp : spps)
        for (const int off : offsets)
            for (int v = 0; v < 5; v++, wave_no++) {
                uint64_t k_pix[kLanes];
                bool live[kLanes];
                for (int l = 0; l < kLanes; l++) {
                    k_pix[l] = cgrt::pixel_key(12345 + (uint64_t)(wave_no / 7), (uint64_t)wave_no * 977 + (uint64_t)l);
                    live[l] = !((wave_no & 1) && l % 5 == 4);
                }
                if (v == 4)
                    for (int l = 0; l < kLanes; l++) live[l] = false;  // a wave tile outside the image
                run_wave(k_pix, live, spp, off, (size_t)(wave_no % 3), 3, wave_no % 4);
            }
}

// ---- the frame plan ----
// C2's launch: 1920 x 1080, 64 samples, the PAIR variant in image order, 15 spheres, thin lens
static FrameInputs c2_frame() {
    FrameInputs in{};
    in.grid.width = 1920;
    in.grid.height = in.grid.rows = 1080;
    in.grid.stripe_nranks = 1;
    in.grid.spp = in.grid.spp_total = 64;
    in.grid.max_depth = 5;
    in.cam.cam[2] = -10;
    in.cam.half_width = 10;
    in.cam.focus_plane = 20;
    in.cam.lens_radius = 0.5;
    in.glass = true;
    in.nt = 256;
    in.prim_obj = -1;
    in.mem_total = 288000000000ull;
    in.n_cu = 256;
    in.waves_per_simd = 4;
    in.image = in.sph = in.pair = in.order_ok = in.aux_stream = in.all_spheres = true;
    in.n_objs = in.n_lds = 15;
    return in;
}
static void plan() {
    const FrameInputs c2 = c2_frame();
    const auto cap_of = [](const FrameInputs &in) {
        const FramePlan p = frame_plan(in, 0);
        const GridParams g = frame_params(in, p);
        CHECK_EQ(g.lens_table_cap, p.order.lens_table_cap);
        CHECK_EQ(g.lens_table_spp, p.order.lens_table_cap ? in.grid.spp : 0);
        CHECK(g.lens_table == nullptr);  // (the launch places it)
        CHECK_EQ(p.order.lens_table_bytes, p.order.lens_table_cap * (size_t)in.grid.spp * 2048);
        return (long long)p.order.lens_table_cap;
    };
    CHECK_EQ(cap_of(c2), 2048);  // 256 MiB / (64 samples x 2 KiB); C2's 1 247 entries of classes 0-2 take 163 MB of it
    // with and without the flag: the launch itself is what it was, only the table's fields differ
    FrameInputs in = c2;
    in.grid.flags = CGRT_GRID_NO_LENS_TABLE;
    CHECK_EQ(cap_of(in), 0);
    {
        const FramePlan a = frame_plan(c2, 0), b = frame_plan(in, 0);
        CHECK_EQ(a.grid_dim, b.grid_dim);
        CHECK_EQ(a.tile_blocks, b.tile_blocks);
        CHECK_EQ(a.scratch.total, b.scratch.total);
        CHECK_EQ(a.order.on, b.order.on);
        CHECK_EQ((int)a.order.class3, (int)b.order.class3);
        CHECK_EQ(a.order.masks, b.order.masks);
        CHECK_EQ(a.order.sure, b.order.sure);
        CHECK_EQ(a.order.lens_stage, b.order.lens_stage);
        CHECK_EQ(a.order.lens_stage, kLensStageLds);
        const RelayPlan &ra = a.relay, &rb = b.relay;
        CHECK_EQ(ra.base.k, rb.base.k);
        CHECK_EQ(ra.base.chunk_spp, rb.base.chunk_spp);
        CHECK_EQ(ra.base.slots, rb.base.slots);
        CHECK_EQ(ra.base.cap, rb.base.cap);
        CHECK_EQ(ra.base.bytes, rb.base.bytes);
        CHECK_EQ(ra.boost.k, rb.boost.k);
        CHECK_EQ(ra.boost.cap, rb.boost.cap);
        CHECK_EQ(ra.boost.bytes, rb.boost.bytes);
        CHECK_EQ(ra.extent, rb.extent);
        CHECK_EQ(ra.order, rb.order);
        CHECK_EQ(ra.start, rb.start);
        CHECK_EQ(ra.start_words, rb.start_words);
        CHECK_EQ(ra.boost_words, rb.boost_words);
        CHECK_EQ(ra.bytes(), rb.bytes());
        CHECK(ra.relays() && ra.boosts());
        GridParams ga = frame_params(c2, a), gb = frame_params(in, b);
        CHECK_EQ(ga.lens_table_cap, 2048);
        CHECK_EQ(ga.lens_table_spp, 64);
        CHECK_EQ(ga.lens_batch, gb.lens_batch);
        ga.lens_table_cap = gb.lens_table_cap;  // with the new fields equal, the parameters are the same bytes
        ga.lens_table_spp = gb.lens_table_spp;
        CHECK(std::memcmp(&ga, &gb, sizeof(GridParams)) == 0);
    }
    // the LDS stage's flag does not touch the table, the table's flag does not touch the LDS stage
    in = c2;
    in.grid.flags = CGRT_GRID_NO_LENS_STAGE;
    CHECK_EQ(cap_of(in), 2048);
    CHECK_EQ(frame_plan(in, 0).order.lens_stage, kLensStageOff);
    // where there is no table: a pinhole, the second launch, no pairs, no tile order, split samples, a scheduled launch
    in = c2;
    in.cam.lens_radius = 0;
    CHECK_EQ(cap_of(in), 0);
    in = c2;
    in.grid.flags = CGRT_GRID_DIFFUSE_TILES;
    CHECK_EQ(cap_of(in), 0);
    in = c2;
    in.grid.flags = CGRT_GRID_NO_SPHERE_PAIRS;
    in.pair = false;
    CHECK_EQ(cap_of(in), 0);
    in = c2;
    in.grid.flags = CGRT_GRID_NO_TILE_ORDER;
    CHECK_EQ(cap_of(in), 0);
    in = c2;
    in.grid.flags = CGRT_GRID_SPLIT_SAMPLES;
    CHECK_EQ(cap_of(in), 0);
    in = c2;
    in.image = false;
    in.sched = true;
    CHECK_EQ(cap_of(in), 0);
    // it depends neither on the relay nor on class 3
    in = c2;
    in.grid.flags = CGRT_GRID_NO_SAMPLE_RELAY;
    CHECK_EQ(cap_of(in), 2048);
    in = c2;
    in.all_special = true;
    CHECK_EQ(cap_of(in), 2048);
    in = c2;
    in.grid.width = 96;
    in.grid.height = in.grid.rows = 54;  // 21 tiles: no larger than the list
    CHECK_EQ(cap_of(in), 21);
    in.grid.spp = in.grid.spp_total = 1;
    CHECK_EQ(cap_of(in), 21);
    // the knobs: off / on, and the budget
    in = c2;
    in.knobs.lens_table = 0;
    CHECK_EQ(cap_of(in), 0);
    in.knobs.lens_table = 1;
    CHECK_EQ(cap_of(in), 2048);
    in.grid.flags = CGRT_GRID_NO_LENS_TABLE;  // off wins
    CHECK_EQ(cap_of(in), 0);
    // who writes the table: unset, only a launch beside its cost probe; the knob on or CGRT_GRID_LENS_TABLE, every launch
    CHECK(!frame_plan(c2, 0).order.lens_table_always);
    CHECK(frame_plan(in, 0).order.lens_table_cap == 0 && !frame_plan(in, 0).order.lens_table_always);
    in.grid.flags = 0;
    CHECK(frame_plan(in, 0).order.lens_table_always);  // (the knob is on)
    in.knobs.lens_table = 0;
    in.grid.flags = CGRT_GRID_LENS_TABLE;  // the launch's flag over the knob
    CHECK_EQ(cap_of(in), 2048);
    CHECK(frame_plan(in, 0).order.lens_table_always);
    in.grid.flags = CGRT_GRID_LENS_TABLE | CGRT_GRID_NO_LENS_TABLE;
    CHECK_EQ(cap_of(in), 0);
    in = c2;
    in.grid.flags = CGRT_GRID_LENS_TABLE;  // the flag changes nothing else of the plan
    CHECK_EQ(cap_of(in), 2048);
    CHECK_EQ(frame_plan(in, 0).grid_dim, frame_plan(c2, 0).grid_dim);
    CHECK_EQ(frame_plan(in, 0).scratch.total, frame_plan(c2, 0).scratch.total);
    CHECK_EQ(CGRT_GRID_LENS_TABLE, 16777216);
    in = c2;
    in.knobs.lens_table_bytes_set = true;
    in.knobs.lens_table_bytes = 2 * 64 * 2048 + 100;  // two entries and a bit
    CHECK_EQ(cap_of(in), 2);
    in.knobs.lens_table_bytes = 64 * 2048 - 1;  // not one entry
    CHECK_EQ(cap_of(in), 0);
    in.knobs.lens_table_bytes = 0;
    CHECK_EQ(cap_of(in), 0);
    CHECK_EQ(lens_table_named("off"), 0);
    CHECK_EQ(lens_table_named("on"), 1);
    CHECK_EQ(lens_table_named(""), -1);
    CHECK_EQ(lens_table_named("area"), -1);
    CHECK_EQ(EyeKnobs{}.lens_table, -1);
    // what the existing tests pin
    CHECK_EQ(lens_stage_named("area"), -1);
    CHECK_EQ(CGRT_GRID_NO_LENS_TABLE, 8388608);
}

int main() {
    layout();
    draws();
    plan();
    std::printf("draws compared: %lld\n", g_draws);
    std::printf("ok: %d failed checks of %lld\n", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
