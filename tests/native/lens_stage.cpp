// Lens points staged ahead of the sample loop (cgrt_lens_stage.h): waves of 64 lanes run the header's stager the way the
// terminal-diffuse body does (trace_grid_body, cgrt_eye.hpp: phase A over the batch, phase B while any lane has a reject
// left, the sample loop rebuilding the point from its slot), and every point is compared with the per-sample rejection loop
// written on cgrt_rng.hpp's Stream -- what lens_disc computes.  Also: the rounds a wave needs per sample, staged and today;
// the LDS slots' layout; the frame plan's conditions.  CPU build with -ffp-contract=off, stand-alone under ASan + UBSan,
// driven by tests/test_lens_stage_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cgrt_frame.h"
#include "cgrt_wg_lds.h"

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

// The reference: uniform_sampling_circle on the sample's lens stream, one rejection loop per sample (lens_disc's result, through
// the Stream's own counter arithmetic); returns the attempts it took
static int lens_reference(uint64_t k_smp, double &sx, double &sy) {
    cgrt::Stream st(k_smp);
    for (int attempts = 1;; attempts++) {
        double ux, uy;
        st.pair(ux, uy);
        sx = ux * 2.0 - 1;
        sy = uy * 2.0 - 1;
        if (sx * sx + sy * sy < 1) return attempts;
    }
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// One wave of the staged body: lanes with key k_pix[l], live[l], all at the launch's samples [s0, s_end) + sample_offset, in
// batches of `batch`.  The workgroup's slot region is allocated exactly (ASan guards its ends); the wave is wave `wave` of it.
struct WaveRun {
    long long samples = 0, rounds_a = 0, rounds_b = 0;  // wave-level: samples started, phase A and phase B trips
    long long draws = 0, deep = 0;                      // lane-level: points compared, points that took >= 6 attempts
};
static WaveRun run_wave(const uint64_t *k_pix, const bool *live, int s0, int s_end, int sample_offset, int batch, int wave) {
    WaveRun r;
    std::vector<uint64_t> lds((size_t)batch * kThreadsWg, 0xdeadbeefdeadbeefull);  // batch slots a thread
    const auto slot = [&](int b, int lane) -> uint64_t & {
        const size_t at = lens_slot_at(b, wave * kLanes + lane, kThreadsWg);
        return lds.at(at / sizeof(uint64_t));
    };
    int batch_first = 0, batch_end = 0;
    for (int s = s0; s < s_end; s++) {
        bool any = false;
        for (int l = 0; l < kLanes; l++) any = any || live[l];
        if (!any) break;  // (no lane starts a sample: the body never stages)
        if (s >= batch_end) {
            const int first = s, count = std::min(batch, s_end - first);
            uint32_t rejected[kLanes];
            for (int l = 0; l < kLanes; l++) {  // phase A
                rejected[l] = 0u;
                for (int b = 0; b < count; b++) {
                    const LensSlot a = lens_stage_first(k_pix[l], (uint64_t)(sample_offset + first + b));
                    slot(b, l) = a.v;
                    rejected[l] |= a.done ? 0u : (1u << b);
                }
                if (!live[l]) rejected[l] = 0u;
            }
            r.rounds_a += count;
            while (true) {  // phase B
                bool left = false;
                for (int l = 0; l < kLanes; l++) left = left || rejected[l] != 0u;
                if (!left) break;
                r.rounds_b++;
                for (int l = 0; l < kLanes; l++) {
                    if (rejected[l] == 0u) continue;
                    const int b = __builtin_ctz(rejected[l]);
                    const LensSlot a = lens_stage_retry(slot(b, l));
                    slot(b, l) = a.v;
                    if (a.done) rejected[l] &= rejected[l] - 1u;
                }
            }
            batch_first = first;
            batch_end = first + count;
        }
        r.samples++;
        for (int l = 0; l < kLanes; l++) {
            if (!live[l]) continue;
            double sx, sy, rx, ry;
            lens_point(slot(s - batch_first, l), sx, sy);
            const int attempts = lens_reference(cgrt::sample_key(k_pix[l], (uint64_t)(sample_offset + s)), rx, ry);
            CHECK(same_bits(sx, rx) && same_bits(sy, ry));
            CHECK(sx * sx + sy * sy < 1);
            r.draws++;
            if (attempts >= 6) r.deep++;
        }
    }
    return r;
}

// today's loop: the wave's rounds for one sample = the attempts of its unluckiest lane
static int rounds_today(const uint64_t *k_pix, int s) {
    int worst = 0;
    for (int l = 0; l < kLanes; l++) {
        double sx, sy;
        worst = std::max(worst, lens_reference(cgrt::sample_key(k_pix[l], (uint64_t)s), sx, sy));
    }
    return worst;
}

static void fill_wave(uint64_t seed, uint64_t first_pixel, uint64_t *k_pix) {
    for (int l = 0; l < kLanes; l++) k_pix[l] = cgrt::pixel_key(seed, first_pixel + (uint64_t)l);
}

static void draws() {
    const int counts[] = {0, 1, 15, 16, 17, 32, 64};
    const int offsets[] = {0, 3, 1000};
    long long total = 0, deep = 0;
    uint64_t k_pix[kLanes];
    bool live[kLanes];
    for (int wv = 0; wv < 48; wv++) {
        fill_wave(12345 + (uint64_t)(wv % 3), (uint64_t)wv * 4099, k_pix);
        // all lanes live; the right-hand columns dead (a partial tile); the lower rows dead; only lane 63 live; none live
        for (int l = 0; l < kLanes; l++) {
            const int form = wv % 5;
            live[l] = form == 0 || (form == 1 && (l & 15) < 9) || (form == 2 && (l >> 4) < 2) || (form == 3 && l == 63);
        }
        for (const int count : counts)
            for (const int batch : {16, 32}) {
                const int first = (wv * 7 + count) % 5 == 0 ? 16 : (wv % 4 == 1 ? 5 : 0);  // a relayed chunk starts behind sample 0
                const WaveRun r = run_wave(k_pix, live, first, first + count, offsets[wv % 3], batch, wv % 4);
                bool any = false;
                for (int l = 0; l < kLanes; l++) any = any || live[l];
                CHECK_EQ(r.samples, any ? count : 0);
                CHECK_EQ(r.rounds_a, any ? count : 0);
                total += r.draws;
                deep += r.deep;
            }
    }
    // streams that need at least 6 attempts, searched for and placed in one wave, one of them in every lane's batch
    int found = 0;
    std::vector<uint64_t> deep_keys;
    for (uint64_t px = 0; found < kLanes && px < 2000000; px++) {
        const uint64_t k = cgrt::pixel_key(99, px);
        double sx, sy;
        for (int s = 0; s < 16; s++)
            if (lens_reference(cgrt::sample_key(k, (uint64_t)s), sx, sy) >= 6) {
                deep_keys.push_back(k);
                found++;
                break;
            }
    }
    CHECK_EQ(found, kLanes);
    if (found == kLanes) {
        for (int l = 0; l < kLanes; l++) live[l] = true;
        const WaveRun r = run_wave(deep_keys.data(), live, 0, 16, 0, 16, 2);
        CHECK(r.deep >= kLanes);
        CHECK(r.rounds_b >= 5);
        total += r.draws;
        deep += r.deep;
    }
    CHECK(total >= 100000);
    CHECK(deep >= kLanes);
    std::printf("draws compared: %lld, of them with >= 6 attempts: %lld\n", total, deep);
}

static void rounds() {
    uint64_t k_pix[kLanes];
    bool live[kLanes];
    for (int l = 0; l < kLanes; l++) live[l] = true;
    const int waves = 1000, spp = 64;
    long long r16 = 0, r32 = 0, today = 0;
    for (int wv = 0; wv < waves; wv++) {
        fill_wave(2024, (uint64_t)wv * kLanes, k_pix);
        const WaveRun a = run_wave(k_pix, live, 0, spp, 0, 16, 0), b = run_wave(k_pix, live, 0, spp, 0, 32, 0);
        r16 += a.rounds_a + a.rounds_b;
        r32 += b.rounds_a + b.rounds_b;
        for (int s = 0; s < 8; s++) today += rounds_today(k_pix, s);  // (8 samples a wave: 8000 wave samples)
    }
    const double m16 = (double)r16 / (waves * spp), m32 = (double)r32 / (waves * spp), mt = (double)today / (waves * 8);
    std::printf("rounds per sample: %.3f at batches of 16, %.3f at 32, today %.3f\n", m16, m32, mt);
    CHECK(m16 <= 1.8);
    CHECK(m32 <= 1.65);
    CHECK(m16 > 1.0 && m32 > 1.0 && m32 < m16);
    CHECK(mt > 3.0);
}

static void slots() {
    // every (slot, thread) has its own 8 bytes inside the region; the region fits the PAIR launch's pending-ray levels
    const size_t bytes = lens_batch_lds(kThreadsWg);
    CHECK_EQ(bytes, 32768);
    CHECK(bytes <= (size_t)kLdsLevels * pending_level_bytes(kThreadsWg));
    CHECK_EQ((size_t)kLdsLevels * pending_level_bytes(kThreadsWg), 38912);
    std::vector<int> seen(bytes / 8, 0);
    for (int b = 0; b < kLensBatch; b++)
        for (int t = 0; t < kThreadsWg; t++) {
            const size_t at = lens_slot_at(b, t, kThreadsWg);
            CHECK(at % 8 == 0 && at + 8 <= bytes);
            if (at + 8 <= bytes) seen[at / 8]++;
        }
    for (const int n : seen) CHECK_EQ(n, 1);
    CHECK_EQ(lens_slot_at(0, 1, kThreadsWg) - lens_slot_at(0, 0, kThreadsWg), 8);  // a wave's lanes are contiguous
}

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
    CHECK_EQ(kLensStageDefault, kLensStageLds);
    {
        const FramePlan p = frame_plan(c2, 0);
        CHECK(p.order.on && p.order.class3 == TileOrderPlan::InKernel);
        CHECK_EQ(p.order.lens_stage, kLensStageLds);
        CHECK_EQ(frame_params(c2, p).lens_batch, 1);
    }
    const auto stage_of = [](const FrameInputs &in) {
        const FramePlan p = frame_plan(in, 0);
        CHECK_EQ(frame_params(in, p).lens_batch, p.order.lens_stage == kLensStageLds ? 1 : 0);
        return p.order.lens_stage;
    };
    FrameInputs in = c2;
    in.grid.flags = CGRT_GRID_NO_LENS_STAGE;
    CHECK_EQ(stage_of(in), kLensStageOff);
    in = c2;
    in.cam.lens_radius = 0;  // a pinhole has no lens to sample
    CHECK_EQ(stage_of(in), kLensStageOff);
    in = c2;
    in.grid.flags = CGRT_GRID_DIFFUSE_TILES;  // the second launch's variant has no such LDS
    CHECK(frame_plan(in, 0).order.class3 == TileOrderPlan::SecondLaunch);
    CHECK_EQ(stage_of(in), kLensStageOff);
    in = c2;
    in.grid.flags = CGRT_GRID_NO_SPHERE_PAIRS;
    in.pair = false;  // the full body renders class 3
    CHECK_EQ(stage_of(in), kLensStageOff);
    in = c2;
    in.grid.flags = CGRT_GRID_NO_TILE_ORDER;
    CHECK_EQ(stage_of(in), kLensStageOff);
    in = c2;
    in.all_special = true;  // no tile can be of class 3
    CHECK_EQ(stage_of(in), kLensStageOff);
    in = c2;
    in.grid.flags = CGRT_GRID_SPLIT_SAMPLES;  // several chunks: no tile order
    CHECK_EQ(frame_plan(in, 0).chunks, 4);
    CHECK_EQ(stage_of(in), kLensStageOff);
    in = c2;
    in.image = false;
    in.sched = true;
    CHECK_EQ(stage_of(in), kLensStageOff);
    // it depends neither on the relay nor on the masks
    in = c2;
    in.grid.flags = CGRT_GRID_NO_SAMPLE_RELAY | CGRT_GRID_NO_SPHERE_MASKS;
    CHECK_EQ(frame_plan(in, 0).relay.base.k, 1);
    CHECK_EQ(stage_of(in), kLensStageLds);
    in = c2;
    in.grid.spp = in.grid.spp_total = 1;
    CHECK_EQ(stage_of(in), kLensStageLds);
    // the knob holds where the flag does not switch the stage off
    in = c2;
    in.knobs.lens_stage = kLensStageOff;
    CHECK_EQ(stage_of(in), kLensStageOff);
    in.knobs.lens_stage = kLensStageLds;
    CHECK_EQ(stage_of(in), kLensStageLds);
    in.grid.flags = CGRT_GRID_NO_LENS_STAGE;
    CHECK_EQ(stage_of(in), kLensStageOff);
    CHECK_EQ(lens_stage_named("off"), kLensStageOff);
    CHECK_EQ(lens_stage_named("lds"), kLensStageLds);
    CHECK_EQ(lens_stage_named(""), -1);
    CHECK_EQ(lens_stage_named("area"), -1);
    CHECK_EQ(EyeKnobs{}.lens_stage, -1);
    // the launch itself is what it was: workgroups, scratch and relay of the plan do not depend on the stage
    in = c2;
    in.grid.flags = CGRT_GRID_NO_LENS_STAGE;
    const FramePlan a = frame_plan(c2, 0), b = frame_plan(in, 0);
    CHECK_EQ(a.grid_dim, b.grid_dim);
    CHECK_EQ(a.scratch.total, b.scratch.total);
    CHECK_EQ(a.relay.base.k, b.relay.base.k);
    CHECK_EQ(a.relay.base.bytes, b.relay.base.bytes);
    CHECK_EQ(a.order.masks, b.order.masks);
}

int main() {
    draws();
    rounds();
    slots();
    plan();
    std::printf("ok: %d failed checks of %lld\n", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
