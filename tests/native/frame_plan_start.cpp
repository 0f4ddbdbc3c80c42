// The frame plan's choice of the relay's start order (cgrt_frame.h: RelayPlan::start, relay_rule): by cost where the launch
// relays by default and names no order, or where asked for; the list otherwise.  RelayPlan::order keeps its meaning -- the
// order of a launch that goes without the table.  Then relay_rule's four decisions over every combination of flags and knobs.
// CPU build under ASan + UBSan, driven by tests/test_relay_start_host.py.
#include <cstdio>
#include <cstdlib>

#include "cgrt_frame.h"

static int g_failed = 0;
static long long g_checks = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        g_checks++;                                                                                             \
        if (a_ != b_) {                                                                                         \
            std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)

// The image-order launch of a glass sphere scene -- ten spheres and nothing else, all in LDS -- by the PAIR variant, on a 288 GB
// device with 256 CUs (frame_plan.cpp's spheres())
static FrameInputs spheres(int W = 200, int rows = 117, int spp = 32) {
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
    in.glass = true;
    in.nt = 256;
    in.prim_obj = -1;
    in.mem_total = 288000000000ull;
    in.n_cu = 256;
    in.waves_per_simd = 4;
    in.image = in.sph = in.pair = in.order_ok = in.aux_stream = in.all_spheres = true;
    in.n_objs = in.n_lds = 10;
    return in;
}

int main() {
    {   // 1920 x 1080 at 64 samples relays by default: the cost start, the interleaved order behind it
        const FramePlan p = frame_plan(spheres(1920, 1080, 64), 0);
        CHECK_EQ(p.relay.base.k, 2);
        CHECK_EQ(p.relay.start, kRelayStartCost);
        CHECK_EQ(p.relay.order, kRelayInterleaved);
        CHECK_EQ(p.relay.extent, kRelayMirror);
        CHECK_EQ(p.relay.probe_spp, kRelayProbeSpp);
        CHECK_EQ(p.grid_dim, 8100);
        CHECK_EQ(p.relay.start_words, 8100 + p.relay.base.cap);  // the launch's workgroups: the host knows neither plan[2] nor plan[3]
        CHECK_EQ(p.relay.start_words, relay_grid(p.grid_dim, p.relay.base.k, p.relay.base.cap));
    }
    CHECK_EQ(kRelayProbeSpp == 1 || kRelayProbeSpp == 2 || kRelayProbeSpp == 4, 1);
    // an order named by flag gives the list, whichever it is
    for (int32_t f : {(int32_t)CGRT_GRID_RELAY_CHUNKS_FIRST, (int32_t)CGRT_GRID_RELAY_MIRROR_FIRST, (int32_t)CGRT_GRID_RELAY_INTERLEAVED}) {
        FrameInputs in = spheres(1920, 1080, 64);
        in.grid.flags = f;
        const FramePlan p = frame_plan(in, 0);
        CHECK_EQ(p.relay.base.k, 2);
        CHECK_EQ(p.relay.start, kRelayStartList);
        CHECK_EQ(p.relay.start_words, 0);
        CHECK_EQ(p.relay.probe_spp, 0);
        in.grid.flags = f | CGRT_GRID_RELAY_COST_START;  // ... unless the cost start is asked for beside it
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartCost);
        CHECK_EQ(frame_plan(in, 0).relay.order, relay_rule(f, in.knobs).order);
    }
    // ... and so does one named by knob
    for (int o : {kRelayChunksFirst, kRelayMirrorFirst, kRelayInterleaved}) {
        FrameInputs in = spheres(1920, 1080, 64);
        in.knobs.relay_order = o;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        CHECK_EQ(frame_plan(in, 0).relay.order, o);
        in.knobs.relay_start = kRelayStartCost;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartCost);
    }
    {   // the extent names no order
        FrameInputs in = spheres(1920, 1080, 64);
        in.grid.flags = CGRT_GRID_RELAY_NO_MIRROR;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartCost);
        CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayGlass);
    }
    {   // no relay: the list, no table
        FrameInputs in = spheres(1920, 1080, 64);
        in.grid.flags = CGRT_GRID_NO_SAMPLE_RELAY;
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 1);
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        CHECK_EQ(frame_plan(in, 0).relay.start_words, 0);
        in.grid.flags = CGRT_GRID_NO_SAMPLE_RELAY | CGRT_GRID_RELAY_COST_START;  // asking does not engage a relay
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        in = spheres();  // 105 tiles: below the gate
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 1);
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        in = spheres(1920, 1080, 31);  // fewer than two chunks of 16
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        in = spheres(1920, 1080, 64);  // the second launch for class 3 relays nothing
        in.grid.flags = CGRT_GRID_DIFFUSE_TILES;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        in = spheres(1920, 1080, 64);  // not the PAIR variant
        in.pair = false;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
    }
    {   // a relay asked for by flag keeps what that flag has always meant; with the cost start asked for too, that
        FrameInputs in = spheres();
        in.grid.flags = CGRT_GRID_SAMPLE_RELAY;
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 2);
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        in.grid.flags = CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_RELAY_COST_START;
        FramePlan p = frame_plan(in, 0);
        CHECK_EQ(p.relay.start, kRelayStartCost);
        CHECK_EQ(p.relay.order, kRelayChunksFirst);
        CHECK_EQ(p.relay.start_words, 105 + p.relay.base.cap);
        in.knobs.relay_tiles = 10;  // a bounded area
        p = frame_plan(in, 0);
        CHECK_EQ(p.relay.base.cap, 10);
        CHECK_EQ(p.relay.start_words, 115);
        in.grid.flags = CGRT_GRID_SAMPLE_RELAY_4 | CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_RELAY_COST_START;
        in.grid.spp = in.grid.spp_total = 64;
        p = frame_plan(in, 0);
        CHECK_EQ(p.relay.base.k, 4);
        CHECK_EQ(p.relay.start_words, 105 + 3 * 10);
    }
    {   // flags before the knob, either way
        FrameInputs in = spheres(1920, 1080, 64);
        in.knobs.relay_start = kRelayStartList;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        CHECK_EQ(frame_plan(in, 0).relay.order, kRelayInterleaved);  // the knob names no order
        in.grid.flags = CGRT_GRID_RELAY_COST_START;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartCost);
        in.knobs.relay_start = kRelayStartCost;
        in.grid.flags = CGRT_GRID_NO_RELAY_COST_START;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        in.grid.flags = CGRT_GRID_NO_RELAY_COST_START | CGRT_GRID_RELAY_COST_START;  // off wins
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        in = spheres();  // the knob on a launch that asked for the relay
        in.grid.flags = CGRT_GRID_SAMPLE_RELAY;
        in.knobs.relay_start = kRelayStartCost;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartCost);
    }
    {   // the probe's samples: the knob's, never more than the launch's
        FrameInputs in = spheres(1920, 1080, 64);
        in.knobs.relay_probe_spp = 4;
        CHECK_EQ(frame_plan(in, 0).relay.probe_spp, 4);
        in.knobs.relay_probe_spp = 1;
        CHECK_EQ(frame_plan(in, 0).relay.probe_spp, 1);
    }
    // The form rules, every combination of flags and knobs.  The expectation is include/cgrt.h's flag comments in this test's
    // own words: a flag holds (the switching-off one wins); else the knob; else a launch with CGRT_GRID_SAMPLE_RELAY relays the
    // glass tiles, chunks first, from the list; else the measured form -- mirror extent, interleaved, and by cost with promotion
    // exactly where the launch names no order; promotion by default only where the cost start is itself the default.
    for (int32_t asked : {0, (int32_t)CGRT_GRID_SAMPLE_RELAY})
        for (int32_t off : {0, (int32_t)CGRT_GRID_NO_SAMPLE_RELAY})
            for (int32_t of : {0, (int32_t)CGRT_GRID_RELAY_CHUNKS_FIRST, (int32_t)CGRT_GRID_RELAY_MIRROR_FIRST, (int32_t)CGRT_GRID_RELAY_INTERLEAVED})
                for (int32_t mf : {0, (int32_t)CGRT_GRID_RELAY_MIRROR, (int32_t)CGRT_GRID_RELAY_NO_MIRROR})
                    for (int32_t sf : {0, (int32_t)CGRT_GRID_RELAY_COST_START, (int32_t)CGRT_GRID_NO_RELAY_COST_START})
                        for (int32_t bf : {0, (int32_t)CGRT_GRID_RELAY_BOOST, (int32_t)CGRT_GRID_NO_RELAY_BOOST})
                            for (int km : {-1, 0, 1})
                                for (int ko : {-1, 0, 1, 2})
                                    for (int ks : {-1, 0, 1})
                                        for (bool kb : {false, true}) {
                                            EyeKnobs kn;
                                            kn.relay_mirror = km;
                                            kn.relay_order = ko;
                                            kn.relay_start = ks;
                                            kn.relay_boost_off = kb;
                                            int extent = asked ? kRelayGlass : kRelayMirror;
                                            if (km >= 0) extent = km ? kRelayMirror : kRelayGlass;
                                            if (mf == CGRT_GRID_RELAY_NO_MIRROR) extent = kRelayGlass;
                                            if (mf == CGRT_GRID_RELAY_MIRROR) extent = kRelayMirror;
                                            int order = asked ? kRelayChunksFirst : kRelayInterleaved;
                                            if (ko >= 0) order = ko;
                                            if (of == CGRT_GRID_RELAY_CHUNKS_FIRST) order = kRelayChunksFirst;
                                            if (of == CGRT_GRID_RELAY_MIRROR_FIRST) order = kRelayMirrorFirst;
                                            if (of == CGRT_GRID_RELAY_INTERLEAVED) order = kRelayInterleaved;
                                            const bool cost_by_default = !asked && of == 0 && ko < 0;
                                            int start = cost_by_default ? kRelayStartCost : kRelayStartList;
                                            if (ks >= 0) start = ks;
                                            if (sf == CGRT_GRID_RELAY_COST_START) start = kRelayStartCost;
                                            if (sf == CGRT_GRID_NO_RELAY_COST_START) start = kRelayStartList;
                                            bool boost = cost_by_default && sf == 0 && ks < 0;
                                            if (kb) boost = false;
                                            if (bf == CGRT_GRID_RELAY_BOOST) boost = true;
                                            if (bf == CGRT_GRID_NO_RELAY_BOOST) boost = false;
                                            const RelayRule got = relay_rule(asked | off | of | mf | sf | bf, kn);
                                            CHECK_EQ(got.extent, extent);
                                            CHECK_EQ(got.order, order);
                                            CHECK_EQ(got.start, start);
                                            CHECK_EQ(got.boost, boost);
                                        }
    // the knob's names
    CHECK_EQ(relay_start_named("list"), kRelayStartList);
    CHECK_EQ(relay_start_named("cost"), kRelayStartCost);
    CHECK_EQ(relay_start_named("0"), kRelayStartList);
    CHECK_EQ(relay_start_named("1"), kRelayStartCost);
    CHECK_EQ(relay_start_named(""), -1);
    CHECK_EQ(relay_start_named("longest"), -1);
    CHECK_EQ(EyeKnobs{}.relay_start, -1);
    CHECK_EQ(EyeKnobs{}.relay_probe_spp, kRelayProbeSpp);
    CHECK_EQ(FramePlan{}.relay.start, kRelayStartList);
    std::printf("%s: %d failed checks of %lld\n", g_failed ? "FAILED" : "ok", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
