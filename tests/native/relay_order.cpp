// The sample relay's launch map with an extent and an order (relay_block_ordered, cgrt_relay.h), which trace_grid_kernel maps
// its workgroups by: every workgroup of the launch renders exactly one (entry, chunk) or leaves, every (entry, chunk) that
// should exist is rendered once, the split entries are the prefix the extent names, and the workgroups of classes 0-1 and of
// class 2 stand where the order says; and the frame plan's choice of both (cgrt_frame.h).  CPU build under ASan + UBSan,
// driven by tests/test_relay_order_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cgrt_frame.h"

static int g_failed = 0;
static long long g_checks = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        g_checks++;                                                      \
        if (!(c)) {                                                      \
            if (g_failed < 50) std::printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case); \
            g_failed++;                                                  \
        }                                                                \
    } while (0)
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        g_checks++;                                                                                             \
        if (a_ != b_) {                                                                                         \
            if (g_failed < 50) std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld  [%s]\n", __FILE__, __LINE__, #a, a_, #b, b_, g_case); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)
static char g_case[160] = "";

// One launch: the list has n_tiles entries (plan[4]), [0, n01) of class 0 or 1 (plan[2]), [n01, n012) of class 2 (plan[3]), the
// rest of class 3; the area holds cap tiles.  What the kernel does with each workgroup, in the kernel's own words
// (trace_grid_kernel, cgrt_eye.hpp).
static void launch(size_t n_tiles, size_t n01, size_t n012, size_t cap, int k, int extent, int order) {
    std::snprintf(g_case, sizeof g_case, "tiles %zu n01 %zu n012 %zu cap %zu k %d extent %d order %d", n_tiles, n01, n012, cap, k, extent, order);
    const size_t grid = relay_grid(n_tiles, k, cap);
    const size_t named = extent == kRelayMirror ? n012 : n01, n_split = named < cap ? named : cap;  // the prefix the extent names
    CHECK_EQ(relay_split_entries((uint32_t)n01, (uint32_t)n012, (uint32_t)cap, extent), n_split);
    const size_t s_a = n_split < n01 ? n_split : n01, s_m = n_split - s_a;
    const long long a = (long long)(n01 + (size_t)(k - 1) * s_a), m = (long long)(n012 - n01 + (size_t)(k - 1) * s_m), t = a + m;
    std::vector<int> seen(n_tiles * (size_t)k, 0);  // [entry][chunk]
    size_t left = 0;
    long long n_a = 0, n_m = 0;               // workgroups of classes 0-1 and of class 2 so far
    long long last_a = -1, last_m = -1;       // entry * k + chunk of the last one of each sequence
    long long last_m_at = -1, first_a_at = -1, first_3_at = -1, last_3 = -1;
    for (size_t b = 0; b < grid; b++) {
        const RelayBlock rb = relay_block_ordered((uint32_t)b, (uint32_t)k, (uint32_t)n01, (uint32_t)n012, (uint32_t)n_tiles, (uint32_t)cap, extent, order);
        if (extent == kRelayGlass && order == kRelayChunksFirst) {  // exactly relay_block
            const RelayBlock old = relay_block((uint32_t)b, (uint32_t)k, (uint32_t)n_split);
            CHECK_EQ(rb.entry >= n_tiles, old.entry >= n_tiles);
            if (old.entry < n_tiles) {
                CHECK_EQ(rb.entry, old.entry);
                CHECK_EQ(rb.chunk, old.chunk);
                CHECK_EQ(rb.split, old.split);
            }
        }
        if (rb.entry >= n_tiles) {  // beyond the list: the workgroup leaves
            CHECK(b >= n_tiles + (size_t)(k - 1) * n_split);
            left++;
            continue;
        }
        CHECK_EQ(left, 0);  // nothing renders behind a workgroup that left
        CHECK(rb.chunk >= 0 && rb.chunk < k);
        CHECK_EQ(rb.split, rb.entry < n_split);
        if (!rb.split) CHECK_EQ(rb.chunk, 0);
        seen[rb.entry * (size_t)k + (size_t)rb.chunk]++;
        const long long key = (long long)rb.entry * k + rb.chunk;
        if (rb.entry >= n012) {  // class 3: in entry order behind everything else
            if (first_3_at < 0) first_3_at = (long long)b;
            CHECK_EQ(b, (size_t)t + (rb.entry - n012));
            CHECK(key > last_3);
            last_3 = key;
            continue;
        }
        CHECK(first_3_at < 0);
        CHECK((long long)b < t);
        if (rb.entry >= n01) {  // class 2
            CHECK(key > last_m);  // the sequence keeps its order
            last_m = key;
            last_m_at = (long long)b;
            n_m++;
        } else {
            CHECK(key > last_a);
            last_a = key;
            if (first_a_at < 0) first_a_at = (long long)b;
            n_a++;
        }
        if (order == kRelayInterleaved) {
            // the prefix of b + 1 workgroups holds its share (b + 1) m / t of class-2 workgroups within one
            const long long d = n_m * t - (long long)(b + 1) * m;
            CHECK(d <= t && -d <= t);
        }
        if (order == kRelayChunksFirst) CHECK_EQ(rb.entry >= n01, (long long)b >= a);
    }
    CHECK_EQ(n_a, a);
    CHECK_EQ(n_m, m);
    if (order == kRelayMirrorFirst && last_m_at >= 0 && first_a_at >= 0) CHECK(last_m_at < first_a_at);  // all of class 2 first
    if (order == kRelayMirrorFirst && n_m > 0) CHECK_EQ(last_m_at, m - 1);
    for (size_t e = 0; e < n_tiles; e++)
        for (int c = 0; c < k; c++) CHECK_EQ(seen[e * (size_t)k + (size_t)c], (e < n_split || c == 0) ? 1 : 0);
    CHECK_EQ(left, (size_t)(k - 1) * (cap - n_split));  // the surplus workgroups
}

int main() {
    const size_t tiles[] = {1, 15, 105, 8100};
    long long launches = 0;
    for (const size_t n : tiles) {
        const size_t ends[] = {0, 1, n / 2, n};  // n012: at 0, 1, the middle and the end
        for (size_t i = 0; i < 4; i++) {
            const size_t n012 = ends[i];
            if (i > 0 && n012 == ends[i - 1]) continue;  // (n == 1: the middle is 0, the end is 1)
            const size_t firsts[] = {0, 1, n012 / 2, n012};  // n01 likewise, within n012
            for (size_t j = 0; j < 4; j++) {
                const size_t n01 = firsts[j];
                bool again = n01 > n012;
                for (size_t d = 0; d < j; d++) again = again || firsts[d] == n01;
                if (again) continue;
                // the area: none, one tile, ends inside classes 0-1, exactly at n01, inside class 2, at n012, the whole list
                const size_t caps[] = {0, 1, n01 / 2, n01, n01 + (n012 - n01) / 2, n012, n};
                for (size_t c = 0; c < 7; c++) {
                    bool dup = false;
                    for (size_t d = 0; d < c; d++) dup = dup || caps[d] == caps[c];
                    if (dup) continue;
                    for (int k = 2; k <= 4; k++)
                        for (int extent = kRelayGlass; extent <= kRelayMirror; extent++)
                            for (int order = kRelayChunksFirst; order <= kRelayInterleaved; order++) {
                                launch(n, n01, n012, caps[c], k, extent, order);
                                launches++;
                            }
                }
            }
        }
    }
    // the workload's frame (1920 x 1080: 649 tiles of classes 0-1, 598 of class 2), two chunks, the area for 1 361 tiles, and
    // four chunks with the area ending inside class 2
    for (int extent = kRelayGlass; extent <= kRelayMirror; extent++)
        for (int order = kRelayChunksFirst; order <= kRelayInterleaved; order++) {
            launch(8100, 649, 1247, 1361, 2, extent, order);
            launch(8100, 649, 1247, 907, 4, extent, order);
        }
    std::snprintf(g_case, sizeof g_case, "frame plan");

    // the plan: extent and order are 0 unless the relay is engaged; a launch that asks for the relay by its flag keeps classes
    // 0-1, chunks first, unless the flags or the knobs name another form; the flags go before the knobs
    {
        FrameInputs in{};
        in.grid.width = 1920;
        in.grid.height = in.grid.rows = 1080;
        in.grid.spp = in.grid.spp_total = 64;
        in.grid.max_depth = 5;
        in.glass = true;
        in.nt = 256;
        in.prim_obj = -1;
        in.mem_total = 288000000000ull;
        in.n_cu = 256;
        in.waves_per_simd = 4;
        in.image = in.sph = in.pair = in.order_ok = true;  // the PAIR variant in tile order
        CHECK_EQ(in.knobs.relay_mirror, -1);
        CHECK_EQ(in.knobs.relay_order, -1);
        {   // the default launch: the measured form
            const FramePlan p = frame_plan(in, 0);
            CHECK_EQ(p.relay.base.k, 2);
            CHECK_EQ(p.relay.extent, kRelayDefaultExtent);
            CHECK_EQ(p.relay.order, kRelayDefaultOrder);
            CHECK_EQ(p.relay.base.cap, 1361);  // 1 247 tiles of classes 0-2 fit
        }
        const int32_t asked[] = {CGRT_GRID_SAMPLE_RELAY, CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_SAMPLE_RELAY_4};
        for (const int32_t f : asked) {
            in.grid.flags = f;
            CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayGlass);
            CHECK_EQ(frame_plan(in, 0).relay.order, kRelayChunksFirst);
            in.grid.flags = f | CGRT_GRID_RELAY_MIRROR | CGRT_GRID_RELAY_INTERLEAVED;
            CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayMirror);
            CHECK_EQ(frame_plan(in, 0).relay.order, kRelayInterleaved);
            in.grid.flags = f | CGRT_GRID_RELAY_MIRROR_FIRST;
            CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayGlass);
            CHECK_EQ(frame_plan(in, 0).relay.order, kRelayMirrorFirst);
            in.grid.flags = f | CGRT_GRID_RELAY_CHUNKS_FIRST | CGRT_GRID_RELAY_NO_MIRROR;
            CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayGlass);
            CHECK_EQ(frame_plan(in, 0).relay.order, kRelayChunksFirst);
        }
        in.grid.flags = CGRT_GRID_RELAY_MIRROR | CGRT_GRID_RELAY_MIRROR_FIRST;  // the default gate, the form named
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 2);
        CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayMirror);
        CHECK_EQ(frame_plan(in, 0).relay.order, kRelayMirrorFirst);
        in.grid.flags = CGRT_GRID_NO_SAMPLE_RELAY | CGRT_GRID_RELAY_MIRROR | CGRT_GRID_RELAY_INTERLEAVED;  // not engaged: today's form
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 1);
        CHECK_EQ(frame_plan(in, 0).relay.extent, 0);
        CHECK_EQ(frame_plan(in, 0).relay.order, 0);
        FrameInputs small = in;  // 200 x 117: below the gate nothing is relayed, whatever form is named
        small.grid.width = 200;
        small.grid.height = small.grid.rows = 117;
        small.grid.flags = CGRT_GRID_RELAY_MIRROR | CGRT_GRID_RELAY_INTERLEAVED;
        CHECK_EQ(frame_plan(small, 0).relay.base.k, 1);
        CHECK_EQ(frame_plan(small, 0).relay.extent, 0);
        CHECK_EQ(frame_plan(small, 0).relay.order, 0);
        // the knobs: where the flags name nothing
        in.knobs.relay_mirror = 1;
        in.knobs.relay_order = kRelayInterleaved;
        for (const int32_t f : {0, (int32_t)CGRT_GRID_SAMPLE_RELAY}) {
            in.grid.flags = f;
            CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayMirror);
            CHECK_EQ(frame_plan(in, 0).relay.order, kRelayInterleaved);
            in.grid.flags = f | CGRT_GRID_RELAY_NO_MIRROR | CGRT_GRID_RELAY_CHUNKS_FIRST;
            CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayGlass);
            CHECK_EQ(frame_plan(in, 0).relay.order, kRelayChunksFirst);
        }
        in.knobs.relay_mirror = 0;
        in.knobs.relay_order = kRelayChunksFirst;
        in.grid.flags = 0;
        CHECK_EQ(frame_plan(in, 0).relay.extent, kRelayGlass);
        CHECK_EQ(frame_plan(in, 0).relay.order, kRelayChunksFirst);
        CHECK_EQ(relay_order_named("chunks_first"), kRelayChunksFirst);
        CHECK_EQ(relay_order_named("mirror_first"), kRelayMirrorFirst);
        CHECK_EQ(relay_order_named("interleaved"), kRelayInterleaved);
        CHECK_EQ(relay_order_named("2"), kRelayInterleaved);
        CHECK_EQ(relay_order_named(""), -1);
        CHECK_EQ(relay_order_named("sideways"), -1);
    }
    std::printf("launches %lld\n", launches);
    std::printf("ok: %d failed checks of %lld\n", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
