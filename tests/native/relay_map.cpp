// The sample relay's index arithmetic (cgrt_relay.h), which the host plans with and trace_grid_kernel maps its workgroups by:
// every workgroup of the launch renders exactly one (entry, chunk) or leaves, every (entry, chunk) that should exist is
// rendered once, a tile's chunks partition its samples, the area's bytes per tile equal the written-out sum, and the capacity
// respects the budget.  CPU build under ASan + UBSan, driven by tests/test_relay_map_host.py.
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
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            g_failed++;                                                  \
        }                                                                \
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

// One launch: the list has n_tiles entries (plan[4]), the first `special` of them of class 0 or 1 (plan[2]), those from
// `first_diffuse` on of class 3 (plan[3]); the area holds cap_split tiles.  What the kernel does with each workgroup, in the
// kernel's own words (trace_grid_kernel, cgrt_eye.hpp).
static void launch(size_t n_tiles, size_t special, size_t first_diffuse, size_t cap_split, int k) {
    const size_t grid = relay_grid(n_tiles, k, cap_split);
    CHECK_EQ(grid, n_tiles + (size_t)(k - 1) * cap_split);
    const size_t n_split = special < cap_split ? special : cap_split;
    std::vector<int> seen(n_tiles * (size_t)k, 0);  // [entry][chunk]
    std::vector<int> diffuse(n_tiles, 0);
    size_t left = 0;
    for (size_t b = 0; b < grid; b++) {
        const RelayBlock rb = relay_block((uint32_t)b, (uint32_t)k, (uint32_t)n_split);
        if (rb.entry >= n_tiles) {  // beyond the list: the workgroup leaves
            left++;
            continue;
        }
        CHECK(rb.chunk >= 0 && rb.chunk < k);
        CHECK_EQ(rb.split, rb.entry < n_split);
        if (!rb.split) CHECK_EQ(rb.chunk, 0);
        seen[rb.entry * (size_t)k + (size_t)rb.chunk]++;
        if (rb.entry >= first_diffuse) diffuse[rb.entry]++;  // the in-kernel diffuse branch compares the entry
    }
    for (size_t e = 0; e < n_tiles; e++) {
        for (int c = 0; c < k; c++) CHECK_EQ(seen[e * (size_t)k + (size_t)c], (e < n_split || c == 0) ? 1 : 0);
        // the entries the diffuse body takes are those of class 3, each once, none of them split (class 3 lies behind class 1)
        CHECK_EQ(diffuse[e], e >= first_diffuse ? 1 : 0);
        if (e >= first_diffuse) CHECK(e >= n_split);
    }
    CHECK_EQ(left, (size_t)(k - 1) * (cap_split - n_split));  // the surplus workgroups
}

int main() {
    const size_t tiles[] = {1, 15, 105, 8100};
    for (const size_t n : tiles) {
        const size_t specials[] = {0, 1, n / 2, n}, caps[] = {0, 1, 3, n};
        for (const size_t special : specials)
            for (const size_t cap : caps) {
                if (special > n || cap > n) continue;  // (n == 1: 3 > n)
                for (int k = 2; k <= 4; k++) {
                    // class 3 begins at or behind the end of class 1: right there, halfway to the end, at the end (none)
                    const size_t firsts[] = {special, special + (n - special) / 2, n};
                    for (const size_t fd : firsts) launch(n, special, fd, cap, k);
                }
            }
    }

    // chunks: K = min(4, spp / 16) from ceil(spp / K) samples each; the chunks' sample ranges partition [0, spp)
    const int spps[] = {32, 33, 48, 64, 70, 1024};
    const int want_k[] = {2, 2, 3, 4, 4, 4}, want_cs[] = {16, 17, 16, 16, 18, 256};
    for (int i = 0; i < 6; i++) {
        for (int max_k = 2; max_k <= 4; max_k++) {
            const int spp = spps[i];
            const RelayChunks rc = relay_chunks(spp, max_k);
            if (max_k == 4) {
                CHECK_EQ(rc.k, want_k[i]);
                CHECK_EQ(rc.chunk_spp, want_cs[i]);
            }
            CHECK(rc.k >= 2 && rc.k <= max_k && rc.chunk_spp >= kRelayMinChunkSpp);
            std::vector<int> hit((size_t)spp, 0);
            int next = 0;
            for (int c = 0; c < rc.k; c++) {
                const int s0 = relay_first_sample(c, rc.chunk_spp), s1 = relay_end_sample(c, rc.chunk_spp, spp);
                CHECK_EQ(s0, next);  // contiguous, in order
                CHECK(s1 > s0 && s1 <= spp && s1 - s0 <= rc.chunk_spp);
                for (int s = s0; s < s1; s++) hit[(size_t)s]++;
                next = s1;
            }
            CHECK_EQ(next, spp);
            for (int s = 0; s < spp; s++) CHECK_EQ(hit[(size_t)s], 1);
        }
    }
    for (int spp = 1; spp < 32; spp++) CHECK_EQ(relay_chunks(spp).k, 1);  // no relay below 32 samples

    // bytes per tile, written out: one arrival word; 256 pixels x 3 fp64 sums; K hit counts and K - 1 value counts per pixel;
    // K - 1 streams of `slots` values of 3 doubles for each of 256 pixels.  slots = chunk_spp * 2^(depth - 1), a multiple of 8.
    for (int k = 2; k <= 4; k++)
        for (int depth = 2; depth <= 5; depth++)
            for (const int cs : {16, 17, 18, 256}) {
                const int slots = relay_slots(cs, depth);
                CHECK(slots >= cs * (1 << (depth - 1)) && slots < cs * (1 << (depth - 1)) + 8 && slots % 8 == 0);
                const size_t want = 4 + 256 * 3 * 8 + (size_t)k * 256 * 4 + (size_t)(k - 1) * 256 * 4 + (size_t)(k - 1) * (size_t)slots * 3 * 256 * 8;
                CHECK_EQ(relay_tile_bytes(k, slots), want);
                // the layout: arrays in order, the first behind the padded arrival words, sizes per tile adding up to the above
                for (const size_t cap : {(size_t)1, (size_t)3, (size_t)649, (size_t)8100}) {
                    const RelayLayout l = relay_layout(cap, k, slots);
                    CHECK_EQ(l.racc, (cap * 4 + 255) / 256 * 256);
                    CHECK_EQ(l.rhits - l.racc, cap * 256 * 3 * 8);
                    CHECK_EQ(l.rcount - l.rhits, cap * (size_t)k * 256 * 4);
                    CHECK_EQ(l.rvals - l.rcount, cap * (size_t)(k - 1) * 256 * 4);
                    CHECK_EQ(l.total - l.rvals, cap * (size_t)(k - 1) * (size_t)slots * 3 * 256 * 8);
                    CHECK_EQ(l.total - l.racc, cap * (want - 4));
                    CHECK(l.racc % 256 == 0 && l.rhits % 8 == 0 && l.rcount % 4 == 0 && l.rvals % 8 == 0);
                }
            }
    // the workload: 64 samples, depth 5, K = 4: 256 slots, 4.7 MB a tile
    CHECK_EQ(relay_slots(16, 5), 256);
    CHECK_EQ(relay_tile_bytes(4, 256), 4731908);

    // capacity: as many tiles as the budget pays for, no more than the launch has, no more than the bound; the area fits the budget
    const size_t mems[] = {288000000000ull, (size_t)16 << 30, (size_t)1 << 30, 1000};
    for (const size_t mem : mems) {
        const size_t budget = relay_budget(mem);
        CHECK(budget <= ((size_t)4 << 30) && budget <= mem / 8 && (budget == ((size_t)4 << 30) || budget == mem / 8));
        for (const size_t n : tiles)
            for (int k = 2; k <= 4; k++)
                for (const long long bound : {0ll, 1ll, 3ll}) {
                    const int slots = relay_slots(relay_chunks(16 * k).chunk_spp, 5);
                    const size_t cap = relay_cap(n, k, slots, budget, bound);
                    CHECK(cap <= n && (bound == 0 || cap <= (size_t)bound));
                    if (cap > 0) CHECK(relay_layout(cap, k, slots).total <= budget);
                    const size_t lim = bound > 0 && (size_t)bound < n ? (size_t)bound : n;
                    if (cap < lim) CHECK(relay_layout(cap + 1, k, slots).total > budget);  // not a tile fewer than fits
                }
    }
    CHECK_EQ(relay_cap(8100, 4, 256, relay_budget(288000000000ull)), 907);  // the workload's frame: 4 GiB / 4.7 MB

    // the plan: FramePlan carries the same numbers, and only for a launch that may relay, with enough samples and tiles
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
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 1);  // not a relay launch
        in.image = in.sph = in.pair = in.order_ok = true;  // the PAIR variant in tile order
        {   // by default two chunks: 32 samples each, 512 slots, 3.15 MB a tile
            const FramePlan q = frame_plan(in, 0);
            CHECK_EQ(q.relay.base.k, 2);
            CHECK_EQ(q.relay.base.chunk_spp, 32);
            CHECK_EQ(q.relay.base.slots, 512);
            CHECK_EQ(relay_tile_bytes(q.relay.base.k, q.relay.base.slots), 4 + 6144 + 2048 + 1024 + 512 * 6144);
            CHECK_EQ(q.relay.base.cap, ((size_t)4 << 30) / relay_tile_bytes(q.relay.base.k, q.relay.base.slots));
        }
        in.grid.flags = CGRT_GRID_SAMPLE_RELAY_4;
        const FramePlan p = frame_plan(in, 0);
        CHECK_EQ(p.relay.base.k, 4);
        CHECK_EQ(p.relay.base.chunk_spp, 16);
        CHECK_EQ(p.relay.base.slots, 256);
        CHECK_EQ(relay_tile_bytes(p.relay.base.k, p.relay.base.slots), 4731908);
        CHECK_EQ(p.relay.base.cap, 907);
        CHECK_EQ(p.relay.base.bytes, relay_layout(907, 4, 256).total);
        CHECK_EQ(p.grid_dim, 8100);  // the surplus is added when the area is there
        CHECK_EQ(relay_grid(p.grid_dim, p.relay.base.k, p.relay.base.cap), 8100 + 3 * 907);
        FrameInputs small = in;  // 200 x 117: 105 tiles < 4 x 256
        small.grid.width = 200;
        small.grid.height = small.grid.rows = 117;
        CHECK_EQ(frame_plan(small, 0).relay.base.k, 1);
        small.grid.flags = CGRT_GRID_SAMPLE_RELAY;
        CHECK_EQ(frame_plan(small, 0).relay.base.k, 2);
        small.grid.flags = CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_SAMPLE_RELAY_4;
        CHECK_EQ(frame_plan(small, 0).relay.base.k, 4);
        CHECK_EQ(frame_plan(small, 0).relay.base.cap, 105);
        small.grid.flags = CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_SAMPLE_RELAY_4 | CGRT_GRID_NO_SAMPLE_RELAY;
        CHECK_EQ(frame_plan(small, 0).relay.base.k, 1);
        in.grid.flags = CGRT_GRID_NO_SAMPLE_RELAY;
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 1);
        in.grid.flags = CGRT_GRID_SAMPLE_RELAY_4;
        in.grid.spp = 31;
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 1);
        in.grid.spp = 70;
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 4);
        CHECK_EQ(frame_plan(in, 0).relay.base.chunk_spp, 18);
        in.knobs.relay_tiles = 3;
        CHECK_EQ(frame_plan(in, 0).relay.base.cap, 3);
        in.grid.flags = 0;
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 2);
        CHECK_EQ(frame_plan(in, 0).relay.base.chunk_spp, 35);
        in.knobs.relay_chunks = 3;
        CHECK_EQ(frame_plan(in, 0).relay.base.k, 3);
    }
    std::printf("ok: %d failed checks of %lld\n", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
