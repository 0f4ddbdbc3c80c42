// The relay's start order by cost (cgrt_relay.h, "The start order by cost"), which the host, relay_start_kernel and the GPU test
// share: for every case the table is a permutation of exactly the items relay_block_ordered enumerates for b < t, the weights
// along it do not increase, and equal weights stand in (entry, chunk) order.  The kernel's own way of counting a rank -- a
// workgroup's worth of weights at a time -- is repeated here in plain C++ and must give the same table.  CPU build under
// ASan + UBSan, driven by tests/test_relay_start_host.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "cgrt_frame.h"

static int g_failed = 0;
static long long g_checks = 0;
static char g_case[200] = "";
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

// how the wave tiles' costs are chosen
enum Costs { Varied, Equal, SomeZero, AllZero };

// A grid of tiles_x x tiles_y tiles whose last column and row of wave tiles are missing (an image that ends inside a tile), a
// list that is some permutation of the tiles, plan = (n01, n012), an area of cap tiles.
static void one_case(uint32_t tiles_x, uint32_t tiles_y, uint32_t n01, uint32_t n012, uint32_t cap, int k, int extent, int spp, Costs costs) {
    const uint32_t n_tiles = tiles_x * tiles_y, wtiles_x = 2 * tiles_x - 1, wtiles_y = 2 * tiles_y - 1;
    const RelayChunks rc = relay_chunks(spp, k);
    std::snprintf(g_case, sizeof g_case, "tiles %ux%u n01 %u n012 %u cap %u k %d (%d x %d of %d) extent %d costs %d", tiles_x, tiles_y, n01, n012, cap, k,
                  rc.k, rc.chunk_spp, spp, extent, (int)costs);
    CHECK_EQ(rc.k, k);
    const RelayItems r{(uint32_t)rc.k, n01, n012, n_tiles, cap, extent, rc.chunk_spp, spp};
    std::vector<uint32_t> list(n_tiles), wcost((size_t)wtiles_x * wtiles_y);
    for (uint32_t e = 0; e < n_tiles; e++) list[e] = (e * 11u + 3u) % n_tiles;  // (11 is coprime to every n_tiles used)
    uint32_t x = 12345u;
    for (uint32_t &c : wcost) {
        x = x * 1664525u + 1013904223u;
        c = costs == Equal ? 9u : costs == AllZero ? 0u : costs == SomeZero ? ((x >> 16) % 3u ? (x >> 20) % 5u : 0u) : 1u + (x >> 12) % 200u;
    }
    const uint32_t t = relay_items_total(r), n_split = relay_split_entries(n01, n012, cap, extent);
    CHECK_EQ(t, n012 + (uint32_t)(rc.k - 1) * n_split);
    CHECK(t <= relay_start_words(n_tiles, rc.k, cap));
    // (one word beyond each array that nobody may write)
    std::vector<uint64_t> weight(t + 1, ~0ull);
    std::vector<uint32_t> start(t + 1, ~0u);
    relay_start_table(r, list.data(), wcost.data(), tiles_x, wtiles_x, wtiles_y, weight.data(), start.data());
    CHECK_EQ(start[t], ~0u);
    CHECK(weight[t] == ~0ull);

    // the items relay_block_ordered enumerates for b < t, in every order it knows: the same set
    std::map<std::pair<uint32_t, int>, int> want;
    for (int order : {kRelayChunksFirst, kRelayMirrorFirst, kRelayInterleaved}) {
        for (uint32_t b = 0; b < t; b++) {
            const RelayBlock rb = relay_block_ordered(b, r.k, n01, n012, n_tiles, cap, extent, order);
            CHECK(rb.entry < n012);
            want[{rb.entry, rb.chunk}] += 1;
        }
    }
    CHECK_EQ(want.size(), t);
    for (const auto &w : want) CHECK_EQ(w.second, 3);
    // beyond t the table is not asked: class 3 as ever
    if (t < relay_grid(n_tiles, rc.k, cap)) CHECK(relay_block_ordered(t, r.k, n01, n012, n_tiles, cap, extent, kRelayInterleaved).entry >= n012);

    // the table: a permutation of exactly those, weights non-increasing, ties in (entry, chunk) order
    std::map<std::pair<uint32_t, int>, int> got;
    uint64_t prev_w = ~0ull;
    long long prev_key = -1;
    for (uint32_t b = 0; b < t; b++) {
        const RelayBlock rb = relay_start_block(start[b], n_split);
        CHECK(rb.entry < n012 && rb.chunk >= 0 && rb.chunk < rc.k);
        if (rb.entry >= n012) continue;
        CHECK_EQ(rb.split, rb.entry < n_split);
        if (!rb.split) CHECK_EQ(rb.chunk, 0);
        got[{rb.entry, rb.chunk}] += 1;
        const uint32_t tc = relay_tile_cost(wcost.data(), list[rb.entry], tiles_x, wtiles_x, wtiles_y);
        // the tile's cost: the largest of the wave tiles it has
        {
            const uint32_t tx = list[rb.entry] % tiles_x, ty = list[rb.entry] / tiles_x;
            uint32_t m = 0;
            for (uint32_t wy = 2 * ty; wy < 2 * ty + 2 && wy < wtiles_y; wy++)
                for (uint32_t wx = 2 * tx; wx < 2 * tx + 2 && wx < wtiles_x; wx++) m = std::max(m, wcost[wy * wtiles_x + wx]);
            CHECK_EQ(tc, m);
        }
        const int samples = rb.split ? relay_end_sample(rb.chunk, rc.chunk_spp, spp) - relay_first_sample(rb.chunk, rc.chunk_spp) : spp;
        CHECK(samples > 0 && samples <= spp);
        const uint64_t w = (uint64_t)tc * (uint64_t)samples;
        CHECK(w == relay_item_weight(rb, tc, r));
        const long long key = (long long)rb.entry * 4 + rb.chunk;
        CHECK(w <= prev_w);
        if (w == prev_w) CHECK(key > prev_key);
        prev_w = w;
        prev_key = key;
    }
    CHECK_EQ(got.size(), t);
    for (const auto &g : got) {
        CHECK_EQ(g.second, 1);
        CHECK_EQ(want.count(g.first), 1);
    }
    // a split entry's chunks add up to the launch's samples
    for (uint32_t e = 0; e < n_split; e++) {
        int sum = 0;
        for (int c = 0; c < rc.k; c++) sum += relay_end_sample(c, rc.chunk_spp, spp) - relay_first_sample(c, rc.chunk_spp);
        CHECK_EQ(sum, spp);
    }

    // the kernel's count (relay_start_kernel): thread i of workgroup blk, the weights a batch of kRelayThreads at a time
    std::vector<uint32_t> start2(t + 1, ~0u);
    const uint32_t words = (uint32_t)relay_start_words(n_tiles, rc.k, cap);
    for (uint32_t blk = 0; blk < (words + kRelayThreads - 1) / kRelayThreads; blk++) {
        if (blk * kRelayThreads >= t) continue;
        for (uint32_t tid = 0; tid < (uint32_t)kRelayThreads; tid++) {
            const uint32_t i = blk * kRelayThreads + tid;
            const uint64_t wi = i < t ? weight[i] : 0;
            uint32_t rank = 0;
            for (uint32_t j0 = 0; j0 < t; j0 += kRelayThreads) {
                const uint32_t n = std::min((uint32_t)kRelayThreads, t - j0);
                for (uint32_t u = 0; u < n; u++) rank += relay_item_before(weight[j0 + u], j0 + u, wi, i) ? 1u : 0u;
            }
            if (i < t) {
                CHECK(rank < t);
                if (rank < t) start2[rank] = relay_start_word(relay_item(i, r));
            }
        }
    }
    for (uint32_t b = 0; b <= t; b++) CHECK_EQ(start2[b], start[b]);
}

int main() {
    // 7 x 15 = 105 tiles (200 x 117 pixels), 4 x 7 = 28 and one tile; spp 32, 40, 64 and a short last chunk (33: 17 + 16; 50: 17 + 17 + 16; 70: 18 + 18 + 18 + 16); cap: 0, below, inside and beyond each class; n01 = 0, n012 = n01, n012 = 0, everything of classes 0-2
    struct Plan { uint32_t n01, n012; };
    for (const auto &dims : {std::pair<uint32_t, uint32_t>{7, 15}, {4, 7}, {1, 1}}) {
        const uint32_t n = dims.first * dims.second;
        const Plan plans[] = {{0, 0}, {0, n / 3}, {n / 4, n / 4}, {n / 5, n / 2}, {n / 3, n}, {n, n}, {1 % (n + 1), 1 % (n + 1)}};
        for (const Plan &pl : plans) {
            if (pl.n012 > n || pl.n01 > pl.n012) continue;
            const uint32_t caps[] = {0, 1, pl.n01 / 2, pl.n01, pl.n01 + (pl.n012 - pl.n01) / 2, pl.n012, pl.n012 + 3, n, n + 7};
            for (uint32_t cap : caps)
                for (int extent : {kRelayGlass, kRelayMirror})
                    for (const auto &ks : {std::pair<int, int>{2, 32}, {2, 40}, {2, 33}, {3, 50}, {4, 64}, {4, 70}})
                        for (Costs c : {Varied, Equal, SomeZero, AllZero}) one_case(dims.first, dims.second, pl.n01, pl.n012, cap, ks.first, extent, ks.second, c);
        }
    }
    // more items than one workgroup of the ranking kernel holds, and than two
    one_case(30, 20, 150, 400, 600, 2, kRelayMirror, 64, Varied);
    one_case(30, 20, 150, 400, 100, 4, kRelayMirror, 64, SomeZero);
    one_case(30, 20, 256, 256, 256, 2, kRelayGlass, 40, Equal);

    // words and blocks
    {
        std::snprintf(g_case, sizeof g_case, "words");
        const RelayBlock b{(uint32_t)((1u << 30) - 1), 3, true};
        const RelayBlock back = relay_start_block(relay_start_word(b), 1u << 30);
        CHECK_EQ(back.entry, b.entry);
        CHECK_EQ(back.chunk, 3);
        CHECK_EQ(back.split, 1);
        CHECK_EQ(relay_start_block(relay_start_word(RelayBlock{5, 0, false}), 5).split, 0);
        CHECK(relay_item_before(3, 9, 2, 0) && !relay_item_before(2, 0, 3, 9) && relay_item_before(2, 0, 2, 1) && !relay_item_before(2, 1, 2, 1));
        // the layout: the table's parts lie behind everything a launch without one has, and hold what they must
        const TileOrderLayout off = tile_order_layout(105, 390, true), on = tile_order_layout(105, 390, true, 210);
        CHECK_EQ(off.wcost.bytes + off.weight.bytes + off.start.bytes, 0);
        CHECK_EQ(on.plan.at, off.plan.at);
        CHECK_EQ(on.wsure.at, off.wsure.at);
        CHECK(on.wcost.at >= off.total && on.wcost.at % 256 == 0 && on.wcost.bytes == 390 * 4);
        CHECK(on.weight.at >= on.wcost.at + on.wcost.bytes && on.weight.at % 256 == 0 && on.weight.bytes == 210 * 8);
        CHECK(on.start.at >= on.weight.at + on.weight.bytes && on.start.at % 256 == 0 && on.start.bytes == 210 * 4);
        CHECK(on.total >= on.start.at + on.start.bytes);
        CHECK_EQ((on.start.at - on.plan.at) % 4, 0);
    }
    std::printf("%s: %d failed checks of %lld\n", g_failed ? "FAILED" : "ok", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
