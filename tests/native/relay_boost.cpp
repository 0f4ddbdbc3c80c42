// Four chunks for the relay's heaviest tiles (cgrt_relay.h, "Four chunks for the heaviest tiles"), which the host, the
// relay_boost_*_kernel launches and the GPU test share.  For every case the promoted set is recomputed from the rule's own words
// -- candidates by the integer threshold, the heaviest first, ties in entry order, as many as the boost area holds -- the table
// is a permutation of exactly the (entry, chunk) items that set defines, every sample of every tile lies in exactly one item,
// weights do not increase and ties stand in (entry, chunk) order, nothing is written beyond the item count, and the kernels' own
// way of counting (a workgroup's worth at a time, over virtual items) gives the same slots and the same table.  Nothing
// promoted: relay_start_table's table, word for word.  Then the frame plan's part.  CPU build under ASan + UBSan, driven by
// tests/test_relay_boost_host.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "cgrt_frame.h"

static int g_failed = 0;
static long long g_checks = 0;
static char g_case[240] = "";
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

enum Costs { Varied, Equal, SomeZero };
enum Threshold { All, Mid, None };  // 0/1; a value with both kinds present (where the costs differ); above every weight

// tiles_x x tiles_y tiles whose last column and row of wave tiles are missing; cap_boost < 0: room for every split entry.
// Returns the promoted entries.
static uint32_t one_case(uint32_t tiles_x, uint32_t tiles_y, uint32_t n01, uint32_t n012, uint32_t cap, int extent, int spp, Costs costs, Threshold th,
                         long long cap_boost) {
    const uint32_t n_tiles = tiles_x * tiles_y, wtiles_x = 2 * tiles_x - 1, wtiles_y = 2 * tiles_y - 1, slots = 1024;
    const RelayChunks rc = relay_chunks(spp, kRelayDefaultChunks), rb = relay_chunks(spp, kRelayMaxChunks);
    std::snprintf(g_case, sizeof g_case, "tiles %ux%u n01 %u n012 %u cap %u extent %d spp %d (%d x %d, boost %d x %d) costs %d threshold %d boost cap %lld",
                  tiles_x, tiles_y, n01, n012, cap, extent, spp, rc.k, rc.chunk_spp, rb.k, rb.chunk_spp, (int)costs, (int)th, cap_boost);
    CHECK_EQ(rc.k, 2);
    const RelayItems r{(uint32_t)rc.k, n01, n012, n_tiles, cap, extent, rc.chunk_spp, spp};
    std::vector<uint32_t> list(n_tiles), wcost((size_t)wtiles_x * wtiles_y);
    for (uint32_t e = 0; e < n_tiles; e++) list[e] = (e * 11u + 3u) % n_tiles;  // (11 is coprime to every n_tiles used)
    uint32_t x = 12345u;
    for (uint32_t &c : wcost) {
        x = x * 1664525u + 1013904223u;
        c = costs == Equal ? 9u : costs == SomeZero ? ((x >> 16) % 3u ? (x >> 20) % 5u : 0u) : 1u + (x >> 12) % 200u;
    }
    const uint32_t n_split = relay_split_entries(n01, n012, cap, extent), t0 = relay_items_total(r);
    std::vector<uint32_t> cost(n012);
    uint64_t S = 0;
    for (uint32_t e = 0; e < n012; e++) {
        cost[e] = relay_tile_cost(wcost.data(), list[e], tiles_x, wtiles_x, wtiles_y);
        S += (uint64_t)cost[e] * (uint64_t)spp;
    }
    // the threshold: cost * chunk_spp * slots * den > num * S
    uint32_t num = 0, den = 1;
    if (th == None) {  // the largest cost fails it: num / den = 4096 / 1 holds up to S >= cost * chunk_spp / 4, else no cost is positive
        num = kRelayBoostMaxTerm;
        for (uint32_t e = 0; e < n_split; e++)
            if ((uint64_t)cost[e] * rc.chunk_spp * slots > (uint64_t)num * S) return 0;  // (a list this small has no such threshold: skipped)
    } else if (th == Mid) {  // the median cost of the split entries: cost * chunk_spp * slots * den > num * S  <=>  cost > median, with den = S, scaled into range
        std::vector<uint32_t> sorted(cost.begin(), cost.begin() + n_split);
        std::sort(sorted.begin(), sorted.end());
        const uint64_t med = n_split ? sorted[n_split / 2] : 0;
        // num / den ~ med * chunk_spp * slots / S, as a fraction with den <= 4096 (rounded down: the median itself may pass)
        den = kRelayBoostMaxTerm;
        const auto num_at = [&](uint32_t d) { return S ? med * (uint64_t)rc.chunk_spp * slots * d / S : 0; };
        while (den > 1 && num_at(den) > kRelayBoostMaxTerm) den /= 2;
        if (num_at(den) > kRelayBoostMaxTerm) return 0;  // (the list is too small for such a threshold: skipped)
        num = (uint32_t)num_at(den);
    }
    const uint32_t bcap = cap_boost < 0 ? n_split : (uint32_t)cap_boost;
    const RelayBoost b{(uint32_t)rb.k, bcap, rb.chunk_spp, num, den, slots};

    // ---- the rule, in its own words
    std::vector<uint32_t> cand;
    for (uint32_t e = 0; e < n_split; e++)
        if (rb.k > rc.k && (unsigned __int128)cost[e] * (unsigned)rc.chunk_spp * slots * den > (unsigned __int128)num * S) cand.push_back(e);
    std::stable_sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t c) { return cost[a] > cost[c]; });  // heaviest first, ties in entry order
    std::vector<uint32_t> want_slot(n_split + 1, 0);
    for (uint32_t i = 0; i < cand.size() && i < bcap; i++) want_slot[cand[i]] = i + 1;
    const uint32_t want_promoted = (uint32_t)std::min<size_t>(cand.size(), bcap);
    std::map<std::pair<uint32_t, int>, uint64_t> want;  // item -> weight
    for (uint32_t e = 0; e < n012; e++) {
        const bool p = e < n_split && want_slot[e];
        const int kc = p ? rb.k : e < n_split ? rc.k : 1, cs = p ? rb.chunk_spp : rc.chunk_spp;
        std::vector<int> seen(spp, 0);
        for (int c = 0; c < kc; c++) {
            const int s0 = kc > 1 ? c * cs : 0, s1 = kc > 1 ? std::min((c + 1) * cs, spp) : spp;
            CHECK(s0 < s1);
            for (int s = s0; s < s1; s++) seen[s]++;
            want[{e, c}] = (uint64_t)cost[e] * (uint64_t)(s1 - s0);
        }
        for (int s = 0; s < spp; s++) CHECK_EQ(seen[s], 1);  // every sample in exactly one item
    }

    // ---- the host function
    const size_t most = t0 + relay_boost_extra(rc.k, rb.k, std::min(bcap, n_split));
    std::vector<uint64_t> weight(most + 1, 0x5555555555555555ull);
    std::vector<uint32_t> start(most + 1, 0xaaaaaaaau), bslot(n_split + 1, 0xaaaaaaaau);
    const RelayBoosted out = relay_boost_table(r, b, list.data(), wcost.data(), tiles_x, wtiles_x, wtiles_y, bslot.data(), weight.data(), start.data());
    CHECK(out.S == S);
    CHECK_EQ(out.promoted, want_promoted);
    CHECK_EQ(out.items, want.size());
    CHECK_EQ(out.items, relay_boost_items(r, b, out.promoted));
    CHECK(out.items <= most);
    CHECK_EQ(bslot[n_split], 0xaaaaaaaau);
    for (uint32_t e = 0; e < n_split; e++) CHECK_EQ(bslot[e], want_slot[e]);
    for (size_t i = out.items; i <= most; i++) {  // nothing beyond the item count
        CHECK_EQ(start[i], 0xaaaaaaaau);
        CHECK(weight[i] == 0x5555555555555555ull);
    }
    std::map<std::pair<uint32_t, int>, int> got;
    uint64_t prev_w = ~0ull;
    long long prev_key = -1;
    for (uint32_t i = 0; i < out.items; i++) {
        const RelayBlock blk = relay_start_block(start[i], n_split);
        CHECK(blk.entry < n012);
        const auto it = want.find({blk.entry, blk.chunk});
        CHECK(it != want.end());
        if (it == want.end()) continue;
        got[{blk.entry, blk.chunk}] += 1;
        const long long key = (long long)blk.entry * 4 + blk.chunk;
        CHECK(it->second <= prev_w);
        if (it->second == prev_w) CHECK(key > prev_key);
        prev_w = it->second;
        prev_key = key;
    }
    CHECK_EQ(got.size(), want.size());
    for (const auto &g : got) CHECK_EQ(g.second, 1);
    if (out.promoted == 0) {  // the table without promotion, word for word
        std::vector<uint64_t> w0(t0 + 1);
        std::vector<uint32_t> s0(t0 + 1);
        relay_start_table(r, list.data(), wcost.data(), tiles_x, wtiles_x, wtiles_y, w0.data(), s0.data());
        CHECK_EQ(out.items, t0);
        for (uint32_t i = 0; i < t0 && i < out.items; i++) CHECK_EQ(start[i], s0[i]);
    }

    // ---- the kernels' counts: relay_boost_promote_kernel (keys a batch at a time), relay_boost_weight_kernel and
    // relay_boost_start_kernel (virtual items v = entry * k_boost + chunk)
    const auto blocks = [](size_t n) { return (uint32_t)((n + kRelayThreads - 1) / kRelayThreads); };
    std::vector<uint32_t> bslot2(n_split + 1, 0xaaaaaaaau);
    uint32_t promoted2 = 0;
    for (uint32_t blk = 0; blk < blocks(cap); blk++) {
        if (blk * kRelayThreads >= n_split) continue;
        for (uint32_t tid = 0; tid < (uint32_t)kRelayThreads; tid++) {
            const uint32_t e = blk * kRelayThreads + tid, ce = e < n_split ? cost[e] : 0u;
            const uint64_t ke = relay_boost_key(e < n_split && relay_boost_candidate(ce, r, b, S), ce);
            uint32_t rank = 0;
            for (uint32_t j0 = 0; j0 < n_split; j0 += kRelayThreads) {
                const uint32_t n = std::min((uint32_t)kRelayThreads, n_split - j0);
                for (uint32_t u = 0; u < n; u++)
                    rank += relay_item_before(relay_boost_key(relay_boost_candidate(cost[j0 + u], r, b, S), cost[j0 + u]), j0 + u, ke, e) ? 1u : 0u;
            }
            if (e >= n_split) continue;
            const bool p = ke != 0 && rank < b.cap;
            bslot2[e] = p ? rank + 1u : 0u;
            promoted2 += p ? 1u : 0u;
        }
    }
    for (uint32_t e = 0; e <= n_split; e++) CHECK_EQ(bslot2[e], bslot[e]);
    CHECK_EQ(promoted2, out.promoted);
    const uint32_t nv = n012 * b.k;
    std::vector<uint64_t> vw(nv + 1, kRelayNoItem);
    for (uint32_t v = 0; v < nv; v++) {
        const uint32_t e = v / b.k, c = v % b.k;
        const bool p = e < n_split && bslot2[e] != 0u;
        vw[v] = relay_boost_weight(c, relay_boost_chunks(e, p, n_split, r, b), p, cost[e], r, b);
    }
    std::vector<uint32_t> start2(most + 1, 0xaaaaaaaau);
    for (uint32_t blk = 0; blk < blocks((size_t)n_tiles * b.k); blk++) {
        if (blk * kRelayThreads >= nv) continue;
        for (uint32_t tid = 0; tid < (uint32_t)kRelayThreads; tid++) {
            const uint32_t v = blk * kRelayThreads + tid;
            const uint64_t wv = v < nv ? vw[v] : kRelayNoItem;
            uint32_t rank = 0;
            for (uint32_t j0 = 0; j0 < nv; j0 += kRelayThreads) {
                const uint32_t n = std::min((uint32_t)kRelayThreads, nv - j0);
                for (uint32_t u = 0; u < n; u++) rank += relay_boost_before(vw[j0 + u], j0 + u, wv, v) ? 1u : 0u;
            }
            if (wv == kRelayNoItem) continue;
            CHECK(rank < out.items);
            if (rank < out.items) start2[rank] = relay_start_word(RelayBlock{v / b.k, (int32_t)(v % b.k), false});
        }
    }
    for (size_t i = 0; i <= most; i++) CHECK_EQ(start2[i], start[i]);
    return out.promoted;
}

static FrameInputs spheres(int W = 200, int rows = 117, int spp = 32) {  // (frame_plan_start.cpp's)
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

static void frame_plan_part() {
    std::snprintf(g_case, sizeof g_case, "frame plan");
    {   // the headline frame promotes by default; everything the plan had keeps its value
        const FramePlan p = frame_plan(spheres(1920, 1080, 64), 0);
        FrameInputs off = spheres(1920, 1080, 64);
        off.grid.flags = CGRT_GRID_NO_RELAY_BOOST;
        const FramePlan q = frame_plan(off, 0);
        CHECK_EQ(p.relay.boosts(), 1);
        CHECK_EQ(q.relay.boosts(), 0);
        CHECK_EQ(p.relay.boost.k, 4);
        CHECK_EQ(p.relay.boost.chunk_spp, 16);
        CHECK_EQ(p.relay.boost.slots, relay_slots(16, 5));
        CHECK_EQ(p.relay.wg_slots, 1024);
        CHECK_EQ(p.relay.num, kRelayBoostNum);
        CHECK_EQ(p.relay.den, kRelayBoostDen);
        CHECK(p.relay.boost.cap > 0 && p.relay.boost.cap <= p.relay.base.cap);
        CHECK_EQ(p.relay.boost.cap, relay_cap(p.relay.base.cap, 4, p.relay.boost.slots, kRelayBoostBudget));
        CHECK(p.relay.boost.bytes <= kRelayBoostBudget && align256(p.relay.base.bytes) + p.relay.boost.bytes <= spheres().mem_total / 8);
        CHECK_EQ(p.relay.boost_words, 2 * p.relay.boost.cap);
        CHECK_EQ(p.relay.grid(p.grid_dim, true) - p.relay.grid(p.grid_dim, false), 2 * p.relay.boost.cap);
        for (const FramePlan *f : {&p, &q}) {
            CHECK_EQ(f->relay.base.k, 2);
            CHECK_EQ(f->relay.base.chunk_spp, 32);
            CHECK_EQ(f->relay.start, kRelayStartCost);
            CHECK_EQ(f->relay.order, kRelayInterleaved);
            CHECK_EQ(f->relay.extent, kRelayMirror);
            CHECK_EQ(f->grid_dim, 8100);
            CHECK_EQ(f->relay.start_words, relay_grid(f->grid_dim, f->relay.base.k, f->relay.base.cap));
        }
        CHECK_EQ(p.relay.base.cap, q.relay.base.cap);
        CHECK_EQ(p.relay.base.bytes, q.relay.base.bytes);
        // the order buffer: the new parts lie behind the old ones, which do not move
        const TileOrderLayout a = tile_order_layout(8100, p.n_wt, true, p.relay.start_words),
                              c = tile_order_layout(8100, p.n_wt, true, p.relay.start_words, p.relay.boost_words, p.relay.base.cap, p.relay.boost.k);
        CHECK_EQ(a.boost.bytes + a.ecost.bytes + a.bweight.bytes + a.bstart.bytes, 0);
        CHECK_EQ(c.start.at, a.start.at);
        CHECK_EQ(c.wcost.at, a.wcost.at);
        CHECK_EQ(c.weight.at, a.weight.at);
        CHECK(c.boost.at >= a.total && c.boost.at % 256 == 0 && c.boost.bytes == (kBoostHead + p.relay.base.cap) * 4);
        CHECK(c.ecost.at >= c.boost.at + c.boost.bytes && c.ecost.bytes == 8100 * 4);
        CHECK(c.bweight.at >= c.ecost.at + c.ecost.bytes && c.bweight.at % 8 == 0 && c.bweight.bytes == 8100 * 4 * 8);
        CHECK(c.bstart.at >= c.bweight.at + c.bweight.bytes && c.bstart.bytes == (p.relay.start_words + p.relay.boost_words) * 4);
        CHECK(c.total >= c.bstart.at + c.bstart.bytes);
    }
    for (int spp : {32, 40}) {  // k_boost == relay_k: nothing to promote to, asked for or not
        FrameInputs in = spheres(1920, 1080, spp);
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        in.grid.flags = CGRT_GRID_RELAY_BOOST;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartCost);
    }
    {   // 48 samples: three chunks
        const FramePlan p = frame_plan(spheres(1920, 1080, 48), 0);
        CHECK_EQ(p.relay.boosts(), 1);
        CHECK_EQ(p.relay.boost.k, 3);
        CHECK_EQ(p.relay.boost.chunk_spp, 16);
        CHECK_EQ(p.relay.base.k, 2);
    }
    {   // flags and knob, flags before the knob; off wins
        FrameInputs in = spheres(1920, 1080, 64);
        in.knobs.relay_boost_off = true;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        in.grid.flags = CGRT_GRID_RELAY_BOOST;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 1);
        in.grid.flags = CGRT_GRID_RELAY_BOOST | CGRT_GRID_NO_RELAY_BOOST;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        in.knobs.relay_boost_off = false;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        in.grid.flags = 0;
        in.knobs.relay_boost_num = 3;
        in.knobs.relay_boost_den = 8;
        CHECK_EQ(frame_plan(in, 0).relay.num, 3);
        CHECK_EQ(frame_plan(in, 0).relay.den, 8);
        in.knobs.relay_boost_tiles = 5;
        CHECK_EQ(frame_plan(in, 0).relay.boost.cap, 5);
        in.knobs.relay_boost_tiles = 0;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
    }
    {   // a cost start asked for by flag or knob is not the default launch: promotion has to be asked for too
        FrameInputs in = spheres(1920, 1080, 64);
        in.grid.flags = CGRT_GRID_RELAY_COST_START;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartCost);
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        in.grid.flags = CGRT_GRID_RELAY_COST_START | CGRT_GRID_RELAY_BOOST;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 1);
        in.grid.flags = CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_RELAY_COST_START | CGRT_GRID_RELAY_BOOST;
        in.grid.width = 200;
        in.grid.height = in.grid.rows = 117;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 1);
    }
    {   // a list start never promotes
        FrameInputs in = spheres(1920, 1080, 64);
        in.grid.flags = CGRT_GRID_NO_RELAY_COST_START | CGRT_GRID_RELAY_BOOST;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        in.grid.flags = CGRT_GRID_RELAY_INTERLEAVED | CGRT_GRID_RELAY_BOOST;
        CHECK_EQ(frame_plan(in, 0).relay.start, kRelayStartList);
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
        in.grid.flags = CGRT_GRID_NO_SAMPLE_RELAY | CGRT_GRID_RELAY_BOOST;
        CHECK_EQ(frame_plan(in, 0).relay.boosts(), 0);
    }
    {   // the knob's values
        bool off = false;
        uint32_t num = 7, den = 9;
        CHECK(relay_boost_named("", off, num, den) && !off && num == 7 && den == 9);
        CHECK(relay_boost_named("3/8", off, num, den) && !off && num == 3 && den == 8);
        CHECK(relay_boost_named("0/1", off, num, den) && num == 0 && den == 1);
        for (const char *bad : {"1/0", "x", "1/", "/2", "-1/2", "1/2/3", "5000/1", "1/5000", "0.5", "1 /2"}) {
            num = 7, den = 9;
            CHECK(!relay_boost_named(bad, off, num, den) && !off && num == 7 && den == 9);
        }
        CHECK(relay_boost_named("off", off, num, den) && off);
    }
}

int main() {
    struct Plan { uint32_t n01, n012; };
    for (const auto &dims : {std::pair<uint32_t, uint32_t>{7, 15}, {4, 7}, {1, 1}}) {
        const uint32_t n = dims.first * dims.second;
        const Plan plans[] = {{0, 0}, {0, n / 3}, {n / 4, n / 4}, {n / 5, n / 2}, {n / 3, n}, {n, n}};
        for (const Plan &pl : plans) {
            const uint32_t caps[] = {0, pl.n01, pl.n01 + (pl.n012 - pl.n01) / 2, n};
            for (uint32_t cap : caps)
                for (int extent : {kRelayGlass, kRelayMirror})
                    for (int spp : {64, 70, 48, 40})
                        for (Costs c : {Varied, Equal, SomeZero})
                            for (Threshold th : {All, Mid, None}) {
                                const uint32_t promoted = one_case(dims.first, dims.second, pl.n01, pl.n012, cap, extent, spp, c, th, -1);
                                if (spp == 40 || th == None) CHECK_EQ(promoted, 0);
                                // 0/1: every split entry (the comparison is strict: but for an entry of cost 0, which weighs nothing)
                                if (spp != 40 && th == All && c != SomeZero) CHECK_EQ(promoted, relay_split_entries(pl.n01, pl.n012, cap, extent));
                                if (spp != 40 && th == All) CHECK(promoted <= relay_split_entries(pl.n01, pl.n012, cap, extent));
                                // a boost area for no tile, for one, and ending inside the promoted set
                                for (long long bc : {0ll, 1ll, (long long)promoted / 2})
                                    if (bc < (long long)promoted || bc == 0) CHECK_EQ(one_case(dims.first, dims.second, pl.n01, pl.n012, cap, extent, spp, c, th, bc), bc);
                            }
        }
    }
    // both kinds present at the mid threshold of a varied list
    {
        const uint32_t p = one_case(7, 15, 21, 52, 105, kRelayMirror, 64, Varied, Mid, -1);
        CHECK(p > 0 && p < 52);
    }
    // more virtual items than one workgroup of the ranking kernels holds, and than nine
    for (int spp : {64, 70, 48, 40}) {
        const uint32_t p = one_case(30, 20, 150, 400, 600, kRelayMirror, spp, Varied, Mid, -1);
        CHECK(spp == 40 ? p == 0 : (p > 0 && p < 400));
        one_case(30, 20, 150, 400, 300, kRelayMirror, spp, SomeZero, All, 77);
        one_case(30, 20, 256, 256, 256, kRelayGlass, spp, Equal, All, 100);
    }
    frame_plan_part();
    std::printf("%s: %d failed checks of %lld\n", g_failed ? "FAILED" : "ok", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
