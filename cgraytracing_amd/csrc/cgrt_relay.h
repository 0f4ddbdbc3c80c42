// The sample relay of tile-order launches, in plain C++ (no HIP): how a tile's samples are cut into chunks, which workgroup of
// the launch renders which (entry, chunk), and where a split tile's values lie in the handle's relay area.  The host plans with
// these functions (cgrt_trace_grid, cgrt_hip.hip), trace_grid_kernel (cgrt_eye.hpp) maps its workgroups with the same ones, and
// tests/native/relay_map.cpp, relay_order.cpp, relay_start.cpp and relay_boost.cpp check them on the CPU.  DESIGN.md section 4.6.
//
// A lane of trace_grid_body owns a pixel and runs its samples one after the other, so a wave lasts as long as its costliest
// pixel: on a refracting sphere ~11 rays a sample, ~700 dependent scene walks at 64 samples.  The relay cuts that chain: the
// first n_split entries of tile_order_kernel's list (classes 0 and 1: some primary ray may meet a refracting sphere; with the
// mirror extent class 2 as well: relay_block_ordered) are each rendered by K workgroups, chunk c taking samples
// [c * chunk_spp, ...).  Chunk 0 sums its samples as ever; a chunk >= 1 parks every Hitpoint value f * adj in its own stream,
// in emission order; the last of the K workgroups to finish adds the streams to chunk 0's sums in chunk order -- the sequence
// of additions of the unsplit loop, so the same bits -- and stores the pixels.
#ifndef CGRT_RELAY_H
#define CGRT_RELAY_H
#include <cstddef>
#include <cstdint>

#include "cgrt_rng.hpp"  // CGRT_HD

static constexpr int kRelayMaxChunks = 4, kRelayMinChunkSpp = 16, kRelayThreads = 256;
static constexpr int kRelayDefaultChunks = 2;  // most chunks unless the launch asks for kRelayMaxChunks (measured: DESIGN.md section 6)
static constexpr int kRelayBatch = 8;  // stream slots the summing workgroup loads at a time (slots is a multiple of it)

// K and the samples of a chunk: K = min(max_chunks, spp / 16), chunk_spp = ceil(spp / K), K again from chunk_spp (the last chunk
// may be short, none is empty).  K == 1: no relay (spp < 32).
struct RelayChunks {
    int32_t k, chunk_spp;
};
CGRT_HD RelayChunks relay_chunks(int32_t spp, int32_t max_chunks = kRelayMaxChunks) {
    int32_t k = spp / kRelayMinChunkSpp;
    if (k > max_chunks) k = max_chunks;
    if (k > kRelayMaxChunks) k = kRelayMaxChunks;
    if (k < 2) return RelayChunks{1, spp};
    const int32_t cs = (spp + k - 1) / k;
    return RelayChunks{(spp + cs - 1) / cs, cs};
}
// samples [first, end) of chunk c
CGRT_HD int32_t relay_first_sample(int32_t c, int32_t chunk_spp) { return c * chunk_spp; }
CGRT_HD int32_t relay_end_sample(int32_t c, int32_t chunk_spp, int32_t spp) { return (c + 1) * chunk_spp < spp ? (c + 1) * chunk_spp : spp; }

// Slots of a parked stream: a sample's ray tree of depth max_depth ends in at most 2^(max_depth - 1) Hitpoints (every level but
// the last may double the rays; a ray at the last level ends), so chunk_spp * 2^(max_depth - 1) is never exceeded; rounded up to
// the summing loop's batch.
CGRT_HD int32_t relay_slots(int32_t chunk_spp, int32_t max_depth) {
    const int32_t s = chunk_spp << (max_depth - 1);
    return (s + kRelayBatch - 1) / kRelayBatch * kRelayBatch;
}

// Which (entry of the list, chunk) workgroup b renders: the first k * n_split workgroups are the split entries' chunks, chunk by
// chunk within an entry; the others render one unsplit entry each.  The caller drops a workgroup whose entry is beyond the list.
struct RelayBlock {
    uint32_t entry;
    int32_t chunk;
    bool split;
};
CGRT_HD RelayBlock relay_block(uint32_t b, uint32_t k, uint32_t n_split) {
    if (b < k * n_split) return RelayBlock{b / k, (int32_t)(b % k), true};
    return RelayBlock{b - (k - 1) * n_split, 0, false};
}
// Workgroups of the launch: the host does not know how many entries are of class 0 or 1 (plan[2]), so it launches for cap_split.
CGRT_HD size_t relay_grid(size_t n_tiles, int32_t k, size_t cap_split) { return n_tiles + (size_t)(k - 1) * cap_split; }

// The launch map with an extent and an order.  The extent names the split entries -- a prefix of the
// list either way, so slot = entry, the relay area and the arrival words are the same for both:
//   kRelayGlass    entries [0, min(n01, cap)): the tiles that may see a refracting sphere (classes 0 and 1; relay_block's)
//   kRelayMirror   entries [0, min(n012, cap)): the class-2 tiles -- a reflecting sphere only -- as well; where cap ends inside
//                  a class the entries beyond it are unsplit
// The order says where the workgroups of the class-2 entries [n01, n012) stand among those of the entries [0, n01); each of the
// two sequences runs through its entries ascending, a split entry's k workgroups chunk by chunk, an unsplit entry's one:
//   kRelayChunksFirst   classes 0-1, then class 2 (with kRelayGlass: relay_block)
//   kRelayMirrorFirst   class 2, then classes 0-1
//   kRelayInterleaved   merged in proportion: with a workgroups of classes 0-1 and m of class 2, position p of the merged run
//                       takes the next class-2 workgroup exactly when floor((p + 1) m / (a + m)) > floor(p m / (a + m)), so every
//                       prefix holds both kinds within one workgroup of their share
// Class 3 follows in entry order.  n01 = plan[2] <= n012 = plan[3] <= n_tiles; a workgroup beyond the list gets entry >= n_tiles
// and the caller drops it.
static constexpr int kRelayGlass = 0, kRelayMirror = 1;
static constexpr int kRelayChunksFirst = 0, kRelayMirrorFirst = 1, kRelayInterleaved = 2;
CGRT_HD uint32_t relay_split_entries(uint32_t n01, uint32_t n012, uint32_t cap, int extent) {
    const uint32_t n = extent == kRelayMirror ? n012 : n01;
    return n < cap ? n : cap;
}
CGRT_HD RelayBlock relay_block_ordered(uint32_t b, uint32_t k, uint32_t n01, uint32_t n012, uint32_t n_tiles, uint32_t cap, int extent, int order) {
    const uint32_t n_split = relay_split_entries(n01, n012, cap, extent);
    const uint32_t s_a = n_split < n01 ? n_split : n01, s_m = n_split - s_a;  // split entries of classes 0-1, of class 2
    // (32-bit throughout: t <= relay_grid, which the launch's grid dimension holds; only the interleaved product is wider)
    const uint32_t a = n01 + (k - 1) * s_a, m = (n012 - n01) + (k - 1) * s_m, t = a + m;  // workgroups of classes 0-1, of class 2
    if (b >= t) {  // class 3 (t = n012 + (k - 1) n_split), or beyond the list
        const uint32_t e = n012 + (b - t);
        return RelayBlock{e < n_tiles ? e : n_tiles, 0, false};
    }
    bool mirror;  // the workgroup is the i-th of class 2, else the i-th of classes 0-1
    uint32_t i;
    if (order == kRelayInterleaved) {
        const uint64_t pm = (uint64_t)b * m, q = pm / t;  // q = class-2 workgroups in front of position b
        mirror = pm - q * t + m >= t;
        i = mirror ? (uint32_t)q : b - (uint32_t)q;
    } else if (order == kRelayMirrorFirst) {
        mirror = b < m;
        i = mirror ? b : b - m;
    } else {
        mirror = b >= a;
        i = mirror ? b - a : b;
    }
    const uint32_t first = mirror ? n01 : 0u, s = mirror ? s_m : s_a;
    if (i < k * s) return RelayBlock{first + i / k, (int32_t)(i % k), true};
    return RelayBlock{first + (i - (k - 1) * s), 0, false};
}

// The start order by cost.  The hardware starts workgroups in index order, so index order is a list
// schedule, and a list schedule is good when the long jobs come first; the class is a poor estimate of a workgroup's length
// (within one class they differ by a factor of four to six).  A probe leaves a cost per wave tile (the wave's iterations over
// the first kRelayProbeSpp samples of its pixels: a count, the same in every run); the ITEMS are the workgroups of classes 0-2,
// exactly those relay_block_ordered gives to b < t, numbered as kRelayChunksFirst does -- entries ascending, a split entry's k
// chunks one after the other, so item order is (entry, chunk) order; an item's weight is its tile's cost (the largest of its
// waves': a workgroup lasts as long as its longest wave) times the samples it runs; the table sends workgroup b to the item of
// rank b in descending weight, ties in item order.  A total order: every rank is a count, no atomics.  Class 3 and the
// workgroups beyond the list follow as in every other form.
static constexpr int kRelayStartList = 0, kRelayStartCost = 1;  // RelayPlan::start
static constexpr int kRelayProbeSpp = 2;                        // samples of the cost probe (measured: DESIGN.md section 6)
struct RelayItems {
    uint32_t k, n01, n012, n_tiles, cap;
    int32_t extent, chunk_spp, spp;
};
CGRT_HD uint32_t relay_items_total(const RelayItems &r) {  // t: the workgroups of classes 0-2
    return r.n012 + (r.k - 1) * relay_split_entries(r.n01, r.n012, r.cap, r.extent);
}
CGRT_HD RelayBlock relay_item(uint32_t i, const RelayItems &r) {
    return relay_block_ordered(i, r.k, r.n01, r.n012, r.n_tiles, r.cap, r.extent, kRelayChunksFirst);
}
CGRT_HD uint64_t relay_item_weight(const RelayBlock &b, uint32_t tile_cost, const RelayItems &r) {
    const int32_t samples = b.split ? relay_end_sample(b.chunk, r.chunk_spp, r.spp) - relay_first_sample(b.chunk, r.chunk_spp) : r.spp;
    return (uint64_t)tile_cost * (uint64_t)(samples > 0 ? samples : 0);
}
// item j starts before item i
CGRT_HD bool relay_item_before(uint64_t wj, uint32_t j, uint64_t wi, uint32_t i) { return wj > wi || (wj == wi && j < i); }
// a word of the table, and the workgroup it names (the entries in front of n_split are the split ones)
CGRT_HD uint32_t relay_start_word(const RelayBlock &b) { return b.entry << 2 | (uint32_t)b.chunk; }
CGRT_HD RelayBlock relay_start_block(uint32_t word, uint32_t n_split) { return RelayBlock{word >> 2, (int32_t)(word & 3u), (word >> 2) < n_split}; }
static_assert(kRelayMaxChunks <= 4, "a table word holds the chunk in two bits");
// Tiles a table can name (entry << 2 in a word) and workgroups it may have to hold: the host knows neither n01 nor n012
static constexpr size_t kRelayStartMaxTiles = (size_t)1 << 30;
CGRT_HD size_t relay_start_words(size_t n_tiles, int32_t k, size_t cap_split) { return relay_grid(n_tiles, k, cap_split); }
// The cost of tile `tile` (ty * tiles_x + tx) from its wave tiles' costs: 2 x 2 wave tiles of 16x4 pixels, those inside the grid
CGRT_HD uint32_t relay_tile_cost(const uint32_t *wcost, uint32_t tile, uint32_t tiles_x, uint32_t wtiles_x, uint32_t wtiles_y) {
    const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
    uint32_t c = 0;
    for (uint32_t w = 0; w < 4; w++) {
        const uint32_t wx = 2 * tx + (w & 1u), wy = 2 * ty + (w >> 1);
        if (wx < wtiles_x && wy < wtiles_y && wcost[wy * wtiles_x + wx] > c) c = wcost[wy * wtiles_x + wx];
    }
    return c;
}
// The whole table on the host (the device spreads the same counts over workgroups: relay_start_kernel): weight[i] of item i,
// start[rank] = its word.  Both arrays hold relay_items_total words.
inline void relay_start_table(const RelayItems &r, const uint32_t *list, const uint32_t *wcost, uint32_t tiles_x, uint32_t wtiles_x,
                              uint32_t wtiles_y, uint64_t *weight, uint32_t *start) {
    const uint32_t t = relay_items_total(r);
    for (uint32_t i = 0; i < t; i++) {
        const RelayBlock b = relay_item(i, r);
        weight[i] = relay_item_weight(b, relay_tile_cost(wcost, list[b.entry], tiles_x, wtiles_x, wtiles_y), r);
    }
    for (uint32_t i = 0; i < t; i++) {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < t; j++) rank += relay_item_before(weight[j], j, weight[i], i) ? 1u : 0u;
        start[rank] = relay_start_word(relay_item(i, r));
    }
}

// Four chunks for the heaviest tiles ("Promotion").  The start order cannot shorten an item, and the
// frame ends with the long items that found a slot late; a launch that starts by cost therefore renders the split entries whose
// items are long -- the PROMOTED ones -- by k_boost = relay_chunks(spp, kRelayMaxChunks).k workgroups instead of k, the others
// as before.  Entry e < n_split (a split entry) is a CANDIDATE when
//     cost_e * base chunk samples * slots * den  >  num * S,     S = sum of cost_e * spp over the entries of classes 0-2,
// that is when its base item alone would hold one of the device's `slots` workgroup slots for more than num/den of the frame's
// even share S / slots.  Integers throughout (64 bits: probe costs are iteration counts of a few samples, far below 2^32, num
// and den at most kRelayBoostMaxTerm), so host and device find the same set.  Promoted tiles park in an area of their own that
// holds `cap` of them: the candidates are ranked by cost, descending, ties in entry order (relay_item_before), the first `cap`
// are promoted, and a promoted entry's rank is its slot in that area.  bslot[e] = slot + 1, 0 for an entry that is not promoted:
// a word per split entry in the order buffer, which is how a workgroup learns its tile's form.
// The items of the table are then, in (entry, chunk) order, a promoted entry's k_boost chunks of boost chunk_spp samples, any
// other split entry's k chunks, an unsplit entry's one; weight and total order as above.  The ranking kernels number them by the
// VIRTUAL index v = entry * k_boost + chunk, chunks an entry has not being skipped: the same order without a prefix sum.
static constexpr uint32_t kRelayBoostMaxTerm = 4096;            // num and den of the threshold
static constexpr uint32_t kRelayBoostNum = 3, kRelayBoostDen = 4;  // the default threshold (measured: DESIGN.md section 6)
static constexpr uint64_t kRelayNoItem = ~(uint64_t)0;          // weight of a virtual index that is no item
// (a word per split entry rather than a bit of the table word: the workgroup needs the tile's boost slot, not only the fact)
static_assert(kRelayStartMaxTiles <= ((size_t)1 << 32) - 1, "bslot[e] = boost slot + 1 <= tiles of a table, in a 32-bit word");
struct RelayBoost {
    uint32_t k, cap;    // chunks of a promoted tile; tiles the boost area holds
    int32_t chunk_spp;  // samples of a promoted tile's chunk
    uint32_t num, den, slots;
};
CGRT_HD bool relay_boost_candidate(uint32_t cost, const RelayItems &r, const RelayBoost &b, uint64_t S) {
    return b.k > r.k && (uint64_t)cost * (uint64_t)r.chunk_spp * (uint64_t)b.slots * (uint64_t)b.den > (uint64_t)b.num * S;
}
// the ranking key of a split entry among the candidates: 0 stands before nothing and is no candidate
CGRT_HD uint64_t relay_boost_key(bool candidate, uint32_t cost) { return candidate ? (uint64_t)cost + 1u : 0u; }
// chunks of entry e, and the samples of its chunk c
CGRT_HD uint32_t relay_boost_chunks(uint32_t e, bool promoted, uint32_t n_split, const RelayItems &r, const RelayBoost &b) {
    return promoted ? b.k : e < n_split ? r.k : 1u;
}
CGRT_HD uint64_t relay_boost_weight(uint32_t c, uint32_t chunks, bool promoted, uint32_t cost, const RelayItems &r, const RelayBoost &b) {
    if (c >= chunks) return kRelayNoItem;
    const int32_t cs = promoted ? b.chunk_spp : r.chunk_spp;
    const int32_t samples = chunks > 1 ? relay_end_sample((int32_t)c, cs, r.spp) - relay_first_sample((int32_t)c, cs) : r.spp;
    return (uint64_t)cost * (uint64_t)(samples > 0 ? samples : 0);
}
// virtual index j stands before virtual index i (both with their weights)
CGRT_HD bool relay_boost_before(uint64_t wj, uint32_t j, uint64_t wi, uint32_t i) { return wj != kRelayNoItem && relay_item_before(wj, j, wi, i); }
// items of the table with `promoted` promoted entries, and the words a launch must hold for them (the host knows no count)
CGRT_HD uint32_t relay_boost_items(const RelayItems &r, const RelayBoost &b, uint32_t promoted) { return relay_items_total(r) + (b.k - r.k) * promoted; }
CGRT_HD size_t relay_boost_extra(int32_t k, int32_t k_boost, size_t cap_boost) { return (size_t)(k_boost - k) * cap_boost; }
// The whole computation on the host (the device: relay_boost_*_kernel, cgrt_eye.hpp).  bslot holds n_split words, weight and
// start relay_items_total(r) + relay_boost_extra(r.k, b.k, min(b.cap, n_split)) at most; returns S, the promoted entries and
// the items.  Nothing promoted: relay_start_table's table, word for word.
struct RelayBoosted {
    uint64_t S;
    uint32_t promoted, items;
};
inline RelayBoosted relay_boost_table(const RelayItems &r, const RelayBoost &b, const uint32_t *list, const uint32_t *wcost, uint32_t tiles_x,
                                      uint32_t wtiles_x, uint32_t wtiles_y, uint32_t *bslot, uint64_t *weight, uint32_t *start) {
    const uint32_t n_split = relay_split_entries(r.n01, r.n012, r.cap, r.extent);
    RelayBoosted out{0, 0, 0};
    for (uint32_t e = 0; e < r.n012; e++) out.S += (uint64_t)relay_tile_cost(wcost, list[e], tiles_x, wtiles_x, wtiles_y) * (uint64_t)r.spp;
    const auto key = [&](uint32_t e) {
        const uint32_t c = relay_tile_cost(wcost, list[e], tiles_x, wtiles_x, wtiles_y);
        return relay_boost_key(relay_boost_candidate(c, r, b, out.S), c);
    };
    for (uint32_t e = 0; e < n_split; e++) {
        const uint64_t ke = key(e);
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n_split; j++) rank += relay_item_before(key(j), j, ke, e) ? 1u : 0u;
        bslot[e] = ke != 0 && rank < b.cap ? rank + 1u : 0u;
        out.promoted += bslot[e] ? 1u : 0u;
    }
    // the items in (entry, chunk) order, then every item's rank
    uint32_t t = 0;
    for (uint32_t e = 0; e < r.n012; e++) {
        const bool p = e < n_split && bslot[e] != 0;
        const uint32_t kc = relay_boost_chunks(e, p, n_split, r, b), cost = relay_tile_cost(wcost, list[e], tiles_x, wtiles_x, wtiles_y);
        for (uint32_t c = 0; c < kc; c++) {
            weight[t] = relay_boost_weight(c, kc, p, cost, r, b);
            start[t++] = relay_start_word(RelayBlock{e, (int32_t)c, kc > 1});  // (parked here, ranked below)
        }
    }
    out.items = t;
    uint32_t *word = new uint32_t[t ? t : 1];
    for (uint32_t i = 0; i < t; i++) word[i] = start[i];
    for (uint32_t i = 0; i < t; i++) {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < t; j++) rank += relay_item_before(weight[j], j, weight[i], i) ? 1u : 0u;
        start[rank] = word[i];
    }
    delete[] word;
    return out;
}
// The boost area: relay_layout(cap, k_boost, slots) behind the base area in the handle's buffer, 3 GiB at most, both areas
// together within an eighth of the device's memory; bound >= 0 (CGRT_RELAY_BOOST_TILES): at most that many tiles
static constexpr size_t kRelayBoostBudget = (size_t)3 << 30;
CGRT_HD size_t relay_boost_budget(size_t mem_total, size_t base_bytes) {
    const size_t left = mem_total / 8 > base_bytes ? mem_total / 8 - base_bytes : 0;
    return left < kRelayBoostBudget ? left : kRelayBoostBudget;
}

// The relay area for cap_split tiles, 256 threads a tile (thread t = pixel t of the tile), array after array:
//   arrive[cap]                     uint32   workgroups of the tile that are through (0 between launches), padded to 256 bytes
//   racc  [cap][3][256]             double   chunk 0's sums r, g, b
//   rhits [cap][k][256]             uint32   Hitpoints of each chunk
//   rcount[cap][k-1][256]           uint32   values parked by chunk c >= 1
//   rvals [cap][k-1][slots][3][256] double   chunk c's stream: value i of pixel t at [i][0..2][t]
struct RelayLayout {
    size_t racc, rhits, rcount, rvals, total;  // byte offsets; arrive is at 0
};
CGRT_HD size_t relay_tile_bytes(int32_t k, int32_t slots) {
    const size_t t = kRelayThreads;
    return sizeof(uint32_t) + 3 * t * sizeof(double) + (size_t)k * t * sizeof(uint32_t) + (size_t)(k - 1) * t * sizeof(uint32_t) +
           (size_t)(k - 1) * (size_t)slots * 3 * t * sizeof(double);
}
CGRT_HD RelayLayout relay_layout(size_t cap, int32_t k, int32_t slots) {
    const size_t t = kRelayThreads;
    RelayLayout l;
    l.racc = (cap * sizeof(uint32_t) + 255) & ~(size_t)255;
    l.rhits = l.racc + cap * 3 * t * sizeof(double);
    l.rcount = l.rhits + cap * (size_t)k * t * sizeof(uint32_t);
    l.rvals = l.rcount + cap * (size_t)(k - 1) * t * sizeof(uint32_t);
    l.total = l.rvals + cap * (size_t)(k - 1) * (size_t)slots * 3 * t * sizeof(double);
    return l;
}
// Tiles the area may hold: 4 GiB, at most an eighth of the device's memory; bound > 0 (CGRT_RELAY_TILES): at most that many
static constexpr size_t kRelayBudget = (size_t)4 << 30;
CGRT_HD size_t relay_budget(size_t mem_total) { return mem_total / 8 < kRelayBudget ? mem_total / 8 : kRelayBudget; }
CGRT_HD size_t relay_cap(size_t n_tiles, int32_t k, int32_t slots, size_t budget, long long bound = 0) {
    size_t cap = budget / relay_tile_bytes(k, slots);
    if (cap > n_tiles) cap = n_tiles;
    if (bound > 0 && cap > (size_t)bound) cap = (size_t)bound;
    while (cap > 0 && relay_layout(cap, k, slots).total > budget) cap--;  // (the arrival words' padding)
    return cap;
}

#endif
