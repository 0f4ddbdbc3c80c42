// The wavefront trace's plan (cgrt_wavefront_plan.h) on the CPU: the sort key against a recursive depth-first walk over the
// leaf sets of random binary trees to depth 31 and at its boundaries, its inverse, the capacities from work_bytes, the default
// work memory, the slice schedule under scripted overflows, and the launch plan of a level (cgrt_rays_plan.h:
// RaysKind::Wavefront) against the nearest-hit query's over the trait sweep of rays_plan.cpp, with the literal kernel names.
// CPU build under ASan + UBSan, driven by tests/test_wavefront_plan_host.py.
#define RAYS_PLAN_NO_MAIN
#include "rays_plan.cpp"

#include <algorithm>
#include <cstdint>
#include <functional>
#include <random>
#include <vector>

#include "cgrt_wavefront_plan.h"

// the leaves of a random binary tree below `path` in emission order: reflected subtree (2p) before the refracted one (2p + 1)
static void grow(std::mt19937_64 &rng, uint32_t path, int level, int max_level, double p_split, double p_one, std::vector<uint32_t> &dfs) {
    const double u = std::uniform_real_distribution<double>(0, 1)(rng);
    if (level == max_level || u >= p_split + p_one || dfs.size() > 50000) {  // a leaf: a Hitpoint
        dfs.push_back(path);
        return;
    }
    grow(rng, path * 2, level + 1, max_level, p_split, p_one, dfs);  // the reflected child always exists
    if (u < p_split) grow(rng, path * 2 + 1, level + 1, max_level, p_split, p_one, dfs);
}

// emission_order() of tests/test_gpu_bounce.py for one root: the bits behind the leading 1, left-aligned in 32 bits
static uint64_t numpy_aligned(uint32_t path) {
    int ln = 0;
    for (int b = 1; b < 32; b++) ln += (path >> b) > 0;
    return ((uint64_t)path - (1ull << ln)) << (32 - ln);
}

static long long run_slices(long long n, long long cap_rays, const std::function<bool(long long, long long)> &overflows, bool *failed,
                            int *slices, int *halvings) {
    WavefrontSlices sl(n, WavefrontCaps{cap_rays, 1});
    long long next = 0, covered = 0;
    int guard = 0;
    while (!sl.done() && guard++ < 100000) {
        const long long b = sl.begin, c = sl.count();
        CHECK_EQ(b, next);  // in order, nothing skipped, nothing twice
        CHECK_EQ(c >= 1 && b + c <= n, 1);
        if (overflows(b, c)) {
            const bool one = c <= 1;
            const bool again = sl.overflowed();
            CHECK_EQ(again, !one);  // CGRT_ERR_LIMIT exactly when a one-root slice overflows
            if (again) CHECK_EQ(sl.count() < c && sl.count() >= 1 && sl.begin == b, 1);
            continue;
        }
        sl.finished();
        next = b + c;
        covered += c;
    }
    *failed = sl.failed;
    *slices = sl.slices;
    *halvings = sl.halvings;
    return covered;
}

int main() {
    std::mt19937_64 rng(20240611);
    // ---- the key orders exactly as the depth-first walk, and as emission_order's aligned bit strings ----
    long long trees = 0, leaves = 0, deepest = 0;
    for (int t = 0; t < 4000; t++) {
        std::vector<uint32_t> dfs;
        const int max_level = 1 + (int)(rng() % 31);  // levels 1..31: paths below 2^31
        // mean children per ray 1.08 or 1.15: most trees reach their last level with tens of leaves, some end early
        const double p_split = t % 4 == 0 ? 0.2 : 0.1, p_one = t % 4 == 0 ? 0.75 : 0.88;
        grow(rng, 1u, 1, max_level, p_split, p_one, dfs);
        trees++;
        leaves += (long long)dfs.size();
        const uint32_t root = t % 5 == 0 ? 0u : t % 5 == 1 ? 0x7FFFFFFEu : (uint32_t)(rng() % 0x7FFFFFFFu);
        std::vector<uint32_t> shuffled = dfs;
        std::shuffle(shuffled.begin(), shuffled.end(), rng);
        std::sort(shuffled.begin(), shuffled.end(), [&](uint32_t a, uint32_t b) { return wavefront_sort_key(root, a) < wavefront_sort_key(root, b); });
        CHECK_EQ(shuffled == dfs, 1);
        for (size_t i = 0; i < dfs.size(); i++) {
            const uint32_t p = dfs[i];
            deepest = std::max<long long>(deepest, wavefront_path_bits(p) + 1);
            const uint64_t k = wavefront_sort_key(root, p);
            CHECK_EQ(wavefront_key_root(k), root);
            CHECK_EQ(wavefront_key_path(k, wavefront_path_bits(p)), p);
            // a tree of max_level levels: no key has a bit below the sort's begin_bit; a leaf's own level puts its last bit there
            CHECK_EQ(k & ((1ull << wavefront_key_begin_bit(max_level)) - 1), 0);
            CHECK_EQ(wavefront_key_begin_bit(wavefront_path_bits(p) + 1), 30 - wavefront_path_bits(p));
            CHECK_EQ((k & ((1ull << 30) - 1)) << 2, numpy_aligned(p));  // the same bit string, two bits further left there
            if (i > 0) CHECK_EQ(wavefront_sort_key(root, dfs[i - 1]) < k, 1);  // distinct and increasing
        }
    }
    CHECK_EQ(trees >= 3000 && deepest == 31, 1);
    // two roots: every key of the lower root is below every key of the higher one
    CHECK_EQ(wavefront_sort_key(6, 0x7FFFFFFFu) < wavefront_sort_key(7, 1u), 1);
    // boundaries: path 1, 2^30, 2^31 - 1; local root 0 and the largest a slice can hold
    const uint32_t top = (uint32_t)(kWavefrontMaxSlots - 1);
    CHECK_EQ(wavefront_sort_key(0, 1u), 0);
    CHECK_EQ(wavefront_sort_key(0, 1u << 30), 0);  // thirty reflections: the string of 30 zeros
    CHECK_EQ(wavefront_sort_key(0, 0x7FFFFFFFu), (1ll << 30) - 1);
    CHECK_EQ(wavefront_sort_key(0, 3u), 1ll << 29);
    CHECK_EQ(wavefront_sort_key(0, 2u), 0);
    CHECK_EQ(wavefront_path_bits(1u), 0);
    CHECK_EQ(wavefront_path_bits(1u << 30), 30);
    CHECK_EQ(wavefront_path_bits(0x7FFFFFFFu), 30);
    CHECK_EQ(wavefront_sort_key(top, 0x7FFFFFFFu), ((long long)top << 30) | ((1ll << 30) - 1));
    CHECK_EQ(wavefront_key_root(wavefront_sort_key(top, 1u << 30)), top);
    CHECK_EQ(wavefront_key_path(wavefront_sort_key(top, 1u << 30), 30), 1u << 30);
    CHECK_EQ(wavefront_key_path(wavefront_sort_key(top, 0x7FFFFFFFu), 30), 0x7FFFFFFFu);
    CHECK_EQ(wavefront_key_path(wavefront_sort_key(0, 1u), 0), 1u);
    CHECK_EQ(wavefront_key_begin_bit(1), 30);
    CHECK_EQ(wavefront_key_begin_bit(5), 26);
    CHECK_EQ(wavefront_key_begin_bit(31), 0);
    CHECK_EQ(wavefront_key_begin_bit(0), 30);
    CHECK_EQ(wavefront_key_begin_bit(1) < wavefront_key_end_bit(1), 1);
    CHECK_EQ(wavefront_sort_key(0, 31u) >> wavefront_key_begin_bit(5), 15);  // level 5's last bit is the lowest one sorted
    // end_bit: every key of a slice of `roots` roots is below 2^end_bit, and one bit less would not do for the largest root
    for (long long roots : {1ll, 2ll, 3ll, 64ll, 65ll, 1000000ll, (long long)kWavefrontMaxSlots}) {
        const int e = wavefront_key_end_bit(roots);
        CHECK_EQ(e > 30 && e <= 62, 1);
        CHECK_EQ(wavefront_sort_key((uint32_t)(roots - 1), 0x7FFFFFFFu) < (1ull << e), 1);
        if (roots > 2) CHECK_EQ(wavefront_sort_key((uint32_t)(roots - 1), 1u) >= (1ull << (e - 1)), 1);
    }

    // ---- capacities never exceed work_bytes; a refusal's byte count is enough ----
    for (int hp = 0; hp < 2; hp++) {
        CHECK_EQ(wavefront_parked_bytes(hp != 0), hp ? 100 : 52);
        CHECK_EQ(wavefront_unit_bytes(hp != 0), hp ? 576 : 384);
        for (long long w : {0ll, 1ll, 383ll, 384ll, 575ll, 576ll, 577ll, 4096ll, 1000003ll, 1ll << 30, 1ll << 40, 1ll << 46}) {
            const WavefrontCaps c = wavefront_caps(w, hp != 0);
            CHECK_EQ(c.rays >= 0 && c.parked >= 0, 1);
            CHECK_EQ(wavefront_bytes_used(c, hp != 0) <= w, 1);
            CHECK_EQ(c.rays <= kWavefrontMaxSlots && c.parked <= kWavefrontMaxSlots && c.parked == 4 * c.rays, 1);
            CHECK_EQ(c.rays >= 1, w >= wavefront_unit_bytes(hp != 0));
        }
        for (long long r : {1ll, 2ll, 1000ll, 3000000ll})
            for (long long p : {1ll, 7ll, 5000ll, 9000000ll}) {
                const WavefrontCaps c = wavefront_caps(wavefront_bytes_for(r, p, hp != 0), hp != 0);
                CHECK_EQ(c.rays >= r && c.parked >= p, 1);
            }
        // the default: within both bounds, and with room for a level of 2n rays and 8n Hitpoints where the bounds allow
        for (long long n : {1ll, 64ll, 10368ll, 2073600ll, 1ll << 36})
            for (long long mem : {1ll << 30, 16ll << 30, 288ll << 30}) {
                const long long w = wavefront_default_work(n, mem, hp != 0);
                CHECK_EQ(w <= (1ll << 30) && w <= mem / 8 && w >= kWavefrontMinWork, 1);
                const WavefrontCaps c = wavefront_caps(w, hp != 0);
                CHECK_EQ(c.rays >= 1 && c.parked >= 1, 1);
                if (w < (1ll << 30) && w < mem / 8) CHECK_EQ(c.rays >= 2 * n && c.parked >= 8 * n, 1);
            }
    }

    // ---- the slice schedule ----
    bool failed = false;
    int slices = 0, halvings = 0;
    // nothing overflows: slices of the queue's capacity
    CHECK_EQ(run_slices(1000, 300, [](long long, long long) { return false; }, &failed, &slices, &halvings), 1000);
    CHECK_EQ(!failed && slices == 4 && halvings == 0, 1);
    CHECK_EQ(run_slices(1, 300, [](long long, long long) { return false; }, &failed, &slices, &halvings), 1);
    CHECK_EQ(!failed && slices == 1 && halvings == 0, 1);
    // a slice fits with at most 100 roots: 300 -> 150 -> 75, and the later slices keep 75
    CHECK_EQ(run_slices(1000, 300, [](long long, long long c) { return c > 100; }, &failed, &slices, &halvings), 1000);
    CHECK_EQ(!failed && halvings == 2 && slices == 14, 1);
    // a heavy region: slices that touch roots [500, 520) fit only one root at a time
    CHECK_EQ(run_slices(1000, 256, [](long long b, long long c) { return b < 520 && b + c > 500 && c > 1; }, &failed, &slices, &halvings), 1000);
    CHECK_EQ(!failed && halvings >= 8, 1);
    // root 700 never fits: everything before it is covered, then the call ends
    CHECK_EQ(run_slices(1000, 256, [](long long b, long long c) { return b <= 700 && b + c > 700; }, &failed, &slices, &halvings), 700);
    CHECK_EQ(failed, 1);
    CHECK_EQ(run_slices(1, 256, [](long long, long long) { return true; }, &failed, &slices, &halvings), 0);
    CHECK_EQ(failed && slices == 0 && halvings == 0, 1);
    // random scripts: a slice overflows when its cost exceeds a budget
    for (int t = 0; t < 200; t++) {
        const long long n = 1 + (long long)(rng() % 5000), cap = 1 + (long long)(rng() % 700);
        std::vector<int> cost((size_t)n);
        for (int &c : cost) c = 1 + (int)(rng() % 9);
        const long long budget = 9 + (long long)(rng() % 900);
        CHECK_EQ(run_slices(n, cap, [&](long long b, long long c) {
                     long long sum = 0;
                     for (long long i = b; i < b + c; i++) sum += cost[(size_t)i];
                     return sum > budget;
                 }, &failed, &slices, &halvings), n);
        CHECK_EQ(failed, 0);
    }

    // ---- a level's launch plan is the nearest-hit query's, field for field ----
    long long inputs = 0;
    for_each_traits([&](const cgrt::DeviceScene &d) {
        for (int depth : {1, 5})
            for (int stats = 0; stats < 2; stats++)
                for (long long n : {1ll, 64ll, 65ll, 100000ll, 1ll << 36}) {
                    const RaysPlan w = rays_plan(d, RaysAsk{depth, stats != 0, RaysKind::Wavefront, n}, kDev);
                    const RaysPlan f = rays_plan(d, RaysAsk{depth, stats != 0, RaysKind::First, n}, kDev);
                    inputs++;
                    CHECK_EQ(w.k.id(), f.k.id());
                    CHECK_EQ(w.k.nt, f.k.nt);
                    CHECK_EQ(w.resident, f.resident);
                    CHECK_EQ(w.lds, f.lds);
                    CHECK_EQ(w.wgs, f.wgs);
                    CHECK_EQ(std::strcmp(w.what(), f.what()), 0);
                    const RayFlags *r = compiled(w.k);
                    CHECK_EQ(r != nullptr, 1);
                    if (r) CHECK_EQ(has_bounce(*r), 1);
                }
    });
    CHECK_EQ(rays_first(RaysKind::Wavefront), 1);

    cgrt::DeviceScene spheres{}, mesh{}, bez{}, many{}, room{};
    spheres.n_objs = spheres.n_lds = 9;
    spheres.all_spheres = spheres.has_glass = 1;
    mesh.n_objs = mesh.n_lds = 7;
    mesh.has_mesh = mesh.has_wide = 1;
    bez.n_objs = bez.n_lds = 7;
    bez.has_bezier = bez.has_glass = 1;
    many.n_objs = 1000;
    many.n_lds = 768;
    many.all_spheres = many.has_glass = 1;
    room.n_objs = 800;
    room.n_lds = 768;
    room.has_mesh = room.has_bezier = room.has_glass = 1;
    check_name(spheres, RaysKind::Wavefront, 5, false, "wavefront_step_kernel<TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=0,NT=256>");
    check_name(mesh, RaysKind::Wavefront, 5, false, "wavefront_step_kernel<TREES=1,BEZ=0,SPH=0,STATS=0,SPILL=0,NT=256>");
    check_name(mesh, RaysKind::Wavefront, 5, true, "wavefront_step_kernel<TREES=1,BEZ=0,SPH=0,STATS=1,SPILL=0,NT=256>");
    check_name(bez, RaysKind::Wavefront, 5, false, "wavefront_step_kernel<TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=0,NT=64>");
    check_name(many, RaysKind::Wavefront, 5, true, "wavefront_step_kernel<TREES=0,BEZ=0,SPH=1,STATS=0,SPILL=1,NT=256>");
    check_name(room, RaysKind::Wavefront, 5, false, "wavefront_step_kernel<TREES=1,BEZ=1,SPH=0,STATS=0,SPILL=1,NT=256>");
    std::printf("trees checked: %lld (%lld leaves, deepest level %lld)\n", trees, leaves, deepest);
    std::printf("plans checked: %lld\n", inputs);
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
