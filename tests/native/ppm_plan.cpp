// The host side of the photon pass (cgrt_ppm_plan.h: ppm_grid, ppm_setup, photon_args, PpmSchedule): the setup on hand-checked
// inputs, and the batch schedule driven by a fake pair counter -- a function of the batch's range -- in place of the GPU:
// coverage, batch bounds, the one-photon overflow, reuse of the batch traced ahead, a produce that fails, and decision traces
// written out by hand from the loop cgrt_ppm_session::photons was before the schedule left it (that loop, without its HIP
// calls, is also kept here as a model and compared step for step over many chunkings).  CPU build under ASan + UBSan, driven
// by tests/test_ppm_plan_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cgrt_ppm_plan.h"

static int g_failed = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        if (a_ != b_) {                                                                                         \
            std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)
#define CHECK_EQD(a, b)                                                                                     \
    do {                                                                                                    \
        const double a_ = (a), b_ = (b);                                                                    \
        if (!(a_ == b_)) {                                                                                  \
            std::printf("FAIL %s:%d: %s == %.17g, expected %s == %.17g\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                     \
        }                                                                                                   \
    } while (0)

// =====================================================================================================
// setup
// =====================================================================================================
static cgrt_photons photons(long long nphotons, int batch = 0, long long pair_cap = 0) {
    cgrt_photons ph{};
    ph.light[1] = 19.999; ph.light[2] = 20;
    ph.jitter = 2; ph.power = 700; ph.alpha = 0.7;
    ph.nphotons = nphotons;
    ph.hashsize = 1000001;
    ph.batch = batch;
    ph.seed = 12345;
    ph.pair_cap = pair_cap;
    return ph;
}

static void setup_values() {
    const long long M = 1 << 20;
    // no hitpoints: the smallest pair buffer, nothing for the producer
    PpmSetup u = ppm_setup(photons(5 * M), 0, false, true);
    CHECK_EQ(u.batch, M);
    CHECK_EQ(u.pair_cap, 1ll << 22);
    CHECK_EQ(u.pair_key_bits, 25);
    CHECK_EQ(u.overlap, 1);
    CHECK_EQ(u.nbuf, 0);
    CHECK_EQ(u.producer_bytes, 0);
    // pair_cap: 128 per hitpoint inside [2^22, 2^27]
    CHECK_EQ(ppm_setup(photons(1), 1000, false, true).pair_cap, 1ll << 22);      // 128 000
    CHECK_EQ(ppm_setup(photons(1), 32768, false, true).pair_cap, 1ll << 22);     // exactly 2^22
    CHECK_EQ(ppm_setup(photons(1), 32769, false, true).pair_cap, 4194432);       // 2^22 + 128
    CHECK_EQ(ppm_setup(photons(1), 786432, false, true).pair_cap, 100663296);    // 1024 x 768: 96 M
    CHECK_EQ(ppm_setup(photons(1), 1 << 20, false, true).pair_cap, 1ll << 27);   // exactly 2^27
    CHECK_EQ(ppm_setup(photons(1), (1 << 20) + 1, false, true).pair_cap, 1ll << 27);
    CHECK_EQ(ppm_setup(photons(1), 1ull << 30, false, true).pair_cap, 1ll << 27);
    // ph.pair_cap overrides it, up to 2^27 and with no lower bound
    CHECK_EQ(ppm_setup(photons(1, 0, 64), 1 << 20, false, true).pair_cap, 64);
    CHECK_EQ(ppm_setup(photons(1, 0, 5000000), 10, false, true).pair_cap, 5000000);
    CHECK_EQ(ppm_setup(photons(1, 0, 1ll << 27), 10, false, true).pair_cap, 1ll << 27);
    CHECK_EQ(ppm_setup(photons(1, 0, (1ll << 27) + 1), 10, false, true).pair_cap, 1ll << 27);
    CHECK_EQ(ppm_setup(photons(1, 0, 1ll << 40), 10, false, true).pair_cap, 1ll << 27);
    // batch: 0 = 2^20, at most 2^20
    CHECK_EQ(ppm_setup(photons(1, 0), 10, false, true).batch, M);
    CHECK_EQ(ppm_setup(photons(1, 3000), 10, false, true).batch, 3000);
    CHECK_EQ(ppm_setup(photons(1, 1), 10, false, true).batch, 1);
    CHECK_EQ(ppm_setup(photons(1, (1 << 20) - 1), 10, false, true).batch, M - 1);
    CHECK_EQ(ppm_setup(photons(1, 1 << 20), 10, false, true).batch, M);
    CHECK_EQ(ppm_setup(photons(1, (1 << 20) + 1), 10, false, true).batch, M);
    CHECK_EQ(ppm_setup(photons(1, 2000000000), 10, false, true).batch, M);
    // sort key = hitpoint << 24 | slot: 24 bits and the bits of the hitpoint count
    CHECK_EQ(ppm_setup(photons(1), 1, false, true).pair_key_bits, 25);
    CHECK_EQ(ppm_setup(photons(1), 2, false, true).pair_key_bits, 26);
    CHECK_EQ(ppm_setup(photons(1), (1 << 24) - 1, false, true).pair_key_bits, 48);
    CHECK_EQ(ppm_setup(photons(1), 1 << 24, false, true).pair_key_bits, 49);
    CHECK_EQ(ppm_setup(photons(1), (1ull << 31) - 1, false, true).pair_key_bits, 55);
    // overlap: never when switched off; one call only with more photons than a batch; a session always
    CHECK_EQ(ppm_setup(photons(10 * M), 10, false, false).overlap, 0);
    CHECK_EQ(ppm_setup(photons(10 * M), 10, true, false).overlap, 0);
    CHECK_EQ(ppm_setup(photons(3000, 3000), 10, false, true).overlap, 0);
    CHECK_EQ(ppm_setup(photons(3001, 3000), 10, false, true).overlap, 1);
    CHECK_EQ(ppm_setup(photons(M), 10, false, true).overlap, 0);
    CHECK_EQ(ppm_setup(photons(M + 1), 10, false, true).overlap, 1);
    CHECK_EQ(ppm_setup(photons(0, 3000), 10, true, true).overlap, 1);
    CHECK_EQ(ppm_setup(photons(0, 3000), 0, true, true).overlap, 1);
    // event buffers: none when nothing will be traced, one without overlap, two with; 8 slots per photon of 9 doubles, a
    // validity byte and four 32-bit sort arrays
    CHECK_EQ(ppm_setup(photons(0, 3000), 10, false, true).nbuf, 0);
    CHECK_EQ(ppm_setup(photons(0, 3000), 0, true, true).nbuf, 0);
    u = ppm_setup(photons(3000, 3000), 10, false, true);
    CHECK_EQ(u.nbuf, 1);
    CHECK_EQ(u.producer_bytes, 3000ll * 8 * 89);
    u = ppm_setup(photons(3001, 3000), 10, false, true);
    CHECK_EQ(u.nbuf, 2);
    CHECK_EQ(u.producer_bytes, 2 * 3000ll * 8 * 89);
    u = ppm_setup(photons(0), 10, true, true);
    CHECK_EQ(u.nbuf, 2);
    CHECK_EQ(u.producer_bytes, 2 * M * 8 * 89);
    u = ppm_setup(photons(0), 10, true, false);
    CHECK_EQ(u.nbuf, 1);
    CHECK_EQ(u.producer_bytes, M * 8 * 89);

    // the switch itself: off only when the variable starts with '0'
    unsetenv("CGRT_PHOTON_OVERLAP");
    CHECK_EQ(photon_overlap_allowed(), 1);
    setenv("CGRT_PHOTON_OVERLAP", "0", 1);
    CHECK_EQ(photon_overlap_allowed(), 0);
    setenv("CGRT_PHOTON_OVERLAP", "1", 1);
    CHECK_EQ(photon_overlap_allowed(), 1);
    setenv("CGRT_PHOTON_OVERLAP", "", 1);
    CHECK_EQ(photon_overlap_allowed(), 1);
    unsetenv("CGRT_PHOTON_OVERLAP");

    // the hash grid: r0 = 200 / 768 by default, the cell the largest length <= r0 that divides 70
    cgrt_photons ph = photons(1);
    PpmGrid g = ppm_grid(ph);
    CHECK_EQ(g.ha.hashsize, 1000001);
    CHECK_EQD(g.r0, 200.0 / 768);
    CHECK_EQD(g.ha.celllength, 70.0 / 269);  // 70 / (200 / 768) = 268.8
    ph.initial_radius = 0.5;
    ph.hashsize = 4099;
    g = ppm_grid(ph);
    CHECK_EQ(g.ha.hashsize, 4099);
    CHECK_EQD(g.r0, 0.5);
    CHECK_EQD(g.ha.celllength, 0.5);  // 70 / 140
    ph.initial_radius = 0.3;
    CHECK_EQD(ppm_grid(ph).ha.celllength, 70.0 / 234);  // 70 / 0.3 = 233.3

    // photon_args: the batch's range and depth beside the emitter's parameters
    ph = photons(1);
    const PhotonArgs pa = photon_args(ph, 123456789012ll, 777, 5);
    CHECK_EQD(pa.light[0], 0); CHECK_EQD(pa.light[1], 19.999); CHECK_EQD(pa.light[2], 20);
    CHECK_EQD(pa.jitter, 2); CHECK_EQD(pa.power, 700); CHECK_EQD(pa.alpha, 0.7);
    CHECK_EQ(pa.first, 123456789012ll);
    CHECK_EQ(pa.count, 777);
    CHECK_EQ(pa.max_depth, 5);
    CHECK_EQ(pa.seed, 12345);
    const EmitArgs ea = emit_args(&ph);
    CHECK_EQD(ea.light[1], 19.999); CHECK_EQD(ea.jitter, 2); CHECK_EQD(ea.power, 700);
    CHECK_EQ(ea.seed, 12345);
}

// =====================================================================================================
// the schedule, driven as cgrt_ppm_session::photons drives it
// =====================================================================================================
typedef unsigned long long (*Counter)(long long first, int count);

enum { kNone = 0, kLookahead = 1, kDrain = 2 };
struct Step {
    int reuse, buf;  // the batch: traced ahead (1) or produced now (0), and its buffer
    long long first;
    int count;
    long long nx_first;  // the batch enqueued under it (-1: none)
    int nx_count, nx_buf;
    int outcome, batch_after;
};
struct Call {
    std::vector<Step> steps;
    int end = kNone;  // kNone: nothing enqueued (what is traced ahead, if anything, stays)
    long long la_first = -1;
    int la_count = 0, la_buf = 0;
    bool limit = false;
    bool failed = false;  // a produce failed: the call returned there
};

// fail_produce: the produce of this call, counted from 0 over the batches produced now, those enqueued under them and the
// lookahead, that fails as a HIP call can (-1: none); photons() returns at once, without set_ahead
static Call drive(PpmSchedule &s, long long count, bool keep_ahead, bool own, Counter f, bool no_hitpoints = false, int fail_produce = -1) {
    Call c;
    int produced = 0;
    const auto produce = [&] { return produced++ != fail_produce; };
    if (!s.begin(s.done + count, own, no_hitpoints)) return c;
    while (s.more()) {
        const PpmBatch b = s.next();
        if (!b.reuse && !produce()) { c.failed = true; return c; }
        const PpmBatch nx = s.following(b);
        if (nx.count) {
            if (!produce()) { c.failed = true; return c; }
            s.set_ahead(nx);
        }
        const PpmOutcome o = s.counted(b, f(b.first, b.count));
        c.steps.push_back(Step{b.reuse, b.buf, b.first, b.count, nx.count ? nx.first : -1, nx.count, nx.count ? nx.buf : 0, (int)o, s.batch});
        if (o == kPpmLimit) {
            c.limit = true;
            break;
        }
    }
    if (!c.limit) {
        bool drain = false;
        const PpmBatch la = s.end(keep_ahead, &drain);
        c.end = drain ? kDrain : (la.count ? kLookahead : kNone);
        if (la.count) {
            if (!produce()) { c.failed = true; return c; }
            s.set_ahead(la);
            c.la_first = la.first; c.la_count = la.count; c.la_buf = la.buf;
        }
    }
    if (own) s.drop_ahead();  // cgrt_ppm_session_add_photon_rays: nothing traced from the caller's arrays outlives the call
    return c;
}

// The loop of cgrt_ppm_session::photons as it stood in cgrt_photon.hpp at commit 8ad707d, the last before PpmSchedule, with
// its HIP calls taken out (none of them fails here): what "the same decisions as before" means, step for step
struct Model {
    int batch = 0, batch_max = 0;
    unsigned long long pair_cap = 0;
    bool overlap = false;
    long long done = 0, ahead_first = -1;
    int ahead_count = 0, ahead_buf = 0, cur = 0;
    unsigned long long n_halvings = 0;
    int count_of(long long first, int batch_now, long long end) const { return (int)((end - first < batch_now) ? (end - first) : batch_now); }
    Call photons(long long last, bool keep_ahead, bool own, Counter f, bool no_hitpoints = false) {
        Call c;
        if (no_hitpoints) {
            done = last > done ? last : done;
            return c;
        }
        if (own) ahead_first = -1;
        const long long call = last - done;
        while (done < last) {
            const long long pa_first = done;
            const int pa_count = count_of(done, batch, last);
            Step st{};
            if (ahead_first == pa_first && ahead_count == pa_count) {
                cur = ahead_buf;
                st.reuse = 1;
            }
            st.buf = cur; st.first = pa_first; st.count = pa_count; st.nx_first = -1;
            ahead_first = -1;
            if (overlap && done + pa_count < last) {
                const long long nx_first = done + pa_count;
                const int nx_count = count_of(nx_first, batch, last);
                ahead_first = nx_first; ahead_count = nx_count; ahead_buf = 1 - cur;
                st.nx_first = nx_first; st.nx_count = nx_count; st.nx_buf = 1 - cur;
            }
            const unsigned long long np = f(pa_first, pa_count);
            if (np > pair_cap) {
                if (pa_count <= 1) {
                    st.outcome = kPpmLimit; st.batch_after = batch;
                    c.steps.push_back(st);
                    c.limit = true;
                    if (own) ahead_first = -1;
                    return c;
                }
                batch = (pa_count < batch ? pa_count : batch) / 2;
                n_halvings++;
                st.outcome = kPpmRedo; st.batch_after = batch;
                c.steps.push_back(st);
                continue;
            }
            done += pa_count;
            if (batch < batch_max && np < pair_cap / 4) batch = batch < batch_max / 2 ? batch * 2 : batch_max;
            st.outcome = kPpmApplied; st.batch_after = batch;
            c.steps.push_back(st);
        }
        if (keep_ahead && overlap) {
            const long long span = call > 0 ? call : (ahead_first == done ? ahead_count : batch);
            if (ahead_first != done || ahead_count != (span < batch ? span : batch)) {
                c.end = kLookahead;
                c.la_first = done; c.la_count = count_of(done, batch, done + span); c.la_buf = 1 - cur;
                ahead_first = c.la_first; ahead_count = c.la_count; ahead_buf = c.la_buf;
            }
        } else {
            ahead_first = -1;
            c.end = kDrain;
        }
        if (own) ahead_first = -1;
        return c;
    }
};

static void check_same(const Call &got, const Call &want, int line) {
    const size_t before = g_failed;
    CHECK_EQ(got.steps.size(), want.steps.size());
    for (size_t k = 0; k < got.steps.size() && k < want.steps.size(); k++) {
        const Step &a = got.steps[k], &b = want.steps[k];
        CHECK_EQ(a.reuse, b.reuse); CHECK_EQ(a.buf, b.buf); CHECK_EQ(a.first, b.first); CHECK_EQ(a.count, b.count);
        CHECK_EQ(a.nx_first, b.nx_first); CHECK_EQ(a.nx_count, b.nx_count); CHECK_EQ(a.nx_buf, b.nx_buf);
        CHECK_EQ(a.outcome, b.outcome); CHECK_EQ(a.batch_after, b.batch_after);
        if ((size_t)g_failed != before) {
            std::printf("  ... at step %zu of the call checked at line %d\n", k, line);
            return;
        }
    }
    CHECK_EQ(got.end, want.end); CHECK_EQ(got.la_first, want.la_first); CHECK_EQ(got.la_count, want.la_count);
    CHECK_EQ(got.la_buf, want.la_buf); CHECK_EQ(got.limit, want.limit);
    if ((size_t)g_failed != before) std::printf("  ... at the end of the call checked at line %d\n", line);
}

static PpmSchedule schedule(int batch, unsigned long long pair_cap, bool overlap) {
    PpmSetup u;
    u.batch = batch; u.pair_cap = pair_cap; u.overlap = overlap;
    PpmSchedule s;
    s.start(u);
    return s;
}
static Model model(int batch, unsigned long long pair_cap, bool overlap) {
    Model m;
    m.batch = m.batch_max = batch; m.pair_cap = pair_cap; m.overlap = overlap;
    return m;
}

// ---- pair counters: functions of the batch's range ----
static unsigned long long half_full(long long, int) { return 500; }                 // never overflows pair_cap 1000, never lets the batch grow
static unsigned long long one_each(long long, int count) { return (unsigned long long)count; }
static unsigned long long dense_then_thin(long long first, int count) {             // radii shrink: photons from 1500 on find a tenth of the pairs
    return first < 1500 ? (unsigned long long)count : (unsigned long long)count / 10;
}
static unsigned long long hot_photon(long long first, int count) {                  // photon 4321 alone overflows every buffer
    return first <= 4321 && 4321 < first + count ? ~0ull : (unsigned long long)count / 8;
}
static unsigned long long ragged(long long first, int count) {                      // pseudo-random density per 97 photons, 0 .. 3 pairs a photon
    unsigned long long s = 0;
    for (long long p = first; p < first + count; p++) s += (unsigned long long)(((p / 97) * 2654435761ull >> 7) & 3);
    return s;
}

// ---- decision traces by hand (batch 3000, pair_cap 1000, overlap) ----
static Call trace(std::vector<Step> steps, int end, long long la_first = -1, int la_count = 0, int la_buf = 0) {
    Call c;
    c.steps = steps; c.end = end; c.la_first = la_first; c.la_count = la_count; c.la_buf = la_buf;
    return c;
}
static void traces() {
    const int A = kPpmApplied, R = kPpmRedo;
    {
        // 1. no overflow: two calls of 7000 photons, lookahead on.  Every batch but the first was traced ahead, buffers alternate.
        PpmSchedule s = schedule(3000, 1000, true);
        //                       reuse buf first count  next: first count buf  outcome batch
        check_same(drive(s, 7000, true, false, half_full),
                   trace({{0, 0, 0, 3000, 3000, 3000, 1, A, 3000},
                          {1, 1, 3000, 3000, 6000, 1000, 0, A, 3000},
                          {1, 0, 6000, 1000, -1, 0, 0, A, 3000}},
                         kLookahead, 7000, 3000, 1), __LINE__);
        check_same(drive(s, 7000, true, false, half_full),
                   trace({{1, 1, 7000, 3000, 10000, 3000, 0, A, 3000},
                          {1, 0, 10000, 3000, 13000, 1000, 1, A, 3000},
                          {1, 1, 13000, 1000, -1, 0, 0, A, 3000}},
                         kLookahead, 14000, 3000, 0), __LINE__);
        CHECK_EQ(s.done, 14000);
        CHECK_EQ(s.n_halvings, 0);
    }
    {
        // 2. two halvings and a grow-back inside one call of 6000 photons, no lookahead.  Photons below 1500 bring a pair each
        // (a batch above 1000 overflows), later ones a tenth (below pair_cap / 4 = 250: the batch doubles, 750 -> 1500 -> 3000).
        // After a redo and after a change of size the batch traced ahead does not match and is produced again, into `cur`.
        PpmSchedule s = schedule(3000, 1000, true);
        check_same(drive(s, 6000, false, false, dense_then_thin),
                   trace({{0, 0, 0, 3000, 3000, 3000, 1, R, 1500},
                          {0, 0, 0, 1500, 1500, 1500, 1, R, 750},
                          {0, 0, 0, 750, 750, 750, 1, A, 750},
                          {1, 1, 750, 750, 1500, 750, 0, A, 750},
                          {1, 0, 1500, 750, 2250, 750, 1, A, 1500},
                          {0, 0, 2250, 1500, 3750, 1500, 1, A, 3000},
                          {0, 0, 3750, 2250, -1, 0, 0, A, 3000}},
                         kDrain), __LINE__);
        CHECK_EQ(s.done, 6000);
        CHECK_EQ(s.n_halvings, 2);
        CHECK_EQ(s.ahead_first, -1);
    }
    {
        // 3. a reduced batch carried across call boundaries, lookahead on: calls of 1, 2999, 500, 0 and 500 photons, a pair a
        // photon.  The 2999-photon call is halved from its own count (2999 -> 1499 -> 749), its last batch of 3 photons lets
        // the size double to 1498, and that is what the lookahead and the calls after it are cut to.
        PpmSchedule s = schedule(3000, 1000, true);
        check_same(drive(s, 1, true, false, one_each), trace({{0, 0, 0, 1, -1, 0, 0, A, 3000}}, kLookahead, 1, 1, 1), __LINE__);
        check_same(drive(s, 2999, true, false, one_each),
                   trace({{0, 0, 1, 2999, -1, 0, 0, R, 1499},  // the lookahead [1, 2) is not this batch: dropped
                          {0, 0, 1, 1499, 1500, 1499, 1, R, 749},
                          {0, 0, 1, 749, 750, 749, 1, A, 749},
                          {1, 1, 750, 749, 1499, 749, 0, A, 749},
                          {1, 0, 1499, 749, 2248, 749, 1, A, 749},
                          {1, 1, 2248, 749, 2997, 3, 0, A, 749},
                          {1, 0, 2997, 3, -1, 0, 0, A, 1498}},
                         kLookahead, 3000, 1498, 1), __LINE__);
        CHECK_EQ(s.n_halvings, 2);
        // fewer photons than the lookahead [3000, 4498): it is dropped, the call's one batch is produced
        check_same(drive(s, 500, true, false, one_each), trace({{0, 0, 3000, 500, -1, 0, 0, A, 1498}}, kLookahead, 3500, 500, 1), __LINE__);
        // an empty call keeps the lookahead [3500, 4000)
        check_same(drive(s, 0, true, false, one_each), trace({}, kNone), __LINE__);
        CHECK_EQ(s.ahead_first, 3500);
        CHECK_EQ(s.ahead_count, 500);
        check_same(drive(s, 500, true, false, one_each), trace({{1, 1, 3500, 500, -1, 0, 0, A, 1498}}, kLookahead, 4000, 500, 0), __LINE__);
        CHECK_EQ(s.done, 4000);
        CHECK_EQ(s.batch, 1498);
    }
}

// ---- coverage, bounds and agreement with the model over many chunkings ----
static std::vector<long long> with_rest(std::vector<long long> chunks, long long total) {
    long long sum = 0;
    for (long long c : chunks) sum += c;
    chunks.push_back(total - sum);
    return chunks;
}
static void chunkings() {
    const long long total = 20000;
    const std::vector<std::vector<long long>> splits = {
        {total}, with_rest({1, 2999, 500, 7000, 37}, total) /* test_batch_machinery_across_calls */, with_rest({3000, 3000, 3000}, total),
        with_rest({0, 1, 0, 0, 2, 5999, 0}, total), with_rest({6000, 6000, 1}, total), std::vector<long long>(200, total / 200)};
    const Counter counters[] = {half_full, one_each, dense_then_thin, ragged};
    const int batches[] = {3000, 2999, 1, 7, 1 << 20};
    for (const auto &split : splits)
        for (const Counter f : counters)
            for (const int batch : batches)
                for (int mode = 0; mode < 4; mode++) {  // overlap x lookahead
                    const bool overlap = mode & 1, lookahead = mode & 2;
                    PpmSchedule s = schedule(batch, 1000, overlap);
                    Model m = model(batch, 1000, overlap);
                    long long at = 0, halvings = 0;
                    for (const long long c : split) {
                        const long long ahead_first = s.ahead_first, call_first = s.done;
                        const int ahead_count = s.ahead_count, ahead_buf = s.ahead_buf;
                        const Call got = drive(s, c, lookahead, false, f);
                        check_same(got, m.photons(m.done + c, lookahead, false, f), __LINE__);
                        bool first_step = true;
                        int prev_buf = -1, prev_nx_buf = -1;
                        for (const Step &st : got.steps) {
                            CHECK_EQ(st.count >= 1 && st.count <= batch, 1);  // never beyond the event buffers
                            CHECK_EQ(st.batch_after >= 1 && st.batch_after <= batch, 1);
                            CHECK_EQ(st.first, at);                            // the applied batches tile [0, total) in order
                            CHECK_EQ(st.first + st.count <= call_first + c, 1);
                            if (st.outcome == kPpmApplied) at += st.count;
                            if (st.outcome == kPpmRedo) halvings++;
                            if (st.nx_first >= 0) {
                                CHECK_EQ(overlap, 1);
                                CHECK_EQ(st.nx_first, st.first + st.count);
                                CHECK_EQ(st.nx_buf, 1 - st.buf);  // never the buffer in hand
                                CHECK_EQ(st.nx_count >= 1 && st.nx_count <= batch, 1);
                            }
                            // traced ahead = exactly this range was enqueued before, in that buffer
                            if (st.reuse && first_step) {
                                CHECK_EQ(ahead_first, st.first); CHECK_EQ(ahead_count, st.count); CHECK_EQ(ahead_buf, st.buf);
                            }
                            if (st.reuse && !first_step) CHECK_EQ(prev_nx_buf, st.buf);
                            if (!st.reuse && !first_step) CHECK_EQ(st.buf, prev_buf);  // produced again into the buffer in hand
                            first_step = false;
                            prev_buf = st.buf;
                            prev_nx_buf = st.nx_first >= 0 ? st.nx_buf : -1;
                        }
                        CHECK_EQ(at, call_first + c);
                        CHECK_EQ(s.done, at);
                        if (lookahead && overlap) {
                            CHECK_EQ(got.end != kDrain, 1);
                            if (c > 0) {  // the lookahead: the next call's first batch if it is as long as this one
                                CHECK_EQ(s.ahead_first, s.done);
                                CHECK_EQ(s.ahead_count, c < s.batch ? c : s.batch);
                                CHECK_EQ(s.ahead_buf, 1 - s.cur);
                            }
                        } else {
                            CHECK_EQ(got.end, kDrain);
                            CHECK_EQ(s.ahead_first, -1);
                        }
                        if (!overlap) CHECK_EQ(s.cur, 0);  // one buffer
                    }
                    CHECK_EQ(at, total);
                    CHECK_EQ(s.n_halvings, halvings);
                    CHECK_EQ(s.batch, m.batch);
                }
}

static void batch_bounds() {
    // halved from a size that is not batch_max / 2^k, then grown back: 3000 -> (a 2999-photon call) 1499 -> 749 -> 1498 -> 2996
    // would pass 3000 at the next doubling; the rule stops at batch_max
    PpmSchedule s = schedule(3000, 1000, true);
    drive(s, 1, true, false, one_each);
    drive(s, 2999, true, false, one_each);
    CHECK_EQ(s.batch, 1498);
    drive(s, 100, true, false, one_each);  // 100 pairs < 250: doubles
    CHECK_EQ(s.batch, 2996);
    drive(s, 100, true, false, one_each);  // 2996 >= batch_max / 2: to batch_max, not 5992
    CHECK_EQ(s.batch, 3000);
    drive(s, 100, true, false, one_each);
    CHECK_EQ(s.batch, 3000);
    // a batch shorter than `batch` is halved from its own count
    s = schedule(1 << 20, 1000, false);
    Call c = drive(s, 2001, false, false, one_each);
    CHECK_EQ(c.steps[0].count, 2001);
    CHECK_EQ(c.steps[0].outcome, kPpmRedo);
    CHECK_EQ(c.steps[0].batch_after, 1000);
    CHECK_EQ(c.steps[1].count, 1000);
    CHECK_EQ(c.steps[1].outcome, kPpmApplied);
    // exactly pair_cap pairs fit; pair_cap / 4 pairs do not let the batch grow, one fewer does
    s = schedule(3000, 1000, false);
    s.batch = 1000;
    CHECK_EQ(s.begin(3000, false, false), 1);
    PpmBatch b = s.next();
    CHECK_EQ(s.counted(b, 1000), kPpmApplied);
    CHECK_EQ(s.batch, 1000);
    b = s.next();
    CHECK_EQ(s.counted(b, 250), kPpmApplied);
    CHECK_EQ(s.batch, 1000);
    b = s.next();
    CHECK_EQ(s.counted(b, 249), kPpmApplied);
    CHECK_EQ(s.batch, 2000);
    CHECK_EQ(s.more(), 0);
}

static void one_photon_overflow() {
    for (int overlap = 0; overlap < 2; overlap++) {
        PpmSchedule s = schedule(3000, 1000, overlap != 0);
        Model m = model(3000, 1000, overlap != 0);
        const Call c = drive(s, 10000, true, false, hot_photon);
        check_same(c, m.photons(10000, true, false, hot_photon), __LINE__);
        CHECK_EQ(c.limit, 1);
        const Step &last = c.steps.back();
        CHECK_EQ(last.first, 4321);
        CHECK_EQ(last.count, 1);
        CHECK_EQ(last.outcome, kPpmLimit);
        CHECK_EQ(s.done, 4321);  // everything before the photon is applied, the photon is not
        CHECK_EQ(s.batch >= 1, 1);
        const unsigned long long halvings = s.n_halvings;
        // the same call again: the same refusal, the state where it was
        const Call again = drive(s, 10000 - s.done, true, false, hot_photon);
        CHECK_EQ(again.limit, 1);
        CHECK_EQ(again.steps.size(), 1);
        CHECK_EQ(s.done, 4321);
        CHECK_EQ(s.n_halvings, halvings);
    }
}

static void ahead_reuse() {
    // both first and count must match
    PpmSchedule s = schedule(3000, 1000, true);
    s.begin(9000, false, false);
    s.ahead_first = 0; s.ahead_count = 2999; s.ahead_buf = 1;
    PpmBatch b = s.next();
    CHECK_EQ(b.reuse, 0); CHECK_EQ(b.buf, 0); CHECK_EQ(s.ahead_first, -1);
    s.ahead_first = 1; s.ahead_count = 3000; s.ahead_buf = 1;
    b = s.next();
    CHECK_EQ(b.reuse, 0); CHECK_EQ(b.buf, 0);
    s.ahead_first = 0; s.ahead_count = 3000; s.ahead_buf = 1;
    b = s.next();
    CHECK_EQ(b.reuse, 1); CHECK_EQ(b.buf, 1); CHECK_EQ(s.cur, 1); CHECK_EQ(s.ahead_first, -1);
    // after an overflow the batch enqueued under the overflowing one is not the batch wanted: produced again
    s = schedule(3000, 1000, true);
    Call c = drive(s, 6000, true, false, one_each);
    CHECK_EQ(c.steps[0].nx_first, 3000);
    CHECK_EQ(c.steps[0].outcome, kPpmRedo);
    CHECK_EQ(c.steps[1].reuse, 0);
    CHECK_EQ(c.steps[1].first, 0);
    CHECK_EQ(c.steps[1].count, 1500);
    // no hitpoints: the call is over at once, all its photons count as done, nothing is traced
    s = schedule(3000, 1000, true);
    c = drive(s, 5000, true, false, one_each, true);
    CHECK_EQ(c.steps.size(), 0); CHECK_EQ(c.end, kNone); CHECK_EQ(s.done, 5000); CHECK_EQ(s.ahead_first, -1);
    // the caller's photons drop the batch traced ahead at the start and leave none behind, whatever keep_ahead says
    for (int keep = 0; keep < 2; keep++) {
        s = schedule(3000, 1000, true);
        Model m = model(3000, 1000, true);
        check_same(drive(s, 3000, true, false, half_full), m.photons(3000, true, false, half_full), __LINE__);
        CHECK_EQ(s.ahead_first, 3000);
        CHECK_EQ(s.ahead_count, 3000);
        c = drive(s, 7000, keep != 0, true, half_full);
        check_same(c, m.photons(10000, keep != 0, true, half_full), __LINE__);
        CHECK_EQ(c.steps[0].reuse, 0);  // [3000, 6000) was traced ahead -- by the built-in emitter
        CHECK_EQ(c.steps[0].first, 3000);
        CHECK_EQ(c.steps[0].count, 3000);
        CHECK_EQ(c.steps[1].reuse, 1);  // inside the call batches are traced ahead as ever
        CHECK_EQ(s.ahead_first, -1);
        CHECK_EQ(s.done, 10000);
        // and the built-in emitter's next call produces its first batch
        c = drive(s, 3000, true, false, half_full);
        check_same(c, m.photons(13000, true, false, half_full), __LINE__);
        CHECK_EQ(c.steps[0].reuse, 0);
    }
    // keep_ahead = false ends in "drain", with or without overlap, and leaves nothing traced ahead
    for (int overlap = 0; overlap < 2; overlap++) {
        s = schedule(3000, 1000, overlap != 0);
        c = drive(s, 7000, false, false, half_full);
        CHECK_EQ(c.end, kDrain); CHECK_EQ(c.la_count, 0); CHECK_EQ(s.ahead_first, -1);
        c = drive(s, 0, false, false, half_full);
        CHECK_EQ(c.end, kDrain); CHECK_EQ(s.ahead_first, -1);
    }
    // lookahead without overlap: one buffer, nothing to trace into: "drain"
    s = schedule(3000, 1000, false);
    c = drive(s, 7000, true, false, half_full);
    CHECK_EQ(c.end, kDrain);
    for (const Step &st : c.steps) { CHECK_EQ(st.nx_first, -1); CHECK_EQ(st.buf, 0); CHECK_EQ(st.reuse, 0); }
    // an empty first call of a session: the lookahead is one batch
    s = schedule(3000, 1000, true);
    c = drive(s, 0, true, false, half_full);
    CHECK_EQ(c.end, kLookahead); CHECK_EQ(c.la_first, 0); CHECK_EQ(c.la_count, 3000); CHECK_EQ(c.la_buf, 1);
    c = drive(s, 0, true, false, half_full);  // and the next empty call keeps it
    CHECK_EQ(c.end, kNone); CHECK_EQ(s.ahead_first, 0); CHECK_EQ(s.ahead_count, 3000);
}

// A produce that fails leaves nothing behind that a later call could take for a batch traced ahead: the buffer was not
// (fully) written and its event never recorded, so the batch is produced again when it is wanted
static void failed_produce() {
    // the lookahead at the end of a call
    PpmSchedule s = schedule(3000, 1000, true);
    Call c = drive(s, 3000, true, false, half_full, false, 1);  // produce 0: the batch, produce 1: the lookahead [3000, 6000)
    CHECK_EQ(c.failed, 1); CHECK_EQ(c.steps.size(), 1); CHECK_EQ(s.done, 3000);
    CHECK_EQ(s.ahead_first, -1);
    c = drive(s, 3000, true, false, half_full);  // the call the lookahead was meant for
    CHECK_EQ(c.failed, 0);
    CHECK_EQ(c.steps[0].first, 3000); CHECK_EQ(c.steps[0].count, 3000);
    CHECK_EQ(c.steps[0].reuse, 0);
    CHECK_EQ(c.end, kLookahead); CHECK_EQ(s.ahead_first, 6000);
    // the batch enqueued under the one in hand: the call fails before anything is applied, the retry starts from scratch
    s = schedule(3000, 1000, true);
    c = drive(s, 7000, true, false, half_full, false, 1);  // produce 1: [3000, 6000) under [0, 3000)
    CHECK_EQ(c.failed, 1); CHECK_EQ(c.steps.size(), 0); CHECK_EQ(s.done, 0);
    CHECK_EQ(s.ahead_first, -1);
    c = drive(s, 7000, true, false, half_full);
    CHECK_EQ(c.steps.size(), 3);
    CHECK_EQ(c.steps[0].first, 0); CHECK_EQ(c.steps[0].reuse, 0);
    CHECK_EQ(c.steps[1].first, 3000); CHECK_EQ(c.steps[1].reuse, 1);
    CHECK_EQ(s.done, 7000);
    // later in a call: [0, 3000) is applied, [3000, 6000) is in hand, and the produce of [6000, 7000) under it fails
    s = schedule(3000, 1000, true);
    c = drive(s, 7000, true, false, half_full, false, 2);
    CHECK_EQ(c.failed, 1); CHECK_EQ(c.steps.size(), 1); CHECK_EQ(s.done, 3000);
    CHECK_EQ(s.ahead_first, -1);  // [3000, 6000) went into the batch in hand, [6000, 7000) never came to be
    c = drive(s, 4000, true, false, half_full);
    CHECK_EQ(c.steps[0].first, 3000); CHECK_EQ(c.steps[0].reuse, 0);
    CHECK_EQ(s.done, 7000);
    // a batch that was traced ahead and whose own produce is therefore skipped is not affected by a later failure
    s = schedule(3000, 1000, true);
    drive(s, 3000, true, false, half_full);
    CHECK_EQ(s.ahead_first, 3000);
    c = drive(s, 3000, true, false, half_full, false, 0);  // the only produce of this call is its lookahead [6000, 9000)
    CHECK_EQ(c.failed, 1); CHECK_EQ(c.steps.size(), 1); CHECK_EQ(c.steps[0].reuse, 1); CHECK_EQ(s.done, 6000);
    CHECK_EQ(s.ahead_first, -1);
}

int main() {
    failed_produce();
    setup_values();
    traces();
    chunkings();
    batch_bounds();
    one_photon_overflow();
    ahead_reuse();
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
