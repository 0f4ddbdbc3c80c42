// The host side of the photon pass in plain C++ (no HIP): the kernel arguments, the setup -- batch size, pair buffer, sort key
// width, whether batches are traced on a second stream, the hash grid's cell -- and the batch schedule: which photons form the
// next batch, whether the batch traced ahead serves it, what to trace ahead, what a pair count does to the batch size.
// cgrt_ppm_session::photons (cgrt_ppm_session.hpp) launches what PpmSchedule decides; tests/native/ppm_plan.cpp checks it on
// the CPU.
#ifndef CGRT_PPM_PLAN_H
#define CGRT_PPM_PLAN_H
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "../../include/cgrt.h"

// =====================================================================================================
// kernel arguments
// =====================================================================================================
static constexpr int kSegStride = 8;  // event slots per photon (MAX_DEPTH = 5 segments)

struct PhotonArgs {
    double light[3], jitter, power, alpha;
    long long first;  // index of the first photon of this batch
    int count;        // photons in this batch
    int max_depth;
    uint64_t seed;
};
struct HashArgs {  // hash.h:20-42
    int hashsize;
    double celllength;
};
struct EmitArgs {
    double light[3], jitter, power;
    uint64_t seed;
};
// What photon_trace_kernel<.., RAYS = true> reads instead of the emitter: the caller's arrays (cgrt_photon_rays), already moved
// to the batch's first photon; keys / draws may be null
struct PhotonRayArgs {
    const double *org, *dir, *flux;
    const unsigned long long *keys;
    const unsigned int *draws;
};

// photons [first, first + count) of `ph`, traced to max_depth
inline PhotonArgs photon_args(const cgrt_photons &ph, long long first, int count, int max_depth) {
    PhotonArgs pa;
    for (int k = 0; k < 3; k++) pa.light[k] = ph.light[k];
    pa.jitter = ph.jitter; pa.power = ph.power; pa.alpha = ph.alpha;
    pa.first = first;
    pa.count = count;
    pa.max_depth = max_depth;
    pa.seed = ph.seed;
    return pa;
}
inline EmitArgs emit_args(const cgrt_photons *ph) {
    EmitArgs ea;
    for (int k = 0; k < 3; k++) ea.light[k] = ph->light[k];
    ea.jitter = ph->jitter; ea.power = ph->power; ea.seed = ph->seed;
    return ea;
}

// =====================================================================================================
// setup
// =====================================================================================================
// The hash grid (hash.h:20-42) and the initial radius
struct PpmGrid {
    HashArgs ha;
    double r0;
};
inline PpmGrid ppm_grid(const cgrt_photons &ph) {
    PpmGrid g;
    g.ha.hashsize = ph.hashsize;
    // main.cpp:84,183: r = 200.0 / height with the reference's COMPILE-TIME height (768) whatever frame is rendered;
    // a host that mirrors a reference built for another height passes that build's 200/height here
    g.r0 = ph.initial_radius > 0 ? ph.initial_radius : 200.0 / 768;
    g.ha.celllength = 70.0 / std::ceil(70.0 / g.r0);  // hash.h:25-26
    return g;
}

// CGRT_PHOTON_OVERLAP=0: one event buffer, everything on the null stream
inline bool photon_overlap_allowed() {
    const char *ov = std::getenv("CGRT_PHOTON_OVERLAP");
    return !(ov && ov[0] == '0');
}

// Batch size, pair buffer and the producer's buffers.  One call traces on a second stream only when it has more photons than
// one batch; a session always does (its calls are not known in advance).
struct PpmSetup {
    int batch = 0;  // photons per batch at the start = the most a batch ever holds (the event buffers' size)
    unsigned long long pair_cap = 0;
    int pair_key_bits = 25;  // sort key = hitpoint << 24 | slot
    // Two event buffers: while batch k's pairs are sorted and replayed (null stream), batch k+1 is traced and its events are
    // put in hash-cell order on the producer's stream.
    bool overlap = false;
    int nbuf = 0;  // event buffers: 0 (nothing will be traced), 1, or 2 and a stream of the producer's own (overlap)
    int64_t producer_bytes = 0;
};
inline PpmSetup ppm_setup(const cgrt_photons &ph, size_t n_hitpoints, bool session, bool overlap_allowed) {
    PpmSetup u;
    u.batch = ph.batch > 0 ? (ph.batch < (1 << 20) ? ph.batch : (1 << 20)) : (1 << 20);
    // pairs per batch: room for 128 per hitpoint, between 4 M and 128 M (3 GiB of keys and values); a batch that overflows is halved
    const unsigned long long want_cap = (unsigned long long)n_hitpoints * 128ull;
    u.pair_cap = want_cap < (1ull << 22) ? (1ull << 22) : (want_cap > (1ull << 27) ? (1ull << 27) : want_cap);
    if (ph.pair_cap > 0) u.pair_cap = (unsigned long long)ph.pair_cap < (1ull << 27) ? (unsigned long long)ph.pair_cap : (1ull << 27);
    while (u.pair_key_bits < 64 && (n_hitpoints >> (u.pair_key_bits - 24)) != 0) u.pair_key_bits++;
    u.overlap = overlap_allowed && (session || ph.nphotons > u.batch);
    if (n_hitpoints > 0 && (session || ph.nphotons > 0)) {
        u.nbuf = u.overlap ? 2 : 1;
        u.producer_bytes = (int64_t)u.nbuf * (u.batch * kSegStride) * (int64_t)(9 * sizeof(double) + 1 + 4 * 4);
    }
    return u;
}

// =====================================================================================================
// the batch schedule
// =====================================================================================================
// Photons [done, last) of a call go through in batches.  A batch is applied whole or not at all: `done` only moves past a
// batch once its pairs fit, so a failure leaves the state of the first `done` photons.  With overlap the batch after the one
// in hand is traced ahead, into the other buffer, on the assumption that the one in hand neither overflows the pair buffer
// nor changes the batch size; a batch traced ahead serves only if it is exactly the batch wanted, else that batch is produced
// again (results do not depend on the batching).
struct PpmBatch {
    long long first = 0;
    int count = 0;  // 0: no batch
    int buf = 0;    // the event buffer it is, or is to be, produced into
    bool reuse = false;  // it was traced ahead: nothing to produce
};
enum PpmOutcome {
    kPpmApplied,  // the pairs fit: sort and apply them, `done` has moved past the batch
    kPpmRedo,     // too many pairs: nothing is applied, the range comes again in smaller batches (same result)
    kPpmLimit     // too many pairs of one photon: CGRT_ERR_LIMIT
};
struct PpmSchedule {
    PpmSetup setup;  // what it runs under: setup.batch is batch_max, the event buffers' size
    int batch = 0;   // photons per batch now
    long long done = 0;          // photons [0, done) are applied
    long long ahead_first = -1;  // the batch traced ahead: its range and buffer (-1: none)
    int ahead_count = 0, ahead_buf = 0, cur = 0;
    uint64_t n_halvings = 0;
    long long last = 0, call = 0;  // the call in hand: its end and its length

    void start(const PpmSetup &u) {
        setup = u;
        batch = u.batch;
    }
    int batch_max() const { return setup.batch; }
    void drop_ahead() { ahead_first = -1; }
    // batch b, proposed by following() or end(), has been enqueued on the producer: only now is it the batch traced ahead (a
    // batch whose produce failed is not, and is produced again when it is wanted)
    void set_ahead(const PpmBatch &b) { ahead_first = b.first; ahead_count = b.count; ahead_buf = b.buf; }
    int clip(long long span) const { return (int)(span < batch ? span : batch); }

    // A call for photons [done, last_).  own_photons: they are the caller's, so a batch traced ahead (the built-in emitter's)
    // is dropped.  false: there are no hitpoints, no photon can change anything and the call is over.
    bool begin(long long last_, bool own_photons, bool no_hitpoints) {
        if (no_hitpoints) {
            done = last_ > done ? last_ : done;
            return false;
        }
        last = last_;
        call = last - done;
        if (own_photons) drop_ahead();
        return true;
    }
    bool more() const { return done < last; }
    // the batch at `done`; it becomes buffer `cur`
    PpmBatch next() {
        PpmBatch b;
        b.first = done;
        b.count = clip(last - done);
        b.reuse = ahead_first == b.first && ahead_count == b.count;
        if (b.reuse) cur = ahead_buf;  // else: first batch, the plan changed (a halving), or a lookahead that does not fit this call
        b.buf = cur;
        drop_ahead();
        return b;
    }
    // the batch to trace under b's search, sort and replay (count 0: none); the caller produces it, then set_ahead()
    PpmBatch following(const PpmBatch &b) const {
        PpmBatch nx;
        if (!setup.overlap || b.first + b.count >= last) return nx;
        nx.first = b.first + b.count;
        nx.count = clip(last - nx.first);
        nx.buf = 1 - cur;
        return nx;
    }
    // b's pairs are counted (the full 64-bit count, stored or not)
    PpmOutcome counted(const PpmBatch &b, unsigned long long npairs) {
        if (npairs > setup.pair_cap) {
            if (b.count <= 1) return kPpmLimit;
            batch = (b.count < batch ? b.count : batch) / 2;
            n_halvings++;
            return kPpmRedo;
        }
        done += b.count;
        // radii shrink as photons arrive: later batches hold fewer pairs.  Never beyond batch_max, the event buffers' size (a
        // batch halved from a size that is not batch_max / 2^k would otherwise double past it)
        if (batch < batch_max() && npairs < setup.pair_cap / 4) batch = batch < batch_max() / 2 ? batch * 2 : batch_max();
        return kPpmApplied;
    }
    // The range is done.  keep_ahead (a session with lookahead) and overlap: the first batch of a next call of as many photons as
    // this one (a run of equal calls is the interactive pattern; an empty call keeps what is there) is traced while the caller
    // looks at the image -- returned unless it is already there (count 0), into buffer 1 - cur: the replay of cur may still be
    // running; the caller produces it, then set_ahead().  Otherwise nothing is traced beyond `last` and *drain says to wait
    // for the producer's stream.
    PpmBatch end(bool keep_ahead, bool *drain) {
        PpmBatch nx;
        *drain = !(keep_ahead && setup.overlap);
        if (*drain) {
            drop_ahead();
            return nx;
        }
        const long long span = call > 0 ? call : (ahead_first == done ? ahead_count : batch);
        if (ahead_first == done && ahead_count == clip(span)) return nx;
        drop_ahead();  // whatever else is there will not serve, and its buffer is the one written next
        nx.first = done;
        nx.count = clip(span);
        nx.buf = 1 - cur;
        return nx;
    }
};

#endif
