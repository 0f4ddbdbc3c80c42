// The wavefront trace's plan in plain C++ (no HIP): the sort key that orders parked Hitpoints as trace() emits them, the
// capacities of ray queue and parked list from the work memory, the slice schedule with its halving rule, and the default
// work memory.  cgrt_wavefront_rays (cgrt_ray_queries.hpp) drives its launches with these, wavefront_step_kernel and
// wavefront_sum_kernel (cgrt_wavefront.hpp) use the key; tests/native/wavefront_plan.cpp checks them on the CPU.
#ifndef CGRT_WAVEFRONT_PLAN_H
#define CGRT_WAVEFRONT_PLAN_H
#include <cstddef>
#include <cstdint>

#include "cgrt_rng.hpp"  // CGRT_HD

static constexpr int kWavefrontMaxDepth = 31;  // path < 2^31: a ray of level L has a path of L bits
static constexpr int kWavefrontPathBits = 30;  // bits of a path behind its leading 1, at most

// ---- the sort key ----
// Emission order within a root is depth first, the reflected subtree (bit 0) before the refracted one (bit 1): the paths
// compared as bit strings behind their leading 1.  Hitpoints are leaves, so no path of a root is a prefix of another and the
// bit strings left-aligned in 30 bits are distinct and order them; the slice-local root goes above them.
CGRT_HD int wavefront_path_bits(uint32_t path) { return 31 - __builtin_clz(path); }  // path in [1, 2^31): 0..30
CGRT_HD uint64_t wavefront_sort_key(uint32_t local_root, uint32_t path) {
    const int ln = wavefront_path_bits(path);
    const uint64_t aligned = (uint64_t)(path - (1u << ln)) << (kWavefrontPathBits - ln);
    return ((uint64_t)local_root << kWavefrontPathBits) | aligned;
}
// The inverse: the root, and the path given the number of bits behind its leading 1 (left-aligned strings do not tell "0" from
// "00": a parked record keeps its path beside the key)
CGRT_HD uint32_t wavefront_key_root(uint64_t key) { return (uint32_t)(key >> kWavefrontPathBits); }
CGRT_HD uint32_t wavefront_key_path(uint64_t key, int bits) {
    const uint32_t aligned = (uint32_t)(key & ((1ull << kWavefrontPathBits) - 1ull));
    return (1u << bits) | (aligned >> (kWavefrontPathBits - bits));
}
// the radix sort's end_bit for a slice of `roots` roots: the keys are below 2^end_bit
CGRT_HD int wavefront_key_end_bit(long long roots) {
    int b = 0;
    while (b < 32 && (1ll << b) < roots) b++;
    return kWavefrontPathBits + (b > 0 ? b : 1);
}
// ... and its begin_bit: in a slice whose deepest level is `levels` a path has at most levels - 1 bits behind its leading 1, so
// the lowest 30 - (levels - 1) bits of every key are zero and need no pass of the sort
CGRT_HD int wavefront_key_begin_bit(int levels) {
    const int bits = levels < 1 ? 0 : (levels - 1 > kWavefrontPathBits ? kWavefrontPathBits : levels - 1);
    return kWavefrontPathBits - bits;
}

// ---- work memory ----
// A queued ray: org, dir, adj, key, path, slice-local root, each an array of its own; there are two queues, the level that
// is read and the level that is appended to.
static constexpr size_t kWavefrontRayBytes = 3 * 24 + 8 + 4 + 4;
// A parked Hitpoint: sort key and index (in and out of the sort), value3 and path; pos3 and normal3 only where hp9 is asked for
static constexpr size_t wavefront_parked_bytes(bool hp) { return 2 * (8 + 4) + 24 + 4 + (hp ? 48 : 0); }
static constexpr long long kWavefrontMaxSlots = (1ll << 31) - 1;  // the sort's size type, and a local root's 32 bits
static constexpr long long kWavefrontMinWork = 4096;

struct WavefrontCaps {
    long long rays;    // slots of each of the two ray queues
    long long parked;  // slots of the parked list
};
// Four parked slots to every slot of a ray queue: a ray tree's Hitpoints accumulate over its levels, a level's rays do not
static constexpr long long kWavefrontParkedPerRay = 4;
static constexpr long long wavefront_unit_bytes(bool hp) {
    return (long long)(2 * kWavefrontRayBytes) + kWavefrontParkedPerRay * (long long)wavefront_parked_bytes(hp);
}
static inline WavefrontCaps wavefront_caps(long long work_bytes, bool hp) {
    long long rays = work_bytes / wavefront_unit_bytes(hp);
    if (rays > kWavefrontMaxSlots / kWavefrontParkedPerRay) rays = kWavefrontMaxSlots / kWavefrontParkedPerRay;
    return WavefrontCaps{rays, kWavefrontParkedPerRay * rays};
}
static inline long long wavefront_bytes_used(const WavefrontCaps &c, bool hp) {
    return c.rays * (long long)(2 * kWavefrontRayBytes) + c.parked * (long long)wavefront_parked_bytes(hp);
}
// the smallest work_bytes whose capacities are at least (rays, parked): what a refusal names
static inline long long wavefront_bytes_for(long long rays, long long parked, bool hp) {
    const long long by_parked = (parked + kWavefrontParkedPerRay - 1) / kWavefrontParkedPerRay;
    return (rays > by_parked ? rays : by_parked) * wavefront_unit_bytes(hp);
}
// work_bytes = 0: room for a level of 2n rays and 8n Hitpoints, within min(1 GiB, an eighth of the device's memory) -- the
// bound of the project's other areas
static inline long long wavefront_default_work(long long n, long long device_bytes, bool hp) {
    long long bound = 1ll << 30;
    if (device_bytes / 8 < bound) bound = device_bytes / 8;
    const long long cap = n < (1ll << 40) ? n : (1ll << 40);
    long long w = wavefront_bytes_for(2 * cap, 8 * cap, hp);
    if (w < kWavefrontMinWork) w = kWavefrontMinWork;
    return w < bound ? w : bound;
}

// ---- slices ----
// The roots are processed in slices in ray order.  A slice starts with as many roots as a queue has slots (level 1 reads the
// caller's arrays, and most rays end before they have two children); a slice whose queue or parked list overflows is redone
// with half its roots -- nothing of it was written --, and the later slices keep the smaller size.  A slice of one root that
// overflows ends the call (CGRT_ERR_LIMIT).
struct WavefrontSlices {
    long long n = 0, begin = 0, size = 0;
    int slices = 0, halvings = 0;
    bool failed = false;
    WavefrontSlices(long long n_, const WavefrontCaps &c) : n(n_), size(c.rays > 1 ? c.rays : 1) {}
    bool done() const { return failed || begin >= n; }
    long long count() const { return size < n - begin ? size : n - begin; }  // roots of the current slice
    void finished() {
        begin += count();
        slices++;
    }
    // false: a single root did not fit
    bool overflowed() {
        if (count() <= 1) {
            failed = true;
            return false;
        }
        size = (count() + 1) / 2;
        halvings++;
        return true;
    }
};

// what the last cgrt_wavefront_rays on a handle did (cgrt_scene_last_wavefront, cgrt_scene_last_wavefront_rays)
struct WavefrontLast {
    long long slices = 0, halvings = 0;
    int levels = 0;
    long long rays[kWavefrontMaxDepth] = {};  // rays traced per level, over the slices that finished
};

#endif
