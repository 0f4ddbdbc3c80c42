// Wavefront trace of caller-supplied rays: wavefront_step_kernel and wavefront_sum_kernel (cgrt_wavefront_rays).  Part of
// libcgrt.so (cgrt_hip.hip).  One level of every ray tree per launch: the persistent-wave block queue, the scene walk and the
// step of bounce_rays_kernel (cgrt_bounce.hpp) -- the same intersect_scene and shade_step expressions, which are the parity
// contract --, but what the step yields stays on the device: a surviving child is appended to the next level's ray queue, a
// Hitpoint to the parked list with the key that sorts it into trace()'s emission order (cgrt_wavefront_plan.h).  After the last
// level the parked list is sorted and wavefront_sum_kernel adds each root's values in that order.  DESIGN.md section 4.17,
// "Wavefront trace".
#ifndef CGRT_WAVEFRONT_HPP
#define CGRT_WAVEFRONT_HPP
#include "cgrt_bounce.hpp"
#include "cgrt_wavefront_plan.h"

// A level's rays, struct of arrays: the caller's own at level 1 (adj, path and root nullptr: (1,1,1), 1 and the ray's index),
// a queue of the work memory afterwards
struct WavefrontQueue {
    double *org, *dir, *adj;  // [cap][3] each
    unsigned long long *key;  // [cap]
    uint32_t *path, *root;    // [cap]
};
// The parked Hitpoints: key and idx are the sort's input (idx[i] = i), pos and nrm nullptr where no records are asked for
struct WavefrontParked {
    unsigned long long *key;
    uint32_t *idx;
    double *val, *pos, *nrm;  // [cap][3] each
    uint32_t *path;
};
// Kernel arguments of wavefront_step_kernel
struct WavefrontParams {
    RayInput in;           // this level's rays
    const double *adj;    // nullptr: (1,1,1)
    const uint32_t *path;  // nullptr: 1
    const uint32_t *root;  // nullptr: the ray's index
    unsigned int *queue;   // head of the block queue (block = 64 consecutive rays), zeroed before the launch
    WavefrontQueue next;   // the next level's queue (not appended to at the last level)
    unsigned long long next_cap;
    WavefrontParked parked;  // key nullptr: Hitpoints are counted, not parked
    unsigned long long parked_cap;
    unsigned long long *next_count, *parked_count;  // slots asked for so far; beyond the capacity: the overflow signal
    double min_adj;
    int32_t last, pad_;  // the last level: no children
};

// The base of `count` consecutive slots for the whole wave: lane 0's atomic, broadcast.  Called with all 64 lanes active.
__device__ __forceinline__ unsigned long long wave_append_base(unsigned long long *counter, int lane, unsigned count) {
    unsigned long long b = 0ull;
    if (lane == 0) b = atomicAdd(counter, (unsigned long long)count);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// a child survives unless max(adj) < min_adj (strict: min_adj = 0 drops nothing)
__device__ __forceinline__ bool wavefront_keeps(V3 adj, double min_adj) { return !(adj.x < min_adj && adj.y < min_adj && adj.z < min_adj); }
__device__ __forceinline__ void wavefront_store_ray(const WavefrontQueue &q, unsigned long long slot, V3 o, V3 d, V3 adj, uint32_t path,
                                                    unsigned long long key, uint32_t root) {
    st3(q.org + 3 * slot, o);
    st3(q.dir + 3 * slot, d);
    st3(q.adj + 3 * slot, adj);
    q.key[slot] = key;
    q.path[slot] = path;
    q.root[slot] = root;
}

// bounce_rays_kernel's loop (cgrt_bounce.hpp) over one level's rays; its plan, LDS layout and launch bounds.  The appends are
// wave-aggregated: one ballot per list, one atomic per wave and list, every lane's slot from the lanes below it.  A slot at
// or beyond the capacity is not written; the advanced counter tells the host.  The order of the appends is not fixed and
// nothing depends on it: a ray's results depend on (org, dir, adj, path, key) alone and the Hitpoints are sorted by key.
template <bool TREES, bool BEZ, bool SPH, bool STATS, bool SPILL, int NT>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kTreeWaves : 4)) void wavefront_step_kernel(DeviceScene sc, WavefrontParams wp,
                                                                                                    unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long wg_cnt[CGRT_NCOUNTERS];
    unsigned long long *wc = wg_counters_begin(wg_cnt, counters);

    extern __shared__ __align__(16) unsigned char lds_raw[];
    const WgLdsPtrs lds = ray_wg_begin<NT, TREES, BEZ, false, SPILL>(sc, lds_raw);
    ObjRec *const lobjs = lds.lobjs;
    const LdsAux aux = lds.aux;

    const int lane = threadIdx.x & 63;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    RayBlocks blocks;
    blocks.begin(wp.queue, wp.in.n, lane);

    // the lane's ray
    uint32_t my_root = 0;
    bool have = false;
    uint64_t key = 0;
    RayState r;
    r.o = mk(0, 0, 0);
    r.d = mk(0, 0, 1);
    r.adj = mk(1, 1, 1);
    r.depth_left = 2;
    r.path = 1;
    uint32_t my_hits = 0, my_rays = 0, my_nodes = 0, my_tris = 0, wave_iters = 0;

    while (true) {
        const bool want = !have;
        const unsigned long long m = __ballot(want);
        if (m != 0ull) {
            const long long u = blocks.draw(m, lane, lanes_below);
            if (want && u < blocks.ray_end) {
                r.o = ld3(wp.in.org + 3 * u);
                r.d = ld3(wp.in.dir + 3 * u);
                r.path = wp.path ? wp.path[u] : 1u;
                const bool skip = ray_is_none(r.d) || r.path == 0u || r.path >= 0x80000000u;
                if (!skip) {  // (a ray that is none leaves nothing behind: the outputs are zeroed ahead of the sum)
                    my_root = wp.root ? wp.root[u] : (uint32_t)u;
                    key = ray_default_key(wp.in, u);
                    r.adj = wp.adj ? ld3(wp.adj + 3 * u) : mk(1, 1, 1);
                    r.depth_left = 2;  // the step never ends a ray for depth: the level count does
                    have = true;
                }
            }
        }
        if (__ballot(have) == 0ull) {
            if (blocks.drained()) break;
            continue;                                       // drew nothing traceable (block boundary, rays that are none)
        }
        wave_iters++;
        // All 64 lanes enter the scene walk together (lanes without a ray carry on == false)
        RayKey rk{key, r.path, false, 0u};
        const SceneHit hit = intersect_scene<TREES, BEZ, SPH, STATS, SPILL, /*PRE*/ false, /*HFONLY*/ false>(
            lobjs, sc.n_lds, sc.n_objs, sc, r.o, r.d, rk, have, aux, my_nodes, my_tris);
        // what the lane's step yields: a Hitpoint (hf at `at`, path hp_path), the reflected child (r), the refracted one (pe)
        bool is_hp = false, has_r = false, has_t = false;
        uint32_t hp_path = 0;
        V3 hf = mk(0, 0, 0);
        Pending pe;
        pe.path = 0;
        RaySurface at;
        at.P = mk(0, 0, 0);
        at.n = mk(0, 0, 0);
        if (have) {
            my_rays++;
            have = false;
            if (hit.id >= 0) {
                hp_path = r.path;
                const RayStep step = shade_step<true, SPILL>(sc, lobjs, hit, r, hf, pe, at);
                if (step == RAY_HITPOINT) {
                    my_hits++;
                    is_hp = true;
                } else if (!wp.last) {  // RAY_END cannot be: depth_left is 2 and the step has its glass branch
                    has_r = wavefront_keeps(r.adj, wp.min_adj);
                    has_t = step == RAY_SPLIT && wavefront_keeps(pe.adj, wp.min_adj);
                }
            }
        }
        // the appends, all lanes together
        const unsigned long long mh = wp.parked.key ? __ballot(is_hp) : 0ull;
        if (mh != 0ull) {
            const unsigned long long slot = wave_append_base(wp.parked_count, lane, (unsigned)__popcll(mh)) + (unsigned)__popcll(mh & lanes_below);
            if (is_hp && slot < wp.parked_cap) {
                wp.parked.key[slot] = wavefront_sort_key(my_root, hp_path);
                wp.parked.idx[slot] = (uint32_t)slot;
                wp.parked.path[slot] = hp_path;
                st3(wp.parked.val + 3 * slot, hf);
                if (wp.parked.pos) {
                    st3(wp.parked.pos + 3 * slot, at.P);
                    st3(wp.parked.nrm + 3 * slot, at.n);
                }
            }
        }
        const unsigned long long mr = __ballot(has_r), mt = __ballot(has_t);
        if ((mr | mt) != 0ull) {
            const unsigned nr = (unsigned)__popcll(mr);
            const unsigned long long base = wave_append_base(wp.next_count, lane, nr + (unsigned)__popcll(mt));
            const unsigned long long slot_r = base + (unsigned)__popcll(mr & lanes_below);
            const unsigned long long slot_t = base + nr + (unsigned)__popcll(mt & lanes_below);
            if (has_r && slot_r < wp.next_cap) wavefront_store_ray(wp.next, slot_r, r.o, r.d, r.adj, r.path, key, my_root);
            if (has_t && slot_t < wp.next_cap) wavefront_store_ray(wp.next, slot_t, pe.o, pe.d, pe.adj, pe.path, key, my_root);
        }
    }  // ray loop

    ray_counters_flush<STATS, true>(wc, lane, my_rays, my_hits, my_nodes, my_tris, wave_iters);
    wg_counters_end(wg_cnt, counters);
}

// Kernel arguments of wavefront_sum_kernel: a slice's parked Hitpoints behind their sorted keys
struct WavefrontSumParams {
    long long m;                          // sorted records
    const unsigned long long *key;        // [m] sorted
    const uint32_t *idx;                  // [m] the parked slot of each
    const double *val, *pos, *nrm;        // the parked arrays (pos, nrm: nullptr unless hp9)
    const uint32_t *path;
    long long first_root;                 // the slice's first ray
    double *acc3;                         // the call's outputs, each may be nullptr
    uint32_t *nhit;
    double *hp9;
    long long *hp_ray;
    uint32_t *hp_path;
    unsigned long long hp_base, hp_cap;   // records of the earlier slices; records at or beyond hp_cap are dropped
};
// One thread per sorted record.  The thread of a root's first record adds the root's values one after the other in fp64 from
// 0.0 -- the order in which trace() adds them, no tree, no reassociation -- and writes acc3 and nhit (roots without Hitpoints
// were zeroed ahead).  Every thread gathers its own record behind the earlier slices'.
__global__ __launch_bounds__(256) void wavefront_sum_kernel(WavefrontSumParams sp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= sp.m) return;
    const uint32_t root = wavefront_key_root(sp.key[i]);
    if ((sp.acc3 || sp.nhit) && (i == 0 || wavefront_key_root(sp.key[i - 1]) != root)) {
        V3 acc = mk(0.0, 0.0, 0.0);
        uint32_t cnt = 0;
        for (long long j = i; j < sp.m && wavefront_key_root(sp.key[j]) == root; j++) {
            acc = acc + ld3(sp.val + 3 * (long long)sp.idx[j]);
            cnt++;
        }
        const long long ray = sp.first_root + (long long)root;
        if (sp.acc3) st3(sp.acc3 + 3 * ray, acc);
        if (sp.nhit) sp.nhit[ray] = cnt;
    }
    const unsigned long long at = sp.hp_base + (unsigned long long)i;
    if (at < sp.hp_cap) {
        const long long k = (long long)sp.idx[i];
        if (sp.hp9) {
            st3(sp.hp9 + 9 * at, ld3(sp.val + 3 * k));
            st3(sp.hp9 + 9 * at + 3, ld3(sp.pos + 3 * k));
            st3(sp.hp9 + 9 * at + 6, ld3(sp.nrm + 3 * k));
        }
        if (sp.hp_ray) sp.hp_ray[at] = sp.first_root + (long long)root;
        if (sp.hp_path) sp.hp_path[at] = sp.path[k];
    }
}
// a finished slice's counters, added to the caller's
__global__ void wavefront_add_counters_kernel(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src) {
    if (threadIdx.x < CGRT_NCOUNTERS && src[threadIdx.x] != 0ull) dst[threadIdx.x] += src[threadIdx.x];
}

#endif
