// Bounce queries for caller-supplied rays: bounce_rays_kernel (cgrt_bounce_rays).  Part of libcgrt.so (cgrt_hip.hip).
// One step of trace() per ray: the scene walk of the nearest-hit query (intersect_scene, cgrt_scene_walk.hpp), then shade_step
// (cgrt_rays.hpp) -- the expressions of the full trace in their order, so a caller's depth loop over this kernel gives the bits
// of trace_rays_kernel.  What the step yields leaves the kernel: the Hitpoint's value, or the child rays with their throughput,
// their place in the ray tree and their key.  No depth limit, no pending rays, no sums.  DESIGN.md section 4.17, "Bounce query".
#ifndef CGRT_BOUNCE_HPP
#define CGRT_BOUNCE_HPP
#include "cgrt_rays.hpp"

// Kernel arguments of bounce_rays_kernel (cgrt_rays / cgrt_bounce of cgrt.h; adj, path and every output pointer may be nullptr)
struct BounceParams {
    long long n;
    const double *org, *dir;
    const unsigned long long *keys;  // nullptr: sample_key(pixel_key(seed, first_index + i), 0)
    long long first_index;
    uint64_t seed;
    const double *adj;     // nullptr: (1,1,1)
    const uint32_t *path;  // nullptr: 1
    uint8_t *step;
    int32_t *hit_obj;
    double *hit_t, *pos, *normal, *value;
    double *child_org, *child_dir, *child_adj;  // [2n][3]: slot i the reflected child of ray i, slot n + i the refracted one
    uint32_t *child_path;
    unsigned long long *child_keys;
    unsigned int *queue;  // head of the block queue (block = 64 consecutive rays), zeroed before the launch
};
static_assert(RAY_HITPOINT == 1 && RAY_CONTINUE == 2 && RAY_SPLIT == 3, "CGRT_STEP_* of cgrt.h are shade_step's values");

__device__ __forceinline__ void st3(double *q, V3 v) {
    q[0] = v.x;
    q[1] = v.y;
    q[2] = v.z;
}

// What ray u leaves behind, through its own index (the lanes of a wave hold arbitrary rays), in three parts so that each leaves
// the registers as soon as it is known.  Each test of a pointer is one of a kernel argument: wave-uniform, a scalar branch
// around the store.  An absent child is zeros: dir = 0, path 0, key 0.
__device__ __forceinline__ void bounce_store_hit(const BounceParams &bp, long long u, int32_t obj, double t, V3 P, V3 n) {
    if (bp.hit_obj) bp.hit_obj[u] = obj;
    if (bp.hit_t) bp.hit_t[u] = t;
    if (bp.pos) st3(bp.pos + 3 * u, P);
    if (bp.normal) st3(bp.normal + 3 * u, n);
}
__device__ __forceinline__ void bounce_store_child(const BounceParams &bp, long long slot, V3 o, V3 d, V3 adj, uint32_t path,
                                                   unsigned long long key) {
    if (bp.child_org) st3(bp.child_org + 3 * slot, o);
    if (bp.child_dir) st3(bp.child_dir + 3 * slot, d);
    if (bp.child_adj) st3(bp.child_adj + 3 * slot, adj);
    if (bp.child_path) bp.child_path[slot] = path;
    if (bp.child_keys) bp.child_keys[slot] = key;
}
__device__ __forceinline__ void bounce_store_no_child(const BounceParams &bp, long long slot) {
    const V3 z = mk(0, 0, 0);
    bounce_store_child(bp, slot, z, z, z, 0u, 0ull);
}
// a miss, or a ray that is not traced
__device__ __forceinline__ void bounce_store_none(const BounceParams &bp, long long u) {
    const V3 z = mk(0, 0, 0);
    if (bp.step) bp.step[u] = (uint8_t)0;
    bounce_store_hit(bp, u, -1, 0.0, z, z);
    if (bp.value) st3(bp.value + 3 * u, z);
    bounce_store_no_child(bp, u);
    bounce_store_no_child(bp, u + bp.n);
}

// Persistent workgroups of NT threads over the block queue of trace_rays_body (cgrt_rays.hpp): a wave draws blocks of 64
// consecutive rays from one queue counter (lane 0's atomic, the next block's already in flight while the current one is walked);
// a lane without a ray takes the next ray of the wave's block, and lanes that drew beyond the block's end draw again from the
// next one.  A ray is one walk and one step, so a lane is free again after every trip; rays that are not traced (dir = 0, a
// path outside [1, 2^31)) get the results of a miss where they are drawn and cost no walk unless the whole wave drew such rays.
// Dynamic LDS: wg_ask_trace's layout without pending rays (cgrt_wg_lds.h), that of trace_rays_kernel<..., FIRST>.
template <bool TREES, bool BEZ, bool SPH, bool STATS, bool SPILL, int NT>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kTreeWaves : 4)) void bounce_rays_kernel(DeviceScene sc, BounceParams bp,
                                                                                                 unsigned long long *__restrict__ counters) {
    static_assert(NT == 256 || NT == 64, "workgroup = 4 waves or 1 wave");
    __shared__ unsigned long long wg_cnt[CGRT_NCOUNTERS];
    unsigned long long *wc = wg_counters_begin(wg_cnt, counters);

    extern __shared__ __align__(16) unsigned char lds_raw[];
    const WgLds lay = wg_lds(wg_ask_trace(NT, TREES, BEZ, false, SPILL, false), sc);
    const WgLdsPtrs lds = wg_lds_carve(lay, lds_raw);
    ObjRec *const lobjs = lds.lobjs;
    const LdsAux aux = lds.aux;
    if (lay.has.nodes)
        wg_stage16<NT>(const_cast<NodeRec *>(aux.lnodes), sc.nodes + sc.trees[sc.cached_tree].node_begin,
                       sc.cached_nodes * (int)(sizeof(NodeRec) / 16));
    wg_stage16<NT>(lobjs, sc.objs, sc.n_lds * (int)(sizeof(ObjRec) / 16));
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const unsigned n_blocks = (unsigned)((bp.n + 63) >> 6);

    // the wave's block: rays [ray_next, ray_end) are still to be handed out (wave-uniform)
    long long ray_next = 0, ray_end = 0;
    bool queue_empty = false;
    unsigned block_ahead = 0;
    if (lane == 0) block_ahead = atomicAdd(bp.queue, 1u);

    // the lane's ray
    long long my_ray = 0;
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
            if (ray_next >= ray_end && !queue_empty) {
                // the block fetched ahead, and the request for the one after it
                const unsigned blk = (unsigned)__builtin_amdgcn_readfirstlane((int)block_ahead);
                if (lane == 0) block_ahead = atomicAdd(bp.queue, 1u);
                if (blk >= n_blocks) {
                    queue_empty = true;
                } else {
                    ray_next = (long long)blk << 6;
                    ray_end = ray_next + 64 < bp.n ? ray_next + 64 : bp.n;
                }
            }
            const long long u = ray_next + (long long)__popcll(m & lanes_below);
            ray_next += (long long)__popcll(m);  // lanes that drew beyond ray_end draw again from the next block
            if (want && u < ray_end) {
                r.o = ld3(bp.org + 3 * u);
                r.d = ld3(bp.dir + 3 * u);
                r.path = bp.path ? bp.path[u] : 1u;
                const bool skip = (r.d.x == 0.0 && r.d.y == 0.0 && r.d.z == 0.0) || r.path == 0u || r.path >= 0x80000000u;
                if (skip) {
                    bounce_store_none(bp, u);  // not a ray: the results of a miss, nothing counted
                } else {
                    my_ray = u;
                    key = bp.keys ? (uint64_t)bp.keys[u] : sample_key(pixel_key(bp.seed, (uint64_t)(bp.first_index + u)), 0);
                    r.adj = bp.adj ? ld3(bp.adj + 3 * u) : mk(1, 1, 1);
                    r.depth_left = 2;  // the step never ends a ray for depth: the caller decides when to stop
                    have = true;
                }
            }
        }
        if (__ballot(have) == 0ull) {
            if (queue_empty && ray_next >= ray_end) break;  // nothing left anywhere
            continue;                                       // drew nothing traceable (block boundary, rays that are none)
        }
        wave_iters++;
        // All 64 lanes enter the scene walk together (lanes without a ray carry on == false)
        RayKey rk{key, r.path, false, 0u};
        const SceneHit hit = intersect_scene<TREES, BEZ, SPH, STATS, SPILL, /*PRE*/ false, /*HFONLY*/ false>(
            lobjs, sc.n_lds, sc.n_objs, sc, r.o, r.d, rk, have, aux, my_nodes, my_tris);
        if (have) {
            my_rays++;
            have = false;
            if (hit.id < 0) {
                bounce_store_none(bp, my_ray);
            } else {
                V3 n = hit.n;
                if (dot(n, r.d) > 0) n = -n;  // main.cpp:73-76
                bounce_store_hit(bp, my_ray, hit.id, hit.t, r.o + r.d * hit.t /* main.cpp:68 */, n);
                V3 hf;
                Pending pe;
                RaySurface at;
                const RayStep step = shade_step<true, SPILL>(sc, lobjs, hit, r, hf, pe, at);
                if (bp.step) bp.step[my_ray] = (uint8_t)step;
                if (step == RAY_HITPOINT) {
                    my_hits++;
                    if (bp.value) st3(bp.value + 3 * my_ray, hf);
                    bounce_store_no_child(bp, my_ray);
                    bounce_store_no_child(bp, my_ray + bp.n);
                } else {  // RAY_END cannot be: depth_left is 2 and the step has its glass branch
                    if (bp.value) st3(bp.value + 3 * my_ray, mk(0, 0, 0));
                    bounce_store_child(bp, my_ray, r.o, r.d, r.adj, r.path, key);  // the reflected child
                    if (step == RAY_SPLIT) bounce_store_child(bp, my_ray + bp.n, pe.o, pe.d, pe.adj, pe.path, key);
                    else bounce_store_no_child(bp, my_ray + bp.n);
                }
            }
        }
    }  // ray loop

    if (wc) {
        // wave reduction, then one LDS atomic per wave and counter; the workgroup adds its sums once (wg_counters_end)
        unsigned long long rr = my_rays, hh = my_hits, nn = my_nodes, tt = my_tris;
        for (int off = 32; off > 0; off >>= 1) {
            rr += __shfl_xor(rr, off);
            hh += __shfl_xor(hh, off);
            if (STATS) {
                nn += __shfl_xor(nn, off);
                tt += __shfl_xor(tt, off);
            }
        }
        if (lane == 0 && (rr | (unsigned long long)wave_iters) != 0ull) {
            atomicAdd(&wc[CGRT_CNT_RAYS], rr);
            atomicAdd(&wc[CGRT_CNT_HITPOINTS], hh);
            atomicAdd(&wc[CGRT_CNT_WAVE_ITERS], (unsigned long long)wave_iters);
            if (STATS) {
                atomicAdd(&wc[CGRT_CNT_NODE_TESTS], nn);
                atomicAdd(&wc[CGRT_CNT_TRI_TESTS], tt);
            }
        }
    }
    wg_counters_end(wg_cnt, counters);
}

#endif
