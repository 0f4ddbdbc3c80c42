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
    RayInput in;
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
    bounce_store_no_child(bp, u + bp.in.n);
}

// Persistent workgroups of NT threads over the block queue (RayBlocks, cgrt_ray_wave.hpp): a wave draws blocks of 64
// consecutive rays from one queue counter (lane 0's atomic, the next block's already in flight while the current one is walked);
// a lane without a ray takes the next ray of the wave's block, and lanes that drew beyond the block's end draw again from the
// next one.  A ray is one walk and one step, so a lane is free again after every trip; rays that are not traced (dir = 0, a
// path outside [1, 2^31)) get the results of a miss where they are drawn and cost no walk unless the whole wave drew such rays.
// Dynamic LDS: wg_ask_trace's layout without pending rays (cgrt_wg_lds.h), that of trace_rays_kernel<..., FIRST>.
template <bool TREES, bool BEZ, bool SPH, bool STATS, bool SPILL, int NT>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kTreeWaves : 4)) void bounce_rays_kernel(DeviceScene sc, BounceParams bp,
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
    blocks.begin(bp.queue, bp.in.n, lane);

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
            const long long u = blocks.draw(m, lane, lanes_below);
            if (want && u < blocks.ray_end) {
                r.o = ld3(bp.in.org + 3 * u);
                r.d = ld3(bp.in.dir + 3 * u);
                r.path = bp.path ? bp.path[u] : 1u;
                const bool skip = ray_is_none(r.d) || r.path == 0u || r.path >= 0x80000000u;
                if (skip) {
                    bounce_store_none(bp, u);  // not a ray: the results of a miss, nothing counted
                } else {
                    my_ray = u;
                    key = ray_default_key(bp.in, u);
                    r.adj = bp.adj ? ld3(bp.adj + 3 * u) : mk(1, 1, 1);
                    r.depth_left = 2;  // the step never ends a ray for depth: the caller decides when to stop
                    have = true;
                }
            }
        }
        if (__ballot(have) == 0ull) {
            if (blocks.drained()) break;
            continue;  // drew nothing traceable (block boundary, rays that are none)
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
                    bounce_store_no_child(bp, my_ray + bp.in.n);
                } else {  // RAY_END cannot be: depth_left is 2 and the step has its glass branch
                    if (bp.value) st3(bp.value + 3 * my_ray, mk(0, 0, 0));
                    bounce_store_child(bp, my_ray, r.o, r.d, r.adj, r.path, key);  // the reflected child
                    if (step == RAY_SPLIT) bounce_store_child(bp, my_ray + bp.in.n, pe.o, pe.d, pe.adj, pe.path, key);
                    else bounce_store_no_child(bp, my_ray + bp.in.n);
                }
            }
        }
    }  // ray loop

    ray_counters_flush<STATS, true>(wc, lane, my_rays, my_hits, my_nodes, my_tris, wave_iters);
    wg_counters_end(wg_cnt, counters);
}

#endif
