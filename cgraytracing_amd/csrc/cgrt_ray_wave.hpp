// The ray-query kernels' shared wave code: what trace_rays_body (cgrt_rays.hpp), occlusion_rays_kernel, bounce_rays_kernel,
// wavefront_step_kernel and aov_grid_kernel all do around their own walk -- the ray list they read, the workgroup's LDS prologue,
// the wave's draw from the block queue, the counter flush.  For this family only: trace_grid_body, the photon kernels and the
// primary walk keep their written-out forms (DESIGN.md sections 4.18 and 4.21).  Included by cgrt_rays.hpp behind cgrt_eye.hpp.
#ifndef CGRT_RAY_WAVE_HPP
#define CGRT_RAY_WAVE_HPP

// What every ray-list kernel reads of a ray list (cgrt_rays of cgrt.h): the head of RayParams, OccParams, BounceParams and
// WavefrontParams.  (Their `queue` stands where each struct had it: the kernel-argument layouts are the ones before RayInput.)
struct RayInput {
    long long n;
    const double *org, *dir;
    const unsigned long long *keys;  // nullptr: sample_key(pixel_key(seed, first_index + i), 0)
    long long first_index;
    uint64_t seed;
};
__device__ __forceinline__ uint64_t ray_default_key(const RayInput &in, long long u) {
    return in.keys ? (uint64_t)in.keys[u] : sample_key(pixel_key(in.seed, (uint64_t)(in.first_index + u)), 0);
}
// dir == 0: not a ray (cgrt_camera_rays' padding rows, an absent child of a bounce) -- nothing traced, nothing counted
__device__ __forceinline__ bool ray_is_none(V3 d) { return d.x == 0.0 && d.y == 0.0 && d.z == 0.0; }

__device__ __forceinline__ void st3(double *q, V3 v) {
    q[0] = v.x;
    q[1] = v.y;
    q[2] = v.z;
}

// The workgroup's dynamic LDS: wg_ask_trace's layout (cgrt_wg_lds.h) turned into pointers, the cached tree's nodes and the
// resident objects staged, one barrier.  Every thread of the workgroup calls it once, ahead of everything else.
template <int NT, bool TREES, bool BEZ, bool GLASS, bool SPILL>
__device__ __forceinline__ WgLdsPtrs ray_wg_begin(const DeviceScene &sc, unsigned char *lds_raw) {
    static_assert(NT == 256 || NT == 64, "workgroup = 4 waves or 1 wave");
    const WgLds lay = wg_lds(wg_ask_trace(NT, TREES, BEZ, GLASS, SPILL, false), sc);
    const WgLdsPtrs lds = wg_lds_carve(lay, lds_raw);
    if (lay.has.nodes)
        wg_stage16<NT>(const_cast<NodeRec *>(lds.aux.lnodes), sc.nodes + sc.trees[sc.cached_tree].node_begin,
                       sc.cached_nodes * (int)(sizeof(NodeRec) / 16));
    wg_stage16<NT>(lds.lobjs, sc.objs, sc.n_lds * (int)(sizeof(ObjRec) / 16));
    __syncthreads();
    return lds;
}

// The most rays of one call.  Blocks of 64 rays are numbered by a 32-bit counter that every wave advances twice more than it
// has blocks for (the draw that finds the queue empty has its successor in flight already): 2^30 blocks leave the persistent
// waves of any launch that room.
static constexpr long long kMaxRays = 1ll << 36;
static_assert(((kMaxRays + 63) >> 6) <= (1ll << 31), "block numbers and the waves' last draws fit the 32-bit queue counter");

// A wave's end of the block queue.  The queue is one counter, zeroed before the launch; a block is 64 consecutive rays.  Lane 0
// holds the number fetched ahead, so the next block's atomic is in flight while the current block is traced.  All of it but
// `ahead` is wave-uniform.
struct RayBlocks {
    unsigned int *head;
    long long n;
    unsigned n_blocks;
    long long ray_next, ray_end;  // rays [ray_next, ray_end) of the wave's block are still to be handed out
    bool empty;
    unsigned ahead;

    // the first request
    __device__ __forceinline__ void begin(unsigned int *queue, long long n_rays, int lane) {
        head = queue;
        n = n_rays;
        n_blocks = (unsigned)((n_rays + 63) >> 6);
        ray_next = ray_end = 0;
        empty = false;
        ahead = 0;
        if (lane == 0) ahead = atomicAdd(head, 1u);
    }
    // The ray index of a lane that wants one, m = the ballot of those lanes (not 0); all lanes call it.  A lane has a ray if its
    // index is below ray_end; lanes that drew beyond it draw again from the next block.
    __device__ __forceinline__ long long draw(unsigned long long m, int lane, unsigned long long lanes_below) {
        if (ray_next >= ray_end && !empty) {
            // the block fetched ahead, and the request for the one after it
            const unsigned blk = (unsigned)__builtin_amdgcn_readfirstlane((int)ahead);
            if (lane == 0) ahead = atomicAdd(head, 1u);
            if (blk >= n_blocks) {
                empty = true;
            } else {
                ray_next = (long long)blk << 6;
                ray_end = ray_next + 64 < n ? ray_next + 64 : n;
            }
        }
        const long long u = ray_next + (long long)__popcll(m & lanes_below);
        ray_next += (long long)__popcll(m);
        return u;
    }
    // nothing left anywhere
    __device__ __forceinline__ bool drained() const { return empty && ray_next >= ray_end; }
};

// A wave's counts into the workgroup's counters (wg_counters_begin's array; nullptr: nothing is counted): wave reduction, then
// one LDS atomic per wave and counter; the workgroup adds its sums once (wg_counters_end).  A wave that traced nothing adds
// nothing.  HITS = false: a query without Hitpoints issues no atomic for them.
template <bool STATS, bool HITS>
__device__ __forceinline__ void ray_counters_flush(unsigned long long *wc, int lane, uint32_t rays, uint32_t hits, uint32_t nodes,
                                                   uint32_t tris, uint32_t wave_iters) {
    if (!wc) return;
    unsigned long long rr = rays, hh = hits, nn = nodes, tt = tris;
    for (int off = 32; off > 0; off >>= 1) {
        rr += __shfl_xor(rr, off);
        if (HITS) hh += __shfl_xor(hh, off);
        if (STATS) {
            nn += __shfl_xor(nn, off);
            tt += __shfl_xor(tt, off);
        }
    }
    if (lane == 0 && (rr | (unsigned long long)wave_iters) != 0ull) {
        atomicAdd(&wc[CGRT_CNT_RAYS], rr);
        if (HITS) atomicAdd(&wc[CGRT_CNT_HITPOINTS], hh);
        atomicAdd(&wc[CGRT_CNT_WAVE_ITERS], (unsigned long long)wave_iters);
        if (STATS) {
            atomicAdd(&wc[CGRT_CNT_NODE_TESTS], nn);
            atomicAdd(&wc[CGRT_CNT_TRI_TESTS], tt);
        }
    }
}

#endif
