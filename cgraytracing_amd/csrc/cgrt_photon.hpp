// Photon pass -- included at the end of cgrt_hip.hip.
//
// Reference: render() main.cpp:223-258 + trace(flag=false) main.cpp:101-128,158-165 + Hashtable hash.h:20-70.
// The reference runs eight OpenMP threads that race on the hitpoints and seed rand() from the clock, so its
// output is not reproducible even against itself.  The semantics implemented -- and pinned bit for bit by the
// oracle and by golden vectors from the compiled reference run on ONE thread -- are its serial meaning:
// photons 0..N-1 one after another, photon i drawing from the keyed stream (seed, i, 0, 'phot') in the
// reference's call order, each diffuse hit updating the hitpoints of the 27 surrounding hash cells.
//
// A hitpoint's evolution (r2, n, flux) depends only on the ORDERED list of photon events that reach it, and
// photon paths do not depend on the hitpoints.  So the serial result is computed in parallel as
//   1. photon_trace_kernel   : one lane per photon; every diffuse hit appends an event {P, n, flux} at a slot
//                              derived from (photon, segment), i.e. in serial order;
//   2. photon_pairs_kernel   : one lane per event; walks the reference's own candidate set -- the buckets the 27
//                              cells hash to (hash.h:35-37), collisions included -- and emits (hitpoint, order)
//                              pairs that pass the static tests (normal, distance against the radius the hitpoint
//                              had at the start of the batch, which only shrinks);
//   3. radix sort of the pairs by (hitpoint, order)                                     [rocprim]
//   4. photon_apply_kernel   : one lane per hitpoint; replays its events in order with the reference's update
//                              (main.cpp:116-122), re-checking the distance against the current radius.
// Hitpoints are kept sorted by (bucket, emission order) = the reference's table order, which is also the order of
// its final gather (main.cpp:252-258); the image is summed per pixel in that order.
#include <rocprim/device/device_radix_sort.hpp>

#include <climits>
#include <memory>

namespace {

constexpr int kSegStride = 8;          // event slots per photon (MAX_DEPTH = 5 segments)
#ifndef CGRT_PHOTON_WAVES
#define CGRT_PHOTON_WAVES 4
#endif
constexpr int kPhotonWaves = CGRT_PHOTON_WAVES;  // waves per SIMD photon_trace_kernel<false> is compiled for
constexpr double kPiRef = 3.14159265358979;  // main.cpp:26

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
__device__ __forceinline__ unsigned ref_hash(int ix, int iy, int iz, int hashsize) {
    return (((unsigned)ix * 73856093u) ^ ((unsigned)iy * 19349663u) ^ ((unsigned)iz * 83492791u)) % (unsigned)hashsize;
}
__device__ __forceinline__ void ref_coord(double x, double y, double z, double cl, int &ix, int &iy, int &iz) {
    ix = (int)floor((x - (-35.0)) / cl);
    iy = (int)floor((y - (-35.0)) / cl);
    iz = (int)floor((z - (-15.0)) / cl);
}

// hitpoint records from the eye pass (10 doubles: f pos normal label) -> sort keys (bucket, emission order)
__global__ void hp_keys_kernel(const double *__restrict__ rec, long long n, HashArgs ha, int rows_w, int spp,
                               unsigned long long *__restrict__ keys, unsigned int *__restrict__ vals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *q = rec + 10 * i;
    int ix, iy, iz;
    ref_coord(q[3], q[4], q[5], ha.celllength, ix, iy, iz);
    const unsigned long long b = ref_hash(ix, iy, iz, ha.hashsize);
    const unsigned long long lab = (unsigned long long)q[9];
    const unsigned long long seq = lab & 15ull, ps = lab >> 4;
    const unsigned long long smp = ps / (unsigned long long)rows_w, pix = ps % (unsigned long long)rows_w;
    // serial emission order of the reference's eye pass: pixel-major, then sample, then DFS position
    const unsigned long long em = ((pix * (unsigned long long)spp + smp) << 4) | seq;
    keys[i] = (b << 44) | em;  // bucket < 2^20, emission key < 2^44
    vals[i] = (unsigned int)i;
}
// sorted order -> structure of arrays + per-bucket start offsets
__global__ void hp_gather_kernel(const double *__restrict__ rec, const unsigned long long *__restrict__ keys,
                                 const unsigned int *__restrict__ vals, long long n, double r2_init,
                                 double *__restrict__ hp /* n x 16 */, double *__restrict__ hps /* n x 8 */,
                                 int *__restrict__ bucket_of) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *q = rec + 10 * (long long)vals[i];
    double *o = hp + 16 * i;
    const unsigned long long em = keys[i] & ((1ull << 44) - 1ull);
    o[0] = (double)(em >> 4);  // pixel*spp + sample (decoded by the caller)
    o[1] = (double)(em & 15ull);
    for (int k = 0; k < 9; k++) o[2 + k] = q[k];
    o[11] = 0; o[12] = 0; o[13] = 0;
    o[14] = r2_init;
    o[15] = 0;
    // what the pair search reads, in half a cache line: {pos, batch-start r2} (every candidate), {normal} (those the
    // radius screen lets through)
    double *c = hps + 8 * i;
    for (int k = 0; k < 3; k++) c[k] = q[3 + k];
    c[3] = r2_init;
    for (int k = 0; k < 3; k++) c[4 + k] = q[6 + k];
    c[7] = 0;
    bucket_of[i] = (int)(keys[i] >> 44);
}
// ---- the same table for Hitpoints of a ray buffer (cgrt_ppm_session_create_rays).  Order contract: inside a bucket the
// Hitpoints stand in the insertion order of a serial loop over texels, for each texel over its rays in ray-index order, for
// each ray in emission order.  (bucket, texel, ray, seq) does not fit one 64-bit key, and the radix sort is stable: the
// records are sorted by their label (ray << 4 | seq) first, then by (bucket << 32 | texel).  For rays in cgrt_camera_rays'
// order without a pixel array (ray = sample * npix + texel) this is hp_keys_kernel's order.
__device__ __forceinline__ unsigned long long ray_texel(const long long *__restrict__ pixel, unsigned long long ray, long long npix) {
    return pixel ? (unsigned long long)pixel[ray] : ray % (unsigned long long)npix;  // (a ray with a Hitpoint has a texel >= 0)
}
__global__ void hp_ray_label_keys_kernel(const double *__restrict__ rec, long long n, unsigned long long *__restrict__ keys,
                                         unsigned int *__restrict__ vals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = (unsigned long long)rec[10 * i + 9];  // < 2^40
    vals[i] = (unsigned int)i;
}
// vals: record indices in label order; keys out: (bucket << 32) | texel, in that order
__global__ void hp_ray_bucket_keys_kernel(const double *__restrict__ rec, const unsigned int *__restrict__ vals, long long n, HashArgs ha,
                                          const long long *__restrict__ pixel, long long npix, unsigned long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *q = rec + 10 * (long long)vals[i];
    int ix, iy, iz;
    ref_coord(q[3], q[4], q[5], ha.celllength, ix, iy, iz);
    const unsigned long long b = ref_hash(ix, iy, iz, ha.hashsize);
    keys[i] = (b << 32) | ray_texel(pixel, (unsigned long long)q[9] >> 4, npix);  // bucket < 2^20, texel < 2^31
}
// hp_gather_kernel for that order: hp[0] = the ray index, hp[1] = the emission index
__global__ void hp_ray_gather_kernel(const double *__restrict__ rec, const unsigned long long *__restrict__ keys,
                                     const unsigned int *__restrict__ vals, long long n, double r2_init, double *__restrict__ hp,
                                     double *__restrict__ hps, int *__restrict__ bucket_of) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *q = rec + 10 * (long long)vals[i];
    double *o = hp + 16 * i;
    const unsigned long long lab = (unsigned long long)q[9];
    o[0] = (double)(lab >> 4);
    o[1] = (double)(lab & 15ull);
    for (int k = 0; k < 9; k++) o[2 + k] = q[k];
    o[11] = 0; o[12] = 0; o[13] = 0;
    o[14] = r2_init;
    o[15] = 0;
    double *c = hps + 8 * i;
    for (int k = 0; k < 3; k++) c[k] = q[3 + k];
    c[3] = r2_init;
    for (int k = 0; k < 3; k++) c[4 + k] = q[6 + k];
    c[7] = 0;
    bucket_of[i] = (int)(keys[i] >> 32);
}
__global__ void bucket_start_kernel(const int *__restrict__ bucket_of, long long n, int hashsize, int *__restrict__ bstart) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > hashsize) return;
    long long lo = 0, hi = n;  // first index with bucket_of >= b
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (bucket_of[mid] < b) lo = mid + 1; else hi = mid;
    }
    bstart[b] = (int)lo;
}

// sampling.h:11-29 on the photon's sequential stream
__device__ __forceinline__ V3 sample_sphere(Stream &rs) {
    while (true) {
        const double x = rs.u01() * 2.0 - 1, y = rs.u01() * 2.0 - 1, z = rs.u01() * 2.0 - 1;
        if (x * x + y * y + z * z <= 1) return normalized(mk(x, y, z));
    }
}

// ---- the built-in emitter, main.cpp:240-246 --------------------------------------------------------------------------
// What photon `index` of cgrt_photons starts with: its origin (the light, jittered in x and z), a direction uniform over the
// sphere (sampling.h:11-20 by rejection), the flux power * 4 PI in each channel, and the stream its bounces go on drawing from
// (rs.n = the draws the emission consumed: 2 + 3 per attempt at the direction).  ONE function is photon_trace_kernel's
// emission, cgrt_photon_emit's kernel and cgrt_photon_emit_host's loop: the device's normalized() and the host's sqrt and
// division are correctly rounded, the rest is plain IEEE arithmetic without contraction, so all three give the same bits
// (as camera_ray does for cgrt_camera_rays / _host).
struct EmitArgs {
    double light[3], jitter, power;
    uint64_t seed;
};
struct EmittedPhoton {
    double o[3], d[3], flux[3];
};
__host__ __device__ __forceinline__ EmittedPhoton photon_emit(const EmitArgs &ea, Stream &rs) {
    EmittedPhoton e;
    const double a = rs.u01() * (2 * ea.jitter) - ea.jitter;
    const double b = rs.u01() * (2 * ea.jitter) - ea.jitter;
    e.o[0] = ea.light[0] + a;
    e.o[1] = ea.light[1] + 0;
    e.o[2] = ea.light[2] + b;
    while (true) {
        double x = rs.u01() * 2.0 - 1, y = rs.u01() * 2.0 - 1, z = rs.u01() * 2.0 - 1;
        if (x * x + y * y + z * z <= 1) {
            camera_normalize(x, y, z);  // vec3.h:36-44 (cgrt_rays.hpp: normalized() on the device)
            e.d[0] = x; e.d[1] = y; e.d[2] = z;
            break;
        }
    }
    e.flux[0] = e.flux[1] = e.flux[2] = ea.power * (kPiRef * 4.0);
    return e;
}
__host__ __device__ __forceinline__ uint64_t photon_key(uint64_t seed, uint64_t index) { return stream_key(seed, index, 0, 0x70686f74ull); }

// What photon_trace_kernel<.., RAYS = true> reads instead: the caller's arrays (cgrt_photon_rays), already moved to the batch's
// first photon; keys / draws may be null
struct PhotonRayArgs {
    const double *org, *dir, *flux;
    const unsigned long long *keys;
    const unsigned int *draws;
};
// Component j of lane's triple in an [n][3] array of doubles, read so that a wave reads whole lines: the wave's 64 triples are
// 192 consecutive doubles (1536 B = twelve 128-byte lines when the array is line-aligned), fetched as three loads of 64
// consecutive doubles -- every load instruction covers four whole lines, where a lane reading its own triple would touch all
// twelve lines three times, a third of each -- and handed to their lanes by three cross-lane reads per component.  `a` points at
// the wave's first triple, nd = 3 * (photons of this wave that exist); called by all 64 lanes.
__device__ __forceinline__ V3 wave_load3(const double *__restrict__ a, int nd, int lane) {
    double r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] = (64 * k + lane < nd) ? a[64 * k + lane] : 0.0;
    double c[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int e = 3 * lane + j, src = e & 63, k = e >> 6;
        const double v0 = __shfl(r[0], src), v1 = __shfl(r[1], src), v2 = __shfl(r[2], src);
        c[j] = k == 0 ? v0 : (k == 1 ? v1 : v2);
    }
    return mk(c[0], c[1], c[2]);
}

// whether photon_trace_kernel<false> keeps the wide walk's first stack entries in LDS: 32 KiB per workgroup, taken only
// while four workgroups (its 4 waves/SIMD) still fit a CU's 160 KiB beside the object list
__host__ __device__ inline bool photon_lds_stack(const DeviceScene &sc) { return sc.has_wide && sc.n_objs <= 56; }
// 1. photon paths.  events: count*kSegStride records of 9 doubles; valid: same count of bytes.
// RAYS: the photons' starts come from the caller's arrays (cgrt_ppm_session_add_photon_rays) instead of the built-in emitter;
// a compile-time choice, so neither form carries the other's code or a branch for it.
template <bool BEZ, bool SPILL = false, bool RAYS = false>
__global__ __launch_bounds__(kThreads, BEZ ? 2 : kPhotonWaves) void photon_trace_kernel(DeviceScene sc, PhotonArgs pa, double *__restrict__ events,
                                                                   unsigned char *__restrict__ valid, PhotonRayArgs ra) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    ObjRec *lobjs = reinterpret_cast<ObjRec *>(lds_raw);
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(sc.objs);
        uint4 *dst = reinterpret_cast<uint4 *>(lobjs);
        const int n16 = sc.n_lds * (int)(sizeof(ObjRec) / 16);
        for (int k = threadIdx.x; k < n16; k += kThreads) dst[k] = src[k];
    }
    __syncthreads();
    unsigned char *lrest = lds_raw + obj_list_lds(sc, kThreads / 64);
    // BEZ: one BezLds per wave behind the object list; the Newton starts continue the photon's own stream
    LdsAux aux{BEZ ? reinterpret_cast<volatile BezLds *>(lrest) + (threadIdx.x >> 6) : nullptr, nullptr};
    if (SPILL) aux.spill = lobjs + sc.n_lds + (threadIdx.x >> 6);
    // without Bezier objects: the first entries of the 4-wide walk's stack live in LDS behind the object list, as in the eye pass
    if (!BEZ && !SPILL && photon_lds_stack(sc)) aux.wstack = reinterpret_cast<uint2 *>(lrest);  // (the SPILL launch reserves no room for it)
    const int p = blockIdx.x * kThreads + threadIdx.x;
    bool alive = p < pa.count;
    Stream rs(photon_key(pa.seed, (uint64_t)(pa.first + (alive ? p : 0))));
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1), flux = mk(0, 0, 0);
    if (RAYS) {
        // all 64 lanes take part in the loads (the cross-lane reads need them); a wave beyond the batch has nothing to read
        const int lane = threadIdx.x & 63, wave_first = p - lane;
        const int nd = 3 * (pa.count - wave_first < 64 ? pa.count - wave_first : 64);
        if (nd > 0) {  // wave-uniform
            o = wave_load3(ra.org + 3 * (size_t)wave_first, nd, lane);
            d = wave_load3(ra.dir + 3 * (size_t)wave_first, nd, lane);
            flux = wave_load3(ra.flux + 3 * (size_t)wave_first, nd, lane);
        }
        if (alive) {
            if (ra.keys) rs.key = ra.keys[p];  // (uniform: a kernel argument)
            if (ra.draws) rs.n = ra.draws[p];
            alive = !(d.x == 0 && d.y == 0 && d.z == 0);  // emitted, goes nowhere: counted by the host, never traced
        }
        if (!alive) {  // an inactive lane rides along with what the built-in form gives it
            o = mk(0, 0, 0);
            d = mk(0, 0, 1);
            flux = mk(0, 0, 0);
        }
    } else if (alive) {  // main.cpp:240-246
        EmitArgs ea;
        ea.light[0] = pa.light[0]; ea.light[1] = pa.light[1]; ea.light[2] = pa.light[2];
        ea.jitter = pa.jitter; ea.power = pa.power; ea.seed = pa.seed;
        const EmittedPhoton e = photon_emit(ea, rs);
        o = mk(e.o[0], e.o[1], e.o[2]);
        d = mk(e.d[0], e.d[1], e.d[2]);
        flux = mk(e.flux[0], e.flux[1], e.flux[2]);
    }
    uint32_t dn = 0, dt = 0;
    for (int seg = 0; seg < pa.max_depth; seg++) {
        if (__ballot(alive) == 0ull) break;
        RayKey rk{rs.key, 1, true, rs.n};
        const SceneHit hit = intersect_scene<true, BEZ, false, false, SPILL>(lobjs, sc.n_lds, sc.n_objs, sc, o, d, rk, alive, aux, dn, dt);
        if (BEZ) rs.n = rk.n0;
        if (!alive) continue;
        if (hit.id < 0) {
            alive = false;
            continue;
        }
        const ObjMat ob = load_mat<SPILL>(lobjs, sc.n_lds, sc.objs, hit.id);
        const V3 P = o + d * hit.t;
        V3 n = hit.n;
        const V3 n_old = n;
        bool into = true;
        if (dot(n, d) > 0) {
            n = -n;
            into = false;
        }
        V3 f = ob.col;
        if (ob.kind == KIND_PLANE && ob.tex >= 0) {
            V3 c;
            if (texture_color(sc.texs[ob.tex], sc.texels, P, c)) f = c;
        }
        const double pmax = (f.x > f.y && f.x > f.z) ? f.x : (f.y > f.z ? f.y : f.z);  // util.h:16-27, main.cpp:79
        const double refl = ob.refl, transp = ob.transp;
        if (refl < kEps && transp < kEps) {
            // diffuse: record the event the serial loop of main.cpp:103-125 would process now
            const size_t slot = (size_t)p * kSegStride + seg;
            double *e = events + 9 * slot;
            e[0] = P.x; e[1] = P.y; e[2] = P.z;
            e[3] = n.x; e[4] = n.y; e[5] = n.z;
            e[6] = flux.x; e[7] = flux.y; e[8] = flux.z;
            valid[slot] = 1;
            V3 nd;
            while (true) {  // uniform_sampling_halfsphere, sampling.h:22-29
                nd = sample_sphere(rs);
                if (dot(nd, n) > 0) break;
            }
            o = P;  // main.cpp:127: no epsilon offset here
            d = nd;
            flux = mulv(f, flux) * (1.0 / pmax);
        } else if (transp < kEps) {
            const V3 nd = d - n * 2.0 * dot(n, d);  // main.cpp:131-134
            o = P + n * kEps;
            d = nd;
            flux = mulv(f, flux) * refl;
        } else {
            const double nc = 1.0, nt = 1.33;  // main.cpp:140-164
            const double nnt = into ? nc / nt : nt / nc;
            const double ddn = dot(d, n);
            const V3 refl_dir = d - n_old * 2.0 * dot(n_old, d);
            const double cos2t = 1 - nnt * nnt * (1 - ddn * ddn);
            if (cos2t < 0) {
                o = P + n * kEps;
                d = refl_dir;
            } else {
                const V3 refr_dir = normalized(d * nnt - n_old * ((into ? 1 : -1) * (ddn * nnt + sqrt(cos2t))));
                if (rs.u01() < 0.5) {  // Russian roulette; the photon's flux is untouched by glass
                    o = P + n * kEps;
                    d = refl_dir;
                } else {
                    o = P - n * kEps;
                    d = refr_dir;
                }
            }
        }
    }
}

// cgrt_photon_emit: one lane per photon, no scene.  Any output may be null.
__global__ __launch_bounds__(256) void photon_emit_kernel(EmitArgs ea, long long first, long long count, double *__restrict__ org,
                                                          double *__restrict__ dir, double *__restrict__ flux,
                                                          unsigned long long *__restrict__ keys, unsigned int *__restrict__ draws) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    Stream rs(photon_key(ea.seed, (uint64_t)(first + i)));
    const EmittedPhoton e = photon_emit(ea, rs);
    for (int k = 0; k < 3; k++) {
        if (org) org[3 * i + k] = e.o[k];
        if (dir) dir[3 * i + k] = e.d[k];
        if (flux) flux[3 * i + k] = e.flux[k];
    }
    if (keys) keys[i] = rs.key;
    if (draws) draws[i] = rs.n;
}

// Spatial order for the pair search: events keyed by their hash-grid cell (invalid slots last).  Lanes of a wave then
// probe the same few buckets, so their loads coalesce and hit in L1 instead of being 64 unrelated L2 round trips.
// Only the ORDER OF THE SEARCH changes; every pair still carries its slot number = serial position.
constexpr unsigned kNoEvent = 0xffffffffu;
__global__ void event_keys_kernel(const double *__restrict__ events, const unsigned char *__restrict__ valid, int nslots,
                                  HashArgs ha, unsigned int *__restrict__ keys, unsigned int *__restrict__ vals) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    unsigned key = kNoEvent;
    if (valid[s]) {
        const double *e = events + 9 * (size_t)s;
        int ix, iy, iz;
        ref_coord(e[0], e[1], e[2], ha.celllength, ix, iy, iz);
        ix = ix < 0 ? 0 : (ix > 1023 ? 1023 : ix);
        iy = iy < 0 ? 0 : (iy > 1023 ? 1023 : iy);
        iz = iz < 0 ? 0 : (iz > 1022 ? 1022 : iz);
        key = ((unsigned)iz << 20) | ((unsigned)iy << 10) | (unsigned)ix;
    }
    keys[s] = key;
    vals[s] = (unsigned)s;
}

// 2. candidate (hitpoint, event) pairs.  One lane per event walks the reference's candidate set: the buckets its 27
// neighbour cells hash to (hash.h:35-37, main.cpp:107-113) -- cells that collide in the table are deliberately NOT
// deduplicated, the reference walks such a bucket once per cell.
// Hits are staged in a per-wave LDS buffer (the walk is wave-uniform: every lane steps through its bucket together, a
// ballot hands out buffer slots) and leave for global memory in blocks: space for everything a workgroup still holds at
// the end is reserved with ONE atomic per workgroup, a wave whose buffer fills up earlier reserves for itself.  A global
// atomic per hit serialises on a single address in L2 -- measured 16 ns each, 13.5 ms per 1.3 M events -- and dominated
// the whole photon pass; counting first and writing in a second walk (the previous form) paid for every probe twice.
constexpr int kWalk = 4;      // bucket entries a lane tests per step of the pair search
constexpr int kPairBuf = 768;  // staged pairs per wave (6 KiB); flushed before an iteration that could overflow it

// `base` is a position in the 64-bit count of ALL pairs the batch produces; only positions below `cap` exist in memory.  The
// count itself is never clamped: the host compares the 64-bit total with cap and redoes an overflowing batch in halves (a
// 32-bit count would wrap at settings within reach -- 5 M events x 1000 hitpoints inside the initial radius -- and pass).
__device__ __forceinline__ void pairs_flush(const unsigned long long *buf, unsigned cnt, unsigned long long base,
                                            unsigned long long *__restrict__ keys, unsigned int *__restrict__ vals,
                                            unsigned long long cap) {
    const int lane = threadIdx.x & 63;
    for (unsigned k = lane; k < cnt; k += 64) {
        const unsigned long long key = buf[k];
        if (base + k < cap) {
            keys[base + k] = key;
            vals[base + k] = (unsigned int)(key & 0xffffffull);  // the slot number is the key's low 24 bits
        }
    }
}

__global__ __launch_bounds__(256) void photon_pairs_kernel(const double *__restrict__ events,
                                                           const unsigned int *__restrict__ order_keys,
                                                           const unsigned int *__restrict__ order, int nslots, HashArgs ha,
                                                           const double *__restrict__ hps, const int *__restrict__ bstart,
                                                           unsigned long long *__restrict__ keys,
                                                           unsigned int *__restrict__ vals,
                                                           unsigned long long *__restrict__ npairs /* [0] pairs, [1] events */,
                                                           unsigned long long cap) {
    __shared__ unsigned long long stage[4][kPairBuf];
    __shared__ unsigned wave_cnt[4], wave_ev[4];
    __shared__ unsigned long long block_base;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = t < nslots && order_keys[t] != kNoEvent;
    const int s = on ? (int)order[t] : 0;
    unsigned long long *buf = stage[wave];
    unsigned cnt = 0;  // wave-uniform: pairs staged in buf
    V3 P = mk(0, 0, 0), n = mk(0, 0, 0);
    int ix = 0, iy = 0, iz = 0;
    if (on) {
        const double *e = events + 9 * (size_t)s;
        P = mk(e[0], e[1], e[2]);
        n = mk(e[3], e[4], e[5]);
        ref_coord(P.x, P.y, P.z, ha.celllength, ix, iy, iz);
        ix -= 1; iy -= 1; iz -= 1;
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (__ballot(on) != 0ull) {
        int i = 0, i1 = 0, ni = 0, ni1 = 0;
        if (on) {
            const unsigned b = ref_hash(ix, iy, iz, ha.hashsize);
            ni = bstart[b];
            ni1 = bstart[b + 1];
        }
        for (int c = 0; c < 27; c++) {
            i = ni; i1 = ni1;
            ni = ni1 = 0;
            if (on && c + 1 < 27) {  // the next cell's bucket bounds are fetched under this cell's walk
                const int c1 = c + 1;
                const unsigned b = ref_hash(ix + c1 / 9, iy + (c1 / 3) % 3, iz + c1 % 3, ha.hashsize);
                ni = bstart[b];
                ni1 = bstart[b + 1];
            }
            while (__ballot(i < i1) != 0ull) {  // all lanes step through their buckets together
                if (cnt > (unsigned)(kPairBuf - 64 * kWalk)) {  // the next step could overflow: this wave reserves for itself
                    unsigned long long base = 0;
                    if (lane == 0) base = atomicAdd(npairs, (unsigned long long)cnt);
                    base = __shfl(base, 0);
                    pairs_flush(buf, cnt, base, keys, vals, cap);
                    cnt = 0;
                }
                // kWalk bucket entries per step (their loads in flight together); pair order in the buffer is free, the
                // pairs are sorted by (hitpoint, slot) afterwards
                bool hit[kWalk];
                V3 dd[kWalk];
                double r2s[kWalk];
                bool cand[kWalk];
                const double2 *h = reinterpret_cast<const double2 *>(hps) + 4 * (size_t)i;  // 64-byte records
#pragma unroll
                for (int u = 0; u < kWalk; u++) {
                    hit[u] = false;
                    cand[u] = i + u < i1;
                    const double2 *g = cand[u] ? h + 4 * u : reinterpret_cast<const double2 *>(hps);
                    const double2 g0 = g[0], g1 = g[1];  // {x, y} {z, r2}
                    dd[u] = mk(g0.x, g0.y, g1.x) - P;    // the reference's differences
                    r2s[u] = g1.y;
                }
                // Single-precision screen of the radius test (fewer than 1 in 300 candidates pass it): the fp64
                // differences rounded to fp32, their squares summed in fp32 -- all terms >= 0, so the result is within
                // 2^-21 relative of the fp64 sum (plus at most 3 * 2^-150 where a square is subnormal); an overflow means
                // a distance no radius reaches, a NaN passes the screen.  The bound is r2 * (1 + 2^-18) converted to
                // nearest (>= r2 * (1 + 2^-19)) plus 1e-37, so nothing the exact test accepts is screened out; survivors
                // take the exact test.
#pragma unroll
                for (int u = 0; u < kWalk; u++) {
                    const float ax = (float)dd[u].x, ay = (float)dd[u].y, az = (float)dd[u].z;
                    const float sq = ax * ax + ay * ay + az * az;
                    const float lim = (float)(r2s[u] * (1.0 + 0x1p-18)) + 1e-37f;
                    if (cand[u] && !(sq > lim)) {
                        const double2 g2 = h[4 * u + 2], g3 = h[4 * u + 3];  // {nx, ny} {nz, -}
                        hit[u] = (dot(mk(g2.x, g2.y, g3.x), n) > kEps) && (dot(dd[u], dd[u]) <= r2s[u]);  // main.cpp:116, batch-start r2
                    }
                }
#pragma unroll
                for (int u = 0; u < kWalk; u++) {
                    const unsigned long long m = __ballot(hit[u]);
                    if (hit[u]) buf[cnt + (unsigned)__popcll(m & lt)] = ((unsigned long long)(i + u) << 24) | (unsigned long long)s;  // s < 2^24
                    cnt += (unsigned)__popcll(m);
                }
                i += kWalk;
            }
        }
    }
    const unsigned nev_wave = (unsigned)__popcll(__ballot(on));
    if (lane == 0) {
        wave_cnt[wave] = cnt;
        wave_ev[wave] = nev_wave;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        const unsigned nev = wave_ev[0] + wave_ev[1] + wave_ev[2] + wave_ev[3];
        block_base = tot ? atomicAdd(npairs, (unsigned long long)tot) : 0ull;
        if (nev) atomicAdd(npairs + 1, (unsigned long long)nev);  // events processed (statistics)
    }
    __syncthreads();
    unsigned long long base = block_base;
    for (int w = 0; w < wave; w++) base += wave_cnt[w];
    pairs_flush(buf, cnt, base, keys, vals, cap);
}

// 4. ordered replay per hitpoint
__global__ void photon_apply_kernel(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ vals,
                                    unsigned int npairs, const double *__restrict__ events, double alpha,
                                    double *__restrict__ hp, double *__restrict__ hps, long long nhp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nhp) return;
    const unsigned long long klo = (unsigned long long)i << 24;
    unsigned int lo = 0, hi = npairs;  // first pair of hitpoint i
    while (lo < hi) {
        const unsigned int mid = (lo + hi) >> 1;
        if (keys[mid] < klo) lo = mid + 1; else hi = mid;
    }
    if (lo >= npairs || (keys[lo] >> 24) != (unsigned long long)i) return;
    double *h = hp + 16 * i;
    const V3 f = mk(h[2], h[3], h[4]), pos = mk(h[5], h[6], h[7]);
    V3 flux = mk(h[11], h[12], h[13]);
    double r2 = h[14];
    int n = (int)h[15];
    // The replay is a serial chain per hitpoint and the kernel ends with its longest chains, so the loads of kChunk pairs
    // (key, slot, event: three dependent levels) are issued together and only the update itself runs in sequence.
    constexpr int kChunk = 4;
    for (unsigned int k = lo; k < npairs;) {
        bool mine[kChunk];
        unsigned int slot[kChunk];
#pragma unroll
        for (int c = 0; c < kChunk; c++) {
            const unsigned int kc = k + (unsigned)c < npairs ? k + (unsigned)c : npairs - 1u;
            mine[c] = k + (unsigned)c < npairs && (keys[kc] >> 24) == (unsigned long long)i;
            slot[c] = vals[kc];
        }
        double e[kChunk][6];
#pragma unroll
        for (int c = 0; c < kChunk; c++) {
            const double *q = events + 9 * (size_t)slot[c];
            e[c][0] = q[0]; e[c][1] = q[1]; e[c][2] = q[2];
            e[c][3] = q[6]; e[c][4] = q[7]; e[c][5] = q[8];
        }
        bool more = true;
#pragma unroll
        for (int c = 0; c < kChunk; c++) {
            more = more && mine[c];  // the hitpoint's pairs are contiguous: the first foreign key ends the replay
            if (more) {
                const V3 dd = pos - mk(e[c][0], e[c][1], e[c][2]);
                if (dot(dd, dd) <= r2) {  // main.cpp:116 against the CURRENT radius (the normal test was static)
                    const double g = (n * alpha + alpha) / (n * alpha + 1.0);  // main.cpp:119
                    r2 *= g;
                    n++;
                    flux = (flux + mulv(f, mk(e[c][3], e[c][4], e[c][5])) * (1.0 / kPiRef)) * g;  // main.cpp:122
                }
            }
        }
        if (!more) break;
        k += kChunk;
    }
    h[11] = flux.x; h[12] = flux.y; h[13] = flux.z;
    h[14] = r2;
    h[15] = (double)n;
    hps[8 * i + 3] = r2;  // the next batch's search radius
}

// ---- the per-pixel index (CSR) the final gather walks.  A hitpoint's pixel and table position never change after the
// table is built, so the index is built once: image_keys_kernel keys every hitpoint by (pixel, table position), a radix
// sort orders them, the sorted values are `order` and pix_start[px] .. pix_start[px+1] is pixel px's range of it.
// pix_start[px] = first position of the sorted keys whose pixel is >= px, px in [0, npix]
__global__ void pix_start_kernel(const unsigned long long *__restrict__ keys, long long nhp, long long npix,
                                 unsigned int *__restrict__ pix_start) {
    const long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (px > npix) return;
    const unsigned long long klo = (unsigned long long)px << 32;
    long long lo = 0, hi = nhp;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < klo) lo = mid + 1; else hi = mid;
    }
    pix_start[px] = (unsigned int)lo;
}
// gammaCorr, util.h:45-47: one byte of main.cpp:403-412
__device__ __forceinline__ unsigned char tonemap_byte(double x) {
    const double v = pow(1 - exp(-x), 1 / 2.2) * 255 + .5;
    return (v >= 0) ? (unsigned char)(int)(v < 255.0 ? v : 255.0) : 0;  // NaN -> 0
}
// final gather, main.cpp:252-258: one lane per pixel sums flux / (PI * r2 * N * spp) over the pixel's hitpoints in table
// order.  image and rgb8 may each be null; rgb8 receives the tone-mapped byte of tonemap_kernel at the flipped row (row 0 =
// top), so a checkpoint needs no second pass over the image.
__global__ void ppm_gather_kernel(const unsigned int *__restrict__ pix_start, const unsigned int *__restrict__ order,
                                  const double *__restrict__ hp, double norm, long long npix, int W, int rows,
                                  double *__restrict__ image, unsigned char *__restrict__ rgb8) {
    const long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= npix) return;
    const unsigned int k1 = pix_start[px + 1];
    double r = 0, g = 0, b = 0;
    for (unsigned int k = pix_start[px]; k < k1; k++) {
        const double *h = hp + 16 * (size_t)order[k];
        const double sc = 1.0 / (kPiRef * h[14] * norm);  // 1/(PI*r2*N*spp), main.cpp:256
        r += h[11] * sc;
        g += h[12] * sc;
        b += h[13] * sc;
    }
    if (image) {
        image[3 * px] = r; image[3 * px + 1] = g; image[3 * px + 2] = b;
    }
    if (rgb8) {
        const long long row = px / W, col = px % W;
        unsigned char *o = rgb8 + ((long long)(rows - 1 - row) * W + col) * 3;
        o[0] = tonemap_byte(r); o[1] = tonemap_byte(g); o[2] = tonemap_byte(b);
    }
}
__global__ void image_keys_kernel(const double *__restrict__ hp, long long nhp, int spp, unsigned long long *__restrict__ keys,
                                  unsigned int *__restrict__ vals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nhp) return;
    const unsigned long long ps = (unsigned long long)hp[16 * i];
    keys[i] = ((ps / (unsigned long long)spp) << 32) | (unsigned long long)i;  // pixel, then table order
    vals[i] = (unsigned int)i;
}

// image_keys_kernel for a ray session: the texel is the ray's
__global__ void image_ray_keys_kernel(const double *__restrict__ hp, long long nhp, const long long *__restrict__ pixel, long long npix,
                                      unsigned long long *__restrict__ keys, unsigned int *__restrict__ vals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nhp) return;
    keys[i] = (ray_texel(pixel, (unsigned long long)hp[16 * i], npix) << 32) | (unsigned long long)i;
    vals[i] = (unsigned int)i;
}

int sort_pairs(GrowBuf &tmp, unsigned long long *kin, unsigned long long *kout, unsigned int *vin, unsigned int *vout, size_t n,
               int end_bit = 64, hipStream_t st = 0) {
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit, st));
    HIP_TRY(tmp.need(tmp_bytes));
    HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit, st));
    return CGRT_OK;
}

// ra: null for the built-in emitter, else the caller's photons of this batch (the RAYS instantiations)
int launch_photon_trace(const cgrt_scene *s, const PhotonArgs &pa, double *events, unsigned char *valid, hipStream_t st = 0,
                        const PhotonRayArgs *ra = nullptr) {
    const DeviceScene &d = s->dev;
    // more objects than the LDS list holds: the variants that read the rest from the uploaded array
    const bool spill = d.n_objs > d.n_lds, bez = d.has_bezier != 0;
    const auto fn = ra ? (spill ? (bez ? &photon_trace_kernel<true, true, true> : &photon_trace_kernel<false, true, true>)
                                : (bez ? &photon_trace_kernel<true, false, true> : &photon_trace_kernel<false, false, true>))
                       : (spill ? (bez ? &photon_trace_kernel<true, true> : &photon_trace_kernel<false, true>)
                                : (bez ? &photon_trace_kernel<true> : &photon_trace_kernel<false>));
    return launch_checked(fn, spill ? "photon_trace_kernel, SPILL" : "photon_trace_kernel", s->device,
                          dim3((pa.count + kThreads - 1) / kThreads), dim3(kThreads),
                          photon_lds((size_t)d.n_lds, spill, bez, photon_lds_stack(d)), st, d, pa, events, valid,
                          ra ? *ra : PhotonRayArgs{});
}

int sort_pairs32(GrowBuf &tmp, unsigned int *kin, unsigned int *kout, unsigned int *vin, unsigned int *vout, size_t n,
                 hipStream_t st = 0) {
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin, kout, vin, vout, n, 0u, 32u, st));
    HIP_TRY(tmp.need(tmp_bytes));
    HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, kin, kout, vin, vout, n, 0u, 32u, st));
    return CGRT_OK;
}

// The producer side of a photon batch (trace -> event keys -> events in hash-cell order) on its own stream, so that the
// batch after the one being replayed is traced meanwhile: photon paths do not depend on hitpoints.
struct PhotonProducer {
    hipStream_t st = nullptr;
    hipEvent_t produced[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    DevBuf ev[2], valid[2], ek0[2], ek1[2], eo0[2], eo1[2];
    GrowBuf tmp;
    ~PhotonProducer() {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
        for (int k = 0; k < 2; k++) {
            if (produced[k]) (void)hipEventDestroy(produced[k]);
            if (consumed[k]) (void)hipEventDestroy(consumed[k]);
        }
    }
    int init(int nbuf, size_t nslots_max, bool own_stream) {
        if (own_stream) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (int k = 0; k < nbuf; k++) {
            HIP_TRY(hipEventCreateWithFlags(&produced[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&consumed[k], hipEventDisableTiming));
            HIP_TRY(ev[k].alloc(nslots_max * 9 * sizeof(double)));
            HIP_TRY(valid[k].alloc(nslots_max));
            HIP_TRY(ek0[k].alloc(nslots_max * 4)); HIP_TRY(ek1[k].alloc(nslots_max * 4));
            HIP_TRY(eo0[k].alloc(nslots_max * 4)); HIP_TRY(eo1[k].alloc(nslots_max * 4));
        }
        return CGRT_OK;
    }
    // enqueue batch `pa` into buffer b (after the replay that last read b has finished); ra: the caller's photons of the batch
    int produce(const cgrt_scene *s, const PhotonArgs &pa, const HashArgs &ha, int b, const PhotonRayArgs *ra = nullptr);
    // null stream: the replay of buffer b is enqueued; b may be overwritten once it has run
    int release(int b) {
        HIP_TRY(hipEventRecord(consumed[b], 0));
        used[b] = true;
        return CGRT_OK;
    }
};

int PhotonProducer::produce(const cgrt_scene *s, const PhotonArgs &pa, const HashArgs &ha, int b, const PhotonRayArgs *ra) {
    const int T = 256;
    const int nslots = pa.count * kSegStride;
    if (used[b]) HIP_TRY(hipStreamWaitEvent(st, consumed[b], 0));
    HIP_TRY(hipMemsetAsync(valid[b].p, 0, (size_t)nslots, st));
    if (const int rc = launch_photon_trace(s, pa, ev[b].as<double>(), valid[b].as<unsigned char>(), st, ra)) return rc;
    hipLaunchKernelGGL(event_keys_kernel, dim3((nslots + T - 1) / T), dim3(T), 0, st, ev[b].as<double>(), valid[b].as<unsigned char>(),
                       nslots, ha, ek0[b].as<unsigned int>(), eo0[b].as<unsigned int>());
    const int rc = sort_pairs32(tmp, ek0[b].as<unsigned int>(), ek1[b].as<unsigned int>(), eo0[b].as<unsigned int>(),
                                eo1[b].as<unsigned int>(), (size_t)nslots, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(produced[b], st));
    return CGRT_OK;
}

}  // namespace

// verification probe: the diffuse hits of photons [first, first+count) -- count*8 slots of 9 doubles {P, n, flux}
// (slot = (photon-first)*8 + path segment) and one validity byte per slot, HOST buffers
extern "C" int cgrt_photon_events(const cgrt_scene *s, const cgrt_photons *ph, int max_depth, int64_t first, int32_t count,
                                  double *events9, uint8_t *valid) {
    if (!s || !s->committed || !ph || !events9 || !valid || count <= 0 || count > (1 << 20) || max_depth < 1 ||
        max_depth > kMaxDepth)
        return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(s->device);
    DevBuf ev, va;
    const size_t nslots = (size_t)count * kSegStride;
    HIP_TRY(ev.alloc(nslots * 9 * sizeof(double)));
    HIP_TRY(va.alloc(nslots));
    HIP_TRY(hipMemset(ev.p, 0, nslots * 9 * sizeof(double)));
    HIP_TRY(hipMemset(va.p, 0, nslots));
    PhotonArgs pa;
    for (int k = 0; k < 3; k++) pa.light[k] = ph->light[k];
    pa.jitter = ph->jitter; pa.power = ph->power; pa.alpha = ph->alpha;
    pa.first = first; pa.count = count; pa.max_depth = max_depth; pa.seed = ph->seed;
    if (const int rc = launch_photon_trace(s, pa, ev.as<double>(), va.as<unsigned char>())) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(events9, ev.p, nslots * 9 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, va.p, nslots, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

// ---- caller-supplied photons: argument checks, the built-in emitter as a producer, the probe -------------------------------
constexpr long long kMaxPhotonRays = 1ll << 36;
// what can be said without a device or a session (so the refusals are the same wherever the struct arrives)
static int check_photon_rays(const cgrt_photon_rays *pr) {
    if (!pr) return fail(CGRT_ERR_INVALID, "null cgrt_photon_rays");
    if (pr->n < 0) return fail(CGRT_ERR_INVALID, "negative photon count");
    if (pr->n > kMaxPhotonRays) return fail(CGRT_ERR_LIMIT, "more than 2^36 photons in one call");
    if (pr->n > 0 && (!pr->org3 || !pr->dir3 || !pr->flux3)) return fail(CGRT_ERR_INVALID, "null org3 / dir3 / flux3");
    return CGRT_OK;
}
static int check_emit(const cgrt_photons *ph, int64_t first, int64_t count) {
    if (!ph) return fail(CGRT_ERR_INVALID, "null cgrt_photons");
    if (first < 0 || count < 0) return fail(CGRT_ERR_INVALID, "negative photon index or count");
    if (count > kMaxPhotonRays) return fail(CGRT_ERR_LIMIT, "more than 2^36 photons in one call");
    if (first > LLONG_MAX - count) return fail(CGRT_ERR_INVALID, "photon index out of range");
    return CGRT_OK;
}
static EmitArgs emit_args(const cgrt_photons *ph) {
    EmitArgs ea;
    for (int k = 0; k < 3; k++) ea.light[k] = ph->light[k];
    ea.jitter = ph->jitter; ea.power = ph->power; ea.seed = ph->seed;
    return ea;
}

extern "C" int cgrt_photon_emit(const cgrt_photons *ph, int64_t first, int64_t count, double *org3, double *dir3, double *flux3,
                                uint64_t *keys, uint32_t *draws, void *stream) {
    if (const int rc = check_emit(ph, first, count)) return rc;
    if (count == 0) return CGRT_OK;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const EmitArgs ea = emit_args(ph);
    // 2^36 photons are 2^28 workgroups: launched in pieces of at most 2^30 photons (a grid's x extent is below 2^31)
    for (long long k0 = 0; k0 < count; k0 += 1ll << 30) {
        const long long m = count - k0 < (1ll << 30) ? count - k0 : (1ll << 30);
        hipLaunchKernelGGL(photon_emit_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, ea, (long long)first + k0, m,
                           org3 ? org3 + 3 * k0 : nullptr, dir3 ? dir3 + 3 * k0 : nullptr, flux3 ? flux3 + 3 * k0 : nullptr,
                           keys ? reinterpret_cast<unsigned long long *>(keys) + k0 : nullptr, draws ? draws + k0 : nullptr);
    }
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

extern "C" int cgrt_photon_emit_host(const cgrt_photons *ph, int64_t first, int64_t count, double *org3, double *dir3,
                                     double *flux3, uint64_t *keys, uint32_t *draws) {
    if (const int rc = check_emit(ph, first, count)) return rc;
    const EmitArgs ea = emit_args(ph);
    for (int64_t i = 0; i < count; i++) {
        Stream rs(photon_key(ea.seed, (uint64_t)(first + i)));
        const EmittedPhoton e = photon_emit(ea, rs);
        for (int k = 0; k < 3; k++) {
            if (org3) org3[3 * i + k] = e.o[k];
            if (dir3) dir3[3 * i + k] = e.d[k];
            if (flux3) flux3[3 * i + k] = e.flux[k];
        }
        if (keys) keys[i] = rs.key;
        if (draws) draws[i] = rs.n;
    }
    return CGRT_OK;
}

// cgrt_photon_events for caller-supplied photons (HOST arrays): uploads them, runs the RAYS instantiation, copies the slots back
extern "C" int cgrt_photon_ray_events(const cgrt_scene *s, const cgrt_photon_rays *pr, uint64_t seed, int64_t first_index,
                                      int max_depth, double *events9, uint8_t *valid) {
    if (const int rc = check_photon_rays(pr)) return rc;
    if (!s || !s->committed || !events9 || !valid || pr->n < 1 || pr->n > (1 << 20) || first_index < 0 || max_depth < 1 ||
        max_depth > kMaxDepth)
        return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(s->device);
    const size_t n = (size_t)pr->n, nslots = n * kSegStride;
    DevBuf ev, va, b_o, b_d, b_f, b_k, b_n;
    HIP_TRY(ev.alloc(nslots * 9 * sizeof(double)));
    HIP_TRY(va.alloc(nslots));
    HIP_TRY(hipMemset(ev.p, 0, nslots * 9 * sizeof(double)));
    HIP_TRY(hipMemset(va.p, 0, nslots));
    PhotonRayArgs ra{};
    HIP_TRY(b_o.alloc(n * 24)); HIP_TRY(b_d.alloc(n * 24)); HIP_TRY(b_f.alloc(n * 24));
    HIP_TRY(hipMemcpy(b_o.p, pr->org3, n * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_d.p, pr->dir3, n * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_f.p, pr->flux3, n * 24, hipMemcpyHostToDevice));
    ra.org = b_o.as<double>(); ra.dir = b_d.as<double>(); ra.flux = b_f.as<double>();
    if (pr->keys) {
        HIP_TRY(b_k.alloc(n * 8));
        HIP_TRY(hipMemcpy(b_k.p, pr->keys, n * 8, hipMemcpyHostToDevice));
        ra.keys = b_k.as<unsigned long long>();
    }
    if (pr->draws) {
        HIP_TRY(b_n.alloc(n * 4));
        HIP_TRY(hipMemcpy(b_n.p, pr->draws, n * 4, hipMemcpyHostToDevice));
        ra.draws = b_n.as<unsigned int>();
    }
    PhotonArgs pa{};
    pa.first = first_index; pa.count = (int)n; pa.max_depth = max_depth; pa.seed = seed;
    if (const int rc = launch_photon_trace(s, pa, ev.as<double>(), va.as<unsigned char>(), 0, &ra)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(events9, ev.p, nslots * 9 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, va.p, nslots, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

// gammaCorr (util.h:45-47) and the vertical flip of main.cpp:403-412
__global__ void tonemap_kernel(const double *__restrict__ image, int W, int H, unsigned char *__restrict__ rgb8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // output byte index, top row first
    const long long n = (long long)W * H * 3;
    if (i >= n) return;
    const long long row = i / ((long long)W * 3), rest = i % ((long long)W * 3);
    rgb8[i] = tonemap_byte(image[(long long)(H - 1 - row) * W * 3 + rest]);
}

namespace {
struct Timer {  // device time between two points of the null stream
    hipEvent_t a = nullptr, b = nullptr;
    Timer() { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void start() { (void)hipEventRecord(a, 0); }
    double stop() {
        (void)hipEventRecord(b, 0);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        return (double)ms;
    }
};
}  // namespace

extern "C" int cgrt_tonemap_rgb8(int device, const double *image, int width, int height, uint8_t *rgb8) {
    if (!image || !rgb8 || width < 1 || height < 1) return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(device);
    const size_t n = (size_t)width * height * 3;
    DevBuf img, out;
    HIP_TRY(img.alloc(n * sizeof(double)));
    HIP_TRY(out.alloc(n));
    HIP_TRY(hipMemcpy(img.p, image, n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(tonemap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, img.as<double>(), width, height,
                       out.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(rgb8, out.p, n, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

// ---- the stages of render() main.cpp:169-258, shared by cgrt_ppm_render (one call) and a live cgrt_ppm_session ----------
// eye_grid() / eye_rays(): the Hitpoint records of a grid or of a ray buffer; table(): the reference's table order and the
// per-pixel index over them.  photon_setup() + photons(last): photons
// [done, last) in batches.  gather(): the image at the current photon count.  Photon i always draws from the keyed stream
// (seed, i) and a hitpoint replays its events in photon order, so the state after photons [0, a) then [a, b) is the state
// after [0, b): how the photons are split into calls and batches never shows in the result.
struct cgrt_ppm_session {
    const cgrt_scene *s = nullptr;
    cgrt_photons ph{};
    // the image the session gathers into, the gather's normaliser and the photons' depth limit: a grid session's grid.width,
    // .rows, .spp, .max_depth; a ray session's cgrt_ray_pixels and rays->max_depth
    int width = 0, rows = 0, spp = 1, max_depth = 0;
    bool striped = false;  // grid session over block-cyclic rows: no rgb8
    bool lookahead = false;  // session: trace the next batch on the producer stream when a call ends
    size_t n = 0;            // hitpoints
    long long npix = 0;
    HashArgs ha{};
    int64_t dev_bytes = 0;  // what this state allocated itself (sort scratch and producer buffers are added by bytes())
    DevBuf hp, hps, bstart, pix_start, order;  // table state and per-pixel index
    DevBuf pk0, pk1, pv0, pv1, npairs;          // (hitpoint, event) pairs of one batch
    DevBuf img, rgb8;                           // session: device image of cgrt_ppm_session_image (host outputs)
    GrowBuf main_tmp;
    PhotonProducer pp;  // declared last of the buffers: its destructor waits for its stream before they are freed
    int64_t pp_bytes = 0;
    bool overlap = false;
    int batch = 0, batch_max = 0, pair_key_bits = 25;
    unsigned long long pair_cap = 0;
    long long done = 0;       // photons [0, done) are applied
    long long ahead_first = -1;  // the batch already enqueued on the producer: its range and buffer
    int ahead_count = 0, ahead_buf = 0, cur = 0;
    uint64_t n_events = 0, n_pairs = 0, n_halvings = 0;
    double ms_eye = 0, ms_table = 0, ms_photons = 0, ms_last_add = 0;
    mutable double ms_last_image = 0;
    mutable hipEvent_t img_a = nullptr, img_b = nullptr;  // session: brackets the last gather (on the stream it ran on)
    mutable bool img_pending = false;                     // img_b recorded, ms_last_image not yet read from it

    ~cgrt_ppm_session() {
        if (img_b) (void)hipEventSynchronize(img_b);
        if (img_a) (void)hipEventDestroy(img_a);
        if (img_b) (void)hipEventDestroy(img_b);
    }
    hipError_t take(DevBuf &b, size_t bytes) {
        dev_bytes += (int64_t)bytes;
        return b.alloc(bytes);
    }
    int64_t bytes() const { return dev_bytes + pp_bytes + (int64_t)main_tmp.cap + (int64_t)pp.tmp.cap; }
    int eye_grid(const cgrt_scene *s_, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_photons *ph_, DevBuf &rec);
    int eye_rays(const cgrt_scene *s_, const cgrt_rays *rays, const cgrt_ray_pixels *px, const cgrt_photons *ph_, DevBuf &rec);
    int table(DevBuf &rec, const int64_t *ray_pixel, bool rays);
    int photon_setup(bool session);
    int photons(long long last, bool keep_ahead, const cgrt_photon_rays *pr = nullptr);
    int gather(double *d_img, unsigned char *d_rgb8, hipStream_t st) const;
};

// ---- eye pass: hitpoint records, device resident (count first, then capture) ----
int cgrt_ppm_session::eye_grid(const cgrt_scene *s_, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_photons *ph_, DevBuf &rec) {
    s = s_; ph = *ph_;
    width = grid->width; rows = grid->rows; spp = grid->spp; max_depth = grid->max_depth;
    striped = grid->stripe_nranks > 1;
    Timer tm;
    tm.start();
    uint64_t nhp = 0;
    int rc = hitpoints_device(s, cam, grid, 0, nullptr, &nhp);
    if (rc) return rc;
    npix = (long long)rows * width;
    n = (size_t)nhp;
    if (n >= (1ull << 31)) return fail(CGRT_ERR_LIMIT, "photon pass: more than 2^31 hitpoints");
    if (n) {
        double *d_rec = nullptr;
        rc = hitpoints_device(s, cam, grid, nhp, &d_rec, &nhp);
        rec.p = d_rec;
        if (rc) return rc;
    }
    ms_eye = tm.stop();
    return CGRT_OK;
}
int cgrt_ppm_session::eye_rays(const cgrt_scene *s_, const cgrt_rays *rays, const cgrt_ray_pixels *px, const cgrt_photons *ph_, DevBuf &rec) {
    s = s_; ph = *ph_;
    width = px->width; rows = px->rows; spp = px->spp; max_depth = rays->max_depth;
    Timer tm;
    tm.start();
    uint64_t nhp = 0;
    int rc = ray_hitpoints_device(s, rays, px->pixel, 0, nullptr, &nhp);
    if (rc) return rc;
    npix = (long long)rows * width;
    n = (size_t)nhp;
    if (n >= (1ull << 31)) return fail(CGRT_ERR_LIMIT, "photon pass: more than 2^31 hitpoints");
    if (n) {
        double *d_rec = nullptr;
        rc = ray_hitpoints_device(s, rays, px->pixel, nhp, &d_rec, &nhp);
        rec.p = d_rec;
        if (rc) return rc;
    }
    ms_eye = tm.stop();
    return CGRT_OK;
}

// ---- the reference's table order: (bucket, insertion order); then the per-pixel index.  rays: the records' labels are
// (ray << 4 | seq) and ray_pixel (DEVICE, or null) maps rays to texels ----
int cgrt_ppm_session::table(DevBuf &rec, const int64_t *ray_pixel, bool rays) {
    Timer tm;
    int rc = CGRT_OK;
    DevBuf bucket_of, k0, k1, v0, v1;
    const long long *pixel = reinterpret_cast<const long long *>(ray_pixel);
    tm.start();
    HIP_TRY(take(hp, n * 16 * sizeof(double)));
    HIP_TRY(take(hps, n * 8 * sizeof(double)));
    HIP_TRY(take(bstart, ((size_t)ph.hashsize + 2) * sizeof(int)));
    HIP_TRY(take(pix_start, ((size_t)npix + 1) * sizeof(unsigned int)));
    HIP_TRY(bucket_of.alloc(n * sizeof(int)));
    HIP_TRY(k0.alloc(n * 8)); HIP_TRY(k1.alloc(n * 8)); HIP_TRY(v0.alloc(n * 4)); HIP_TRY(v1.alloc(n * 4));
    ha.hashsize = ph.hashsize;
    // main.cpp:84,183: r = 200.0 / height with the reference's COMPILE-TIME height (768) whatever frame is rendered;
    // a host that mirrors a reference built for another height passes that build's 200/height here
    const double r0 = ph.initial_radius > 0 ? ph.initial_radius : 200.0 / 768;
    ha.celllength = 70.0 / std::ceil(70.0 / r0);  // hash.h:25-26
    const int T = 256;
    const unsigned nb = (unsigned)((n + T - 1) / T);
    if (n && rays) {
        hipLaunchKernelGGL(hp_ray_label_keys_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), (long long)n, k0.as<unsigned long long>(),
                           v0.as<unsigned int>());
        rc = sort_pairs(main_tmp, k0.as<unsigned long long>(), k1.as<unsigned long long>(), v0.as<unsigned int>(), v1.as<unsigned int>(), n, 40);
        if (rc) return rc;
        hipLaunchKernelGGL(hp_ray_bucket_keys_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), v1.as<unsigned int>(), (long long)n, ha,
                           pixel, npix, k0.as<unsigned long long>());
        rc = sort_pairs(main_tmp, k0.as<unsigned long long>(), k1.as<unsigned long long>(), v1.as<unsigned int>(), v0.as<unsigned int>(), n, 52);
        if (rc) return rc;
        hipLaunchKernelGGL(hp_ray_gather_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), k1.as<unsigned long long>(),
                           v0.as<unsigned int>(), (long long)n, r0 * r0, hp.as<double>(), hps.as<double>(), bucket_of.as<int>());
        hipLaunchKernelGGL(image_ray_keys_kernel, dim3(nb), dim3(T), 0, 0, hp.as<double>(), (long long)n, pixel, npix,
                           k0.as<unsigned long long>(), v0.as<unsigned int>());
        rc = sort_pairs(main_tmp, k0.as<unsigned long long>(), k1.as<unsigned long long>(), v0.as<unsigned int>(), v1.as<unsigned int>(), n);
        if (rc) return rc;
    } else if (n) {
        hipLaunchKernelGGL(hp_keys_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), (long long)n, ha, (int)npix, spp,
                           k0.as<unsigned long long>(), v0.as<unsigned int>());
        rc = sort_pairs(main_tmp, k0.as<unsigned long long>(), k1.as<unsigned long long>(), v0.as<unsigned int>(), v1.as<unsigned int>(), n);
        if (rc) return rc;
        hipLaunchKernelGGL(hp_gather_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), k1.as<unsigned long long>(),
                           v1.as<unsigned int>(), (long long)n, r0 * r0, hp.as<double>(), hps.as<double>(), bucket_of.as<int>());
        hipLaunchKernelGGL(image_keys_kernel, dim3(nb), dim3(T), 0, 0, hp.as<double>(), (long long)n, spp,
                           k0.as<unsigned long long>(), v0.as<unsigned int>());
        rc = sort_pairs(main_tmp, k0.as<unsigned long long>(), k1.as<unsigned long long>(), v0.as<unsigned int>(), v1.as<unsigned int>(), n);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(bucket_start_kernel, dim3((ph.hashsize + 1 + T - 1) / T), dim3(T), 0, 0, bucket_of.as<int>(),
                       (long long)n, ph.hashsize, bstart.as<int>());
    hipLaunchKernelGGL(pix_start_kernel, dim3((unsigned)((npix + 1 + T - 1) / T)), dim3(T), 0, 0, k1.as<unsigned long long>(),
                       (long long)n, npix, pix_start.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    order.p = v1.release();  // hitpoint indices by pixel, then table order
    dev_bytes += (int64_t)(n ? n * 4 : 16);
    ms_table = tm.stop();
    return CGRT_OK;
}

// Batch size, pair buffers and the producer.  One call traces on a second stream only when it has more photons than one
// batch; a session always does (its calls are not known in advance).  CGRT_PHOTON_OVERLAP=0: one buffer, null stream.
int cgrt_ppm_session::photon_setup(bool session) {
    batch = ph.batch > 0 ? (ph.batch < (1 << 20) ? ph.batch : (1 << 20)) : (1 << 20);
    batch_max = batch;
    const int nslots_max = batch * kSegStride;
    // pairs per batch: room for 128 per hitpoint, between 4 M and 128 M (3 GiB of keys and values); a batch that overflows is halved
    const unsigned long long want_cap = (unsigned long long)n * 128ull;
    pair_cap = want_cap < (1ull << 22) ? (1ull << 22) : (want_cap > (1ull << 27) ? (1ull << 27) : want_cap);
    if (ph.pair_cap > 0) pair_cap = (unsigned long long)ph.pair_cap < (1ull << 27) ? (unsigned long long)ph.pair_cap : (1ull << 27);
    // Two event buffers: while batch k's pairs are sorted and replayed (null stream), batch k+1 is traced and its events are
    // put in hash-cell order on the producer's stream.
    const char *ov = std::getenv("CGRT_PHOTON_OVERLAP");
    overlap = !(ov && ov[0] == '0') && (session || ph.nphotons > batch);
    if (n > 0 && (session || ph.nphotons > 0)) {
        const int nbuf = overlap ? 2 : 1;
        const int rc = pp.init(nbuf, (size_t)nslots_max, overlap);
        if (rc) return rc;
        pp_bytes = (int64_t)nbuf * nslots_max * (9 * sizeof(double) + 1 + 4 * 4);
    }
    HIP_TRY(take(pk0, (size_t)pair_cap * 8)); HIP_TRY(take(pk1, (size_t)pair_cap * 8));
    HIP_TRY(take(pv0, (size_t)pair_cap * 4)); HIP_TRY(take(pv1, (size_t)pair_cap * 4));
    HIP_TRY(take(npairs, 16));
    pair_key_bits = 25;  // key = hitpoint << 24 | slot
    while (pair_key_bits < 64 && (n >> (pair_key_bits - 24)) != 0) pair_key_bits++;
    return CGRT_OK;
}

// Photons [done, last), applied on the null stream.  A batch is applied whole or not at all: `done` only moves past a batch
// once its pairs fit, so a failure leaves the state of the first `done` photons.  keep_ahead: when the range is done, the
// next batch from `done` is enqueued on the producer stream for the next call (which uses it if it starts with exactly
// that batch; it is sized for a call as long as this one); otherwise nothing is traced beyond `last` and the producer stream
// is drained.
// pr: the photons [done, last) are the caller's (pr->n = last - done; DEVICE arrays) instead of the built-in emitter's.  Inside the
// call batch k+1 is traced under batch k's replay as ever; a batch traced ahead by an earlier add_photons is not pr's and is
// dropped, and the caller passes keep_ahead = false: the photons after `last` are not known, and the drain is what makes pr's
// arrays read before the call returns.
int cgrt_ppm_session::photons(long long last, bool keep_ahead, const cgrt_photon_rays *pr) {
    if (n == 0) {  // no hitpoint can change: nothing to trace
        done = last > done ? last : done;
        return CGRT_OK;
    }
    const long long call_first = done;
    if (pr) ahead_first = -1;
    // the caller's arrays at photon `first` of this call (a batch's PhotonRayArgs)
    auto ray_args = [&](long long first) {
        const size_t k = (size_t)(first - call_first);
        PhotonRayArgs ra;
        ra.org = pr->org3 + 3 * k;
        ra.dir = pr->dir3 + 3 * k;
        ra.flux = pr->flux3 + 3 * k;
        ra.keys = pr->keys ? reinterpret_cast<const unsigned long long *>(pr->keys) + k : nullptr;
        ra.draws = pr->draws ? pr->draws + k : nullptr;
        return ra;
    };
    auto produce = [&](const PhotonArgs &pa, int b) {
        if (!pr) return pp.produce(s, pa, ha, b);
        const PhotonRayArgs ra = ray_args(pa.first);
        return pp.produce(s, pa, ha, b, &ra);
    };
    const int T = 256;
    const unsigned nb = (unsigned)((n + T - 1) / T);
    auto batch_args = [&](long long first, int batch_now, long long end) {
        PhotonArgs pa;
        for (int k = 0; k < 3; k++) pa.light[k] = ph.light[k];
        pa.jitter = ph.jitter; pa.power = ph.power; pa.alpha = ph.alpha;
        pa.first = first;
        pa.count = (int)((end - first < batch_now) ? (end - first) : batch_now);
        pa.max_depth = max_depth;
        pa.seed = ph.seed;
        return pa;
    };
    int rc = CGRT_OK;
    const long long call = last - done;
    while (done < last) {
        const PhotonArgs pa = batch_args(done, batch, last);
        const int nslots = pa.count * kSegStride;
        if (ahead_first == pa.first && ahead_count == pa.count) {
            cur = ahead_buf;
        } else {  // first batch, the plan changed (a halving), or a lookahead that does not fit this call: produce it now
            rc = produce(pa, cur);
            if (rc) return rc;
        }
        ahead_first = -1;
        if (overlap && done + pa.count < last) {
            // Enqueue the NEXT batch now, so that it is traced under this batch's search, sort and replay.  Its range assumes
            // this batch neither overflows the pair buffer nor changes the batch size; if it does, the range will not match
            // at the top of the loop and the batch is produced again (results do not depend on the batching).
            const PhotonArgs nx = batch_args(done + pa.count, batch, last);
            rc = produce(nx, 1 - cur);
            if (rc) return rc;
            ahead_first = nx.first; ahead_count = nx.count; ahead_buf = 1 - cur;
        }
        if (pp.st) HIP_TRY(hipStreamWaitEvent(0, pp.produced[cur], 0));
        HIP_TRY(hipMemsetAsync(npairs.p, 0, 16, 0));
        hipLaunchKernelGGL(photon_pairs_kernel, dim3((nslots + T - 1) / T), dim3(T), 0, 0, pp.ev[cur].as<double>(),
                           pp.ek1[cur].as<unsigned int>(), pp.eo1[cur].as<unsigned int>(), nslots, ha, hps.as<double>(), bstart.as<int>(),
                           pk0.as<unsigned long long>(), pv0.as<unsigned int>(), npairs.as<unsigned long long>(), pair_cap);
        HIP_TRY(hipGetLastError());
        unsigned long long np2[2] = {0, 0};  // pairs (the full 64-bit count, stored or not), events
        HIP_TRY(hipMemcpy(np2, npairs.p, 16, hipMemcpyDeviceToHost));
        if (np2[0] > pair_cap) {  // nothing has been applied yet: redo this range in smaller batches (same result)
            rc = pp.release(cur);
            if (rc) return rc;
            if (pa.count <= 1) return fail(CGRT_ERR_LIMIT, "photon pass: one photon's pairs exceed the pair buffer");
            batch = (pa.count < batch ? pa.count : batch) / 2;
            n_halvings++;
            continue;
        }
        const unsigned int np = (unsigned int)np2[0];  // <= pair_cap <= 2^27
        done += pa.count;
        n_events += np2[1];
        // radii shrink as photons arrive: later batches hold fewer pairs.  Never beyond batch_max, the event buffers' size (a
        // batch halved from a size that is not batch_max / 2^k would otherwise double past it)
        if (batch < batch_max && np < pair_cap / 4) batch = batch < batch_max / 2 ? batch * 2 : batch_max;
        if (np != 0) {
            n_pairs += np;
            rc = sort_pairs(main_tmp, pk0.as<unsigned long long>(), pk1.as<unsigned long long>(), pv0.as<unsigned int>(),
                            pv1.as<unsigned int>(), np, pair_key_bits);
            if (rc) return rc;
            hipLaunchKernelGGL(photon_apply_kernel, dim3(nb), dim3(T), 0, 0, pk1.as<unsigned long long>(), pv1.as<unsigned int>(), np,
                               pp.ev[cur].as<double>(), ph.alpha, hp.as<double>(), hps.as<double>(), (long long)n);
            HIP_TRY(hipGetLastError());
        }
        rc = pp.release(cur);
        if (rc) return rc;
    }
    if (keep_ahead && overlap) {
        // the lookahead: the first batch of a next call of as many photons as this one (a run of equal calls is the interactive
        // pattern), traced while the caller looks at the image.  Buffer 1 - cur: the replay of cur may still be running.
        const long long span = call > 0 ? call : (ahead_first == done ? ahead_count : batch);  // an empty call keeps it
        if (ahead_first != done || ahead_count != (span < batch ? span : batch)) {
            const PhotonArgs nx = batch_args(done, batch, done + span);
            rc = pp.produce(s, nx, ha, 1 - cur);
            if (rc) return rc;
            ahead_first = nx.first; ahead_count = nx.count; ahead_buf = 1 - cur;
        }
    } else if (pp.st) {
        ahead_first = -1;
        HIP_TRY(hipStreamSynchronize(pp.st));
    }
    return CGRT_OK;
}

// The image at `done` photons into device buffers (either may be null), enqueued on `st`.
int cgrt_ppm_session::gather(double *d_img, unsigned char *d_rgb8, hipStream_t st) const {
    const int T = 256;
    hipLaunchKernelGGL(ppm_gather_kernel, dim3((unsigned)((npix + T - 1) / T)), dim3(T), 0, st, static_cast<const unsigned int *>(pix_start.p),
                       static_cast<const unsigned int *>(order.p), static_cast<const double *>(hp.p), (double)done * spp, npix, width, rows,
                       d_img, d_rgb8);
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

static int check_photons(const cgrt_photons *ph) {
    if (ph->nphotons < 0 || ph->hashsize < 1 || ph->hashsize > (1 << 20) || ph->batch < 0 || !(ph->initial_radius >= 0) ||
        ph->pair_cap < 0)
        return fail(CGRT_ERR_INVALID, "bad photon parameters");
    return CGRT_OK;
}

extern "C" int cgrt_ppm_render(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid,
                               const cgrt_photons *ph, cgrt_ppm_result *out) {
    int rc = check_grid(s, cam, grid);
    if (rc) return rc;
    if (!ph || !out) return fail(CGRT_ERR_INVALID, "null argument");
    if ((rc = check_photons(ph))) return rc;
    if (grid->stripe_nranks > 1 && out->rgb8)
        return fail(CGRT_ERR_UNSUPPORTED, "photon pass: rgb8 needs contiguous rows; tone-map the assembled frame (cgrt_tonemap_rgb8)");
    ON_DEVICE(s->device);
    cgrt_ppm_session run;
    {
        DevBuf rec;
        rc = run.eye_grid(s, cam, grid, ph, rec);
        out->ms_eye = run.ms_eye;
        if (rc == CGRT_OK) rc = run.table(rec, nullptr, false);
        out->ms_table = run.ms_table;
        if (rc) return rc;
    }
    // ---- photons, in batches ----
    Timer tm;
    tm.start();
    rc = run.photon_setup(false);
    if (rc == CGRT_OK) rc = run.photons(ph->nphotons, false);
    out->n_events = run.n_events;
    out->n_pairs = run.n_pairs;
    out->n_batch_halvings = run.n_halvings;
    if (rc) return rc;
    out->ms_photons = tm.stop();
    // ---- final gather + tone map ----
    tm.start();
    const long long npix = run.npix;
    DevBuf img, rgb8;
    HIP_TRY(img.alloc((size_t)npix * 3 * sizeof(double)));
    if (out->rgb8) HIP_TRY(rgb8.alloc((size_t)npix * 3));
    rc = run.gather(img.as<double>(), out->rgb8 ? rgb8.as<unsigned char>() : nullptr, 0);
    if (rc) return rc;
    out->ms_gather = tm.stop();
    if (out->image) HIP_TRY(hipMemcpy(out->image, img.p, (size_t)npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out->rgb8) HIP_TRY(hipMemcpy(out->rgb8, rgb8.p, (size_t)npix * 3, hipMemcpyDeviceToHost));
    out->hp_count = run.n;
    if (out->hp16 && out->hp_cap) {
        const size_t m = run.n < out->hp_cap ? run.n : (size_t)out->hp_cap;
        HIP_TRY(hipMemcpy(out->hp16, run.hp.p, m * 16 * sizeof(double), hipMemcpyDeviceToHost));
    }
    return CGRT_OK;
}

// ---- resumable photon mapping: the state above, kept between calls -------------------------------------------------
// what both creators do behind the table: the photon buffers and ph.nphotons photons
static int session_first_photons(cgrt_ppm_session &p) {
    Timer tm;
    tm.start();
    int rc = p.photon_setup(true);
    if (rc == CGRT_OK) rc = p.photons(p.ph.nphotons, p.lookahead);
    p.ms_last_add = tm.stop();
    p.ms_photons = p.ms_last_add;
    return rc;
}
extern "C" int cgrt_ppm_session_create(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid,
                                       const cgrt_photons *ph, int flags, cgrt_ppm_session **out) {
    if (!out) return fail(CGRT_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = check_grid(s, cam, grid);
    if (rc) return rc;
    if (!ph) return fail(CGRT_ERR_INVALID, "null argument");
    if ((rc = check_photons(ph))) return rc;
    if (flags & ~CGRT_PPM_SESSION_NO_LOOKAHEAD) return fail(CGRT_ERR_INVALID, "unknown session flags");
    ON_DEVICE(s->device);
    std::unique_ptr<cgrt_ppm_session> p(new (std::nothrow) cgrt_ppm_session());
    if (!p) return fail(CGRT_ERR_LIMIT, "out of host memory");
    p->lookahead = !(flags & CGRT_PPM_SESSION_NO_LOOKAHEAD);
    HIP_TRY(hipEventCreate(&p->img_a));
    HIP_TRY(hipEventCreate(&p->img_b));
    {
        DevBuf rec;
        if ((rc = p->eye_grid(s, cam, grid, ph, rec))) return rc;
        if ((rc = p->table(rec, nullptr, false))) return rc;
    }
    if ((rc = session_first_photons(*p))) return rc;
    *out = p.release();
    return CGRT_OK;
}

extern "C" int cgrt_ppm_session_create_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_pixels *px,
                                            const cgrt_photons *ph, int flags, cgrt_ppm_session **out) {
    if (!out) return fail(CGRT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!s || !rays || !px || !ph) return fail(CGRT_ERR_INVALID, "null argument");
    if (px->width <= 0 || px->rows <= 0 || px->spp <= 0) return fail(CGRT_ERR_INVALID, "ray pixels: width, rows and spp must be positive");
    if ((long long)px->width * px->rows >= (1ll << 31)) return fail(CGRT_ERR_LIMIT, "ray pixels: 2^31 texels or more");
    int rc = check_photons(ph);
    if (rc) return rc;
    if (flags & ~CGRT_PPM_SESSION_NO_LOOKAHEAD) return fail(CGRT_ERR_INVALID, "unknown session flags");
    if ((rc = check_capture_rays(s, rays))) return rc;  // (the last of the checks: it is the one that looks at the scene's state)
    ON_DEVICE(s->device);
    std::unique_ptr<cgrt_ppm_session> p(new (std::nothrow) cgrt_ppm_session());
    if (!p) return fail(CGRT_ERR_LIMIT, "out of host memory");
    p->lookahead = !(flags & CGRT_PPM_SESSION_NO_LOOKAHEAD);
    HIP_TRY(hipEventCreate(&p->img_a));
    HIP_TRY(hipEventCreate(&p->img_b));
    {
        DevBuf rec;
        if ((rc = p->eye_rays(s, rays, px, ph, rec))) return rc;
        if ((rc = p->table(rec, px->pixel, true))) return rc;
        HIP_TRY(hipDeviceSynchronize());  // px->pixel and the records are read before the call returns
    }
    if ((rc = session_first_photons(*p))) return rc;
    *out = p.release();
    return CGRT_OK;
}

extern "C" void cgrt_ppm_session_destroy(cgrt_ppm_session *p) {
    if (!p) return;
    DeviceGuard g(p->s->device);
    if (g.err == hipSuccess) (void)hipStreamSynchronize(0);
    delete p;  // waits for the last gather and the producer stream (lookahead) before freeing
}

extern "C" int cgrt_ppm_session_add_photons(cgrt_ppm_session *p, int64_t count) {
    if (!p || count < 0 || count > LLONG_MAX - p->done) return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(p->s->device);
    if (p->img_pending) HIP_TRY(hipStreamWaitEvent(0, p->img_b, 0));  // a gather on a caller's stream reads hp
    Timer tm;
    tm.start();
    const int rc = p->photons(p->done + count, p->lookahead);
    p->ms_last_add = tm.stop();  // also when a batch failed: what was applied before it has finished
    p->ms_photons += p->ms_last_add;
    return rc;
}

extern "C" int cgrt_ppm_session_add_photon_rays(cgrt_ppm_session *p, const cgrt_photon_rays *pr) {
    if (const int rc = check_photon_rays(pr)) return rc;
    if (!p || pr->n > LLONG_MAX - p->done) return fail(CGRT_ERR_INVALID, "bad argument");
    if (pr->n == 0) return CGRT_OK;
    ON_DEVICE(p->s->device);
    if (p->img_pending) HIP_TRY(hipStreamWaitEvent(0, p->img_b, 0));  // a gather on a caller's stream reads hp
    // the producer stream does not wait for the null stream: arrays a kernel on the null stream still writes must be complete
    if (p->pp.st) HIP_TRY(hipStreamSynchronize(0));
    Timer tm;
    tm.start();
    const int rc = p->photons(p->done + pr->n, false, pr);
    // also when a batch failed: nothing traced ahead from pr's arrays outlives the call
    p->ahead_first = -1;
    if (p->pp.st) {
        const hipError_t e = hipStreamSynchronize(p->pp.st);
        if (e != hipSuccess && rc == CGRT_OK) return fail(CGRT_ERR_DEVICE, std::string("producer stream: ") + hipGetErrorString(e));
    }
    p->ms_last_add = tm.stop();
    p->ms_photons += p->ms_last_add;
    return rc;
}

static int session_image_args(const cgrt_ppm_session *p, const uint8_t *rgb8) {
    if (!p) return fail(CGRT_ERR_INVALID, "null session");
    if (p->done == 0) return fail(CGRT_ERR_INVALID, "photon session: no photon yet (the image would be flux / (PI r2 0))");
    if (rgb8 && p->striped)
        return fail(CGRT_ERR_UNSUPPORTED, "photon session: rgb8 needs contiguous rows; tone-map the assembled frame (cgrt_tonemap_rgb8)");
    return CGRT_OK;
}

extern "C" int cgrt_ppm_session_image(const cgrt_ppm_session *cp, double *image, uint8_t *rgb8) {
    int rc = session_image_args(cp, rgb8);
    if (rc) return rc;
    cgrt_ppm_session *p = const_cast<cgrt_ppm_session *>(cp);  // the image buffers are scratch, not state
    ON_DEVICE(p->s->device);
    const size_t npix = (size_t)p->npix;
    if (image && !p->img.p) HIP_TRY(p->take(p->img, npix * 3 * sizeof(double)));
    if (rgb8 && !p->rgb8.p) HIP_TRY(p->take(p->rgb8, npix * 3));
    HIP_TRY(hipEventRecord(p->img_a, 0));
    rc = p->gather(image ? p->img.as<double>() : nullptr, rgb8 ? p->rgb8.as<unsigned char>() : nullptr, 0);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(p->img_b, 0));
    HIP_TRY(hipEventSynchronize(p->img_b));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->img_a, p->img_b));
    p->ms_last_image = ms;
    p->img_pending = false;
    if (image) HIP_TRY(hipMemcpy(image, p->img.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (rgb8) HIP_TRY(hipMemcpy(rgb8, p->rgb8.p, npix * 3, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

extern "C" int cgrt_ppm_session_image_device(const cgrt_ppm_session *p, double *image, uint8_t *rgb8, void *stream) {
    int rc = session_image_args(p, rgb8);
    if (rc) return rc;
    ON_DEVICE(p->s->device);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipEventRecord(p->img_a, st));
    if ((rc = p->gather(image, rgb8, st))) return rc;
    HIP_TRY(hipEventRecord(p->img_b, st));
    p->img_pending = true;  // the next add_photons waits for it; get_info reads its time
    return CGRT_OK;
}

extern "C" int cgrt_ppm_session_hitpoints(const cgrt_ppm_session *p, double *hp16, uint64_t cap, uint64_t *count) {
    if (!p || !count || (cap > 0 && !hp16)) return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(p->s->device);
    *count = p->n;
    const size_t m = p->n < cap ? p->n : (size_t)cap;
    if (m) HIP_TRY(hipMemcpy(hp16, p->hp.p, m * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

extern "C" int cgrt_ppm_session_get_info(const cgrt_ppm_session *p, cgrt_ppm_session_info *out) {
    if (!p || !out) return fail(CGRT_ERR_INVALID, "null argument");
    if (p->img_pending) {
        ON_DEVICE(p->s->device);
        HIP_TRY(hipEventSynchronize(p->img_b));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->img_a, p->img_b));
        p->ms_last_image = ms;
        p->img_pending = false;
    }
    out->photons_done = p->done;
    out->hp_count = p->n;
    out->n_events = p->n_events;
    out->n_pairs = p->n_pairs;
    out->n_batch_halvings = p->n_halvings;
    out->device_bytes = p->bytes();
    out->ms_eye = p->ms_eye;
    out->ms_table = p->ms_table;
    out->ms_photons = p->ms_photons;
    out->ms_last_add = p->ms_last_add;
    out->ms_last_image = p->ms_last_image;
    return CGRT_OK;
}

// ---- PNG (host): signature, IHDR, one IDAT of stored deflate blocks, IEND -------------------------------------------
namespace {
struct Crc32 {
    uint32_t table[256];
    Crc32() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    }
    uint32_t run(uint32_t crc, const unsigned char *p, size_t n) const {
        for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
        return crc;
    }
};
void put32(std::vector<unsigned char> &v, uint32_t x) {
    v.push_back((unsigned char)(x >> 24)); v.push_back((unsigned char)(x >> 16));
    v.push_back((unsigned char)(x >> 8)); v.push_back((unsigned char)x);
}
bool write_chunk(FILE *f, const Crc32 &crc, const char type[4], const std::vector<unsigned char> &data) {
    std::vector<unsigned char> head;
    put32(head, (uint32_t)data.size());
    head.insert(head.end(), type, type + 4);
    uint32_t c = crc.run(0xffffffffu, head.data() + 4, 4);
    c = crc.run(c, data.data(), data.size()) ^ 0xffffffffu;
    std::vector<unsigned char> tail;
    put32(tail, c);
    return std::fwrite(head.data(), 1, head.size(), f) == head.size() &&
           (data.empty() || std::fwrite(data.data(), 1, data.size(), f) == data.size()) &&
           std::fwrite(tail.data(), 1, 4, f) == 4;
}
}  // namespace

extern "C" int cgrt_write_png(const char *path, int width, int height, const uint8_t *rgb8) {
    if (!path || !rgb8 || width < 1 || height < 1 || (uint64_t)width * height > (1ull << 28))
        return fail(CGRT_ERR_INVALID, "bad argument");
    // raw scanlines: filter byte 0 + width*3 bytes
    const size_t stride = (size_t)width * 3, raw_n = (stride + 1) * height;
    std::vector<unsigned char> raw(raw_n);
    for (int y = 0; y < height; y++) {
        raw[(stride + 1) * y] = 0;
        std::memcpy(&raw[(stride + 1) * y + 1], rgb8 + stride * y, stride);
    }
    std::vector<unsigned char> z;
    z.reserve(raw_n + raw_n / 65535 * 5 + 16);
    z.push_back(0x78); z.push_back(0x01);  // zlib header: deflate, 32 K window, no preset dictionary
    uint32_t a = 1, b = 0;                 // adler32
    for (size_t off = 0; off < raw_n; off += 65535) {
        const size_t len = raw_n - off < 65535 ? raw_n - off : 65535;
        z.push_back(off + len == raw_n ? 1 : 0);  // BFINAL, BTYPE = 00 (stored)
        z.push_back((unsigned char)(len & 0xff)); z.push_back((unsigned char)(len >> 8));
        z.push_back((unsigned char)(~len & 0xff)); z.push_back((unsigned char)((~len >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + off, raw.begin() + off + len);
        for (size_t i = 0; i < len; i += 5552) {  // adler32 with deferred modulo
            const size_t m = len - i < 5552 ? len - i : 5552;
            for (size_t k = 0; k < m; k++) { a += raw[off + i + k]; b += a; }
            a %= 65521u; b %= 65521u;
        }
    }
    put32(z, (b << 16) | a);
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(CGRT_ERR_IO, std::string("cannot open ") + path);
    static const Crc32 crc;
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<unsigned char> ihdr;
    put32(ihdr, (uint32_t)width); put32(ihdr, (uint32_t)height);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);  // 8-bit RGB
    const bool ok = std::fwrite(sig, 1, 8, f) == 8 && write_chunk(f, crc, "IHDR", ihdr) && write_chunk(f, crc, "IDAT", z) &&
                    write_chunk(f, crc, "IEND", std::vector<unsigned char>());
    if (std::fclose(f) != 0 || !ok) return fail(CGRT_ERR_IO, std::string("write failed: ") + path);
    return CGRT_OK;
}
