// From a batch's events to the image: event_keys_kernel and PhotonProducer (trace, then events in hash-cell order, on a stream of
// its own), the pair search, the ordered replay per hitpoint, and the final gather over the per-pixel index.
namespace {

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
    const int rc = sort_pairs(tmp, ek0[b].as<unsigned int>(), ek1[b].as<unsigned int>(), eo0[b].as<unsigned int>(),
                              eo1[b].as<unsigned int>(), (size_t)nslots, 32, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(produced[b], st));
    return CGRT_OK;
}

}  // namespace
