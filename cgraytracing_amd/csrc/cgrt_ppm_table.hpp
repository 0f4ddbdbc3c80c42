// The photon pass's hitpoint table: the kernels that put the eye pass's Hitpoint records into the reference's table order
// (grid and ray-buffer forms), those that do the same for Hitpoint records of the caller's, and build the per-pixel index over
// them, and PpmTable::build, which launches them.
#include <rocprim/device/device_radix_sort.hpp>

namespace {

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

// ---- the same table for caller-supplied Hitpoint records (cgrt_ppm_session_create_hitpoints), read from the caller's arrays.
// Order contract: inside a bucket by texel, then by ray id, then by the record's path in emission order (hp_path_key of
// cgrt_hp_order.h), then by position in the input -- the ray form's order with a record's own texel and any number of records
// per ray.  The radix sort is stable, so the passes run least significant first: path key, ray id, (bucket << 32 | texel).  A
// record that is not kept (cgrt.h: its texel, path, ray or pos) sorts behind every kept one in the ray pass and in the bucket pass.
struct HpRecords {
    const double *hp9;
    const long long *ray;
    const unsigned int *path;
    const long long *pixel;
    long long n, npix;
};
static constexpr unsigned int kHpDropped = 0xFFFFFFFFu;  // texel of a record that is not kept

__device__ __forceinline__ long long hp_rec_ray(const HpRecords &r, long long i) { return r.ray ? r.ray[i] : i; }
// the texel record i gathers into, or -1: the record is dropped
__device__ __forceinline__ long long hp_rec_texel(const HpRecords &r, long long i) {
    const long long ray = hp_rec_ray(r, i);
    if (!hp_ray_ok(ray)) return -1;
    if (r.path && !hp_path_ok(r.path[i])) return -1;
    const double *q = r.hp9 + 9 * i;
    if (!(isfinite(q[3]) && isfinite(q[4]) && isfinite(q[5]))) return -1;
    const long long t = r.pixel ? r.pixel[i] : ray % r.npix;
    return t >= 0 && t < r.npix ? t : -1;
}
// texel[i] (kHpDropped: not kept), vals[i] = i, stats = {largest ray id among the kept, records kept} (zeroed by the caller)
__global__ void hp_rec_mark_kernel(HpRecords r, unsigned int *__restrict__ texel, unsigned int *__restrict__ vals,
                                   unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_max[256];
    __shared__ unsigned int s_cnt[256];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mx = 0;
    unsigned int kept = 0;
    if (i < r.n) {
        const long long t = hp_rec_texel(r, i);
        texel[i] = t < 0 ? kHpDropped : (unsigned int)t;
        vals[i] = (unsigned int)i;
        if (t >= 0) {
            mx = (unsigned long long)hp_rec_ray(r, i);
            kept = 1;
        }
    }
    s_max[threadIdx.x] = mx;
    s_cnt[threadIdx.x] = kept;
    __syncthreads();
    for (unsigned int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            if (s_max[threadIdx.x + s] > s_max[threadIdx.x]) s_max[threadIdx.x] = s_max[threadIdx.x + s];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_cnt[0]) {
        atomicMax(&stats[0], s_max[0]);
        atomicAdd(&stats[1], (unsigned long long)s_cnt[0]);
    }
}
// pass 1, in input order (vals is still the identity): the path's total key; a dropped record's key does not matter
__global__ void hp_rec_path_keys_kernel(const unsigned int *__restrict__ path, long long n, unsigned long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int p = path[i];
    keys[i] = hp_path_ok(p) ? hp_path_key(p) : 0ull;
}
// pass 2, in the order of vals: the ray id; dropped_key (the largest kept id + 1) for a record that is not kept
__global__ void hp_rec_ray_keys_kernel(const long long *__restrict__ ray, const unsigned int *__restrict__ texel,
                                       const unsigned int *__restrict__ vals, long long n, unsigned long long dropped_key,
                                       unsigned long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int r = vals[i];
    keys[i] = texel[r] == kHpDropped ? dropped_key : (unsigned long long)ray[r];
}
// keys, vals: the records by (ray, path, input position), the dropped ones last.  rank[record] = its position minus the start of
// its ray's run: hp16[1].  A rank, not a label: nothing is decoded from it, so it has no 4-bit limit
__global__ void hp_rec_rank_kernel(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ vals, long long n,
                                   unsigned long long dropped_key, unsigned int *__restrict__ rank) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    if (k == dropped_key) return;
    long long lo = 0, hi = i;  // first index with keys >= k
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    rank[vals[i]] = (unsigned int)(i - lo);
}
// pass 3, in the order of vals: (bucket << 32) | texel; a dropped record gets the bucket `hashsize`, behind every real one
__global__ void hp_rec_bucket_keys_kernel(const double *__restrict__ hp9, const unsigned int *__restrict__ texel,
                                          const unsigned int *__restrict__ vals, long long n, HashArgs ha,
                                          unsigned long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int r = vals[i];
    const unsigned int t = texel[r];
    if (t == kHpDropped) {
        keys[i] = (unsigned long long)ha.hashsize << 32;
        return;
    }
    const double *q = hp9 + 9 * (long long)r;
    int ix, iy, iz;
    ref_coord(q[3], q[4], q[5], ha.celllength, ix, iy, iz);
    keys[i] = ((unsigned long long)ref_hash(ix, iy, iz, ha.hashsize) << 32) | t;  // bucket < 2^20, texel < 2^31
}
// hp_ray_gather_kernel for the m kept records in table order (keys, vals: pass 3's output): hp[0] = the ray id, hp[1] = the rank;
// and, the texel being in the key, the per-pixel index's keys (pixel, then table order) as image_ray_keys_kernel writes them
__global__ void hp_rec_gather_kernel(HpRecords in, const unsigned int *__restrict__ rank, const unsigned long long *__restrict__ keys,
                                     const unsigned int *__restrict__ vals, long long m, double r2_init, double *__restrict__ hp,
                                     double *__restrict__ hps, int *__restrict__ bucket_of, unsigned long long *__restrict__ img_keys,
                                     unsigned int *__restrict__ img_vals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long r = (long long)vals[i];
    const double *q = in.hp9 + 9 * r;
    double *o = hp + 16 * i;
    o[0] = (double)hp_rec_ray(in, r);
    o[1] = rank ? (double)rank[r] : 0.0;
    for (int k = 0; k < 9; k++) o[2 + k] = q[k];
    o[11] = 0; o[12] = 0; o[13] = 0;
    o[14] = r2_init;
    o[15] = 0;
    double *c = hps + 8 * i;
    for (int k = 0; k < 3; k++) c[k] = q[3 + k];
    c[3] = r2_init;
    for (int k = 0; k < 3; k++) c[4 + k] = q[6 + k];
    c[7] = 0;
    const unsigned long long key = keys[i];
    bucket_of[i] = (int)(key >> 32);
    img_keys[i] = ((key & 0xFFFFFFFFull) << 32) | (unsigned long long)i;
    img_vals[i] = (unsigned int)i;
}

// radix sort of (key, value) pairs by the keys' low end_bit bits; K: unsigned long long or unsigned int
template <class K>
int sort_pairs(GrowBuf &tmp, K *kin, K *kout, unsigned int *vin, unsigned int *vout, size_t n, int end_bit = (int)(8 * sizeof(K)),
               hipStream_t st = 0) {
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit, st));
    HIP_TRY(tmp.need(tmp_bytes));
    HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit, st));
    return CGRT_OK;
}

// The Hitpoints in the reference's table order -- (bucket, insertion order) -- and the per-pixel index over them
struct PpmTable {
    size_t n = 0;  // hitpoints
    long long npix = 0;
    HashArgs ha{};
    DevBuf hp, hps, bstart, pix_start, order;
    int64_t dev_bytes = 0;  // what build() allocated and keeps

    hipError_t take(DevBuf &b, size_t bytes) {
        dev_bytes += (int64_t)bytes;
        return b.alloc(bytes);
    }
    // rec: the n records of the eye pass.  rays: their labels are (ray << 4 | seq) and ray_pixel (DEVICE, or null) maps rays to
    // texels; else they are a grid's, of npix pixels with spp samples.  tmp: sort scratch.
    int build(DevBuf &rec, const cgrt_photons &ph, int spp, const int64_t *ray_pixel, bool rays, GrowBuf &tmp);
    // in: the caller's Hitpoint records (DEVICE arrays, read here and not afterwards); sets n to the number kept.  npix is set.
    int build(const cgrt_hitpoints &in, const cgrt_photons &ph, GrowBuf &tmp);
};

int PpmTable::build(DevBuf &rec, const cgrt_photons &ph, int spp, const int64_t *ray_pixel, bool rays, GrowBuf &tmp) {
    int rc = CGRT_OK;
    DevBuf bucket_of, k0, k1, v0, v1;
    const long long *pixel = reinterpret_cast<const long long *>(ray_pixel);
    HIP_TRY(take(hp, n * 16 * sizeof(double)));
    HIP_TRY(take(hps, n * 8 * sizeof(double)));
    HIP_TRY(take(bstart, ((size_t)ph.hashsize + 2) * sizeof(int)));
    HIP_TRY(take(pix_start, ((size_t)npix + 1) * sizeof(unsigned int)));
    HIP_TRY(bucket_of.alloc(n * sizeof(int)));
    HIP_TRY(k0.alloc(n * 8)); HIP_TRY(k1.alloc(n * 8)); HIP_TRY(v0.alloc(n * 4)); HIP_TRY(v1.alloc(n * 4));
    const PpmGrid g = ppm_grid(ph);
    ha = g.ha;
    const double r0 = g.r0;
    const int T = 256;
    const unsigned nb = (unsigned)((n + T - 1) / T);
    unsigned long long *const K0 = k0.as<unsigned long long>(), *const K1 = k1.as<unsigned long long>();
    unsigned int *const V0 = v0.as<unsigned int>(), *const V1 = v1.as<unsigned int>();
    if (n && rays) {
        hipLaunchKernelGGL(hp_ray_label_keys_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), (long long)n, K0, V0);
        if ((rc = sort_pairs(tmp, K0, K1, V0, V1, n, 40))) return rc;
        hipLaunchKernelGGL(hp_ray_bucket_keys_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), V1, (long long)n, ha, pixel, npix, K0);
        if ((rc = sort_pairs(tmp, K0, K1, V1, V0, n, 52))) return rc;
        hipLaunchKernelGGL(hp_ray_gather_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), K1, V0, (long long)n, r0 * r0, hp.as<double>(),
                           hps.as<double>(), bucket_of.as<int>());
        hipLaunchKernelGGL(image_ray_keys_kernel, dim3(nb), dim3(T), 0, 0, hp.as<double>(), (long long)n, pixel, npix, K0, V0);
        if ((rc = sort_pairs(tmp, K0, K1, V0, V1, n))) return rc;
    } else if (n) {
        hipLaunchKernelGGL(hp_keys_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), (long long)n, ha, (int)npix, spp, K0, V0);
        if ((rc = sort_pairs(tmp, K0, K1, V0, V1, n))) return rc;
        hipLaunchKernelGGL(hp_gather_kernel, dim3(nb), dim3(T), 0, 0, rec.as<double>(), K1, V1, (long long)n, r0 * r0, hp.as<double>(),
                           hps.as<double>(), bucket_of.as<int>());
        hipLaunchKernelGGL(image_keys_kernel, dim3(nb), dim3(T), 0, 0, hp.as<double>(), (long long)n, spp, K0, V0);
        if ((rc = sort_pairs(tmp, K0, K1, V0, V1, n))) return rc;
    }
    hipLaunchKernelGGL(bucket_start_kernel, dim3((ph.hashsize + 1 + T - 1) / T), dim3(T), 0, 0, bucket_of.as<int>(),
                       (long long)n, ph.hashsize, bstart.as<int>());
    hipLaunchKernelGGL(pix_start_kernel, dim3((unsigned)((npix + 1 + T - 1) / T)), dim3(T), 0, 0, K1, (long long)n, npix,
                       pix_start.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    order.p = v1.release();  // hitpoint indices by pixel, then table order
    dev_bytes += (int64_t)(n ? n * 4 : 16);
    return CGRT_OK;
}

int PpmTable::build(const cgrt_hitpoints &in, const cgrt_photons &ph, GrowBuf &tmp) {
    int rc = CGRT_OK;
    const size_t nin = (size_t)in.n;
    DevBuf bucket_of, kbuf[2], vbuf[2], texel, rank, stats;
    const PpmGrid g = ppm_grid(ph);
    ha = g.ha;
    const double r0 = g.r0;
    const int T = 256;
    const unsigned nb_in = (unsigned)((nin + T - 1) / T);
    HIP_TRY(take(bstart, ((size_t)ph.hashsize + 2) * sizeof(int)));
    HIP_TRY(take(pix_start, ((size_t)npix + 1) * sizeof(unsigned int)));
    for (int k = 0; k < 2; k++) {
        HIP_TRY(kbuf[k].alloc(nin * 8));
        HIP_TRY(vbuf[k].alloc(nin * 4));
    }
    // a pass reads K[0] / V[0] and the sort writes K[1] / V[1]; the values then change places, the keys are made anew
    unsigned long long *const K[2] = {kbuf[0].as<unsigned long long>(), kbuf[1].as<unsigned long long>()};
    int vin = 0;
    auto V = [&](int which) { return vbuf[vin ^ which].as<unsigned int>(); };
    const HpRecords recs{in.hp9, reinterpret_cast<const long long *>(in.ray), in.path, reinterpret_cast<const long long *>(in.pixel),
                         (long long)nin, npix};
    n = 0;
    unsigned long long st[2] = {0, 0};  // largest kept ray id, records kept
    if (nin) {
        HIP_TRY(texel.alloc(nin * 4));
        HIP_TRY(stats.alloc(16));
        HIP_TRY(hipMemsetAsync(stats.p, 0, 16, 0));
        hipLaunchKernelGGL(hp_rec_mark_kernel, dim3(nb_in), dim3(T), 0, 0, recs, texel.as<unsigned int>(), V(0),
                           stats.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(st, stats.p, 16, hipMemcpyDeviceToHost));
        n = (size_t)st[1];
    }
    HIP_TRY(take(hp, n * 16 * sizeof(double)));
    HIP_TRY(take(hps, n * 8 * sizeof(double)));
    HIP_TRY(bucket_of.alloc(n * sizeof(int)));
    if (n) {
        const unsigned nb = (unsigned)((n + T - 1) / T);
        if (in.ray) {  // (without ids every record is a ray of its own: input order is the order, and every rank is 0)
            if (in.path) {
                hipLaunchKernelGGL(hp_rec_path_keys_kernel, dim3(nb_in), dim3(T), 0, 0, in.path, (long long)nin, K[0]);
                if ((rc = sort_pairs(tmp, K[0], K[1], V(0), V(1), nin, kHpPathKeyBits))) return rc;
                vin ^= 1;
            }
            const unsigned long long dropped_key = st[0] + 1;  // <= 2^36
            hipLaunchKernelGGL(hp_rec_ray_keys_kernel, dim3(nb_in), dim3(T), 0, 0, recs.ray, texel.as<unsigned int>(), V(0),
                               (long long)nin, dropped_key, K[0]);
            if ((rc = sort_pairs(tmp, K[0], K[1], V(0), V(1), nin, hp_key_bits(dropped_key)))) return rc;
            vin ^= 1;
            HIP_TRY(rank.alloc(nin * 4));
            hipLaunchKernelGGL(hp_rec_rank_kernel, dim3(nb_in), dim3(T), 0, 0, K[1], V(0), (long long)nin, dropped_key,
                               rank.as<unsigned int>());
        }
        hipLaunchKernelGGL(hp_rec_bucket_keys_kernel, dim3(nb_in), dim3(T), 0, 0, in.hp9, texel.as<unsigned int>(), V(0), (long long)nin,
                           ha, K[0]);
        if ((rc = sort_pairs(tmp, K[0], K[1], V(0), V(1), nin, kHpTexelBits + hp_key_bits((uint64_t)ph.hashsize)))) return rc;
        vin ^= 1;
        // the kept records are the first n; the image keys go where the sort's input was
        hipLaunchKernelGGL(hp_rec_gather_kernel, dim3(nb), dim3(T), 0, 0, recs, rank.as<unsigned int>(), K[1], V(0), (long long)n, r0 * r0,
                           hp.as<double>(), hps.as<double>(), bucket_of.as<int>(), K[0], V(1));
        vin ^= 1;
        if ((rc = sort_pairs(tmp, K[0], K[1], V(0), V(1), n))) return rc;
        vin ^= 1;
    }
    hipLaunchKernelGGL(bucket_start_kernel, dim3((ph.hashsize + 1 + T - 1) / T), dim3(T), 0, 0, bucket_of.as<int>(), (long long)n,
                       ph.hashsize, bstart.as<int>());
    hipLaunchKernelGGL(pix_start_kernel, dim3((unsigned)((npix + 1 + T - 1) / T)), dim3(T), 0, 0, K[1], (long long)n, npix,
                       pix_start.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    // hitpoint indices by pixel, then table order.  The input's arrays are read by kernels enqueued above: the caller waits
    order.p = vbuf[vin].release();
    dev_bytes += (int64_t)(nin ? nin * 4 : 16);
    return CGRT_OK;
}

}  // namespace
