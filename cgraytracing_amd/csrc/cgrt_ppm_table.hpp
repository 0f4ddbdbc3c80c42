// The photon pass's hitpoint table: the kernels that put the eye pass's Hitpoint records into the reference's table order
// (grid and ray-buffer forms) and build the per-pixel index over them, and PpmTable::build, which launches them.
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

}  // namespace
