// Stochastic progressive photon mapping (Hachisuka & Jensen 2009): cgrt_sppm_session -- statistics that belong to the TEXEL
// (N, R2, tau) and live for the session, Hitpoints that live for one pass -- its kernels and the cgrt_sppm_* entry points.
//
// A pass is the photon pass of cgrt_ppm_session.hpp with another ending.  Its stages up to the sorted pairs are that file's, the
// same code: the Hitpoint capture of a grid or of rays, PpmTable::build, PhotonProducer, photon_pairs_kernel, sort_pairs, the
// batches PpmSchedule decides.  Every Hitpoint searches with its texel's radius, which does not change while the pass runs, so
// the pairs that pass the search's two tests ARE the accepted set: there is no replay against a shrinking radius.  Per
// Hitpoint the accepted photons' flux is summed in slot order (sppm_hitpoint_sum_kernel, once per applied batch), per texel the
// Hitpoints' sums in the per-pixel index order, and the texel takes sppm_update (cgrt_sppm_plan.h) once
// (sppm_pixel_update_kernel, when every batch of the pass has been applied).  A failing pass therefore never touches the
// texels.
#include "cgrt_sppm_plan.h"

namespace {

// the texel of Hitpoint i of the pass's table: image_keys_kernel's (a grid's label pixel * spp + sample) or
// image_ray_keys_kernel's (the ray index, through the caller's map)
__device__ __forceinline__ unsigned long long sppm_texel(const double *__restrict__ hp, long long i, int spp, bool rays,
                                                         const long long *__restrict__ pixel, long long npix) {
    const unsigned long long lab = (unsigned long long)hp[16 * i];
    return rays ? ray_texel(pixel, lab, npix) : lab / (unsigned long long)spp;
}

// the session's texels before the first pass
__global__ void sppm_init_kernel(double r2_init, long long npix, double *__restrict__ px) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    double *s = px + kSppmPixelDoubles * p;
    s[0] = 0;
    s[1] = r2_init;
    for (int k = 2; k < kSppmPixelDoubles; k++) s[k] = 0;
}

// 1. one lane per Hitpoint of the new table: its search radius is its texel's, its sums start at zero
__global__ void sppm_seed_radius_kernel(double *__restrict__ hp, double *__restrict__ hps, long long nhp, int spp, int rays,
                                        const long long *__restrict__ pixel, long long npix, const double *__restrict__ px) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nhp) return;
    const unsigned long long t = sppm_texel(hp, i, spp, rays != 0, pixel, npix);
    const double r2 = t < (unsigned long long)npix ? px[kSppmPixelDoubles * t + 1] : 0.0;  // (the table holds no other texel)
    double *h = hp + 16 * i;
    h[11] = 0; h[12] = 0; h[13] = 0;
    h[14] = r2;
    h[15] = 0;
    hps[8 * i + 3] = r2;
}

// 3. per Hitpoint, the left fold over its pairs of one batch in slot order (photon, then segment), continued from the batches
// before: Phi_h += f * flux / PI (the expression inside photon_apply_kernel), M_h += 1.  The first pair by binary search and
// the chunked loads (key -> slot -> event) are photon_apply_kernel's.
__global__ void sppm_hitpoint_sum_kernel(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ vals,
                                         unsigned int npairs, const double *__restrict__ events, double *__restrict__ hp,
                                         long long nhp) {
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
    const V3 f = mk(h[2], h[3], h[4]);
    V3 phi = mk(h[11], h[12], h[13]);
    double m = h[15];
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
        double e[kChunk][3];
#pragma unroll
        for (int c = 0; c < kChunk; c++) {
            const double *q = events + 9 * (size_t)slot[c];
            e[c][0] = q[6]; e[c][1] = q[7]; e[c][2] = q[8];
        }
        bool more = true;
#pragma unroll
        for (int c = 0; c < kChunk; c++) {
            more = more && mine[c];  // the hitpoint's pairs are contiguous: the first foreign key ends the fold
            if (more) {
                phi = phi + mulv(f, mk(e[c][0], e[c][1], e[c][2])) * (1.0 / kPiRef);
                m += 1.0;
            }
        }
        if (!more) break;
        k += kChunk;
    }
    h[11] = phi.x; h[12] = phi.y; h[13] = phi.z;
    h[15] = m;
}

// 4 + 5. one lane per texel: the left fold from 0 over its Hitpoints in the per-pixel index order, then sppm_update
__global__ void sppm_pixel_update_kernel(const unsigned int *__restrict__ pix_start, const unsigned int *__restrict__ order,
                                         const double *__restrict__ hp, double alpha, long long npix, double *__restrict__ px) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const unsigned int k0 = pix_start[p], k1 = pix_start[p + 1];
    double phi[3] = {0, 0, 0}, m = 0;
    for (unsigned int k = k0; k < k1; k++) {
        const double *h = hp + 16 * (size_t)order[k];
        phi[0] += h[11]; phi[1] += h[12]; phi[2] += h[13];
        m += h[15];
    }
    double *s = px + kSppmPixelDoubles * p;
    double N = s[0], R2 = s[1], tau[3] = {s[2], s[3], s[4]};
    sppm_update(N, R2, tau, m, phi, alpha);
    s[0] = N; s[1] = R2;
    s[2] = tau[0]; s[3] = tau[1]; s[4] = tau[2];
    s[5] = m;
    s[6] = (double)(k1 - k0);
    s[7] = 0;
}

// image[p] = tau / (PI * R2 * photons_done * spp); image and rgb8 may each be null, rgb8 as ppm_gather_kernel writes it
__global__ void sppm_image_kernel(const double *__restrict__ px, double norm, long long npix, int W, int rows,
                                  double *__restrict__ image, unsigned char *__restrict__ rgb8) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const double *s = px + kSppmPixelDoubles * p;
    const double sc = 1.0 / (kPiRef * s[1] * norm);
    const double r = s[2] * sc, g = s[3] * sc, b = s[4] * sc;
    if (image) {
        image[3 * p] = r; image[3 * p + 1] = g; image[3 * p + 2] = b;
    }
    if (rgb8) {
        const long long row = p / W, col = p % W;
        unsigned char *o = rgb8 + ((long long)(rows - 1 - row) * W + col) * 3;
        o[0] = tonemap_byte(r); o[1] = tonemap_byte(g); o[2] = tonemap_byte(b);
    }
}

}  // namespace

struct cgrt_sppm_session {
    const cgrt_scene *s = nullptr;
    cgrt_photons ph{};  // nphotons is not used
    int width = 0, rows = 0, spp = 1, photon_depth = 0;
    long long npix = 0;
    bool have_stripe = false;  // a grid pass has fixed `stripe`
    uint64_t geometry_gen = 0;  // the scene's refit count at creation: the texels' statistics are those of that geometry
    SppmStripe stripe;
    DevBuf px;                       // [npix][kSppmPixelDoubles], for the session's life
    std::unique_ptr<PpmTable> tab;   // the last pass's Hitpoints (null before the first pass and after a failed one)
    GrowBuf pk0, pk1, pv0, pv1;      // (hitpoint, event) pairs of one batch; they grow with the largest pass's pair_cap
    DevBuf npairs, img, rgb8;
    int64_t dev_bytes = 0;  // px, npairs, img, rgb8
    int64_t producer_bytes = 0;
    GrowBuf main_tmp;
    PhotonProducer pp;  // declared last of the buffers: its destructor waits for its stream before they are freed
    bool pp_ready = false, pp_broken = false;
    long long photons_done = 0, passes = 0;
    uint64_t n_events = 0, n_pairs = 0, n_halvings = 0;
    double ms_eye = 0, ms_table = 0, ms_photons = 0, ms_update = 0;
    hipEvent_t img_b = nullptr;  // behind the last image on a caller's stream: the next pass waits for it
    bool img_pending = false;

    ~cgrt_sppm_session() {
        if (img_b) {
            (void)hipEventSynchronize(img_b);
            (void)hipEventDestroy(img_b);
        }
    }
    hipError_t take(DevBuf &b, size_t bytes) {
        dev_bytes += (int64_t)bytes;
        return b.alloc(bytes);
    }
    int64_t bytes() const {
        return dev_bytes + (tab ? tab->dev_bytes : 0) + producer_bytes + (int64_t)(pk0.cap + pk1.cap + pv0.cap + pv1.cap) +
               (int64_t)main_tmp.cap + (int64_t)pp.tmp.cap;
    }
    bool striped() const { return have_stripe && stripe.nranks > 1; }
    template <class Capture> int pass(Capture capture, const int64_t *ray_pixel, bool rays, long long count);
    int photons(PpmTable &t, long long count, uint64_t &events, uint64_t &pairs);
    int image(double *d_img, unsigned char *d_rgb8, hipStream_t st) const;
};

// Photons [photons_done, photons_done + count) against table t, applied on the null stream batch by batch as a fresh PpmSchedule
// decides: cgrt_ppm_session::photons with the sum in the replay's place, its own photons only and nothing traced ahead when it
// ends.  Nothing of the session's state changes here: the caller commits the pass.
int cgrt_sppm_session::photons(PpmTable &t, long long count, uint64_t &events, uint64_t &pairs) {
    if (pp_broken) return fail(CGRT_ERR_DEVICE, "sppm session: the photon producer could not be set up");
    const PpmSetup setup = ppm_setup(ph, t.n, true, photon_overlap_allowed());
    if (!pp_ready) {  // the event buffers' size is ph.batch's: set up once
        if (const int rc = pp.init(setup.nbuf, (size_t)setup.batch * kSegStride, setup.overlap)) {
            pp_broken = true;
            return rc;
        }
        pp_ready = true;
        producer_bytes = setup.producer_bytes;
    }
    HIP_TRY(pk0.need((size_t)setup.pair_cap * 8)); HIP_TRY(pk1.need((size_t)setup.pair_cap * 8));
    HIP_TRY(pv0.need((size_t)setup.pair_cap * 4)); HIP_TRY(pv1.need((size_t)setup.pair_cap * 4));
    PpmSchedule sched;  // a fresh one per pass: nothing is traced ahead from one pass to the next
    sched.start(setup);
    sched.done = photons_done;
    (void)sched.begin(photons_done + count, false, false);
    const PairBufs pb{static_cast<unsigned long long *>(pk0.p), static_cast<unsigned long long *>(pk1.p), static_cast<unsigned int *>(pv0.p),
                      static_cast<unsigned int *>(pv1.p), npairs.as<unsigned long long>()};
    const int T = 256;
    const unsigned nb = (unsigned)((t.n + T - 1) / T);
    const int rc = photon_batches(
        sched, pp, t, pb, main_tmp, events, pairs,
        [&](const PpmBatch &b) { return pp.produce(s, photon_args(ph, b.first, b.count, photon_depth), t.ha, b.buf); },
        [&](unsigned int np, int cur) -> int {  // 3. the sums, in the replay's place
            hipLaunchKernelGGL(sppm_hitpoint_sum_kernel, dim3(nb), dim3(T), 0, 0, pb.k1, pb.v1, np, pp.ev[cur].as<double>(), t.hp.as<double>(),
                               (long long)t.n);
            HIP_TRY(hipGetLastError());
            return CGRT_OK;
        });
    n_halvings += sched.n_halvings;  // they happened, whatever becomes of the pass
    if (pp.st) HIP_TRY(hipStreamSynchronize(pp.st));  // also after a failed batch: nothing traced ahead outlives the pass
    return rc;
}

// One pass.  capture(cap, &d_rec, &count): hitpoints_device over the pass's grid or ray_hitpoints_device over its rays;
// ray_pixel, rays: see PpmTable::build
template <class Capture>
int cgrt_sppm_session::pass(Capture capture, const int64_t *ray_pixel, bool rays, long long count) {
    if (img_pending) {  // an image on a caller's stream reads the texels
        HIP_TRY(hipStreamWaitEvent(0, img_b, 0));
        img_pending = false;
    }
    tab.reset();  // the last pass's Hitpoints go before the new ones come: a session never holds two tables
    std::unique_ptr<PpmTable> t(new (std::nothrow) PpmTable());
    if (!t) return fail(CGRT_ERR_LIMIT, "out of host memory");
    Timer tm;
    int rc = CGRT_OK;
    {
        DevBuf rec;
        tm.start();
        uint64_t nhp = 0;
        if ((rc = capture(0, nullptr, &nhp))) return rc;
        if (nhp >= (1ull << 31)) return fail(CGRT_ERR_LIMIT, "sppm pass: more than 2^31 hitpoints");
        t->npix = npix;
        t->n = (size_t)nhp;
        if (t->n) {
            double *d_rec = nullptr;
            rc = capture(nhp, &d_rec, &nhp);
            rec.p = d_rec;
            if (rc) return rc;
        }
        ms_eye = tm.stop();
        tm.start();
        if ((rc = t->build(rec, ph, spp, ray_pixel, rays, main_tmp))) return rc;
        const int T = 256;
        if (t->n) {
            hipLaunchKernelGGL(sppm_seed_radius_kernel, dim3((unsigned)((t->n + T - 1) / T)), dim3(T), 0, 0, t->hp.as<double>(),
                               t->hps.as<double>(), (long long)t->n, spp, rays ? 1 : 0, reinterpret_cast<const long long *>(ray_pixel), npix,
                               px.as<double>());
            HIP_TRY(hipGetLastError());
        }
        ms_table = tm.stop();  // (waits: ray_pixel and the records have been read)
    }
    uint64_t events = 0, pairs = 0;
    tm.start();
    if (t->n && count > 0) rc = photons(*t, count, events, pairs);
    ms_photons = tm.stop();
    if (rc) return rc;  // the texels are those of the pass before
    tm.start();
    const int T = 256;
    hipLaunchKernelGGL(sppm_pixel_update_kernel, dim3((unsigned)((npix + T - 1) / T)), dim3(T), 0, 0, t->pix_start.as<unsigned int>(),
                       t->order.as<unsigned int>(), t->hp.as<double>(), ph.alpha, npix, px.as<double>());
    HIP_TRY(hipGetLastError());
    ms_update = tm.stop();
    tab = std::move(t);
    n_events += events;
    n_pairs += pairs;
    photons_done += count;
    passes++;
    return CGRT_OK;
}

int cgrt_sppm_session::image(double *d_img, unsigned char *d_rgb8, hipStream_t st) const {
    const int T = 256;
    hipLaunchKernelGGL(sppm_image_kernel, dim3((unsigned)((npix + T - 1) / T)), dim3(T), 0, st, static_cast<const double *>(px.p),
                       (double)photons_done * spp, npix, width, rows, d_img, d_rgb8);
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

extern "C" int cgrt_sppm_update_host(double N, double R2, const double *tau3, double M, const double *phi3, double alpha, double *out5) {
    if (!tau3 || !phi3 || !out5) return fail(CGRT_ERR_INVALID, "null argument");
    double tau[3] = {tau3[0], tau3[1], tau3[2]};
    sppm_update(N, R2, tau, M, phi3, alpha);
    out5[0] = N; out5[1] = R2;
    out5[2] = tau[0]; out5[3] = tau[1]; out5[4] = tau[2];
    return CGRT_OK;
}

extern "C" int cgrt_sppm_check_host(int32_t width, int32_t rows, int32_t spp, int32_t photon_depth, const cgrt_photons *ph, int32_t flags,
                                    const cgrt_grid *grid) {
    int code = CGRT_OK;
    if (const char *msg = sppm_create_args(width, rows, spp, photon_depth, ph, flags, &code)) return fail(code, msg);
    if (grid)
        if (const char *msg = sppm_pass_grid_args(width, rows, spp, grid, nullptr)) return fail(CGRT_ERR_INVALID, msg);
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_create(const cgrt_scene *s, int32_t width, int32_t rows, int32_t spp, int32_t photon_depth,
                                        const cgrt_photons *ph, int32_t flags, cgrt_sppm_session **out) {
    if (!out) return fail(CGRT_ERR_INVALID, "null argument");
    *out = nullptr;
    int code = CGRT_OK;
    if (const char *msg = sppm_create_args(width, rows, spp, photon_depth, ph, flags, &code)) return fail(code, msg);
    if (!s) return fail(CGRT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");  // (the last of the checks: it looks at the scene's state)
    ON_DEVICE(s->device);
    std::unique_ptr<cgrt_sppm_session> p(new (std::nothrow) cgrt_sppm_session());
    if (!p) return fail(CGRT_ERR_LIMIT, "out of host memory");
    p->s = s;
    p->geometry_gen = s->geometry_gen;
    p->ph = *ph;
    p->ph.nphotons = 0;
    p->width = width; p->rows = rows; p->spp = spp; p->photon_depth = photon_depth;
    p->npix = (long long)width * rows;
    HIP_TRY(hipEventCreateWithFlags(&p->img_b, hipEventDisableTiming));
    HIP_TRY(p->take(p->px, (size_t)p->npix * kSppmPixelDoubles * sizeof(double)));
    HIP_TRY(p->take(p->npairs, 16));
    const double r0 = ppm_grid(p->ph).r0;
    const int T = 256;
    hipLaunchKernelGGL(sppm_init_kernel, dim3((unsigned)((p->npix + T - 1) / T)), dim3(T), 0, 0, r0 * r0, p->npix, p->px.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    *out = p.release();
    return CGRT_OK;
}

extern "C" void cgrt_sppm_session_destroy(cgrt_sppm_session *p) {
    if (!p) return;
    DeviceGuard g(p->s->device);
    if (g.err == hipSuccess) (void)hipStreamSynchronize(0);
    delete p;  // waits for the last image and the producer stream before freeing
}

static int sppm_count_ok(const cgrt_sppm_session *p, int64_t nphotons) {
    if (nphotons < 0 || nphotons > LLONG_MAX - p->photons_done) return fail(CGRT_ERR_INVALID, "sppm pass: bad photon count");
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_pass_grid(cgrt_sppm_session *p, const cgrt_camera *cam, const cgrt_grid *grid, int64_t nphotons) {
    if (!p) return fail(CGRT_ERR_INVALID, "null session");
    if (p->geometry_gen != p->s->geometry_gen) return fail(CGRT_ERR_INVALID, kRefitStale);  // (image, pixels, get_info go on working)
    int rc = check_grid(p->s, cam, grid);
    if (rc) return rc;
    if (const char *msg = sppm_pass_grid_args(p->width, p->rows, p->spp, grid, p->have_stripe ? &p->stripe : nullptr))
        return fail(CGRT_ERR_INVALID, msg);
    if ((rc = sppm_count_ok(p, nphotons))) return rc;
    ON_DEVICE(p->s->device);
    rc = p->pass(grid_capture(p->s, cam, grid), nullptr, false, nphotons);
    if (rc == CGRT_OK && !p->have_stripe) {
        p->stripe = sppm_stripe(grid);
        p->have_stripe = true;
    }
    return rc;
}

extern "C" int cgrt_sppm_session_pass_rays(cgrt_sppm_session *p, const cgrt_rays *rays, const int64_t *pixel, int64_t nphotons) {
    if (!p) return fail(CGRT_ERR_INVALID, "null session");
    if (p->geometry_gen != p->s->geometry_gen) return fail(CGRT_ERR_INVALID, kRefitStale);
    int rc = check_capture_rays(p->s, rays);
    if (rc) return rc;
    if ((rc = sppm_count_ok(p, nphotons))) return rc;
    ON_DEVICE(p->s->device);
    const cgrt_scene *s = p->s;
    const auto capture = [=](uint64_t cap, double **d_rec, uint64_t *count) { return ray_hitpoints_device(s, rays, pixel, cap, d_rec, count); };
    return p->pass(capture, pixel, true, nphotons);
}

static int sppm_image_args(const cgrt_sppm_session *p, const uint8_t *rgb8) {
    if (!p) return fail(CGRT_ERR_INVALID, "null session");
    if (p->photons_done == 0) return fail(CGRT_ERR_INVALID, "sppm session: no photon yet (the image would be tau / (PI R2 0))");
    if (rgb8 && p->striped())
        return fail(CGRT_ERR_UNSUPPORTED, "sppm session: rgb8 needs contiguous rows; tone-map the assembled frame (cgrt_tonemap_rgb8)");
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_image(const cgrt_sppm_session *cp, double *image, uint8_t *rgb8) {
    int rc = sppm_image_args(cp, rgb8);
    if (rc) return rc;
    cgrt_sppm_session *p = const_cast<cgrt_sppm_session *>(cp);  // the image buffers are scratch, not state
    ON_DEVICE(p->s->device);
    const size_t npix = (size_t)p->npix;
    if (image && !p->img.p) HIP_TRY(p->take(p->img, npix * 3 * sizeof(double)));
    if (rgb8 && !p->rgb8.p) HIP_TRY(p->take(p->rgb8, npix * 3));
    if ((rc = p->image(image ? p->img.as<double>() : nullptr, rgb8 ? p->rgb8.as<unsigned char>() : nullptr, 0))) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    if (image) HIP_TRY(hipMemcpy(image, p->img.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (rgb8) HIP_TRY(hipMemcpy(rgb8, p->rgb8.p, npix * 3, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_image_device(const cgrt_sppm_session *cp, double *image, uint8_t *rgb8, void *stream) {
    int rc = sppm_image_args(cp, rgb8);
    if (rc) return rc;
    cgrt_sppm_session *p = const_cast<cgrt_sppm_session *>(cp);
    ON_DEVICE(p->s->device);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = p->image(image, rgb8, st))) return rc;
    HIP_TRY(hipEventRecord(p->img_b, st));
    p->img_pending = true;  // the next pass waits for it
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_pixels(const cgrt_sppm_session *p, double *px8) {
    if (!p || !px8) return fail(CGRT_ERR_INVALID, "null argument");
    ON_DEVICE(p->s->device);
    HIP_TRY(hipMemcpy(px8, p->px.p, (size_t)p->npix * kSppmPixelDoubles * sizeof(double), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_last_hitpoints(const cgrt_sppm_session *p, double *hp16, uint64_t cap, uint64_t *count) {
    if (!p || !count || (cap > 0 && !hp16)) return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(p->s->device);
    const size_t n = p->tab ? p->tab->n : 0;
    *count = n;
    const size_t m = n < cap ? n : (size_t)cap;
    if (m) HIP_TRY(hipMemcpy(hp16, p->tab->hp.p, m * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_get_info(const cgrt_sppm_session *p, cgrt_sppm_session_info *out) {
    if (!p || !out) return fail(CGRT_ERR_INVALID, "null argument");
    out->passes = p->passes;
    out->photons_done = p->photons_done;
    out->hp_count = p->tab ? p->tab->n : 0;
    out->n_events = p->n_events;
    out->n_pairs = p->n_pairs;
    out->n_batch_halvings = p->n_halvings;
    out->device_bytes = p->bytes();
    out->ms_eye = p->ms_eye;
    out->ms_table = p->ms_table;
    out->ms_photons = p->ms_photons;
    out->ms_update = p->ms_update;
    return CGRT_OK;
}
