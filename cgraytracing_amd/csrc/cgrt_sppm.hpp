// Stochastic progressive photon mapping (Hachisuka & Jensen 2009): cgrt_sppm_session -- statistics that belong to the TEXEL
// (N, R2, tau) and live for the session, Hitpoints that live for one pass -- its kernels and the cgrt_sppm_* entry points.
//
// A pass is the photon pass of cgrt_ppm_session.hpp with another ending.  Its stages up to the sorted pairs are that file's, the
// same code: the Hitpoint capture of a grid or of rays, PpmTable::build, PhotonProducer, photon_pairs_kernel, sort_pairs, the
// batches PpmSchedule decides.  The session's host core (eye capture, pair buffers, producer setup, byte accounting, the image
// paths, the Hitpoint read-back, destroy) is PhotonSession of cgrt_photon_session.hpp, shared with cgrt_ppm_session.
// Every Hitpoint searches with its texel's radius, which does not change while the pass runs, so
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

struct cgrt_sppm_session : PhotonSession {  // (ph.nphotons is not used)
    static constexpr const char *kWho = "sppm session";
    int photon_depth = 0;
    bool have_stripe = false;  // a grid pass has fixed `stripe`
    SppmStripe stripe;
    DevBuf px;                       // [texels()][kSppmPixelDoubles], for the session's life
    std::unique_ptr<PpmTable> tab;   // the last pass's Hitpoints (null before the first pass and after a failed one)
    long long photons_done = 0, passes = 0;
    uint64_t n_halvings = 0;
    double ms_update = 0;

    ~cgrt_sppm_session() { settle(); }
    long long done() const { return photons_done; }
    bool is_striped() const { return have_stripe && stripe.nranks > 1; }
    const PpmTable *hitpoint_table() const { return tab.get(); }
    int64_t bytes() const { return PhotonSession::bytes(tab.get()); }
    template <class Capture> int pass(Capture capture, const int64_t *ray_pixel, bool rays, long long count);
    int photons(PpmTable &t, long long count, uint64_t &events, uint64_t &pairs);
    int gather(double *d_img, unsigned char *d_rgb8, hipStream_t st) const;
};

// Photons [photons_done, photons_done + count) against table t, applied on the null stream batch by batch as a fresh PpmSchedule
// decides: cgrt_ppm_session::photons with the sum in the replay's place, its own photons only and nothing traced ahead when it
// ends.  Nothing of the session's state changes here: the caller commits the pass.
int cgrt_sppm_session::photons(PpmTable &t, long long count, uint64_t &events, uint64_t &pairs) {
    const PpmSetup setup = ppm_setup(ph, t.n, true, photon_overlap_allowed());
    int rc = producer(setup, kWho);
    if (rc == CGRT_OK) rc = pair_buffers(setup.pair_cap);  // they grow with the largest pass's pair_cap
    if (rc) return rc;
    PpmSchedule sched;  // a fresh one per pass: nothing is traced ahead from one pass to the next
    sched.start(setup);
    sched.done = photons_done;
    (void)sched.begin(photons_done + count, false, false);
    const int T = 256;
    const unsigned nb = (unsigned)((t.n + T - 1) / T);
    rc = photon_batches(
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
    int rc = wait_image();  // an image on a caller's stream reads the texels
    if (rc) return rc;
    img_pending = false;  // the null stream is behind it now, and nothing here reads its time
    tab.reset();  // the last pass's Hitpoints go before the new ones come: a session never holds two tables
    std::unique_ptr<PpmTable> t(new (std::nothrow) PpmTable());
    if (!t) return fail(CGRT_ERR_LIMIT, "out of host memory");
    const long long npix = texels();
    {
        DevBuf rec;
        t->npix = npix;
        if ((rc = capture_eye(capture, "sppm pass", rec, t->n))) return rc;
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

int cgrt_sppm_session::gather(double *d_img, unsigned char *d_rgb8, hipStream_t st) const {
    const int T = 256;
    const long long npix = texels();
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
    p->open(s, *ph, width, rows, spp);
    p->ph.nphotons = 0;
    p->photon_depth = photon_depth;
    if (const int rc = p->events_ok(cgrt_sppm_session::kWho)) return rc;
    const long long npix = p->texels();
    HIP_TRY(p->take(p->px, (size_t)npix * kSppmPixelDoubles * sizeof(double)));
    HIP_TRY(p->take(p->npairs, 16));
    const double r0 = ppm_grid(p->ph).r0;
    const int T = 256;
    hipLaunchKernelGGL(sppm_init_kernel, dim3((unsigned)((npix + T - 1) / T)), dim3(T), 0, 0, r0 * r0, npix, p->px.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    *out = p.release();
    return CGRT_OK;
}

extern "C" void cgrt_sppm_session_destroy(cgrt_sppm_session *p) { session_destroy(p); }

static int sppm_count_ok(const cgrt_sppm_session *p, int64_t nphotons) {
    if (nphotons < 0 || nphotons > LLONG_MAX - p->photons_done) return fail(CGRT_ERR_INVALID, "sppm pass: bad photon count");
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_pass_grid(cgrt_sppm_session *p, const cgrt_camera *cam, const cgrt_grid *grid, int64_t nphotons) {
    if (!p) return fail(CGRT_ERR_INVALID, "null session");
    int rc = p->fresh();
    if (rc == CGRT_OK) rc = check_grid(p->s, cam, grid);
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
    int rc = p->fresh();
    if (rc == CGRT_OK) rc = check_capture_rays(p->s, rays);
    if (rc) return rc;
    if ((rc = sppm_count_ok(p, nphotons))) return rc;
    ON_DEVICE(p->s->device);
    const cgrt_scene *s = p->s;
    const auto capture = [=](uint64_t cap, double **d_rec, uint64_t *count) { return ray_hitpoints_device(s, rays, pixel, cap, d_rec, count); };
    return p->pass(capture, pixel, true, nphotons);
}

extern "C" int cgrt_sppm_session_image(const cgrt_sppm_session *p, double *image, uint8_t *rgb8) {
    return session_image(p, image, rgb8, nullptr);
}

extern "C" int cgrt_sppm_session_image_device(const cgrt_sppm_session *p, double *image, uint8_t *rgb8, void *stream) {
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return session_image(p, image, rgb8, &st);
}

extern "C" int cgrt_sppm_session_pixels(const cgrt_sppm_session *p, double *px8) {
    if (!p || !px8) return fail(CGRT_ERR_INVALID, "null argument");
    ON_DEVICE(p->s->device);
    HIP_TRY(hipMemcpy(px8, p->px.p, (size_t)p->texels() * kSppmPixelDoubles * sizeof(double), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

extern "C" int cgrt_sppm_session_last_hitpoints(const cgrt_sppm_session *p, double *hp16, uint64_t cap, uint64_t *count) {
    return session_hitpoints(p, hp16, cap, count);
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
