// What the photon-mapping front ends share on the host: PhotonSession, the core that cgrt_ppm_session
// (cgrt_ppm_session.hpp; also the state of one cgrt_ppm_render call) and cgrt_sppm_session (cgrt_sppm.hpp) derive from, and the
// entry points that are the same for both session kinds (image, image_device, the Hitpoint read-back, destroy).  Each of these
// is written once here: the two-call eye capture, the pair buffers, the producer's one-time setup, the byte accounting, the
// image to the host or into the caller's device buffers with the wait that protects it, and the stale-geometry test.  What a
// session kind does with its photons -- its table's lifetime, its batch loop's apply step, its counters -- stays in its file.
#include <climits>
#include <memory>

namespace {
// Device time between two points of a stream.  One pair of events, made once and recorded again for every measurement.
struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    Timer() { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void start() { (void)hipEventRecord(a, 0); }
    hipError_t read(double *ms) const {  // waits for b
        hipError_t e = hipEventSynchronize(b);
        float f = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&f, a, b);
        if (e == hipSuccess) *ms = (double)f;
        return e;
    }
    double stop() {
        double ms = 0;
        (void)hipEventRecord(b, 0);
        (void)read(&ms);
        return ms;
    }
};
}  // namespace

// The pair buffers of one batch: the search writes (k0, v0), the sort (k1, v1); npairs = {pairs, events} of the batch
struct PairBufs {
    unsigned long long *k0, *k1;
    unsigned int *v0, *v1;
    unsigned long long *npairs;
};

struct PhotonSession {
    const cgrt_scene *s = nullptr;
    cgrt_photons ph{};
    int width = 0, rows = 0, spp = 1;  // the image the session gathers into and the gather's normaliser
    uint64_t geometry_gen = 0;  // the scene's refit count at creation: Hitpoints and texel statistics are those of that geometry
    int64_t dev_bytes = 0;       // what take() allocated
    int64_t producer_bytes = 0;  // the producer's event buffers, once it is set up
    GrowBuf pk0, pk1, pv0, pv1;  // (hitpoint, event) pairs of one batch; they grow with the largest pair_cap asked for
    DevBuf npairs, img, rgb8;    // img, rgb8: device scratch of image_host
    PairBufs pb{};               // over the five above, as pair_buffers() left them
    GrowBuf main_tmp;
    PhotonProducer pp;  // declared last of the buffers: its destructor waits for its stream before they are freed
    bool pp_ready = false, pp_broken = false;
    uint64_t n_events = 0, n_pairs = 0;
    double ms_eye = 0, ms_table = 0, ms_photons = 0;
    Timer tm;      // the stages, on the null stream
    Timer img_tm;  // brackets the last image, on the stream it ran on
    mutable double ms_last_image = 0;
    mutable bool img_pending = false;  // img_tm.b recorded, ms_last_image not yet read from it

    void open(const cgrt_scene *s_, const cgrt_photons &ph_, int width_, int rows_, int spp_) {
        s = s_; ph = ph_; width = width_; rows = rows_; spp = spp_; geometry_gen = s->geometry_gen;
    }
    long long texels() const { return (long long)rows * width; }
    int events_ok(const char *who) const {
        if (tm.a && tm.b && img_tm.a && img_tm.b) return CGRT_OK;
        return fail(CGRT_ERR_DEVICE, std::string(who) + ": hipEventCreate failed");
    }
    // photon work refuses a scene refitted since the session was made (image, hitpoints, pixels and get_info go on working)
    int fresh() const { return geometry_gen != s->geometry_gen ? fail(CGRT_ERR_INVALID, kRefitStale) : CGRT_OK; }
    hipError_t take(DevBuf &b, size_t bytes) {
        dev_bytes += (int64_t)bytes;
        return b.alloc(bytes);
    }
    // with the session's table, if it holds one
    int64_t bytes(const PpmTable *t) const {
        return dev_bytes + (t ? t->dev_bytes : 0) + producer_bytes + (int64_t)(pk0.cap + pk1.cap + pv0.cap + pv1.cap) +
               (int64_t)main_tmp.cap + (int64_t)pp.tmp.cap;
    }
    // a derived session's destructor calls it before its own buffers go: the last image and the producer's stream may read them
    void settle() {
        if (img_tm.b) (void)hipEventSynchronize(img_tm.b);
        if (pp.st) (void)hipStreamSynchronize(pp.st);
    }

    // ---- eye pass: Hitpoint records, device resident (count first, then capture).  capture(cap, &d_rec, &count) is
    // hitpoints_device over a grid or ray_hitpoints_device over a ray buffer.  rec, n: the records; ms_eye: its time ----
    template <class Capture> int capture_eye(Capture capture, const char *who, DevBuf &rec, size_t &n) {
        tm.start();
        uint64_t nhp = 0;
        int rc = capture(0, nullptr, &nhp);
        if (rc) return rc;
        if (nhp >= (1ull << 31)) return fail(CGRT_ERR_LIMIT, std::string(who) + ": more than 2^31 hitpoints");
        n = (size_t)nhp;
        if (n) {
            double *d_rec = nullptr;
            rc = capture(nhp, &d_rec, &nhp);
            rec.p = d_rec;
            if (rc) return rc;
        }
        ms_eye = tm.stop();
        return CGRT_OK;
    }

    // ---- photon buffers.  The producer is set up by the first setup that traces anything (the event buffers' size is
    // ph.batch's); a failed setup is remembered and reported by every later call ----
    int producer(const PpmSetup &setup, const char *who) {
        if (pp_broken) return fail(CGRT_ERR_DEVICE, std::string(who) + ": the photon producer could not be set up");
        if (pp_ready || !setup.nbuf) return CGRT_OK;
        if (const int rc = pp.init(setup.nbuf, (size_t)setup.batch * kSegStride, setup.overlap)) {
            pp_broken = true;
            return rc;
        }
        pp_ready = true;
        producer_bytes = setup.producer_bytes;
        return CGRT_OK;
    }
    // pb over room for pair_cap pairs: a session of one table asks once, one with a table per pass asks per pass
    int pair_buffers(unsigned long long pair_cap) {
        HIP_TRY(pk0.need((size_t)pair_cap * 8)); HIP_TRY(pk1.need((size_t)pair_cap * 8));
        HIP_TRY(pv0.need((size_t)pair_cap * 4)); HIP_TRY(pv1.need((size_t)pair_cap * 4));
        if (!npairs.p) HIP_TRY(take(npairs, 16));
        pb = PairBufs{static_cast<unsigned long long *>(pk0.p), static_cast<unsigned long long *>(pk1.p), static_cast<unsigned int *>(pv0.p),
                      static_cast<unsigned int *>(pv1.p), npairs.as<unsigned long long>()};
        return CGRT_OK;
    }

    // ---- the image.  launch(d_image, d_rgb8, stream) enqueues the session's gather at `done` photons; either may be null ----
    // before null-stream work that writes what an image on a caller's stream may still be reading (Hitpoints, texels).  The flag
    // stays for image_time; a session that reports no image time clears it itself
    int wait_image() {
        if (img_pending) HIP_TRY(hipStreamWaitEvent(0, img_tm.b, 0));
        return CGRT_OK;
    }
    // ms_last_image of a bracket not read yet (waits for it)
    int image_time() const {
        if (img_pending) {
            HIP_TRY(img_tm.read(&ms_last_image));
            img_pending = false;
        }
        return CGRT_OK;
    }
    // into the caller's device buffers on stream st; returns when it is enqueued.  The session has one bracket: an image still
    // pending on another stream is put in front of this one, so that whoever waits for img_tm.b waits for both
    template <class Launch> int image_device(Launch launch, double *d_image, unsigned char *d_rgb8, hipStream_t st) {
        if (img_pending) HIP_TRY(hipStreamWaitEvent(st, img_tm.b, 0));
        HIP_TRY(hipEventRecord(img_tm.a, st));
        if (const int rc = launch(d_image, d_rgb8, st)) return rc;
        HIP_TRY(hipEventRecord(img_tm.b, st));
        img_pending = true;  // the next photon work waits for it; image_time reads its time
        return CGRT_OK;
    }
    // into host arrays, through device scratch the session keeps
    template <class Launch> int image_host(Launch launch, double *h_image, uint8_t *h_rgb8) {
        const size_t npix = (size_t)texels();
        if (h_image && !img.p) HIP_TRY(take(img, npix * 3 * sizeof(double)));
        if (h_rgb8 && !rgb8.p) HIP_TRY(take(rgb8, npix * 3));
        int rc = image_device(launch, h_image ? img.as<double>() : nullptr, h_rgb8 ? rgb8.as<unsigned char>() : nullptr, 0);
        if (rc == CGRT_OK) rc = image_time();
        if (rc) return rc;
        if (h_image) HIP_TRY(hipMemcpy(h_image, img.p, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
        if (h_rgb8) HIP_TRY(hipMemcpy(h_rgb8, rgb8.p, npix * 3, hipMemcpyDeviceToHost));
        return CGRT_OK;
    }
};

// The first `cap` Hitpoints of table t (null: none) to the host as hp16; *count: all of them
static int hitpoints_to_host(const PpmTable *t, double *hp16, uint64_t cap, uint64_t *count) {
    const size_t n = t ? t->n : 0;
    *count = n;
    const size_t m = n < cap ? n : (size_t)cap;
    if (m) HIP_TRY(hipMemcpy(hp16, t->hp.p, m * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

// ---- the entry points that are one for both session kinds.  S: kWho, done(), is_striped(), gather(), hitpoint_table() ----
// st null: to host arrays; else into the caller's device buffers on *st
template <class S> static int session_image(const S *cp, double *image, uint8_t *rgb8, const hipStream_t *st) {
    if (!cp) return fail(CGRT_ERR_INVALID, "null session");
    S *p = const_cast<S *>(cp);  // the image scratch and its events are not the session's state
    if (p->done() == 0) return fail(CGRT_ERR_INVALID, std::string(S::kWho) + ": no photon yet (the image divides by the photon count)");
    if (rgb8 && p->is_striped())
        return fail(CGRT_ERR_UNSUPPORTED, std::string(S::kWho) + ": rgb8 needs contiguous rows; tone-map the assembled frame (cgrt_tonemap_rgb8)");
    ON_DEVICE(p->s->device);
    const auto launch = [p](double *d_image, unsigned char *d_rgb8, hipStream_t on) { return p->gather(d_image, d_rgb8, on); };
    return st ? p->image_device(launch, image, rgb8, *st) : p->image_host(launch, image, rgb8);
}

template <class S> static int session_hitpoints(const S *p, double *hp16, uint64_t cap, uint64_t *count) {
    if (!p || !count || (cap > 0 && !hp16)) return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(p->s->device);
    return hitpoints_to_host(p->hitpoint_table(), hp16, cap, count);
}

template <class S> static void session_destroy(S *p) {
    if (!p) return;
    DeviceGuard g(p->s->device);
    if (g.err == hipSuccess) (void)hipStreamSynchronize(0);
    delete p;  // settle() waits for the last image and the producer stream before anything is freed
}
