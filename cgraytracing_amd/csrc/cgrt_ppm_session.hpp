// Photon pass: cgrt_ppm_session -- the state of a photon-mapping run -- its stages (eye, table,
// photons in batches as PpmSchedule of cgrt_ppm_plan.h decides, gather) and the cgrt_ppm_* entry points.  What it shares with
// cgrt_sppm_session (cgrt_sppm.hpp) -- the eye capture, the pair buffers, the producer's setup, the byte accounting, the image
// to the host or the device, the Hitpoint read-back, destroy, the stage timer -- is PhotonSession of cgrt_photon_session.hpp.
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

// ---- the batch loop of every photon stage (cgrt_ppm_session::photons; a pass of cgrt_sppm_session) ---------------------------
// The photons of the call `sched` has begun, against table `tab`, applied on the null stream batch by batch as `sched` decides.
// produce(batch) enqueues a batch on the producer.  apply(np, buf) launches what consumes an applied batch: its np pairs sorted
// by (hitpoint, slot) in (pb.k1, pb.v1) and the events of buffer buf.  n_events, n_pairs: added to for every applied batch.
template <class Produce, class Apply>
static int photon_batches(PpmSchedule &sched, PhotonProducer &pp, PpmTable &tab, const PairBufs &pb, GrowBuf &tmp, uint64_t &n_events,
                          uint64_t &n_pairs, Produce produce, Apply apply) {
    const int T = 256;
    int rc = CGRT_OK;
    while (sched.more()) {
        const PpmBatch b = sched.next();
        const int nslots = b.count * kSegStride, cur = b.buf;
        if (!b.reuse && (rc = produce(b))) return rc;
        // the NEXT batch now, so that it is traced under this batch's search, sort and replay
        const PpmBatch nx = sched.following(b);
        if (nx.count) {
            if ((rc = produce(nx))) return rc;
            sched.set_ahead(nx);
        }
        if (pp.st) HIP_TRY(hipStreamWaitEvent(0, pp.produced[cur], 0));
        HIP_TRY(hipMemsetAsync(pb.npairs, 0, 16, 0));
        hipLaunchKernelGGL(photon_pairs_kernel, dim3((nslots + T - 1) / T), dim3(T), 0, 0, pp.ev[cur].as<double>(),
                           pp.ek1[cur].as<unsigned int>(), pp.eo1[cur].as<unsigned int>(), nslots, tab.ha, tab.hps.as<double>(),
                           tab.bstart.as<int>(), pb.k0, pb.v0, pb.npairs, sched.setup.pair_cap);
        HIP_TRY(hipGetLastError());
        unsigned long long np2[2] = {0, 0};  // pairs (the full 64-bit count, stored or not), events
        HIP_TRY(hipMemcpy(np2, pb.npairs, 16, hipMemcpyDeviceToHost));
        const PpmOutcome o = sched.counted(b, np2[0]);
        if (o != kPpmApplied) {  // nothing has been applied yet
            if ((rc = pp.release(cur))) return rc;
            if (o == kPpmLimit) return fail(CGRT_ERR_LIMIT, "photon pass: one photon's pairs exceed the pair buffer");
            continue;
        }
        const unsigned int np = (unsigned int)np2[0];  // <= pair_cap <= 2^27
        n_events += np2[1];
        if (np != 0) {
            n_pairs += np;
            if ((rc = sort_pairs(tmp, pb.k0, pb.k1, pb.v0, pb.v1, np, sched.setup.pair_key_bits))) return rc;
            if ((rc = apply(np, cur))) return rc;
        }
        if ((rc = pp.release(cur))) return rc;
    }
    return CGRT_OK;
}

// ---- the stages of render() main.cpp:169-258, shared by cgrt_ppm_render (one call) and a live cgrt_ppm_session ----------
// eye(): the Hitpoint records of a grid or of a ray buffer; table(): the reference's table order and the per-pixel index over
// them (PpmTable).  photon_setup() + photons(last): photons [done, last) in batches.  gather(): the image at the current
// photon count.  Photon i always draws from the keyed stream
// (seed, i) and a hitpoint replays its events in photon order, so the state after photons [0, a) then [a, b) is the state
// after [0, b): how the photons are split into calls and batches never shows in the result.
struct cgrt_ppm_session : PhotonSession {
    static constexpr const char *kWho = "photon session";
    // width, rows, spp and the photons' depth limit: a grid session's grid.width, .rows, .spp, .max_depth; a ray session's
    // cgrt_ray_pixels and rays->max_depth; a hitpoint session's cgrt_hitpoints fields
    int max_depth = 0;
    bool striped = false;  // grid session over block-cyclic rows: no rgb8
    bool lookahead = false;  // session: trace the next batch on the producer stream when a call ends
    PpmTable tab;            // the hitpoints in table order and the per-pixel index
    PpmSchedule sched;  // the setup, which photons are applied (sched.done), the batch size, the batch traced ahead
    double ms_last_add = 0;

    ~cgrt_ppm_session() { settle(); }
    long long done() const { return sched.done; }
    bool is_striped() const { return striped; }
    const PpmTable *hitpoint_table() const { return &tab; }
    int64_t bytes() const { return PhotonSession::bytes(&tab); }
    void frame(const cgrt_scene *s_, const cgrt_photons *ph_, int width_, int rows_, int spp_, int max_depth_, bool striped_) {
        open(s_, *ph_, width_, rows_, spp_);
        max_depth = max_depth_;
        striped = striped_;
        tab.npix = texels();
    }
    // eye pass (capture: see PhotonSession::capture_eye); frame() has been called
    template <class Capture> int eye(Capture capture, DevBuf &rec) { return capture_eye(capture, "photon pass", rec, tab.n); }
    int table(DevBuf &rec, const int64_t *ray_pixel, bool rays);
    int table(const cgrt_hitpoints &in);
    int photon_setup(bool session);
    int photons(long long last, bool keep_ahead, const cgrt_photon_rays *pr = nullptr);
    int gather(double *d_img, unsigned char *d_rgb8, hipStream_t st) const;
};

static auto grid_capture(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid) {
    return [=](uint64_t cap, double **d_rec, uint64_t *count) { return hitpoints_device(s, cam, grid, cap, d_rec, count); };
}

int cgrt_ppm_session::table(DevBuf &rec, const int64_t *ray_pixel, bool rays) {
    tm.start();
    if (const int rc = tab.build(rec, ph, spp, ray_pixel, rays, main_tmp)) return rc;
    ms_table = tm.stop();
    return CGRT_OK;
}

// The table of a session whose Hitpoints are the caller's records: there is no eye stage (ms_eye stays 0); frame() has been called
int cgrt_ppm_session::table(const cgrt_hitpoints &in) {
    tm.start();
    if (const int rc = tab.build(in, ph, main_tmp)) return rc;
    ms_table = tm.stop();
    return CGRT_OK;
}

// Batch size, pair buffers and the producer (ppm_setup decides)
int cgrt_ppm_session::photon_setup(bool session) {
    sched.start(ppm_setup(ph, tab.n, session, photon_overlap_allowed()));
    if (const int rc = producer(sched.setup, "photon pass")) return rc;
    return pair_buffers(sched.setup.pair_cap);
}

// Photons [done, last), applied on the null stream, batch by batch as `sched` decides.  keep_ahead: when the range is done,
// the next batch from `done` is enqueued on the producer stream for the next call; otherwise nothing is traced beyond `last`
// and the producer stream is drained.
// pr: the photons [done, last) are the caller's (pr->n = last - done; DEVICE arrays) instead of the built-in emitter's.  Inside the
// call batch k+1 is traced under batch k's replay as ever; a batch traced ahead by an earlier add_photons is not pr's and is
// dropped, and the caller passes keep_ahead = false: the photons after `last` are not known, and the drain is what makes pr's
// arrays read before the call returns.
int cgrt_ppm_session::photons(long long last, bool keep_ahead, const cgrt_photon_rays *pr) {
    if (!sched.begin(last, pr != nullptr, tab.n == 0)) return CGRT_OK;  // no hitpoint can change: nothing to trace
    const long long call_first = sched.done;
    // enqueue batch b on the producer; from: the caller's arrays, read at photon b.first of this call, or null: the emitter
    auto produce = [&](const PpmBatch &b, const cgrt_photon_rays *from) {
        const PhotonArgs pa = photon_args(ph, b.first, b.count, max_depth);
        if (!from) return pp.produce(s, pa, tab.ha, b.buf);
        const size_t k = (size_t)(b.first - call_first);
        PhotonRayArgs ra;
        ra.org = from->org3 + 3 * k;
        ra.dir = from->dir3 + 3 * k;
        ra.flux = from->flux3 + 3 * k;
        ra.keys = from->keys ? reinterpret_cast<const unsigned long long *>(from->keys) + k : nullptr;
        ra.draws = from->draws ? from->draws + k : nullptr;
        return pp.produce(s, pa, tab.ha, b.buf, &ra);
    };
    const int T = 256;
    const unsigned nb = (unsigned)((tab.n + T - 1) / T);
    int rc = photon_batches(
        sched, pp, tab, pb, main_tmp, n_events, n_pairs, [&](const PpmBatch &b) { return produce(b, pr); },
        [&](unsigned int np, int cur) -> int {  // 4. the ordered replay
            hipLaunchKernelGGL(photon_apply_kernel, dim3(nb), dim3(T), 0, 0, pb.k1, pb.v1, np, pp.ev[cur].as<double>(), ph.alpha,
                               tab.hp.as<double>(), tab.hps.as<double>(), (long long)tab.n);
            HIP_TRY(hipGetLastError());
            return CGRT_OK;
        });
    if (rc) return rc;
    bool drain = false;
    const PpmBatch ahead = sched.end(keep_ahead, &drain);  // the lookahead is the built-in emitter's, whoever's the call's photons were
    if (ahead.count) {
        if ((rc = produce(ahead, nullptr))) return rc;
        sched.set_ahead(ahead);
    }
    if (drain && pp.st) HIP_TRY(hipStreamSynchronize(pp.st));
    return CGRT_OK;
}

// The image at `done` photons into device buffers (either may be null), enqueued on `st`.
int cgrt_ppm_session::gather(double *d_img, unsigned char *d_rgb8, hipStream_t st) const {
    const int T = 256;
    hipLaunchKernelGGL(ppm_gather_kernel, dim3((unsigned)((tab.npix + T - 1) / T)), dim3(T), 0, st,
                       static_cast<const unsigned int *>(tab.pix_start.p), static_cast<const unsigned int *>(tab.order.p),
                       static_cast<const double *>(tab.hp.p), (double)sched.done * spp, tab.npix, width, rows, d_img, d_rgb8);
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
    run.frame(s, ph, grid->width, grid->rows, grid->spp, grid->max_depth, grid->stripe_nranks > 1);
    if ((rc = run.events_ok("photon pass"))) return rc;
    {
        DevBuf rec;
        rc = run.eye(grid_capture(s, cam, grid), rec);
        out->ms_eye = run.ms_eye;
        if (rc == CGRT_OK) rc = run.table(rec, nullptr, false);
        out->ms_table = run.ms_table;
        if (rc) return rc;
    }
    // ---- photons, in batches ----
    run.tm.start();
    rc = run.photon_setup(false);
    if (rc == CGRT_OK) rc = run.photons(ph->nphotons, false);
    out->n_events = run.n_events;
    out->n_pairs = run.n_pairs;
    out->n_batch_halvings = run.sched.n_halvings;
    if (rc) return rc;
    out->ms_photons = run.tm.stop();
    // ---- final gather + tone map, then the Hitpoints ----
    const auto gather = [&run](double *d_img, unsigned char *d_rgb8, hipStream_t st) { return run.gather(d_img, d_rgb8, st); };
    run.tm.start();  // ms_gather: from before the scratch is allocated to behind the gather
    if ((rc = run.image_host(gather, out->image, out->rgb8))) return rc;
    float ms_gather = 0;
    HIP_TRY(hipEventElapsedTime(&ms_gather, run.tm.a, run.img_tm.b));
    out->ms_gather = ms_gather;
    return hitpoints_to_host(&run.tab, out->hp16, out->hp16 ? out->hp_cap : 0, &out->hp_count);
}

// ---- resumable photon mapping: the state above, kept between calls -------------------------------------------------
// What the creators do behind their argument checks: the session and its events, the eye pass (capture: see eye()), the table
// (ray_pixel, rays: see PpmTable::build) -- or, with hps, no eye pass and the table of the caller's records --, the photon
// buffers and ph->nphotons photons.
template <class Capture>
static int session_create(const cgrt_scene *s, const cgrt_photons *ph, int flags, int width, int rows, int spp, int max_depth,
                          bool striped, Capture capture, const int64_t *ray_pixel, bool rays, cgrt_ppm_session **out,
                          const cgrt_hitpoints *hps = nullptr) {
    ON_DEVICE(s->device);
    std::unique_ptr<cgrt_ppm_session> p(new (std::nothrow) cgrt_ppm_session());
    if (!p) return fail(CGRT_ERR_LIMIT, "out of host memory");
    p->lookahead = !(flags & CGRT_PPM_SESSION_NO_LOOKAHEAD);
    p->frame(s, ph, width, rows, spp, max_depth, striped);
    int rc = p->events_ok(cgrt_ppm_session::kWho);
    if (rc) return rc;
    if (hps) {
        if ((rc = p->table(*hps))) return rc;
        HIP_TRY(hipDeviceSynchronize());  // the records are read before the call returns
    } else {
        DevBuf rec;
        if ((rc = p->eye(capture, rec))) return rc;
        if ((rc = p->table(rec, ray_pixel, rays))) return rc;
        if (rays) HIP_TRY(hipDeviceSynchronize());  // ray_pixel and the records are read before the call returns
    }
    p->tm.start();
    rc = p->photon_setup(true);
    if (rc == CGRT_OK) rc = p->photons(p->ph.nphotons, p->lookahead);
    p->ms_last_add = p->tm.stop();
    p->ms_photons = p->ms_last_add;
    if (rc) return rc;
    *out = p.release();
    return CGRT_OK;
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
    return session_create(s, ph, flags, grid->width, grid->rows, grid->spp, grid->max_depth, grid->stripe_nranks > 1,
                          grid_capture(s, cam, grid), nullptr, false, out);
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
    const auto capture = [=](uint64_t cap, double **d_rec, uint64_t *count) {
        return ray_hitpoints_device(s, rays, px->pixel, cap, d_rec, count);
    };
    return session_create(s, ph, flags, px->width, px->rows, px->spp, rays->max_depth, false, capture, px->pixel, true, out);
}

extern "C" int cgrt_ppm_session_create_hitpoints(const cgrt_scene *s, const cgrt_hitpoints *hps, const cgrt_photons *ph, int flags,
                                                 cgrt_ppm_session **out) {
    if (!out) return fail(CGRT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!s || !hps || !ph) return fail(CGRT_ERR_INVALID, "null argument");
    if (hps->n < 0) return fail(CGRT_ERR_INVALID, "hitpoints: negative record count");
    if (hps->n > 0 && !hps->hp9) return fail(CGRT_ERR_INVALID, "hitpoints: null hp9");
    if (hps->width <= 0 || hps->rows <= 0 || hps->spp <= 0) return fail(CGRT_ERR_INVALID, "hitpoints: width, rows and spp must be positive");
    if (hps->max_depth < 1 || hps->max_depth > kMaxDepth) return fail(CGRT_ERR_INVALID, "hitpoints: max_depth must be 1..5");
    int rc = check_photons(ph);
    if (rc) return rc;
    if (flags & ~CGRT_PPM_SESSION_NO_LOOKAHEAD) return fail(CGRT_ERR_INVALID, "unknown session flags");
    if ((long long)hps->width * hps->rows >= (1ll << 31)) return fail(CGRT_ERR_LIMIT, "hitpoints: 2^31 texels or more");
    if (hps->n >= (1ll << 31)) return fail(CGRT_ERR_LIMIT, "hitpoints: 2^31 records or more");
    // (the last of the checks: it is the one that looks at the scene's state) whatever n is: the session traces photons through it
    if (!s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    const auto no_eye = [](uint64_t, double **, uint64_t *) { return CGRT_OK; };
    return session_create(s, ph, flags, hps->width, hps->rows, hps->spp, hps->max_depth, false, no_eye, nullptr, false, out, hps);
}

extern "C" void cgrt_ppm_session_destroy(cgrt_ppm_session *p) { session_destroy(p); }

// `count` more photons: the built-in emitter's, or (pr) the caller's
static int session_add(cgrt_ppm_session *p, long long count, const cgrt_photon_rays *pr) {
    int rc = p->fresh();
    if (rc) return rc;
    ON_DEVICE(p->s->device);
    if ((rc = p->wait_image())) return rc;  // a gather on a caller's stream reads hp
    // the producer stream does not wait for the null stream: arrays a kernel on the null stream still writes must be complete
    if (pr && p->pp.st) HIP_TRY(hipStreamSynchronize(0));
    p->tm.start();
    rc = p->photons(p->sched.done + count, pr ? false : p->lookahead, pr);
    if (pr) {  // also when a batch failed: nothing traced ahead from pr's arrays outlives the call
        p->sched.drop_ahead();
        if (p->pp.st) {
            const hipError_t e = hipStreamSynchronize(p->pp.st);
            if (e != hipSuccess && rc == CGRT_OK) return fail(CGRT_ERR_DEVICE, std::string("producer stream: ") + hipGetErrorString(e));
        }
    }
    p->ms_last_add = p->tm.stop();  // also when a batch failed: what was applied before it has finished
    p->ms_photons += p->ms_last_add;
    return rc;
}

extern "C" int cgrt_ppm_session_add_photons(cgrt_ppm_session *p, int64_t count) {
    if (!p || count < 0 || count > LLONG_MAX - p->sched.done) return fail(CGRT_ERR_INVALID, "bad argument");
    return session_add(p, count, nullptr);
}

extern "C" int cgrt_ppm_session_add_photon_rays(cgrt_ppm_session *p, const cgrt_photon_rays *pr) {
    if (const int rc = check_photon_rays(pr)) return rc;
    if (!p || pr->n > LLONG_MAX - p->sched.done) return fail(CGRT_ERR_INVALID, "bad argument");
    if (pr->n == 0) return CGRT_OK;
    return session_add(p, pr->n, pr);
}

extern "C" int cgrt_ppm_session_image(const cgrt_ppm_session *p, double *image, uint8_t *rgb8) {
    return session_image(p, image, rgb8, nullptr);
}

extern "C" int cgrt_ppm_session_image_device(const cgrt_ppm_session *p, double *image, uint8_t *rgb8, void *stream) {
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return session_image(p, image, rgb8, &st);
}

extern "C" int cgrt_ppm_session_hitpoints(const cgrt_ppm_session *p, double *hp16, uint64_t cap, uint64_t *count) {
    return session_hitpoints(p, hp16, cap, count);
}

extern "C" int cgrt_ppm_session_get_info(const cgrt_ppm_session *p, cgrt_ppm_session_info *out) {
    if (!p || !out) return fail(CGRT_ERR_INVALID, "null argument");
    if (p->img_pending) {  // the time of an image on a caller's stream is read when it is asked for
        ON_DEVICE(p->s->device);
        if (const int rc = p->image_time()) return rc;
    }
    out->photons_done = p->sched.done;
    out->hp_count = p->tab.n;
    out->n_events = p->n_events;
    out->n_pairs = p->n_pairs;
    out->n_batch_halvings = p->sched.n_halvings;
    out->device_bytes = p->bytes();
    out->ms_eye = p->ms_eye;
    out->ms_table = p->ms_table;
    out->ms_photons = p->ms_photons;
    out->ms_last_add = p->ms_last_add;
    out->ms_last_image = p->ms_last_image;
    return CGRT_OK;
}
