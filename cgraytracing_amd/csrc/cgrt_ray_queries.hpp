// Caller-supplied rays: the ray-list kernels' dispatch table (cgrt_variants.h), their one launch path over rays_plan
// (cgrt_rays_plan.h), the argument checks and the C entry points -- full trace and nearest-hit query, Hitpoint capture, occlusion,
// bounce, wavefront trace, camera rays, hit attributes.  Part of libcgrt.so; included by cgrt_hip.hip, which has the handle, the checked launch and the
// host staging.

// The table's rows: a variant's trace_rays_kernel and, where the variant has one, its capture, occlusion, bounce and wavefront forms
using RaysKernel = void (*)(DeviceScene, RayParams, unsigned long long *);
using CaptureKernel = void (*)(DeviceScene, RayParams, RaySink);
using OcclusionKernel = void (*)(DeviceScene, OccParams, unsigned long long *);
using BounceKernel = void (*)(DeviceScene, BounceParams, unsigned long long *);
using WavefrontKernel = void (*)(DeviceScene, WavefrontParams, unsigned long long *);
struct RayKernels {
    int id;  // RayFlags::id()
    RaysKernel trace;
    CaptureKernel capture;      // nullptr unless has_capture
    OcclusionKernel occlusion;  // nullptr unless has_occlusion
    BounceKernel bounce;        // nullptr unless has_bounce
    WavefrontKernel wavefront;  // nullptr unless has_bounce
};
template <bool T, bool B, bool G, bool P, bool S, bool SP, bool F, int NT>
static constexpr RayKernels ray_kernels_row() {
    constexpr RayFlags f{T, B, G, P, S, SP, F, NT};
    RayKernels r{f.id(), &trace_rays_kernel<T, B, G, P, S, SP, F, NT>, nullptr, nullptr, nullptr, nullptr};
    if constexpr (has_capture(f)) r.capture = &capture_rays_kernel<T, B, G, P, SP, NT>;
    if constexpr (has_occlusion(f)) r.occlusion = &occlusion_rays_kernel<T, B, P, S, SP, NT>;
    if constexpr (has_bounce(f)) r.bounce = &bounce_rays_kernel<T, B, P, S, SP, NT>;
    if constexpr (has_bounce(f)) r.wavefront = &wavefront_step_kernel<T, B, P, S, SP, NT>;
    return r;
}
#define CGRT_X(T, B, G, P, S, SP, F, NT) ray_kernels_row<T != 0, B != 0, G != 0, P != 0, S != 0, SP != 0, F != 0, NT>(),
static const RayKernels kRayKernels[] = {CGRT_RAY_VARIANTS(CGRT_X)};
#undef CGRT_X

// One launch of a ray-list kernel: the plan, the scene as the kernel sees it and the table's row
struct RaysLaunch {
    RaysPlan plan;
    DeviceScene dev;  // the general variant's copy holds its resident objects
    const RayKernels *row;
};
static RaysPlan rays_plan_for(const cgrt_scene *s, const cgrt_rays *rays, RaysKind kind) {
    const bool general = rays_general(s->dev);
    const RayKernels *g = general ? variant_row(kRayKernels, rays_general_flags(rays_first(kind))) : nullptr;
    const RaysDevice dev{s->n_cu, general ? device_lds_bytes(s->device) : kLdsBytes,
                         g ? kernel_static_lds(reinterpret_cast<const void *>(g->trace)) : kStaticLdsAllowance};
    return rays_plan(s->dev, RaysAsk{rays->max_depth, (rays->flags & CGRT_RAYS_STATS) != 0, kind, rays->n}, dev);
}
// ... refused where no kernel of `kind` was built for the plan's variant
static int rays_launch(const cgrt_scene *s, const cgrt_rays *rays, RaysKind kind, RaysLaunch &L) {
    static const char *const form[] = {"", "", "capture ", "occlusion ", "bounce ", "wavefront "};
    L.plan = rays_plan_for(s, rays, kind);
    L.dev = with_resident(s->dev, L.plan.resident);
    L.row = variant_row(kRayKernels, L.plan.k);
    if (!L.row || (kind == RaysKind::Capture && !L.row->capture) || (kind == RaysKind::Occlusion && !L.row->occlusion) ||
        (kind == RaysKind::Bounce && !L.row->bounce) || (kind == RaysKind::Wavefront && !L.row->wavefront))
        return fail(CGRT_ERR_UNSUPPORTED, std::string(L.plan.what()) + ": no " + form[(int)kind] + "kernel built for this variant");
    return CGRT_OK;
}
// The queue's head lives in the handle's launch scratch (launches on one handle are ordered by the caller), `tail` bytes of
// the caller's own behind it at +256: made sure of and reset
static int ray_queue(const cgrt_scene *s, size_t tail, hipStream_t st, unsigned int **queue) {
    if (s->scratch.need(256 + tail) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CGRT_ERR_DEVICE, "cannot allocate launch scratch (ray queue)");
    }
    HIP_TRY(hipMemsetAsync(s->scratch.p, 0, sizeof(unsigned int), st));
    *queue = reinterpret_cast<unsigned int *>(s->scratch.p);
    return CGRT_OK;
}
static void fill_ray_inputs(RayInput &in, const cgrt_rays *r) {
    in.n = r->n;
    in.org = r->org3;
    in.dir = r->dir3;
    in.keys = reinterpret_cast<const unsigned long long *>(r->keys);
    in.first_index = r->first_index;
    in.seed = r->seed;
}
template <class... P>
static int launch_rays(const cgrt_scene *s, const RaysLaunch &L, void (*fn)(DeviceScene, P...), hipStream_t st, typename same_type<P>::type... args) {
    return launch_checked(fn, L.plan.what(), s->device, dim3((unsigned)L.plan.wgs), dim3((unsigned)L.plan.k.nt), L.plan.lds, st, L.dev, args...);
}

// A ray list and the scene it meets.  own_ok: the entry point's other pointers; own_null: what to say of an output it cannot
// do without.  traced: the rays are traced, so max_depth counts (where `depth`) and the scene must be committed, both looked at
// before the count's limit; else the rays are only looked up, and with none of them nothing of the scene is looked at.
static int check_ray_list(const cgrt_scene *s, const cgrt_rays *r, bool own_ok, const char *own_null, bool traced, bool depth) {
    if (!s || !r || !own_ok) return fail(CGRT_ERR_INVALID, "null argument");
    if (r->n < 0) return fail(CGRT_ERR_INVALID, "negative ray count");
    if (r->n > 0 && (!r->org3 || !r->dir3)) return fail(CGRT_ERR_INVALID, "null org3 / dir3");
    if (own_null) return fail(CGRT_ERR_INVALID, own_null);
    if (traced && depth && (r->max_depth < 1 || r->max_depth > kMaxDepth)) return fail(CGRT_ERR_INVALID, "max_depth must be 1..5");
    if (traced && !s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    if (r->n > kMaxRays) return fail(CGRT_ERR_LIMIT, "more than 2^36 rays in one call");
    if (r->n > 0 && !s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    return CGRT_OK;
}
// a nearest-hit query (neither acc3 nor nhit asked for) does not read max_depth
static int check_rays(const cgrt_scene *s, const cgrt_rays *r, const cgrt_ray_results *out) {
    return check_ray_list(s, r, out != nullptr, nullptr, true, out && (out->acc3 || out->nhit));
}
// What the Hitpoint capture reads of a ray set: every ray is traced in full, so max_depth always counts
static int check_capture_rays(const cgrt_scene *s, const cgrt_rays *r) { return check_ray_list(s, r, true, nullptr, true, true); }
static int check_occlusion(const cgrt_scene *s, const cgrt_rays *r, const cgrt_occlusion *occ) {
    return check_ray_list(s, r, occ != nullptr, occ && !occ->occluded ? "null occluded" : nullptr, false, false);
}
static int check_bounce(const cgrt_scene *s, const cgrt_rays *r, const cgrt_bounce *b) {
    return check_ray_list(s, r, b != nullptr, nullptr, false, false);
}
static int check_wavefront(const cgrt_scene *s, const cgrt_rays *r, const cgrt_wavefront *wf) {
    const char *own = nullptr;
    if (wf) {
        if (wf->max_depth < 1 || wf->max_depth > kWavefrontMaxDepth) own = "max_depth must be 1..31";
        else if (!(wf->min_adj >= 0.0)) own = "min_adj must be >= 0";
        else if (wf->work_bytes < 0) own = "negative work_bytes";
        else if (wf->hp_cap > 0 && !wf->hp9 && !wf->hp_ray && !wf->hp_path) own = "hp_cap > 0 with null hp9, hp_ray and hp_path";
    }
    return check_ray_list(s, r, wf != nullptr, own, false, false);
}
static bool bounce_asks(const cgrt_bounce *b) {
    return b->step || b->hit_obj || b->hit_t || b->pos3 || b->normal3 || b->value3 || b->child_org3 || b->child_dir3 || b->child_adj3 ||
           b->child_path || b->child_keys;
}
static int check_hit_attributes(const cgrt_scene *s, const cgrt_rays *r, const int32_t *hit_obj, const double *hit_t,
                                const cgrt_hit_attributes *out) {
    return check_ray_list(s, r, out && hit_obj && hit_t, nullptr, false, false);
}
// The rows / stripes / samples of a grid that cgrt_camera_rays reads (max_depth, spp_total and flags are not looked at)
static int check_camera_rays(const cgrt_camera *cam, const cgrt_grid *g) {
    if (!cam || !g) return fail(CGRT_ERR_INVALID, "null argument");
    if (const int rc = check_grid_rows(cam, g, false)) return rc;
    if ((long long)g->spp * g->rows > (1ll << 38) / g->width) return fail(CGRT_ERR_LIMIT, "more than 2^38 camera rays in one call");
    return CGRT_OK;
}

// The staged copy of a host ray list: org3, dir3 and, where given, keys
static cgrt_rays stage_rays(HostStage &hs, const cgrt_rays *rays, bool keys) {
    const size_t n = (size_t)rays->n;
    cgrt_rays dr = *rays;
    dr.org3 = hs.in(rays->org3, n * 24);
    dr.dir3 = hs.in(rays->dir3, n * 24);
    dr.keys = keys ? hs.in(rays->keys, n * 8) : nullptr;
    return dr;
}
static constexpr size_t kCounterBytes = CGRT_NCOUNTERS * sizeof(uint64_t);

// The ray-buffer form of hitpoints_device: capture_rays_kernel over rays' DEVICE arrays (pixel: DEVICE, or nullptr) into a
// device buffer of `cap` records; *count = Hitpoints produced.  *d_rec_out is hipMalloc'ed here (caller frees) unless
// cap == 0.  Runs on the null stream and synchronises.
static int ray_hitpoints_device(const cgrt_scene *s, const cgrt_rays *rays, const int64_t *pixel, uint64_t cap, double **d_rec_out,
                                uint64_t *count) {
    *count = 0;
    if (rays->n == 0) return CGRT_OK;
    RaysLaunch L;
    int rc = rays_launch(s, rays, RaysKind::Capture, L);
    if (rc) return rc;
    DevBuf b_rec, b_cnt;
    HIP_TRY(b_rec.alloc((cap ? cap : 1) * 10 * sizeof(double)));
    HIP_TRY(b_cnt.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemset(b_cnt.p, 0, sizeof(unsigned long long)));
    unsigned int *queue = nullptr;
    if ((rc = ray_queue(s, 0, 0, &queue))) return rc;
    RayParams rp{};
    fill_ray_inputs(rp.in, rays);
    rp.queue = queue;
    rp.max_depth = rays->max_depth;
    const RaySink sink{b_rec.as<double>(), b_cnt.as<unsigned long long>(), (unsigned long long)cap,
                       reinterpret_cast<const long long *>(pixel)};
    if ((rc = launch_rays(s, L, L.row->capture, 0, rp, sink))) return rc;
    return capture_finish("ray hitpoint kernel: ", b_rec, b_cnt, cap, d_rec_out, count);
}

// The table behind `prim`: a host-built tree's tris[] are in the reference's leaf order (HostTree::leaf_ids maps it to
// construction order), a device-built tree's in construction order already (cgrt_devbuild.hpp).
static int need_tri_ids(const cgrt_scene *s) {
    if (s->tri_ids.p) return CGRT_OK;
    size_t total = 0;
    for (const TreeRec &tr : s->tree_recs) total = std::max(total, (size_t)tr.tri_begin + (size_t)tr.ntris);
    std::vector<int32_t> ids(std::max(total, (size_t)1), -1);
    for (size_t ti = 0; ti < s->tree_recs.size(); ti++) {
        const TreeRec &tr = s->tree_recs[ti];
        const HostTree &T = s->host.trees[ti];
        for (size_t k = 0; k < (size_t)tr.ntris; k++)
            ids[(size_t)tr.tri_begin + k] = T.dev_kind ? (int32_t)k : T.leaf_ids[k];
    }
    if (s->tri_ids.need(ids.size() * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CGRT_ERR_DEVICE, "cannot allocate the hit-attribute triangle table");
    }
    const hipError_t e = hipMemcpy(s->tri_ids.p, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        s->tri_ids.release();
        return fail(CGRT_ERR_DEVICE, std::string("hit-attribute triangle table: ") + hipGetErrorString(e));
    }
    return CGRT_OK;
}

// ---- the wavefront trace (cgrt_wavefront.hpp, cgrt_wavefront_plan.h) ----
// What the host reads back after every level: the slots asked for in the next level's queue and in the parked list, and the
// slice's own counters.  It lives behind the queue's head in the handle's launch scratch (+256).
struct WavefrontControl {
    unsigned long long next_count, parked_count, cnt[CGRT_NCOUNTERS];
};
// The work memory carved into the two ray queues, the parked list and the sort's outputs: wavefront_bytes_used() bytes, the
// 8-byte arrays ahead of the 4-byte ones
struct WavefrontMem {
    WavefrontQueue q[2];
    WavefrontParked parked;
    unsigned long long *key_out;
    uint32_t *idx_out;
};
static WavefrontMem wavefront_carve(void *base, const WavefrontCaps &c, bool hp) {
    unsigned char *p = static_cast<unsigned char *>(base);
    auto take = [&p](size_t bytes) {
        void *r = p;
        p += bytes;
        return r;
    };
    const size_t Q = (size_t)c.rays, P = (size_t)c.parked;
    WavefrontMem m{};
    for (WavefrontQueue &q : m.q) {
        q.org = static_cast<double *>(take(Q * 24));
        q.dir = static_cast<double *>(take(Q * 24));
        q.adj = static_cast<double *>(take(Q * 24));
    }
    m.parked.val = static_cast<double *>(take(P * 24));
    if (hp) {
        m.parked.pos = static_cast<double *>(take(P * 24));
        m.parked.nrm = static_cast<double *>(take(P * 24));
    }
    for (WavefrontQueue &q : m.q) q.key = static_cast<unsigned long long *>(take(Q * 8));
    m.parked.key = static_cast<unsigned long long *>(take(P * 8));
    m.key_out = static_cast<unsigned long long *>(take(P * 8));
    for (WavefrontQueue &q : m.q) {
        q.path = static_cast<uint32_t *>(take(Q * 4));
        q.root = static_cast<uint32_t *>(take(Q * 4));
    }
    m.parked.idx = static_cast<uint32_t *>(take(P * 4));
    m.idx_out = static_cast<uint32_t *>(take(P * 4));
    m.parked.path = static_cast<uint32_t *>(take(P * 4));
    return m;
}

// One slice's levels: roots [b, b + c) of the caller's arrays, level by level until max_depth, an empty level or an overflow.
// *h is the control block as the last level left it, level_rays[] the rays each level traced.
static int wavefront_levels(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_wavefront *wf, const WavefrontMem &mem,
                            const WavefrontCaps &caps, bool park, long long b, long long c, unsigned int *queue, WavefrontControl *d_ctl,
                            hipStream_t st, WavefrontControl *h, long long *level_rays, bool *overflow) {
    *overflow = false;
    HIP_TRY(hipMemsetAsync(d_ctl, 0, sizeof(WavefrontControl), st));
    long long n_in = c;
    unsigned long long rays_before = 0;
    for (int level = 1; level <= wf->max_depth; level++) {
        HIP_TRY(hipMemsetAsync(queue, 0, sizeof(unsigned int), st));
        if (level > 1) HIP_TRY(hipMemsetAsync(&d_ctl->next_count, 0, sizeof(unsigned long long), st));
        cgrt_rays lr = *rays;
        lr.n = n_in;
        RaysLaunch L;
        int rc = rays_launch(s, &lr, RaysKind::Wavefront, L);
        if (rc) return rc;
        WavefrontParams wp{};
        wp.in.n = n_in;
        wp.queue = queue;
        wp.in.seed = rays->seed;
        if (level == 1) {  // the caller's arrays
            wp.in.org = rays->org3 + 3 * b;
            wp.in.dir = rays->dir3 + 3 * b;
            wp.in.keys = rays->keys ? reinterpret_cast<const unsigned long long *>(rays->keys) + b : nullptr;
            wp.in.first_index = rays->first_index + b;
        } else {
            const WavefrontQueue &in = mem.q[level & 1];
            wp.in.org = in.org;
            wp.in.dir = in.dir;
            wp.adj = in.adj;
            wp.in.keys = in.key;
            wp.path = in.path;
            wp.root = in.root;
        }
        wp.next = mem.q[(level + 1) & 1];
        wp.next_cap = (unsigned long long)caps.rays;
        if (park) wp.parked = mem.parked;
        wp.parked_cap = (unsigned long long)caps.parked;
        wp.next_count = &d_ctl->next_count;
        wp.parked_count = &d_ctl->parked_count;
        wp.min_adj = wf->min_adj;
        wp.last = level == wf->max_depth;
        if ((rc = launch_rays(s, L, L.row->wavefront, st, wp, d_ctl->cnt))) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, d_ctl, sizeof(WavefrontControl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        level_rays[level - 1] = (long long)(h->cnt[CGRT_CNT_RAYS] - rays_before);
        rays_before = h->cnt[CGRT_CNT_RAYS];
        if (h->next_count > (unsigned long long)caps.rays || h->parked_count > (unsigned long long)caps.parked) {
            *overflow = true;
            return CGRT_OK;
        }
        if (h->next_count == 0) break;
        n_in = (long long)h->next_count;
    }
    return CGRT_OK;
}

// The slices of a call (WavefrontSlices): each one's levels, then the sort of its parked Hitpoints and their sums
static int wavefront_run(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_wavefront *wf, unsigned long long *counters,
                         uint64_t *hp_count, hipStream_t st) {
    const bool hp = wf->hp_cap > 0 && wf->hp9;
    const bool park = wf->acc3 || wf->nhit || wf->hp_cap > 0;
    const long long work = wf->work_bytes ? wf->work_bytes : wavefront_default_work(rays->n, (long long)s->mem_total, hp);
    const WavefrontCaps caps = wavefront_caps(work, hp);
    WavefrontLast &last = s->wavefront_last;
    last = WavefrontLast{};
    if (caps.rays < 1 || caps.parked < 1)
        return fail(CGRT_ERR_LIMIT, "wavefront trace: one ray needs at least " + std::to_string(wavefront_bytes_for(1, 1, hp)) +
                                        " bytes of work memory, " + std::to_string(work) + " given");
    if (s->wavefront_work.need((size_t)wavefront_bytes_used(caps, hp)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CGRT_ERR_DEVICE, "cannot allocate " + std::to_string(wavefront_bytes_used(caps, hp)) + " bytes of wavefront work memory");
    }
    const WavefrontMem mem = wavefront_carve(s->wavefront_work.p, caps, hp);
    unsigned int *queue = nullptr;
    int rc = ray_queue(s, 256, st, &queue);
    if (rc) return rc;
    WavefrontControl *d_ctl = reinterpret_cast<WavefrontControl *>(reinterpret_cast<unsigned char *>(s->scratch.p) + 256);
    static_assert(sizeof(WavefrontControl) <= 256, "the control block is the ray queue's tail");

    unsigned long long hp_total = 0;
    for (WavefrontSlices sl(rays->n, caps); !sl.done();) {
        const long long b = sl.begin, c = sl.count();
        WavefrontControl h{};
        long long level_rays[kWavefrontMaxDepth] = {};
        bool overflow = false;
        if ((rc = wavefront_levels(s, rays, wf, mem, caps, park, b, c, queue, d_ctl, st, &h, level_rays, &overflow))) return rc;
        if (overflow) {
            const bool again = sl.overflowed();
            last.slices = sl.slices;
            last.halvings = sl.halvings;
            if (again) continue;
            const long long need = wavefront_bytes_for((long long)std::max(h.next_count, 1ull), (long long)std::max(h.parked_count, 1ull), hp);
            return fail(CGRT_ERR_LIMIT, "wavefront trace: the tree of ray " + std::to_string(b) + " needs at least " + std::to_string(need) +
                                            " bytes of work memory, " + std::to_string(work) + " given");
        }
        // nothing of the slice has been written so far: zeros for the roots without Hitpoints, then the sums in emission order
        if (wf->acc3) HIP_TRY(hipMemsetAsync(wf->acc3 + 3 * b, 0, (size_t)c * 24, st));
        if (wf->nhit) HIP_TRY(hipMemsetAsync(wf->nhit + b, 0, (size_t)c * 4, st));
        const long long m = park ? (long long)h.parked_count : 0;
        if (m > 0) {
            size_t tmp_bytes = 0;
            int deepest = 0;  // the slice's deepest level with a ray: no Hitpoint lies below it
            for (int l = 0; l < kWavefrontMaxDepth; l++)
                if (level_rays[l] > 0) deepest = l + 1;
            const unsigned begin_bit = (unsigned)wavefront_key_begin_bit(deepest), end_bit = (unsigned)wavefront_key_end_bit(c);
            HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, mem.parked.key, mem.key_out, mem.parked.idx, mem.idx_out, (unsigned)m,
                                              begin_bit, end_bit, st));
            if (s->wavefront_sort.need(tmp_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(CGRT_ERR_DEVICE, "cannot allocate the wavefront sort's temporary storage");
            }
            HIP_TRY(rocprim::radix_sort_pairs(s->wavefront_sort.p, tmp_bytes, mem.parked.key, mem.key_out, mem.parked.idx, mem.idx_out,
                                              (unsigned)m, begin_bit, end_bit, st));
            WavefrontSumParams sp{};
            sp.m = m;
            sp.key = mem.key_out;
            sp.idx = mem.idx_out;
            sp.val = mem.parked.val;
            sp.pos = mem.parked.pos;
            sp.nrm = mem.parked.nrm;
            sp.path = mem.parked.path;
            sp.first_root = b;
            sp.acc3 = wf->acc3;
            sp.nhit = wf->nhit;
            sp.hp9 = wf->hp9;
            sp.hp_ray = reinterpret_cast<long long *>(wf->hp_ray);
            sp.hp_path = wf->hp_path;
            sp.hp_base = hp_total;
            sp.hp_cap = wf->hp_cap;
            hipLaunchKernelGGL(wavefront_sum_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, sp);
            HIP_TRY(hipGetLastError());
        }
        if (counters) {
            hipLaunchKernelGGL(wavefront_add_counters_kernel, dim3(1), dim3(64), 0, st, counters, d_ctl->cnt);
            HIP_TRY(hipGetLastError());
        }
        hp_total += h.cnt[CGRT_CNT_HITPOINTS];
        sl.finished();
        last.slices = sl.slices;
        last.halvings = sl.halvings;
        for (int l = 0; l < kWavefrontMaxDepth; l++) {
            last.rays[l] += level_rays[l];
            if (level_rays[l] > 0 && l + 1 > last.levels) last.levels = l + 1;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (hp_count) *hp_count = hp_total;
    return CGRT_OK;
}

extern "C" {

int cgrt_trace_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_results *out, uint64_t *counters, void *stream) {
    int rc = check_rays(s, rays, out);
    if (rc) return rc;
    if (rays->n == 0) return CGRT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(s->device);
    const bool first = !out->acc3 && !out->nhit;  // nearest-hit query: one scene walk per ray
    RaysLaunch L;
    if ((rc = rays_launch(s, rays, first ? RaysKind::First : RaysKind::Full, L))) return rc;
    // where the normals' signs are recounted below without the caller asking for hit_obj, the winners go behind the queue's head
    const bool sign_pass = out->hit_normal3 && L.dev.has_wide && !(rays->flags & CGRT_RAYS_NO_SIGN_PASS);
    const size_t own_obj = sign_pass && !out->hit_obj ? (size_t)rays->n * sizeof(int32_t) : 0;
    unsigned int *queue = nullptr;
    if ((rc = ray_queue(s, own_obj, st, &queue))) return rc;
    RayParams rp{};
    fill_ray_inputs(rp.in, rays);
    rp.queue = queue;
    rp.max_depth = rays->max_depth;
    rp.acc = out->acc3;
    rp.nhit = out->nhit;
    rp.hit_obj = own_obj ? reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(s->scratch.p) + 256) : out->hit_obj;
    rp.hit_t = out->hit_t;
    rp.hit_normal = out->hit_normal3;
    if ((rc = launch_rays(s, L, L.row->trace, st, rp, reinterpret_cast<unsigned long long *>(counters)))) return rc;
    // an opaque mesh's normal gets the reference's sign (ray_normal_sign_kernel)
    if (sign_pass) hipLaunchKernelGGL(ray_normal_sign_kernel, dim3((unsigned)((rays->n + 255) / 256)), dim3(256), 0, st, L.dev, rp);
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

int cgrt_trace_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_results *out, char *name, size_t cap) {
    if (!s || !rays || !name || cap == 0 || (!out && !(rays->flags & CGRT_RAYS_HITPOINTS))) return fail(CGRT_ERR_INVALID, "null argument");
    // CGRT_RAYS_HITPOINTS: the capture's launch, out is not looked at
    const RaysKind kind = (rays->flags & CGRT_RAYS_HITPOINTS) ? RaysKind::Capture : (!out->acc3 && !out->nhit) ? RaysKind::First : RaysKind::Full;
    if (kind != RaysKind::First && (rays->max_depth < 1 || rays->max_depth > kMaxDepth)) return fail(CGRT_ERR_INVALID, "max_depth must be 1..5");
    if (!s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    ON_DEVICE(s->device);
    rays_plan_for(s, rays, kind).name(kind, name, cap);
    return CGRT_OK;
}

int cgrt_trace_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_ray_results *out, uint64_t *counters) {
    int rc = check_rays(s, rays, out);
    if (rc) return rc;
    const size_t n = (size_t)rays->n;
    if (n == 0) {
        if (counters) std::memset(counters, 0, kCounterBytes);
        return CGRT_OK;
    }
    ON_DEVICE(s->device);
    HostStage hs;
    const cgrt_rays dr = stage_rays(hs, rays, true);
    cgrt_ray_results dout{};
    dout.acc3 = hs.out(out->acc3, n * 24);
    dout.nhit = hs.out(out->nhit, n * 4);
    dout.hit_obj = hs.out(out->hit_obj, n * 4);
    dout.hit_t = hs.out(out->hit_t, n * 8);
    dout.hit_normal3 = hs.out(out->hit_normal3, n * 24);
    uint64_t *d_cnt = hs.out_always(counters, kCounterBytes, true);
    if ((rc = hs.error())) return rc;
    return hs.finish(cgrt_trace_rays(s, &dr, &dout, d_cnt, nullptr));
}

int cgrt_occlusion_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_occlusion *occ, uint64_t *counters, void *stream) {
    int rc = check_occlusion(s, rays, occ);
    if (rc) return rc;
    if (rays->n == 0) return CGRT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(s->device);
    RaysLaunch L;
    if ((rc = rays_launch(s, rays, RaysKind::Occlusion, L))) return rc;
    unsigned int *queue = nullptr;
    if ((rc = ray_queue(s, 0, st, &queue))) return rc;
    OccParams rp{};
    fill_ray_inputs(rp.in, rays);
    rp.queue = queue;
    rp.tmax = occ->tmax;
    rp.occluded = occ->occluded;
    rp.skip_transparent = (rays->flags & CGRT_RAYS_SKIP_TRANSPARENT) != 0;
    if ((rc = launch_rays(s, L, L.row->occlusion, st, rp, reinterpret_cast<unsigned long long *>(counters)))) return rc;
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

int cgrt_occlusion_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, char *name, size_t cap) {
    if (!s || !rays || !name || cap == 0) return fail(CGRT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    ON_DEVICE(s->device);
    rays_plan_for(s, rays, RaysKind::Occlusion).name(RaysKind::Occlusion, name, cap);
    return CGRT_OK;
}

int cgrt_occlusion_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_occlusion *occ, uint64_t *counters) {
    int rc = check_occlusion(s, rays, occ);
    if (rc) return rc;
    const size_t n = (size_t)rays->n;
    if (n == 0) {
        if (counters) std::memset(counters, 0, kCounterBytes);
        return CGRT_OK;
    }
    ON_DEVICE(s->device);
    HostStage hs;
    const cgrt_rays dr = stage_rays(hs, rays, true);
    cgrt_occlusion docc{};
    docc.tmax = hs.in(occ->tmax, n * 8);
    docc.occluded = hs.out(occ->occluded, n);
    uint64_t *d_cnt = hs.out_always(counters, kCounterBytes, true);
    if ((rc = hs.error())) return rc;
    return hs.finish(cgrt_occlusion_rays(s, &dr, &docc, d_cnt, nullptr));
}

int cgrt_bounce_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_bounce *b, uint64_t *counters, void *stream) {
    int rc = check_bounce(s, rays, b);
    if (rc) return rc;
    if (rays->n == 0 || !bounce_asks(b)) return CGRT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ON_DEVICE(s->device);
    RaysLaunch L;
    if ((rc = rays_launch(s, rays, RaysKind::Bounce, L))) return rc;
    unsigned int *queue = nullptr;
    if ((rc = ray_queue(s, 0, st, &queue))) return rc;
    BounceParams bp{};
    fill_ray_inputs(bp.in, rays);
    bp.queue = queue;
    bp.adj = b->adj3;
    bp.path = b->path;
    bp.step = b->step;
    bp.hit_obj = b->hit_obj;
    bp.hit_t = b->hit_t;
    bp.pos = b->pos3;
    bp.normal = b->normal3;
    bp.value = b->value3;
    bp.child_org = b->child_org3;
    bp.child_dir = b->child_dir3;
    bp.child_adj = b->child_adj3;
    bp.child_path = b->child_path;
    bp.child_keys = reinterpret_cast<unsigned long long *>(b->child_keys);
    if ((rc = launch_rays(s, L, L.row->bounce, st, bp, reinterpret_cast<unsigned long long *>(counters)))) return rc;
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

int cgrt_bounce_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, char *name, size_t cap) {
    if (!s || !rays || !name || cap == 0) return fail(CGRT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    ON_DEVICE(s->device);
    rays_plan_for(s, rays, RaysKind::Bounce).name(RaysKind::Bounce, name, cap);
    return CGRT_OK;
}

int cgrt_bounce_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_bounce *b, uint64_t *counters) {
    int rc = check_bounce(s, rays, b);
    if (rc) return rc;
    const size_t n = (size_t)rays->n;
    if (n == 0 || !bounce_asks(b)) {
        if (counters) std::memset(counters, 0, kCounterBytes);
        return CGRT_OK;
    }
    ON_DEVICE(s->device);
    HostStage hs;
    const cgrt_rays dr = stage_rays(hs, rays, true);
    cgrt_bounce db{};
    db.adj3 = hs.in(b->adj3, n * 24);
    db.path = hs.in(b->path, n * 4);
    db.step = hs.out(b->step, n);
    db.hit_obj = hs.out(b->hit_obj, n * 4);
    db.hit_t = hs.out(b->hit_t, n * 8);
    db.pos3 = hs.out(b->pos3, n * 24);
    db.normal3 = hs.out(b->normal3, n * 24);
    db.value3 = hs.out(b->value3, n * 24);
    db.child_org3 = hs.out(b->child_org3, 2 * n * 24);
    db.child_dir3 = hs.out(b->child_dir3, 2 * n * 24);
    db.child_adj3 = hs.out(b->child_adj3, 2 * n * 24);
    db.child_path = hs.out(b->child_path, 2 * n * 4);
    db.child_keys = hs.out(b->child_keys, 2 * n * 8);
    uint64_t *d_cnt = hs.out_always(counters, kCounterBytes, true);
    if ((rc = hs.error())) return rc;
    return hs.finish(cgrt_bounce_rays(s, &dr, &db, d_cnt, nullptr));
}

int cgrt_wavefront_rays(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_wavefront *wf, uint64_t *counters, uint64_t *hp_count,
                        void *stream) {
    int rc = check_wavefront(s, rays, wf);
    if (rc) return rc;
    if (hp_count) *hp_count = 0;
    if (rays->n == 0) return CGRT_OK;
    ON_DEVICE(s->device);
    return wavefront_run(s, rays, wf, reinterpret_cast<unsigned long long *>(counters), hp_count, reinterpret_cast<hipStream_t>(stream));
}

int cgrt_wavefront_rays_variant(const cgrt_scene *s, const cgrt_rays *rays, char *name, size_t cap) {
    if (!s || !rays || !name || cap == 0) return fail(CGRT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    ON_DEVICE(s->device);
    rays_plan_for(s, rays, RaysKind::Wavefront).name(RaysKind::Wavefront, name, cap);
    return CGRT_OK;
}

int cgrt_wavefront_rays_host(const cgrt_scene *s, const cgrt_rays *rays, const cgrt_wavefront *wf, uint64_t *counters, uint64_t *hp_count) {
    int rc = check_wavefront(s, rays, wf);
    if (rc) return rc;
    if (hp_count) *hp_count = 0;
    const size_t n = (size_t)rays->n;
    if (n == 0) {
        if (counters) std::memset(counters, 0, kCounterBytes);
        return CGRT_OK;
    }
    ON_DEVICE(s->device);
    HostStage hs;
    const cgrt_rays dr = stage_rays(hs, rays, true);
    cgrt_wavefront dw = *wf;
    dw.acc3 = hs.out(wf->acc3, n * 24);
    dw.nhit = hs.out(wf->nhit, n * 4);
    dw.hp9 = hs.out(wf->hp9, (size_t)wf->hp_cap * 72, true);
    dw.hp_ray = hs.out(wf->hp_ray, (size_t)wf->hp_cap * 8, true);
    dw.hp_path = hs.out(wf->hp_path, (size_t)wf->hp_cap * 4, true);
    uint64_t *d_cnt = hs.out_always(counters, kCounterBytes, true);
    if ((rc = hs.error())) return rc;
    return hs.finish(cgrt_wavefront_rays(s, &dr, &dw, d_cnt, hp_count, nullptr));
}

int cgrt_scene_last_wavefront(const cgrt_scene *s, int64_t *slices, int64_t *halvings, int32_t *levels) {
    NEED_COMMITTED(s, true);
    if (slices) *slices = s->wavefront_last.slices;
    if (halvings) *halvings = s->wavefront_last.halvings;
    if (levels) *levels = s->wavefront_last.levels;
    return CGRT_OK;
}

int cgrt_scene_last_wavefront_rays(const cgrt_scene *s, int64_t *rays31) {
    NEED_COMMITTED(s, rays31);
    for (int l = 0; l < kWavefrontMaxDepth; l++) rays31[l] = s->wavefront_last.rays[l];
    return CGRT_OK;
}

int cgrt_camera_rays(const cgrt_camera *cam, const cgrt_grid *grid, double *org3, double *dir3, uint64_t *keys, void *stream) {
    int rc = check_camera_rays(cam, grid);
    if (rc) return rc;
    const GridParams g = grid_params(cam, grid);
    const long long total = (long long)grid->spp * grid->rows * grid->width;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g,
                       org3, dir3, reinterpret_cast<unsigned long long *>(keys), total);
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

int cgrt_camera_rays_host(const cgrt_camera *cam, const cgrt_grid *grid, double *org3, double *dir3, uint64_t *keys) {
    int rc = check_camera_rays(cam, grid);
    if (rc) return rc;
    const GridParams g = grid_params(cam, grid);
    size_t i = 0;
    for (int k = 0; k < grid->spp; k++)
        for (int j = 0; j < grid->rows; j++)
            for (int w = 0; w < grid->width; w++, i++) {
                const CameraRay c = camera_ray(g, j, w, g.sample_offset + k);
                for (int a = 0; a < 3; a++) {
                    if (org3) org3[3 * i + a] = c.o[a];
                    if (dir3) dir3[3 * i + a] = c.d[a];
                }
                if (keys) keys[i] = c.key;
            }
    return CGRT_OK;
}

int cgrt_trace_rays_hitpoints(const cgrt_scene *s, const cgrt_rays *rays, double *hp10, uint64_t cap, uint64_t *count) {
    int rc = check_capture_rays(s, rays);
    if (rc) return rc;
    if (!count || (cap > 0 && !hp10)) return fail(CGRT_ERR_INVALID, "null output");
    ON_DEVICE(s->device);
    double *d_rec = nullptr;
    uint64_t n = 0;
    rc = ray_hitpoints_device(s, rays, nullptr, cap, &d_rec, &n);
    return hitpoints_to_host(rc, d_rec, n, hp10, cap, count);
}

// ---- hit attributes of caller-supplied rays (cgrt_hit_attr.hpp) ----
int cgrt_ray_hit_attributes(const cgrt_scene *s, const cgrt_rays *rays, const int32_t *hit_obj, const double *hit_t,
                            const cgrt_hit_attributes *out, void *stream) {
    int rc = check_hit_attributes(s, rays, hit_obj, hit_t, out);
    if (rc) return rc;
    if (rays->n == 0 || (!out->prim && !out->uv2 && !out->color3 && !out->material2)) return CGRT_OK;
    ON_DEVICE(s->device);
    if (out->prim && (rc = need_tri_ids(s))) return rc;
    HitAttrParams hp{};
    hp.n = rays->n;
    hp.org = rays->org3;
    hp.dir = rays->dir3;
    hp.hit_obj = hit_obj;
    hp.hit_t = hit_t;
    hp.prim = out->prim;
    hp.uv = out->uv2;
    hp.color = out->color3;
    hp.material = out->material2;
    hp.tri_ids = out->prim ? reinterpret_cast<const int32_t *>(s->tri_ids.p) : nullptr;
    hipLaunchKernelGGL(ray_hit_attributes_kernel, dim3((unsigned)((rays->n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), s->dev, hp);
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

int cgrt_ray_hit_attributes_host(const cgrt_scene *s, const cgrt_rays *rays, const int32_t *hit_obj, const double *hit_t,
                                 const cgrt_hit_attributes *out) {
    int rc = check_hit_attributes(s, rays, hit_obj, hit_t, out);
    if (rc) return rc;
    const size_t n = (size_t)rays->n;
    if (n == 0) return CGRT_OK;
    ON_DEVICE(s->device);
    HostStage hs;
    const cgrt_rays dr = stage_rays(hs, rays, false);
    const int32_t *d_obj = hs.in(hit_obj, n * 4);
    const double *d_t = hs.in(hit_t, n * 8);
    cgrt_hit_attributes dout{};
    dout.prim = hs.out(out->prim, n * 4);
    dout.uv2 = hs.out(out->uv2, n * 16);
    dout.color3 = hs.out(out->color3, n * 24);
    dout.material2 = hs.out(out->material2, n * 16);
    if ((rc = hs.error())) return rc;
    return hs.finish(cgrt_ray_hit_attributes(s, &dr, d_obj, d_t, &dout, nullptr));
}

}  // extern "C"
