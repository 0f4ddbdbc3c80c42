// The host side of a sphere scene's tile-order launch: what the handle keeps for it between launches (the order buffer and the
// sample relay's area, each with the event and stream that order their users), the steps that prepare a launch (order_tiles,
// relay_prepare, the lens table's lens_table_prepare / _join and LensTableGuard, and the cost start's two: cost_start_begin and
// cost_start_rank, with the probe between them launched by cgrt_hip.hip), the guard that closes a cgrt_trace_grid over both, and what the cgrt_scene_last_* read-backs report.  What a
// launch does is frame_plan's decision (TileOrderPlan, RelayPlan; cgrt_frame.h).  Part of libcgrt.so (cgrt_hip.hip).
#ifndef CGRT_TILE_ORDER_HPP
#define CGRT_TILE_ORDER_HPP

enum class Capturing { None, Active, Unknown };
static Capturing stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus c = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &c) != hipSuccess) {
        (void)hipGetLastError();
        return Capturing::Unknown;
    }
    return c == hipStreamCaptureStatusNone ? Capturing::None : Capturing::Active;
}

// Tile order of image-order launches (tile_order_kernel): the scene's reflecting / refracting spheres (read at commit; ok: the
// scene is spheres and planes with 1..kOrderSpheresMax of them), the order buffer (TileOrderLayout) -- launch scratch like the
// handle's `scratch`, kept apart so that the frame plan's layout stays what it is -- and what the last cgrt_trace_grid did: the
// tiles it ordered (0: none), the wave tiles it wrote sphere masks for (0: none) and sure spheres for (0: none), where the parts
// lie, and who rendered class 3.  Key::masks: bit 0 -- masks asked for, bit 1 -- sure tiles asked for.
// What the buffer holds: the order depends on nothing but Key, so a launch with the key of the buffer's contents runs no
// ordering kernel (reused).  ev is recorded behind the kernel on `stream`; a reusing launch on another stream waits for it.
// commit_gen: this commit's number.
struct TileOrderState {
    OrderSpheres spheres{};
    bool ok = false;
    GrowBuf buf;
    struct Key {
        double cam[3], half_width, focus_plane, lens_radius;
        int32_t W, H, rows, row_offset, stripe_rows, stripe_rank, stripe_nranks, masks;
        uint64_t commit_gen;
        const void *buf;
    };
    static_assert(sizeof(Key) == 96, "Key is compared as bytes: no padding");
    Key key{};
    uint64_t commit_gen = 0;
    bool valid = false, reused = false;
    bool captured = false;  // a launch on this handle was captured into a graph: its replays rewrite the buffer at times the handle does not see, so nothing is reused any more
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;
    size_t tiles = 0, mask_wtiles = 0, sure_wtiles = 0;
    TileOrderLayout at;
    TileOrderPlan::Class3 class3 = TileOrderPlan::None;
    int lens_stage = kLensStageOff;  // how that launch's in-kernel terminal-diffuse body drew its lens points
    // The relay's cost start (cgrt_relay.h; cost_start_begin, cost_start_rank): the probe's costs and the start table lie behind the
    // rest of the buffer and are kept with the order -- never beyond it: a launch that did not reuse the order has neither.  The
    // costs depend, beyond Key, on CostKey; the table on the costs and on TableKey.  start_words: the table's part in the last
    // launch (0: it had none), start_wtiles its wave tiles, start_reused: it ran neither probe nor ranking.
    struct CostKey {
        uint64_t seed;
        int32_t max_depth, probe_spp;
        static CostKey of(const RelayPlan &r, const GridParams &g) { return CostKey{g.seed, g.max_depth, r.probe_spp}; }
    };
    // (boost_k == 0: a table without promoted tiles, in `start`; else the promoted form's, in `bstart`, with what it depends on)
    struct TableKey {
        int32_t spp, k, chunk_spp, cap, extent, boost_k, boost_cap, boost_num, boost_den, boost_wg_slots;
        static TableKey of(const RelayPlan &r) {
            const RelayBoost b = r.boost_rule();
            return TableKey{r.spp, r.base.k, r.base.chunk_spp, (int32_t)r.base.cap, r.extent, (int32_t)b.k, (int32_t)b.cap, (int32_t)b.num, (int32_t)b.den, (int32_t)b.slots};
        }
    };
    static_assert(sizeof(CostKey) == 16 && sizeof(TableKey) == 40, "compared as bytes: no padding");
    CostKey cost_key{};
    TableKey table_key{};
    bool cost_valid = false, table_valid = false, start_reused = false;
    size_t start_words = 0, start_wtiles = 0;
    // the last launch's table was the promoted form's (RelayBoost of it, with the threshold; k == 0: it was not)
    RelayBoost boost{};

    void begin_launch() {
        tiles = mask_wtiles = sure_wtiles = start_words = start_wtiles = 0;
        boost = RelayBoost{};
        reused = start_reused = false;
        class3 = TileOrderPlan::None;
        lens_stage = kLensStageOff;
    }
    void release() {
        buf.release();
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    template <class T> int read(const Region &r, T *dst, size_t count) const {
        HIP_TRY(hipMemcpy(dst, reinterpret_cast<const unsigned char *>(buf.p) + r.at, count * sizeof(T), hipMemcpyDeviceToHost));
        return CGRT_OK;
    }
    int read_plan(uint32_t *plan) const {  // plan[0 .. kOrderClasses] of the last launch, once the device is through with it
        HIP_TRY(hipDeviceSynchronize());
        return read(at.plan, plan, kOrderClasses + 1);
    }
};

// The sample relay's area (cgrt_relay.h; launch scratch like `scratch`, allocated by the first launch that relays, sized by the
// largest): refused -- the smallest size the device has refused (such a launch goes unrelayed); zeroed -- the arrival words
// known to be 0 (the kernel leaves them so; a launch that failed on the way does not vouch for it: dirty); ev is recorded
// behind a relaying launch on `stream`, and a relaying launch on another stream waits for it -- the area is one.  last: the plan
// the last cgrt_trace_grid relayed with (one that does not relay: it did not); its boost part only where that launch promoted.
struct RelayState {
    GrowBuf buf;
    size_t refused = 0, zeroed = 0;
    size_t boost_zeroed = 0, boost_zeroed_at = 0;  // the boost area's arrival words known to be 0, and where that area began
    bool dirty = false;
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;
    bool recorded = false;
    RelayPlan last;

    void begin_launch() { last = RelayPlan{}; }
    void release() {
        buf.release();
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
};

// The tile order of an image-order launch over a scene with reflecting or refracting spheres (tile_order_kernel, cgrt_eye.hpp):
// one small launch in front of the eye launch, on its stream, that lists the tiles the costly ones first; g then maps the
// eye launch's workgroups through the list.  The buffer is launch scratch of the handle, written and read on this stream.
// p.order.masks: the launch also writes the wave tiles' sphere masks (GridParams::wmask) for the terminal-diffuse body;
// p.order.sure: sure_first_kernel follows it and writes the sure spheres (GridParams::wsure), kept and reused with the rest.
// The kernel reads the camera, the frame geometry (W, H, rows, row offset, stripe) and the committed scene, nothing else: when
// the buffer still holds the result for exactly these (TileOrderState::Key -- the passes of a progressive render, the frames of
// a still camera) nothing is launched and g points at it.  The eye launch only reads the buffer (plan[0..4], the list, the
// masks; plan[kOrderArrived] is back at 0 when the kernel ends), so it is as the kernel left it.  The contents are not trusted
// beyond a commit, a reallocation, a cgrt_trace_grid that returned an error (TileOrderGuard drops the key on every such exit) or
// a stream capture (a captured launch runs later, or never, and again at every replay: from the first capture on, the handle
// neither reuses nor leaves a key; a stream whose state cannot be asked counts as captured).
// One handle serves one stream at a time (cgrt.h, "Threading"): a launch with another key rewrites the buffer, and the event only
// orders a reusing launch behind the kernel that wrote it, not a rewrite behind another stream's readers.
// no_reuse (CGRT_NO_ORDER_REUSE=1, a measurement aid): every launch runs the kernel.
static int order_tiles(TileOrderState &o, const DeviceScene &dev, const FramePlan &p, GridParams &g, bool no_reuse, Capturing capturing,
                       hipStream_t st) {
    const int tiles_x = (g.W + kTileW - 1) / kTileW, tiles_y = (g.rows + kTileH - 1) / kTileH;
    const size_t n = (size_t)tiles_x * tiles_y;
    const bool masks = p.order.masks, sure = masks && p.order.sure;
    const TileOrderLayout at = p.relay.order_layout(n, p.n_wt, sure);
    const bool grown = at.total > o.buf.cap;
    if (grown) o.valid = false;
    if (o.buf.need(at.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CGRT_ERR_DEVICE, "cannot allocate launch scratch (tile order)");
    }
    unsigned char *base = reinterpret_cast<unsigned char *>(o.buf.p);
    uint32_t *plan = at.plan.in<uint32_t>(base), *list = at.list.in<uint32_t>(base);
    uint32_t *wmask = masks ? at.wmask.in<uint32_t>(base) : nullptr;
    unsigned char *wsure = sure ? at.wsure.in<unsigned char>(base) : nullptr;
    const TileOrderState::Key key{{g.cam[0], g.cam[1], g.cam[2]}, g.half_width, g.focus_plane, g.lens_radius, g.W, g.H, g.rows, g.row_offset,
                                  g.stripe_rows, g.stripe_rank, g.stripe_nranks, (masks ? 1 : 0) | (sure ? 2 : 0), o.commit_gen, o.buf.p};
    if (capturing != Capturing::None) o.captured = true;
    const bool plain = !o.captured && !no_reuse;
    o.reused = plain && o.valid && std::memcmp(&key, &o.key, sizeof(key)) == 0;
    if (o.reused) {
        if (st != o.stream) HIP_TRY(hipStreamWaitEvent(st, o.ev, 0));
    } else {
        o.valid = o.cost_valid = o.table_valid = false;  // (costs and table are of the order they were found for)
        if (grown) HIP_TRY(hipMemsetAsync(plan, 0, at.plan.bytes, st));  // plan[kOrderArrived]
        const unsigned blocks = (unsigned)std::min((p.n_wt + 1023) / 1024, (size_t)64);
        hipLaunchKernelGGL(tile_order_kernel, dim3(blocks), dim3(1024), 0, st, g, o.spheres, dev, tiles_x, tiles_y, plan, list,
                           at.tile_cls.in<unsigned char>(base), at.wave_cls.in<unsigned char>(base), wmask);
        if (sure)
            hipLaunchKernelGGL(sure_first_kernel, dim3((unsigned)((p.n_wt + 255) / 256)), dim3(256), 0, st, g, dev, tiles_x,
                               at.tile_cls.in<unsigned char>(base), wmask, wsure);
        if (plain && hipPeekAtLastError() == hipSuccess) {
            if (!o.ev && hipEventCreateWithFlags(&o.ev, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                o.ev = nullptr;
            }
            if (o.ev && hipEventRecord(o.ev, st) == hipSuccess) {
                o.key = key;
                o.stream = st;
                o.valid = true;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    g.plan = plan;
    g.border = list;
    g.wmask = wmask;
    g.wsure = wsure;
    g.tile_order = kOrderAll;
    o.tiles = n;
    o.mask_wtiles = masks ? p.n_wt : 0;
    o.sure_wtiles = sure ? p.n_wt : 0;
    o.at = at;
    o.class3 = p.order.class3;
    o.lens_stage = p.order.lens_stage;
    return CGRT_OK;
}

// The sample relay of a tile-order launch of the PAIR variants (cgrt_relay.h; p.relays()): the handle's relay area and g's relay
// fields.  Returns false -- the launch goes unrelayed, which is no error -- when the stream is being captured (the area, its
// event and the handle's record of both belong to launches that run now) or its state cannot be asked, or the area cannot be
// had.  The arrival words are 0 whenever no launch is in flight: zeroed here when the area is new or grown, when more of them
// are needed than were zeroed, or after a launch that did not go through; reset by the kernel otherwise.
static bool relay_prepare(RelayState &r, const RelayPlan &p, GridParams &g, Capturing capturing, hipStream_t st) {
    if (capturing != Capturing::None) return false;
    const auto ok = [](hipError_t e) { return e == hipSuccess || ((void)hipGetLastError(), false); };
    const size_t bytes = p.bytes(), boost_at = p.boost_at();
    if (r.refused && bytes >= r.refused) return false;
    if (bytes > r.buf.cap) {
        if (r.recorded) (void)ok(hipEventSynchronize(r.ev));  // the launches that use the old area are through before it is freed
        r.zeroed = r.boost_zeroed = 0;
        if (!ok(r.buf.need(bytes))) {
            r.refused = bytes;
            return false;
        }
    }
    if (!r.ev && !ok(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming))) {
        r.ev = nullptr;
        return false;
    }
    if (r.recorded && st != r.stream && !ok(hipStreamWaitEvent(st, r.ev, 0))) return false;
    unsigned char *buf = reinterpret_cast<unsigned char *>(r.buf.p);
    if ((r.dirty || p.base.cap > r.zeroed) && !ok(hipMemsetAsync(buf, 0, p.base.cap * sizeof(uint32_t), st))) return false;
    r.zeroed = p.base.cap;  // (the words beyond this launch's lie in its arrays)
    if (p.boosts() && (r.dirty || boost_at != r.boost_zeroed_at || p.boost.cap > r.boost_zeroed) &&
        !ok(hipMemsetAsync(buf + boost_at, 0, p.boost.cap * sizeof(uint32_t), st)))
        return false;
    r.boost_zeroed = p.boosts() ? p.boost.cap : 0;  // (without a boost area this launch's arrays may lie over the words)
    r.boost_zeroed_at = p.boosts() ? boost_at : r.boost_zeroed_at;
    r.dirty = true;  // until the launch is through (TileOrderGuard::commit)
    p.place(g, buf);
    return true;
}

// The relay's start order by cost (cgrt_relay.h; behind order_tiles and relay_prepare on their stream, when the plan has
// start == kRelayStartCost and the launch relays), in two steps with the probe between them.  The probe is the launch's own
// kernel over entries [0, plan[3]) of the list with the first probe_spp samples of every pixel; it stores nothing but each wave's
// iteration count in wcost (relay_cost_start, cgrt_hip.hip).  Ranking kernels turn the costs into the table, and g maps its
// workgroups of classes 0-2 through it.  Costs and table stay in the order buffer and are reused with the order, as long as what
// else they depend on (CostKey, TableKey) is the same; where only the table's key differs the probe is not run again.
struct CostStart {
    uint32_t *wcost = nullptr;  // where the probe leaves its costs; nullptr: the layout has no table, the launch goes by its list
    bool have_cost = false, have_table = false;  // what the buffer still holds
    TileOrderState::CostKey cost_key{};  // this launch's
    TileOrderState::TableKey table_key{};
};
// whether the buffer still holds this launch's costs (else relay_cost_start runs the probe)
static bool costs_kept(const TileOrderState &o, const TileOrderState::CostKey &k) {
    return o.reused && o.cost_valid && std::memcmp(&k, &o.cost_key, sizeof(k)) == 0;
}
// ... asked ahead of cost_start_begin, behind order_tiles, of a launch whose relay starts by cost: the probe will run
static bool cost_probe_due(const TileOrderState &o, const RelayPlan &r, const GridParams &g) {
    return o.at.wcost.in<uint32_t>(reinterpret_cast<unsigned char *>(o.buf.p)) != nullptr && !costs_kept(o, TileOrderState::CostKey::of(r, g));
}
// what is still valid; costs that are not are zeroed for the probe
static int cost_start_begin(TileOrderState &o, const RelayPlan &r, const GridParams &g, hipStream_t st, CostStart &c) {
    c.wcost = o.at.wcost.in<uint32_t>(reinterpret_cast<unsigned char *>(o.buf.p));
    if (!c.wcost) return CGRT_OK;
    c.cost_key = TileOrderState::CostKey::of(r, g);
    c.table_key = TileOrderState::TableKey::of(r);
    c.have_cost = costs_kept(o, c.cost_key);
    c.have_table = c.have_cost && o.table_valid && std::memcmp(&c.table_key, &o.table_key, sizeof(c.table_key)) == 0;
    o.cost_valid = o.table_valid = false;
    if (!c.have_cost) HIP_TRY(hipMemsetAsync(c.wcost, 0, o.at.wcost.bytes, st));
    return CGRT_OK;
}
// rank (unless the table is still valid) and record: the keys, g's table and the launch's record.  With promoted tiles
// (p.relay.boosts()) the table is the promoted form's, in its own parts of the buffer.
static int cost_start_rank(TileOrderState &o, const FramePlan &p, const CostStart &c, GridParams &g, hipStream_t st) {
    const RelayPlan &r = p.relay;
    const TileOrderLayout &at = o.at;
    unsigned char *base = reinterpret_cast<unsigned char *>(o.buf.p);
    const bool boost = r.boosts();
    if (!c.have_table) {
        const RelayStartArgs a{r.items(0, 0, 0), (uint32_t)((g.W + kTileW - 1) / kTileW), (uint32_t)p.wtiles_x, (uint32_t)p.wtiles_y};
        const auto blocks = [](size_t threads) { return dim3((unsigned)((threads + kRelayThreads - 1) / kRelayThreads)); };
        const dim3 nt(kRelayThreads);
        if (boost) {
            const RelayBoostArgs ba{a, r.boost_rule()};
            const size_t n_tiles = (size_t)p.tile_blocks, n_virtual = n_tiles * (size_t)r.boost.k;
            uint32_t *head = at.boost.in<uint32_t>(base), *bslot = at.bslot.in<uint32_t>(base), *ecost = at.ecost.in<uint32_t>(base);
            unsigned long long *bweight = at.bweight.in<unsigned long long>(base);
            HIP_TRY(hipMemsetAsync(head, 0, kBoostHead * sizeof(uint32_t), st));
            hipLaunchKernelGGL(relay_boost_cost_kernel, blocks(n_tiles), nt, 0, st, ba, g.plan, g.border, c.wcost, ecost, head);
            hipLaunchKernelGGL(relay_boost_promote_kernel, blocks(r.base.cap), nt, 0, st, ba, g.plan, ecost, head, bslot);
            hipLaunchKernelGGL(relay_boost_weight_kernel, blocks(n_virtual), nt, 0, st, ba, g.plan, ecost, bslot, head, bweight);
            hipLaunchKernelGGL(relay_boost_start_kernel, blocks(n_virtual), nt, 0, st, ba, g.plan, bweight, at.bstart.in<uint32_t>(base));
        } else {
            unsigned long long *weight = at.weight.in<unsigned long long>(base);
            hipLaunchKernelGGL(relay_weight_kernel, blocks(r.start_words), nt, 0, st, a, g.plan, g.border, c.wcost, weight);
            hipLaunchKernelGGL(relay_start_kernel, blocks(r.start_words), nt, 0, st, a, g.plan, weight, at.start.in<uint32_t>(base));
        }
    }
    // the order's event now stands behind the table too (a reusing launch on another stream waits for it)
    if (o.valid && (c.have_table || (hipPeekAtLastError() == hipSuccess && hipEventRecord(o.ev, st) == hipSuccess))) {
        if (!c.have_table) o.stream = st;
        o.cost_key = c.cost_key;
        o.table_key = c.table_key;
        o.cost_valid = o.table_valid = true;
    } else if (o.valid) {
        (void)hipGetLastError();
        o.valid = false;
    }
    g.relay_start_at = at.word(boost ? at.bstart : at.start);
    g.relay_boost_at = boost ? at.word(at.boost) : 0u;
    o.boost = r.boost_rule();
    o.start_words = r.start_words;
    o.start_wtiles = p.n_wt;
    o.start_reused = c.have_table;
    return CGRT_OK;
}

// The lens table (cgrt_lens_stage.h; launch scratch like the relay area: allocated by the first launch that uses it, sized by the
// largest, freed with the scene; not a part of FramePlan::scratch).  refused: the smallest size the device has refused (such a
// launch goes without a table).  ev is recorded behind every launch that read the table, on `stream`; a launch on another stream
// waits for it before it reads or rewrites the table -- the table is one.  What it holds: the draws depend on seed, sample_offset,
// spp and the pixel set, their place on the order list, so the table is kept with the tile order -- valid while the order is
// reused and Key, which holds the order's own key, is the same.  cap, reused: the last launch's (cap == 0: it read no table).
// A launch that has to write the table does so on the handle's second stream where it has one (ev_fork / ev_built; joining: the
// launch's stream has yet to wait for it).  Beside the cost probe and the ranking kernels, which leave most of the device idle,
// that costs the frame nothing; with nothing beside it the kernel takes longer than the frame gains, so unless the plan says
// lens_table_always a launch writes the table only where its probe is due and otherwise goes without one.
struct LensTableState {
    GrowBuf buf;
    size_t refused = 0;
    hipEvent_t ev = nullptr, ev_fork = nullptr, ev_built = nullptr;
    bool joining = false;
    hipStream_t stream = nullptr;
    bool recorded = false;
    struct Key {
        TileOrderState::Key order;
        uint64_t seed;
        int32_t sample_offset, spp;
        uint64_t cap;
        const void *buf;
    };
    static_assert(sizeof(Key) == 128, "Key is compared as bytes: no padding");
    Key key{}, pending{};
    bool valid = false, keep = false, reused = false;
    size_t cap = 0;

    void begin_launch() {
        cap = 0;
        reused = keep = joining = false;
    }
    void release() {
        buf.release();
        for (hipEvent_t *e : {&ev, &ev_fork, &ev_built}) {
            if (*e) (void)hipEventDestroy(*e);
            *e = nullptr;
        }
    }
};
// st waits for the table where it is being written on the second stream (ahead of the frame; a no-op otherwise)
static int lens_table_join(LensTableState &t, hipStream_t st) {
    if (!t.joining) return CGRT_OK;
    t.joining = false;
    HIP_TRY(hipStreamWaitEvent(st, t.ev_built, 0));
    return CGRT_OK;
}
// The lens table of a launch whose plan has one (p.order.lens_table_cap > 0; behind order_tiles on its stream), and g's fields.
// Returns false -- the launch's bodies of classes 0-2 draw sample by sample, in the kernels without a table, which is no error --
// when the stream is being captured or its state cannot be asked, or the table cannot be had.  Unless the table still holds this
// launch's draws, lens_table_kernel writes them here: on `aux` (the handle's second stream; nullptr: on st), behind what st holds
// so far -- the ordering kernel, and every earlier reader of the table -- and lens_table_join makes st wait for it ahead of the
// frame.  beside_probe: the launch's cost probe is due (cost_probe_due); without it, and without lens_table_always, a launch
// that would have to write the table goes without one too, and the table stays what it was.
// no_reuse (CGRT_NO_ORDER_REUSE=1): every launch writes them.
static bool lens_table_prepare(LensTableState &t, const TileOrderState &o, const FramePlan &p, GridParams &g, bool no_reuse, bool beside_probe,
                               Capturing capturing, hipStream_t st, hipStream_t aux) {
    const auto ok = [](hipError_t e) { return e == hipSuccess || ((void)hipGetLastError(), false); };
    const auto none = [&g] {
        g.lens_table = nullptr;
        g.lens_table_cap = g.lens_table_spp = 0;
        return false;
    };
    const size_t bytes = p.order.lens_table_bytes, cap = p.order.lens_table_cap;
    if (capturing != Capturing::None || bytes == 0) return none();
    if (t.refused && bytes >= t.refused) return none();
    const bool may_write = p.order.lens_table_always || beside_probe;
    if (bytes > t.buf.cap) {
        if (!may_write) return none();  // (a table that small holds nothing of this launch's)
        // the launches that read the old table, and a kernel that wrote it for a launch that failed, are through before it is freed
        if (t.recorded) (void)ok(hipEventSynchronize(t.ev));
        if (t.ev_built) (void)ok(hipEventSynchronize(t.ev_built));
        t.valid = false;
        if (!ok(t.buf.need(bytes))) {
            t.refused = bytes;
            return none();
        }
    }
    if (!t.ev && !ok(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming))) {
        t.ev = nullptr;
        return none();
    }
    if (t.recorded && st != t.stream && !ok(hipStreamWaitEvent(st, t.ev, 0))) return none();
    // (o.valid: the order's key is this launch's -- order_tiles leaves none behind a capture or under no_reuse)
    const LensTableState::Key key{o.key, g.seed, g.sample_offset, g.spp, (uint64_t)cap, t.buf.p};
    t.keep = o.valid && !no_reuse;
    t.reused = t.keep && o.reused && t.valid && std::memcmp(&key, &t.key, sizeof(key)) == 0;
    if (!t.reused && !may_write) return none();
    if (!t.reused) {
        t.valid = false;
        const auto event = [&ok](hipEvent_t &e) { return e || ok(hipEventCreateWithFlags(&e, hipEventDisableTiming)) || (e = nullptr, false); };
        hipStream_t ks = st;
        if (aux && event(t.ev_fork) && event(t.ev_built) && ok(hipEventRecord(t.ev_fork, st)) && ok(hipStreamWaitEvent(aux, t.ev_fork, 0))) ks = aux;
        hipLaunchKernelGGL(lens_table_kernel, dim3((unsigned)cap), dim3(kThreads), 0, ks, g, reinterpret_cast<uint64_t *>(t.buf.p));
        const bool launched = ok(hipPeekAtLastError());
        if (ks != st) {
            if (ok(hipEventRecord(t.ev_built, ks))) t.joining = true;
            else (void)ok(hipStreamSynchronize(ks));  // (no event to wait for: the table is written before st goes on)
        }
        if (!launched) {
            (void)lens_table_join(t, st);
            return none();
        }
    }
    g.lens_table = reinterpret_cast<const uint64_t *>(t.buf.p);
    t.pending = key;
    t.cap = cap;
    return true;
}
// A cgrt_trace_grid's hold on the table, like TileOrderGuard's on the order: the last launch's record is cleared, and an exit
// without commit leaves neither a key nor a record of a table read, and st behind a kernel still writing on the second stream.
struct LensTableGuard {
    LensTableState &t;
    hipStream_t st;
    bool through = false;
    LensTableGuard(LensTableState &table, hipStream_t stream) : t(table), st(stream) { t.begin_launch(); }
    LensTableGuard(const LensTableGuard &) = delete;
    LensTableGuard &operator=(const LensTableGuard &) = delete;
    ~LensTableGuard() {
        if (through) return;
        if (lens_table_join(t, st) != CGRT_OK) (void)hipGetLastError();
        t.valid = t.reused = false;
        t.cap = 0;
    }
    // the launch went out on st without an error; tabled: it reads the table
    int commit(bool tabled) {
        through = true;
        if (!tabled) return CGRT_OK;
        HIP_TRY(hipEventRecord(t.ev, st));
        t.stream = st;
        t.recorded = true;
        if (t.keep) {
            t.key = t.pending;
            t.valid = true;
        }
        return CGRT_OK;
    }
};

// A cgrt_trace_grid's hold on both states, from the point where it starts to touch them: the last launch's record is cleared,
// and every exit without commit drops the stored order's key -- only a call that went through leaves one -- and leaves the
// relay area dirty, so that its arrival words are zeroed before they are used again.
struct TileOrderGuard {
    TileOrderState &order;
    RelayState &relay;
    const RelayPlan *relayed = nullptr;  // the plan relay_prepare placed in the launch (nullptr: it goes unrelayed)
    bool through = false;
    TileOrderGuard(TileOrderState &o, RelayState &r) : order(o), relay(r) {
        order.begin_launch();
        relay.begin_launch();
    }
    TileOrderGuard(const TileOrderGuard &) = delete;
    TileOrderGuard &operator=(const TileOrderGuard &) = delete;
    ~TileOrderGuard() {
        if (!through) order.valid = false;
    }
    // the launch g went out on st without an error
    int commit(const GridParams &g, hipStream_t st) {
        if (relayed) {
            HIP_TRY(hipEventRecord(relay.ev, st));
            relay.stream = st;
            relay.recorded = true;
            relay.last = *relayed;
            if (!g.relay_boost_at) relay.last.boost = RelayArea{};  // (it had no promoted table: nothing lies in the boost area)
            relay.dirty = false;
        }
        through = true;
        return CGRT_OK;
    }
};

// ---- what the last cgrt_trace_grid on the handle did (the cgrt_scene_last_* entry points, on the scene's device) ----
static int last_tile_order(const TileOrderState &o, uint32_t *plan5, uint32_t *list, uint8_t *cls, int64_t cap, int64_t *n_tiles) {
    const size_t n = o.tiles;
    *n_tiles = (int64_t)n;
    if (n == 0 || cap < (int64_t)n) return CGRT_OK;
    uint32_t plan[kOrderClasses + 1];
    int rc = o.read_plan(plan5 ? plan5 : plan);
    if (rc || (list && (rc = o.read(o.at.list, list, n)))) return rc;
    return cls ? o.read(o.at.tile_cls, cls, n) : CGRT_OK;
}
static int last_sphere_masks(const TileOrderState &o, uint32_t *masks, int64_t cap, int64_t *n_wave_tiles) {
    const size_t n_wt = o.mask_wtiles;
    *n_wave_tiles = (int64_t)n_wt;
    if (n_wt == 0 || o.tiles == 0 || !masks || cap < (int64_t)n_wt) return CGRT_OK;
    HIP_TRY(hipDeviceSynchronize());
    return o.read(o.at.wmask, masks, n_wt);
}
static int last_sure_tiles(const TileOrderState &o, uint8_t *sure, int64_t cap, int64_t *n_wave_tiles) {
    const size_t n_wt = o.sure_wtiles;
    *n_wave_tiles = (int64_t)n_wt;
    if (n_wt == 0 || o.tiles == 0 || !sure || cap < (int64_t)n_wt) return CGRT_OK;
    HIP_TRY(hipDeviceSynchronize());
    return o.read(o.at.wsure, sure, n_wt);
}
// the class-3 tiles of the last launch's order, when that launch gave them to the terminal-diffuse body in the form asked for
static int last_class3_tiles(const TileOrderState &o, TileOrderPlan::Class3 form, int64_t *n_tiles) {
    *n_tiles = 0;
    if (o.class3 != form || o.tiles == 0) return CGRT_OK;
    uint32_t plan[kOrderClasses + 1];
    if (int rc = o.read_plan(plan)) return rc;
    *n_tiles = (int64_t)plan[kOrderClasses] - (int64_t)plan[3];
    return CGRT_OK;
}
// the tiles of the last launch whose workgroups staged their lens draws in LDS batches: its in-kernel class-3 tiles
static int last_lens_stage(const TileOrderState &o, int64_t *lds_tiles, int64_t *area_tiles) {
    *lds_tiles = *area_tiles = 0;
    return o.lens_stage == kLensStageLds ? last_class3_tiles(o, TileOrderPlan::InKernel, lds_tiles) : CGRT_OK;
}
// the list entries of the last launch whose workgroups read their lens draws from the table -- its entries of classes 0-2 below
// the table's capacity --, that capacity, and whether the launch found the table written
static int last_lens_table(const TileOrderState &o, const LensTableState &t, int64_t *entries, int64_t *capacity, int32_t *reused) {
    *entries = *capacity = 0;
    *reused = 0;
    if (t.cap == 0 || o.tiles == 0) return CGRT_OK;
    uint32_t plan[kOrderClasses + 1];
    if (int rc = o.read_plan(plan)) return rc;
    *entries = (int64_t)std::min((size_t)plan[3], t.cap);
    *capacity = (int64_t)t.cap;
    *reused = t.reused ? 1 : 0;
    return CGRT_OK;
}
static int last_sample_relay(const TileOrderState &o, const RelayState &r, int64_t *tiles, int32_t *chunks, int64_t *parked_values) {
    *tiles = *parked_values = 0;
    *chunks = 0;
    const RelayPlan &l = r.last;
    if (!l.relays() || o.tiles == 0) return CGRT_OK;
    uint32_t plan[kOrderClasses + 1];
    if (int rc = o.read_plan(plan)) return rc;
    const size_t n_split = relay_split_entries(plan[2], plan[3], (uint32_t)l.base.cap, l.extent);  // the entries in fact split
    *tiles = (int64_t)n_split;
    if (n_split == 0) return CGRT_OK;
    *chunks = l.base.k;
    // rcount[tile][chunk - 1][thread] of the first n_split tiles is one run of words
    const size_t per_base = (size_t)(l.base.k - 1) * kRelayThreads;
    std::vector<uint32_t> cnt(n_split * per_base);
    const unsigned char *area = reinterpret_cast<const unsigned char *>(r.buf.p);
    HIP_TRY(hipMemcpy(cnt.data(), area + relay_layout(l.base.cap, l.base.k, l.base.slots).rcount, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (l.boost.k == 0 || o.boost.k == 0) {
        for (uint32_t c : cnt) *parked_values += (int64_t)c;
        return CGRT_OK;
    }
    // promoted tiles: their counts lie in the boost area, at their boost slots (the base slot's are of an earlier launch)
    std::vector<uint32_t> bslot(n_split);
    if (int rc = o.read(o.at.bslot, bslot.data(), n_split)) return rc;
    const size_t per = (size_t)(l.boost.k - 1) * kRelayThreads;
    std::vector<uint32_t> bcnt(l.boost.cap * per);
    HIP_TRY(hipMemcpy(bcnt.data(), area + l.boost_at() + relay_layout(l.boost.cap, l.boost.k, l.boost.slots).rcount, bcnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < n_split; e++) {
        if (bslot[e] > l.boost.cap) continue;
        const uint32_t *v = bslot[e] ? &bcnt[(size_t)(bslot[e] - 1) * per] : &cnt[e * per_base];
        for (size_t i = 0; i < (bslot[e] ? per : per_base); i++) *parked_values += (int64_t)v[i];
    }
    return CGRT_OK;
}
// promotion in the last launch: the head of the boost part and, where asked for, bslot of the relayed entries
static int last_relay_boost(const TileOrderState &o, const RelayState &r, int64_t *promoted, int32_t *k_boost, int64_t *boost_cap, uint64_t *cost_sum,
                            int32_t *num, int32_t *den, int32_t *wg_slots, uint32_t *bslot, int64_t slot_cap) {
    *promoted = *boost_cap = 0;
    *k_boost = *num = *den = *wg_slots = 0;
    *cost_sum = 0;
    if (o.boost.k == 0 || r.last.boost.k == 0 || o.start_words == 0 || o.tiles == 0) return CGRT_OK;
    uint32_t plan[kOrderClasses + 1], head[kBoostHead];
    if (int rc = o.read_plan(plan)) return rc;
    if (int rc = o.read(o.at.boost, head, kBoostHead)) return rc;
    *promoted = (int64_t)head[kBoostPromoted];
    *k_boost = (int32_t)o.boost.k;
    *boost_cap = (int64_t)o.boost.cap;
    *cost_sum = (uint64_t)head[kBoostS] | (uint64_t)head[kBoostS + 1] << 32;
    *num = (int32_t)o.boost.num;
    *den = (int32_t)o.boost.den;
    *wg_slots = (int32_t)o.boost.slots;
    const size_t n_split = relay_split_entries(plan[2], plan[3], (uint32_t)r.last.base.cap, r.last.extent);
    if (bslot && n_split > 0 && slot_cap >= (int64_t)n_split) return o.read(o.at.bslot, bslot, n_split);
    return CGRT_OK;
}
// the start table of the last launch, its wave tiles' probe costs and the workgroups it ordered
static int last_relay_start(const TileOrderState &o, const RelayState &r, uint32_t *start, int64_t start_cap, uint32_t *wcost, int64_t cost_cap,
                            int64_t *t, int64_t *n_wave_tiles, int32_t *reused) {
    *t = *n_wave_tiles = 0;
    *reused = 0;
    if (o.start_words == 0 || o.tiles == 0 || !r.last.relays()) return CGRT_OK;
    uint32_t plan[kOrderClasses + 1];
    if (int rc = o.read_plan(plan)) return rc;
    size_t n = relay_items_total(r.last.items(plan[2], plan[3], plan[kOrderClasses]));
    const bool boosted = o.boost.k != 0 && r.last.boost.k != 0;  // the promoted form's table: its own part, its count in the head
    if (boosted) {
        uint32_t head[kBoostHead];
        if (int rc = o.read(o.at.boost, head, kBoostHead)) return rc;
        n = head[kBoostItems];
    }
    if (n > (boosted ? o.at.bstart.bytes / sizeof(uint32_t) : o.start_words))
        return fail(CGRT_ERR_DEVICE, "relay start table: more workgroups than the table holds");
    *t = (int64_t)n;
    *n_wave_tiles = (int64_t)o.start_wtiles;
    *reused = o.start_reused ? 1 : 0;
    if (start && start_cap >= (int64_t)n && n > 0)
        if (int rc = o.read(boosted ? o.at.bstart : o.at.start, start, n)) return rc;
    if (wcost && cost_cap >= (int64_t)o.start_wtiles && o.start_wtiles > 0)
        if (int rc = o.read(o.at.wcost, wcost, o.start_wtiles)) return rc;
    return CGRT_OK;
}
static void last_relay_form(const TileOrderState &o, const RelayState &r, int32_t *mirror, int32_t *order) {
    const bool relayed = r.last.relays() && o.tiles != 0;
    *mirror = relayed ? (r.last.extent == kRelayMirror ? 1 : 0) : -1;
    *order = relayed ? r.last.order : -1;
}

#endif
