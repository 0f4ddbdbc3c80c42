// libcgrt.so -- gfx950 (MI355X, CDNA4) kernels and the C ABI of include/cgrt.h.
//
// One kernel, trace_grid_kernel, replaces the reference's serial pixel/sample loop (main.cpp:185-219) and
// the recursive trace() under it (main.cpp:42-100,129-157):
//   * a workgroup = 4 wavefronts = a 32x8 pixel tile; each wave owns a 16x4 sub-tile, one pixel per lane;
//   * the top-level object list (`objs`, main.cpp:277) is staged once per workgroup in LDS and walked by all
//     64 lanes in lockstep (kind is wave-uniform, so the type dispatch is a scalar branch, not a virtual call);
//   * recursion is an explicit per-lane stack of pending refracted rays (<= 4 entries: depth budget 5) and a
//     lane that finishes a sample's ray tree immediately starts its next sample (persistent-lane loop);
//   * all geometry is fp64 with FMA contraction disabled, so hit decisions are the reference's decisions;
//   * the per-pixel accumulator is summed in fp64 in the reference's own order, scaled by 1/spp, rounded once
//     to fp32 and written through an LDS transpose as 384-byte contiguous row segments.
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build()).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/cgrt.h"
#include "cgrt_build.h"
#include "cgrt_refit_plan.h"
#include "cgrt_rng.hpp"
#include "cgrt_types.h"

// device code, in dependency order
#include "cgrt_device_math.hpp"
#include "cgrt_grid.hpp"
#include "cgrt_traverse.hpp"
#include "cgrt_bezier.hpp"
#include "cgrt_scene_walk.hpp"
#include "cgrt_eye.hpp"
#include "cgrt_primwalk.hpp"
#include "cgrt_rays.hpp"
#include "cgrt_occlusion.hpp"
#include "cgrt_bounce.hpp"
#include "cgrt_wavefront.hpp"
#include "cgrt_hit_attr.hpp"

using namespace cgrt;

// =====================================================================================================
// host side: scene handle, upload, C ABI
// =====================================================================================================
// Grow-only device scratch, reused by later launches or batches (hipFree synchronises, so it is not freed per use): a larger
// request frees it and allocates the new size; a failed one leaves it empty
struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    ~GrowBuf() { release(); }
    hipError_t need(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(CGRT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Every entry point that works on a scene's device switches to it for the duration of the call only: one host thread may
// drive several GPUs (or run under a framework with its own current device) and must find its device unchanged afterwards.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = (err == hipSuccess);
        }
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define ON_DEVICE(dev)          \
    DeviceGuard dev_guard_(dev); \
    if (dev_guard_.err != hipSuccess) return fail(CGRT_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(dev_guard_.err))

struct DevBuf {  // RAII for device temporaries: freed on every return path
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    void *release() { void *q = p; p = nullptr; return q; }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};
// Host staging of a *_host entry point: device copies of its inputs, device room for its outputs, and after the call the wait
// and the copies back.  A failed allocation or upload is kept (error()) and makes the later ones no-ops; all is freed on return.
class HostStage {
    struct Back { void *host; const void *dev; size_t bytes; };
    std::vector<void *> bufs;
    std::vector<Back> backs;
    int rc_ = CGRT_OK;
    void *alloc(size_t bytes, const void *from, bool zeroed) {
        void *p = nullptr;
        if (rc_) return nullptr;
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) bufs.push_back(p);
        if (e == hipSuccess && from) e = hipMemcpy(p, from, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && zeroed) e = hipMemset(p, 0, bytes);
        if (e != hipSuccess) rc_ = fail(CGRT_ERR_DEVICE, std::string("host staging: ") + hipGetErrorString(e));
        return rc_ ? nullptr : p;
    }
public:
    HostStage() = default;
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage() { for (void *p : bufs) (void)hipFree(p); }
    int error() const { return rc_; }
    // the device copy of `bytes` at host (nullptr where host is: an optional input stays null)
    template <class T> T *in(const T *host, size_t bytes) { return host ? static_cast<T *>(alloc(bytes, host, false)) : nullptr; }
    // device room for an output, copied to host by finish (nullptr where host is: an optional output stays null) ...
    template <class T> T *out(T *host, size_t bytes, bool zeroed = false) { return host ? out_always(host, bytes, zeroed) : nullptr; }
    // ... and for one the kernels write whether the caller wants it or not
    template <class T> T *out_always(T *host, size_t bytes, bool zeroed = false) {
        T *p = static_cast<T *>(alloc(bytes, nullptr, zeroed));
        if (p && host) backs.push_back({host, p, bytes});
        return p;
    }
    // after the call that returned rc: waits for the kernels and, only if all went well, copies the outputs back
    int finish(int rc) {
        if (rc == CGRT_OK) {
            const hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) rc = fail(CGRT_ERR_DEVICE, std::string("kernel: ") + hipGetErrorString(e));
        }
        if (rc == CGRT_OK)
            for (const Back &b : backs) HIP_TRY(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
        return rc;
    }
};

#include "cgrt_tile_order.hpp"

#include "cgrt_mesh_bounds.hpp"
#include "cgrt_devbuild.hpp"

// What refits and rebuilds of one mesh object keep on the handle (cgrt_mesh_edit.hpp): a scene that never edits a mesh pays nothing
struct RefitNode {
    int32_t parent, slot, need, pad;  // RefitPlan::parent, ::slot, ::arrivals
};
struct RefitPlanDev {  // the plan (cgrt_refit_plan.h) and its device copy behind the words every refit clears on its stream
    RefitPlan plan;
    DevBuf mem;  // [keys | arrival counters] [nodes] [src, rec]
    size_t bytes = 0, clear_bytes = 0;
    unsigned long long *keys = nullptr;
    int *arrive = nullptr;
    const RefitNode *nodes = nullptr;
    const int2 *srcrec = nullptr;
};
struct MeshEdit {
    std::unique_ptr<RefitPlanDev> plan;  // built by the mesh's first refit; a rebuild changes the topology and resets it
    int64_t refits = 0;
    double ms_plan = 0;  // wall-clock of building and uploading the plan (the read-backs of that refit included)
    devbuild::MeshScratch scratch;  // the builder's scratch with staging records, allocated by the mesh's first rebuild
    int64_t rebuilds = 0;
    int32_t balanced = 0, levels = 0, readbacks = 0;  // what the last rebuild did
    double ms_last = 0;
};

struct cgrt_scene {
    HostScene host;
    bool committed = false;
    int device = -1;
    DeviceScene dev{};
    std::vector<void *> allocs;
    int64_t device_bytes = 0;
    // launch scratch (chunk sums, schedule, deferred Hitpoint values: ScratchLayout); reused by later launches on this handle
    // (launches on one handle are ordered by the caller: cgrt.h, "Threading")
    mutable GrowBuf scratch;
    mutable size_t scratch_refused = 0;  // smallest scratch size this device has refused (0: none yet): not asked for again
    // what a sphere scene's tile-order launches keep on the handle (cgrt_tile_order.hpp)
    mutable TileOrderState order;
    mutable RelayState relay;
    mutable LensTableState lens;
    size_t mem_total = 0;                // memory of the scene's device (read at commit; bounds the deferred-value budget)
    int n_cu = 256;                      // compute units of the scene's device (read at commit; wave slots of the scheduler)
    // second stream + fork/join events for the light-tile launch that runs beside the full one (created at commit)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    cgrt_build_info build_info{};  // filled by cgrt_scene_commit
    std::vector<TreeRec> tree_recs;  // host copy of dev.trees (where a device-built tree's records live)
    // cgrt_ray_hit_attributes' prim: per record of dev.tris the triangle's index in its tree's construction order.  Built and
    // uploaded by the first call that asks for prim (a scene that never asks pays nothing); immutable afterwards
    mutable GrowBuf tri_ids;
    // cgrt_wavefront_rays: ray queues and parked Hitpoints, the sort's temporary storage, and what the last call did
    mutable GrowBuf wavefront_work, wavefront_sort;
    mutable WavefrontLast wavefront_last;
    // the eye kernels the last eye pass on the handle launched (launch_eye, primary_walk), probes included: host state, cleared
    // by every entry point that runs an eye pass, read by cgrt_scene_last_eye_launches
    mutable EyeLaunchLog eye_log;
    // cgrt_scene_refit_mesh, cgrt_scene_rebuild_mesh: per edited mesh object its record, and the count of edits of the scene:
    // the photon-mapping sessions remember the one they were created under
    std::map<int, MeshEdit> edits;
    uint64_t geometry_gen = 0;
    // cgrt_scene_mesh_cost: one partial sum per workgroup of tree_cost_kernel
    mutable GrowBuf cost_partials;
};

template <class T>
static int upload(cgrt_scene *s, const std::vector<T> &v, const T **out, size_t extra = 0) {  // extra: records of room behind v
    *out = nullptr;
    size_t bytes = (v.size() + extra) * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);  // keep pointers non-null
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    s->allocs.push_back(p);
    s->device_bytes += (int64_t)bytes;
    if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const T *>(p);
    return CGRT_OK;
}

#include "cgrt_mesh_edit.hpp"

extern "C" {

int cgrt_version(void) { return CGRT_VERSION; }

int cgrt_look_at(const double eye[3], const double target[3], const double up_hint[3], double fov_x_deg, double focus_distance,
                 double lens_radius, cgrt_posed_camera *out) {
    if (!eye || !target || !up_hint || !out) return fail(CGRT_ERR_INVALID, "cgrt_look_at: null argument");
    if (const char *bad = look_at_camera(eye, target, up_hint, fov_x_deg, focus_distance, lens_radius, out)) return fail(CGRT_ERR_INVALID, bad);
    return CGRT_OK;
}
const char *cgrt_last_error(void) { return g_err.c_str(); }

int cgrt_scene_create(cgrt_scene **out) {
    if (!out) return fail(CGRT_ERR_INVALID, "cgrt_scene_create: null out");
    *out = new (std::nothrow) cgrt_scene();
    if (!*out) return fail(CGRT_ERR_INVALID, "out of memory");
    // CGRT_BUILD=device: the default of cgrt_scene_set_build for scenes created from now on (row f3)
    if (const char *e = std::getenv("CGRT_BUILD")) (*out)->host.build_mode = std::strcmp(e, "device") == 0 ? CGRT_BUILD_DEVICE : CGRT_BUILD_HOST;
    return CGRT_OK;
}

void cgrt_scene_destroy(cgrt_scene *s) {
    if (!s) return;
    if (!s->allocs.empty() || s->scratch.p || s->order.buf.p || s->relay.buf.p || s->lens.buf.p || s->lens.ev || s->tri_ids.p || s->aux_stream || s->order.ev || s->relay.ev || !s->edits.empty() || s->cost_partials.p) {
        DeviceGuard g(s->device);
        if (g.err == hipSuccess) {
            for (void *p : s->allocs) (void)hipFree(p);
            s->scratch.release();
            s->order.release();
            s->relay.release();
            s->lens.release();
            s->tri_ids.release();
            s->edits.clear();
            s->cost_partials.release();
            if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
            if (s->ev_join) (void)hipEventDestroy(s->ev_join);
            if (s->aux_stream) (void)hipStreamDestroy(s->aux_stream);
        }
    }
    delete s;
}

#define NEED_OPEN(s)                                                          \
    if (!(s)) return fail(CGRT_ERR_INVALID, "null scene");                    \
    if ((s)->committed) return fail(CGRT_ERR_INVALID, "scene already committed")

static int added(cgrt_scene *s, int r) {
    if (r == -2) return fail(CGRT_ERR_IO, s->host.error);
    if (r < 0) return fail(CGRT_ERR_INVALID, s->host.error);
    if ((int)s->host.objs.size() > kMaxObjs) return fail(CGRT_ERR_LIMIT, "more than 2^20 top-level objects");
    return r;
}

int cgrt_scene_set_build(cgrt_scene *s, int mode) {
    NEED_OPEN(s);
    if (mode != CGRT_BUILD_HOST && mode != CGRT_BUILD_DEVICE) return fail(CGRT_ERR_INVALID, "unknown build mode");
    s->host.build_mode = mode;
    return CGRT_OK;
}
int cgrt_scene_build_info(const cgrt_scene *s, cgrt_build_info *out) {
    if (!s || !out) return fail(CGRT_ERR_INVALID, "null argument");
    *out = s->build_info;
    out->mode = s->host.build_mode;
    out->ms_host_build = s->host.host_build_ms;
    return CGRT_OK;
}

int cgrt_scene_add_sphere(cgrt_scene *s, const double c[3], double r, const double sc[3], double refl, double transp) {
    NEED_OPEN(s);
    if (!c || !sc) return fail(CGRT_ERR_INVALID, "null argument");
    return added(s, s->host.add_sphere(c, r, sc, refl, transp));
}
int cgrt_scene_add_texture(cgrt_scene *s, const uint8_t *rgb, int rows, int cols, const double n[3], const double p[3],
                           double lx, double ly, int isbump) {
    NEED_OPEN(s);
    if (!n || !p) return fail(CGRT_ERR_INVALID, "null argument");
    int r = s->host.add_texture(rgb, rows, cols, n, p, lx, ly, isbump);
    return r < 0 ? fail(CGRT_ERR_INVALID, s->host.error) : r;
}
int cgrt_scene_add_plane(cgrt_scene *s, const double p[3], const double n[3], const double sc[3], double refl,
                         double transp, int tex_id) {
    NEED_OPEN(s);
    if (!p || !n || !sc) return fail(CGRT_ERR_INVALID, "null argument");
    try {  // the tree build allocates and starts threads: nothing may unwind through the C ABI
        return added(s, s->host.add_plane(p, n, sc, refl, transp, tex_id));
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string("plane: ") + e.what());
    }
}
int cgrt_scene_add_mesh_file(cgrt_scene *s, const char *filename, double a, const double b[3], const double sc[3],
                             double refl, double transp, int typeofdata) {
    NEED_OPEN(s);
    if (!filename || !b || !sc) return fail(CGRT_ERR_INVALID, "null argument");
    try {
        return added(s, s->host.add_mesh_file(filename, a, b, sc, refl, transp, typeofdata));
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string("mesh: ") + e.what());
    }
}
int cgrt_scene_add_mesh_triangles(cgrt_scene *s, const double *tri9, int ntri, const double sc[3], double refl,
                                  double transp, int typeofdata) {
    NEED_OPEN(s);
    if (!sc) return fail(CGRT_ERR_INVALID, "null argument");
    try {
        return added(s, s->host.add_mesh_triangles(tri9, ntri, sc, refl, transp, typeofdata));
    } catch (const std::exception &e) {
        return fail(CGRT_ERR_LIMIT, std::string("mesh: ") + e.what());
    }
}
int cgrt_scene_add_bezier(cgrt_scene *s, const double *cp3, int ncp, const double pos[3], const double sc[3],
                          double refl, double transp) {
    NEED_OPEN(s);
    if (!pos || !sc) return fail(CGRT_ERR_INVALID, "null argument");
    return added(s, s->host.add_bezier(cp3, ncp, pos, sc, refl, transp));
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Row f3 (cgrt_devbuild.hpp): the device builds fill the room scene_layout() left behind the host-built records and finish what
// only they know -- a floor's height range; a mesh's 4-wide node count, bmax, bounding sphere and cover spheres (appended to H.cover)
static int device_builds(HostScene &H, SceneLayout &L, const DeviceScene &d) {
    int rc = CGRT_OK;
    for (size_t ti = 0; ti < H.trees.size(); ti++) {
        HostTree &t = H.trees[ti];
        TreeRec &tr = L.trees[ti];
        if (t.dev_kind == 2) {
            const HostTexture &tx = H.textures[(size_t)t.dev_tex];
            HFieldRec &hf = L.hfields[(size_t)tr.hfield];
            devbuild::BumpResult br;
            if ((rc = devbuild::build_bump_floor(d.texels + L.texs[(size_t)t.dev_tex].texel_begin, tx.rows, tx.cols, tx.p, tx.lenx,
                                                 tx.leny, t.dev_plane_y, const_cast<HCellRec *>(d.hcells) + hf.cell_begin,
                                                 const_cast<HCellY *>(d.hcell_y) + hf.cell_begin,
                                                 const_cast<TriRec *>(d.tris) + tr.tri_begin, br)))
                return rc;
            hf.ylo = br.ylo;
            hf.yhi = br.yhi;
            t.hfield.ylo = br.ylo;
            t.hfield.yhi = br.yhi;
        } else if (t.dev_kind == 1) {
            devbuild::MeshResult mr;
            const MeshSlots at = mesh_slots(d, tr, t.dev_obj, (int)ti, 0);
            if ((rc = devbuild::build_mesh_hierarchy(t.tri9.data(), (int)t.dev_ntri, at.tris, at.otris, at.wnodes, mr))) return rc;
            t.cover_first = H.cover.size() / 4;  // the spheres are appended: room for them first
            t.cover_n = (int)(mr.cover.size() / 4);
            H.cover.resize(H.cover.size() + mr.cover.size());
            apply_mesh_result(H, t, tr, t.dev_obj, mr);
        }
    }
    return CGRT_OK;
}

// every array of the scene, device builds included; fills d's pointers
static int upload_scene(cgrt_scene *s, SceneLayout &L, const CommitKnobs &k, DeviceScene &d, double &ms_device_build) {
    HostScene &H = s->host;
    int rc = CGRT_OK;
    // the large arrays first: the device builds write into the room behind the host-built records
    if ((rc = upload(s, L.nodes, &d.nodes))) return rc;
    if ((rc = upload(s, L.tris, &d.tris, L.room_tris))) return rc;
    if ((rc = upload(s, L.texels, &d.texels))) return rc;
    if ((rc = upload(s, L.hcells, &d.hcells, L.room_hcells))) return rc;
    if ((rc = upload(s, L.hcell_y, &d.hcell_y, L.room_hcells))) return rc;
    if ((rc = upload(s, L.otris, &d.otris, L.room_otris))) return rc;
    if ((rc = upload(s, L.tboxes, &d.tboxes))) return rc;
    if ((rc = upload(s, L.wnodes, &d.wnodes, L.room_wnodes))) return rc;
    if (L.n_dev_trees > 0) {
        const auto t_build0 = std::chrono::steady_clock::now();
        if ((rc = device_builds(H, L, d))) return rc;
        ms_device_build = ms_since(t_build0);
    }
    // then the ones the builds finish
    if ((rc = upload(s, H.objs, &d.objs))) return rc;
    if ((rc = upload(s, L.trees, &d.trees))) return rc;
    if ((rc = upload(s, L.texs, &d.texs))) return rc;
    if ((rc = upload(s, H.beziers, &d.beziers))) return rc;
    if ((rc = upload(s, H.bez_slabs, &d.bez_slabs))) return rc;
    if (k.no_bezier_cull) d.bez_slabs = nullptr;
    if ((rc = upload(s, L.hfields, &d.hfields))) return rc;
    if ((rc = upload(s, H.cover, &d.cover))) return rc;
    return CGRT_OK;
}

// the light-tile / diffuse-tile launch's stream and fork/join events; without them every tile is rendered by the full variant
// (diffuse: a sphere-only scene the tile order serves, whose class-3 tiles get the terminal-diffuse variant)
static void open_light_stream(cgrt_scene *s, AuxPriority priority, DeviceScene &d, bool diffuse) {
    if (!(d.light_ok || diffuse) || s->aux_stream) return;
    // the light launch yields to the scheduled one: lowest stream priority
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    const int prio = priority == AUX_SAME ? 0 : priority == AUX_HIGH ? prio_greatest : prio_least;
    if (hipStreamCreateWithPriority(&s->aux_stream, hipStreamNonBlocking, prio) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess) {
        // all three or none: aux_stream != nullptr is what the launches ask
        (void)hipGetLastError();
        if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
        if (s->ev_join) (void)hipEventDestroy(s->ev_join);
        if (s->aux_stream) (void)hipStreamDestroy(s->aux_stream);
        s->ev_fork = s->ev_join = nullptr;
        s->aux_stream = nullptr;
        d.light_ok = 0;
    }
}

// A commit that fails leaves the scene open, with no device memory and with H.cover as before (the device builds append to it):
// a later commit starts from scratch.
int cgrt_scene_commit(cgrt_scene *s, int device) {
    NEED_OPEN(s);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CGRT_ERR_DEVICE, "no such HIP device");
    ON_DEVICE(device);
    s->device = device;
    HostScene &H = s->host;
    const auto t_commit0 = std::chrono::steady_clock::now();
    const CommitKnobs knobs = commit_knobs();
    SceneLayout L = scene_layout(H, knobs);
    DeviceScene d{};
    double ms_device_build = 0;
    const size_t cover_host = H.cover.size();
    if (int rc = upload_scene(s, L, knobs, d, ms_device_build)) {
        for (void *p : s->allocs) (void)hipFree(p);
        s->allocs.clear();
        s->device_bytes = 0;
        s->device = -1;
        H.cover.resize(cover_host);
        return rc;
    }
    scene_traits(H, L.trees, knobs, d);
    {   // the spheres tile_order_kernel orders an image-order launch by
        OrderSpheres &os = s->order.spheres;
        os = OrderSpheres{};
        size_t special = 0;
        for (const ObjRec &o : H.objs) {
            if (o.kind != KIND_SPHERE || (o.refl < kEps && o.transp < kEps)) continue;
            if (special < (size_t)kOrderSpheresMax) {
                for (int k = 0; k < 3; k++) os.s[special][k] = o.a[k];
                os.s[special][3] = std::sqrt(o.s0);
                if (!(o.transp < kEps)) os.transp |= 1u << special;
            }
            special++;
        }
        os.n = (uint32_t)std::min(special, (size_t)kOrderSpheresMax);
        s->order.ok = !d.has_mesh && !d.has_bezier && special >= 1 && special <= (size_t)kOrderSpheresMax;
    }
    open_light_stream(s, knobs.aux_priority, d, s->order.ok && d.all_spheres != 0);
    s->dev = d;
    s->committed = true;
    static std::atomic<uint64_t> commits{0};
    s->order.commit_gen = ++commits;  // what an earlier commit left in the order buffer is not this scene's
    s->order.valid = false;
    s->tree_recs = std::move(L.trees);
    size_t fr = 0, tot = 0;
    s->mem_total = hipMemGetInfo(&fr, &tot) == hipSuccess ? tot : ((size_t)32 << 30);
    if (hipDeviceGetAttribute(&s->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || s->n_cu <= 0) {
        (void)hipGetLastError();
        s->n_cu = 256;
    }
    s->build_info.n_device_trees = L.n_dev_trees;
    s->build_info.ms_device_build = ms_device_build;
    s->build_info.ms_commit = ms_since(t_commit0);
    return CGRT_OK;
}

int cgrt_scene_get_stats(const cgrt_scene *s, cgrt_scene_stats *out) {
    if (!s || !out) return fail(CGRT_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    const HostScene &H = s->host;
    out->n_objects = (int32_t)H.objs.size();
    int64_t bytes = 0;
    for (auto &o : H.objs) {
        if (o.kind == KIND_SPHERE) { out->n_spheres++; bytes += 88; }
        if (o.kind == KIND_PLANE) { out->n_planes++; bytes += 100; }
        if (o.kind == KIND_MESH) out->n_meshes++;
        if (o.kind == KIND_BEZIER) { out->n_beziers++; bytes += 24 * 6 + 100; }
    }
    out->n_textures = (int32_t)H.textures.size();
    out->n_trees = (int32_t)H.trees.size();
    for (auto &t : H.trees) {
        if (t.dev_kind) {  // never built on the host: the counts the reference's tree over these triangles would have
            out->n_triangles += t.dev_ntri;
            out->n_nodes += ref_node_count(t.dev_ntri);
            continue;
        }
        out->n_triangles += (int64_t)t.tris.size();
        out->n_nodes += (int64_t)t.nodes.size();
    }
    bytes += 56 * out->n_nodes + 72 * out->n_triangles;
    for (auto &t : H.textures) bytes += 3 * (int64_t)t.rows * t.cols;
    out->scene_bytes_fp64 = bytes;
    out->device_bytes = s->device_bytes + (int64_t)s->scratch.cap + (int64_t)s->order.buf.cap + (int64_t)s->tri_ids.cap;  // uploaded scene + the handle's launch scratch (+ the hit-attribute table once asked for)
    for (const auto &e : s->edits)  // (+ the refit plans and the rebuilds' scratch)
        out->device_bytes += (int64_t)((e.second.plan ? e.second.plan->bytes : 0) + e.second.scratch.bytes);
    out->device_bytes += (int64_t)s->cost_partials.cap;
    out->committed = s->committed ? 1 : 0;
    return CGRT_OK;
}

int cgrt_scene_tree_sizes(const cgrt_scene *s, int t, int32_t *nnodes, int32_t *nleaftris, int32_t *ntris) {
    if (!s || t < 0 || t >= (int)s->host.trees.size()) return fail(CGRT_ERR_INVALID, "bad tree index");
    const HostTree &T = s->host.trees[t];
    // (a refitted tree: the reference's tree over the OLD vertices describes nothing any more -- empty, as for a device-built one)
    if (nnodes) *nnodes = T.refitted ? 0 : (int32_t)T.nodes.size();  // the reference's tree (fingerprints); the device hierarchy is T.bvh
    if (nleaftris) *nleaftris = T.refitted ? 0 : (int32_t)T.leaf_ids.size();
    if (ntris) *ntris = T.dev_kind ? (int32_t)T.dev_ntri : (int32_t)(T.tri9.size() / 9);  // device-built: no reference tree exists (0 nodes)
    return CGRT_OK;
}
int cgrt_scene_bvh_dump(const cgrt_scene *s, int t, int32_t *nnodes, float *box6, int32_t *skip_leaf2) {
    if (!s || t < 0 || t >= (int)s->host.trees.size()) return fail(CGRT_ERR_INVALID, "bad tree index");
    const HostTree &T = s->host.trees[t];
    if (nnodes) *nnodes = T.refitted ? 0 : T.bvh_nodes;
    for (size_t i = 0; i < (T.refitted ? 0 : T.bvh.size()); i++) {
        if (box6) {
            for (int k = 0; k < 3; k++) {
                box6[6 * i + k] = T.bvh[i].lo[k];
                box6[6 * i + 3 + k] = T.bvh[i].hi[k];
            }
        }
        if (skip_leaf2) {
            skip_leaf2[2 * i] = T.bvh[i].skip;
            skip_leaf2[2 * i + 1] = T.bvh[i].leaf;
        }
    }
    return CGRT_OK;
}
int cgrt_scene_wide_dump(const cgrt_scene *s, int t, int32_t *nwide, int32_t *stack_need, float *box24, int32_t *ref4) {
    if (!s || t < 0 || t >= (int)s->host.trees.size()) return fail(CGRT_ERR_INVALID, "bad tree index");
    const HostTree &T = s->host.trees[t];
    std::vector<WideNodeRec> from_device;
    const bool on_device = tree_lives_on_device(s, t);
    const int32_t n_device = on_device ? s->tree_recs[(size_t)t].nwide : 0;
    if (on_device && (box24 || ref4))
        if (const int rc = read_device_tree(s, t, &from_device, nullptr)) return rc;
    const std::vector<WideNodeRec> &wide = (T.dev_kind == 1 || on_device) ? from_device : T.wide;
    if (nwide) *nwide = on_device ? n_device : T.dev_kind == 1 ? T.dev_nwide : (int32_t)T.wide.size();
    if (stack_need) *stack_need = T.wide_stack;
    for (size_t i = 0; i < wide.size(); i++) {
        const WideNodeRec &w = wide[i];
        for (int k = 0; k < 4; k++) {
            if (box24) {
                float *q = box24 + (4 * i + (size_t)k) * 6;
                q[0] = w.lox[k]; q[1] = w.loy[k]; q[2] = w.loz[k];
                q[3] = w.hix[k]; q[4] = w.hiy[k]; q[5] = w.hiz[k];
            }
            if (ref4) ref4[4 * i + (size_t)k] = w.ref[k];
        }
    }
    return CGRT_OK;
}
int cgrt_scene_bvh_order(const cgrt_scene *s, int t, int32_t *tri_level, int32_t *order) {
    if (!s || t < 0 || t >= (int)s->host.trees.size()) return fail(CGRT_ERR_INVALID, "bad tree index");
    const HostTree &T = s->host.trees[t];
    if (tri_level) *tri_level = T.tri_level ? 1 : 0;
    if (order && tree_lives_on_device(s, t)) {  // built on the device: k = the triangle's construction index; refitted: the
        std::vector<OTriRec> ot;                // records the refit left, k as it was
        if (const int rc = read_device_tree(s, t, nullptr, &ot)) return rc;
        for (size_t j = 0; j < ot.size(); j++) order[j] = ot[j].k;
        return CGRT_OK;
    }
    if (order)
        for (size_t j = 0; j < T.otris.size(); j++) order[j] = T.otris[j].k;
    return CGRT_OK;
}
int cgrt_scene_tree_dump(const cgrt_scene *s, int t, int32_t *node_lr_size, int32_t *leaf_ids, double *bbox,
                         double *tri9) {
    if (!s || t < 0 || t >= (int)s->host.trees.size()) return fail(CGRT_ERR_INVALID, "bad tree index");
    const HostTree &T = s->host.trees[t];
    if (node_lr_size && !T.refitted) std::memcpy(node_lr_size, T.node_lr_size.data(), T.node_lr_size.size() * sizeof(int32_t));
    if (leaf_ids && !T.refitted) std::memcpy(leaf_ids, T.leaf_ids.data(), T.leaf_ids.size() * sizeof(int32_t));
    if (bbox && !T.refitted) std::memcpy(bbox, T.bbox.data(), T.bbox.size() * sizeof(double));
    if (tri9) std::memcpy(tri9, T.tri9.data(), T.tri9.size() * sizeof(double));
    return CGRT_OK;
}

}  // extern "C"

#include "cgrt_refit.hpp"
#include "cgrt_rebuild.hpp"
#include "cgrt_tree_cost.hpp"

// ---- LDS of a launch ----
// A workgroup may use at most a CU's LDS (MI355X: 160 KiB): the kernel's static __shared__ bytes plus the dynamic bytes of
// the launch.  Each launch family's dynamic bytes come from one function of cgrt_variants.h, and every launch goes through
// launch_checked, which refuses a launch that would not fit (CGRT_ERR_LIMIT, naming the launch and the bytes) and asks for
// more than the default 64 KiB where needed.  The static bytes are the compiler's (hipFuncGetAttributes).
static_assert(sizeof(BezLds) == kBezLdsBytes, "cgrt_wg_lds.h: BezLds");
static_assert(sizeof(uint2) == 8 && sizeof(Pending) == kPendDoubles * sizeof(double) + 2 * sizeof(uint32_t), "cgrt_wg_lds.h: stack entries");

static size_t device_lds_bytes(int device) {
    static std::mutex mu;
    static std::map<int, size_t> known;
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || v <= 0) {
        (void)hipGetLastError();
        v = (int)kLdsBytes;
    }
    return known[device] = (size_t)v;
}
static size_t kernel_static_lds(const void *fn) {
    static std::mutex mu;
    static std::map<const void *, size_t> known;
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find(fn);
    if (it != known.end()) return it->second;
    hipFuncAttributes a{};
    size_t b = kStaticLdsAllowance;
    if (hipFuncGetAttributes(&a, fn) == hipSuccess) b = a.sharedSizeBytes;
    else (void)hipGetLastError();
    return known[fn] = b;
}
static int lds_check(const void *fn, size_t dyn, int device, const char *what) {
    const size_t st = kernel_static_lds(fn), lim = device_lds_bytes(device);
    if (st + dyn > lim)
        return fail(CGRT_ERR_LIMIT, std::string(what) + ": needs " + std::to_string(dyn) + " B of dynamic LDS + " + std::to_string(st) +
                                        " B static, more than the " + std::to_string(lim) + " B a workgroup may use");
    if (dyn > ((size_t)64 << 10) &&
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess)
        (void)hipGetLastError();  // not needed / not supported by this runtime: the launch itself will tell
    return CGRT_OK;
}
template <class T> struct same_type { using type = T; };
// Launches `fn` with `lds` bytes of dynamic LDS once lds_check has passed it (returns its error otherwise).  The attribute is
// per kernel; setting it again is harmless.  A failed launch shows in hipGetLastError, as with <<<...>>>.
template <class... P>
static int launch_checked(void (*fn)(P...), const char *what, int device, dim3 grid, dim3 block, size_t lds, hipStream_t st,
                          typename same_type<P>::type... args) {
    const void *k = reinterpret_cast<const void *>(fn);
    if (const int rc = lds_check(k, lds, device, what)) return rc;
    void *argv[] = {&args...};
    (void)hipLaunchKernel(k, grid, block, argv, lds, st);
    return CGRT_OK;
}

// A dispatch table's row for a variant's flags, by id() (the eye kernels' table below, the ray-list kernels' in
// cgrt_ray_queries.hpp); nullptr: no such instantiation was compiled
template <class Row, size_t N, class Flags>
static const Row *variant_row(const Row (&table)[N], const Flags &f) {
    for (const Row &e : table)
        if (e.id == f.id()) return &e;
    return nullptr;
}

// The instantiations of the eye kernels that are launched: CGRT_EYE_VARIANTS (cgrt_variants.h), expanded.
using GridKernel = void (*)(DeviceScene, GridParams, float *, uint32_t *, unsigned long long *, HitpointSink);
using SchedKernel = void (*)(DeviceScene, GridParams, float *, uint32_t *, unsigned long long *);
struct EyeKernels {
    int id;             // EyeFlags::id()
    GridKernel grid;    // trace_grid_kernel
    SchedKernel sched;  // trace_grid_sched_kernel where the scheduled form runs these flags, else nullptr
};
template <bool SCHED, bool T, bool B, bool D, bool G, bool P, bool S, int NT>
static constexpr SchedKernel sched_kernel() {
    if constexpr (SCHED) return &trace_grid_sched_kernel<T, B, D, G, P, S, NT>;
    else return nullptr;
}
#define CGRT_X(T, B, D, G, P, S, H, NT, SP, HF, DF, PR, ST, LT, SCHED)                                                                      \
    {EyeFlags{T != 0, B != 0, D != 0, G != 0, P != 0, S != 0, H != 0, SP != 0, HF != 0, NT, DF != 0, PR != 0, ST != 0, LT != 0}.id(),       \
     &trace_grid_kernel<T != 0, B != 0, D != 0, G != 0, P != 0, S != 0, H != 0, NT, SP != 0, HF != 0, DF != 0, PR != 0, ST != 0, LT != 0>, \
     sched_kernel<SCHED != 0, T != 0, B != 0, D != 0, G != 0, P != 0, S != 0, NT>()},
static const EyeKernels kEyeKernels[] = {CGRT_EYE_VARIANTS(CGRT_X)};
#undef CGRT_X
// ... and those of a posed launch: CGRT_EYE_POSED_VARIANTS, every one with POSE
template <bool SCHED, bool T, bool B, bool D, bool G, bool P, bool S, int NT>
static constexpr SchedKernel sched_posed_kernel() {
    if constexpr (SCHED) return &trace_grid_sched_kernel<T, B, D, G, P, S, NT, true>;
    else return nullptr;
}
#define CGRT_X(T, B, D, G, P, S, H, NT, SP, HF, DF, PR, ST, LT, SCHED)                                                                            \
    {EyeFlags{T != 0, B != 0, D != 0, G != 0, P != 0, S != 0, H != 0, SP != 0, HF != 0, NT, DF != 0, PR != 0, ST != 0, LT != 0, true}.id(),       \
     &trace_grid_kernel<T != 0, B != 0, D != 0, G != 0, P != 0, S != 0, H != 0, NT, SP != 0, HF != 0, DF != 0, PR != 0, ST != 0, LT != 0, true>, \
     sched_posed_kernel<SCHED != 0, T != 0, B != 0, D != 0, G != 0, P != 0, S != 0, NT>()},
static const EyeKernels kEyePosedKernels[] = {CGRT_EYE_POSED_VARIANTS(CGRT_X)};
#undef CGRT_X
static const EyeKernels *eye_kernels(const EyeFlags &f) { return f.pose ? variant_row(kEyePosedKernels, f) : variant_row(kEyeKernels, f); }

// Objects the most general variant (the Hitpoint capture, or the eye pass's SPILL form) keeps resident: the scene's n_lds when
// its list fits beside the variant's other LDS, else as many as fit beside one staging record per wave (the SPILL variant
// then reads the rest from `objs`).
static int general_resident(const cgrt_scene *s, bool dof, bool hps, bool posed) {
    const DeviceScene &d = s->dev;
    const EyeFlags gf = general_flags(dof, hps, true);
    const size_t st = kernel_static_lds(reinterpret_cast<const void *>(eye_kernels(posed ? posed_flags(gf) : gf)->grid));
    const size_t lim = device_lds_bytes(s->device);
    if (eye_lds(general_flags(dof, hps, d.n_objs > d.n_lds), d) + st <= lim) return d.n_lds;
    const long long room = (long long)lim - (long long)(st + eye_lds(general_flags(dof, hps, true), with_resident(d, 0)));
    return (int)std::max(0ll, std::min(room / (long long)sizeof(ObjRec), (long long)d.n_lds));
}

// ---- the eye pass's launch plan ----
// One launch of the eye pass: which kernel (form and template flags), the scene as it sees it and its dynamic LDS
struct EyeLaunch {
    EyeForm form;
    EyeFlags k;       // k.nt is the block size
    DeviceScene dev;  // the general variant's copy holds its resident objects (with_resident)
    size_t lds;       // dynamic LDS bytes
    const char *what() const {  // the launch's name in a refusal
        static const char *const names[] = {"eye pass", "eye pass", "eye pass, SPILL (spheres)", "eye pass, SPILL (general)",
                                            "Hitpoint capture", "eye pass, light tiles", "eye pass, light tiles (HFONLY)",
                                            "eye pass, diffuse tiles"};
        return form <= EyeForm::Sched && k.bez ? "eye pass (Bezier)" : names[(int)form];
    }
};

// The scene's inside spheres whose guarded loop pays (cgrt_inside_sphere.h): what a PAIR launch hands its kernel
static InsideTrait inside_paying(const DeviceScene &d) {
    InsideTrait t{};
    for (int k = 0; k < d.inside.n; k++)
        if (inside_pays(d.inside, k, d.n_lds)) {
            t.idx[t.n] = d.inside.idx[k], t.mask[t.n] = d.inside.mask[k], t.rin2[t.n] = d.inside.rin2[k];
            t.n++;
        }
    return t;
}

// The eye pass's main launch for (scene, camera, grid): the Hitpoint capture (capture), else cgrt_trace_grid's.
static EyeLaunch eye_launch(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const EyeKnobs &kn, bool capture) {
    const DeviceScene &d = s->dev;
    // which kernel: eye_choice (cgrt_variants.h), in plain C++ so that tests/native/posed_plan.cpp can walk it
    const EyeSceneTraits traits{d.all_spheres != 0, d.has_mesh != 0, d.has_bezier != 0, d.has_glass != 0, d.single_ray != 0, s->order.ok, d.n_objs, d.n_lds};
    const EyeChoice c = eye_choice(traits, *cam, *grid, kn.force_reorder, capture);
    EyeLaunch L;
    L.form = c.form;
    L.k = c.k;
    L.dev = d;
    if (L.form == EyeForm::Capture || L.form == EyeForm::SpillGen) {
        // the most general variant keeps as many objects resident as fit beside its other LDS, and spills only the rest
        L.dev = with_resident(d, general_resident(s, L.k.dof, capture, L.k.pose));
        L.k.spill = L.dev.n_objs > L.dev.n_lds;
    }
    // Inside trips (cgrt_inside_sphere.h): the PAIR kernels get the scene's candidates whose guarded loop pays -- none under
    // CGRT_GRID_NO_INSIDE_TRIPS or the knob CGRT_INSIDE_TRIPS=off, which is the pair loop alone in the same kernel
    L.dev.inside = InsideTrait{};
    if (L.k.pair && !(grid->flags & CGRT_GRID_NO_INSIDE_TRIPS) && !kn.no_inside_trips) L.dev.inside = inside_paying(d);
    L.lds = eye_lds(L.k, L.dev) + (L.form == EyeForm::Image || L.form == EyeForm::Sched ? (size_t)kn.lds_pad : 0);
    return L;
}
// The light tiles' launch beside the scheduled form (classify_kernel): bump-mapped planes take the tree-capable variant, or
// only its height-field walk where that is all they need (HFONLY: no node cache and no wide-walk stack in its LDS).
static EyeLaunch light_launch(const DeviceScene &d, bool dof, const EyeKnobs &kn) {
    const bool trees = d.light_trees != 0, hf = trees && d.light_hf_only && !kn.no_hfonly;
    EyeLaunch L;
    L.form = hf ? EyeForm::LightHF : EyeForm::Light;
    L.k = light_flags(trees, dof, hf);
    L.dev = d;
    L.lds = eye_lds(L.k, d);
    return L;
}
// The diffuse tiles' launch beside an image-order launch of a sphere-only scene (class 3 of tile_order_kernel's list): the
// terminal-diffuse variant, the object list its only LDS.  frame_plan decides when it is issued (TileOrderPlan::SecondLaunch).
static EyeLaunch diffuse_launch(const DeviceScene &d, bool dof) {
    EyeLaunch L;
    L.form = EyeForm::Diffuse;
    L.k = diffuse_flags(dof);
    L.dev = d;
    L.lds = eye_lds(L.k, d);
    return L;
}
static void diffuse_name(const EyeLaunch &L, char *name, size_t cap) {
    std::snprintf(name, cap, "trace_grid_kernel<TREES=0,BEZ=0,DOF=%d,GLASS=0,SPH=1,STATS=0,HPS=0,NT=%d,DIFF=1>", (int)L.k.dof, L.k.nt);
}
// What launch_eye would refuse, asked ahead of a launch that must not be left half issued
static int check_eye(const EyeLaunch &L, int device) {
    const EyeKernels *e = eye_kernels(L.k);
    if (!e) return fail(CGRT_ERR_UNSUPPORTED, std::string(L.what()) + ": no kernel built for this variant");
    return lds_check(reinterpret_cast<const void *>(e->grid), L.lds, device, L.what());
}
// Launches the plan's kernel on the scene's device: trace_grid_sched_kernel when `sched`, else trace_grid_kernel.  A launch that
// went out is noted in the handle's eye_log.
static int launch_eye(const EyeLaunch &L, bool sched, const cgrt_scene *s, const GridParams &g, dim3 gd, hipStream_t st, float *rgb,
                      uint32_t *nhit, unsigned long long *cnt, HitpointSink sink = HitpointSink{nullptr, nullptr, 0}) {
    const dim3 block((unsigned)L.k.nt);
    const EyeKernels *e = eye_kernels(L.k);
    if (!e || (sched && !e->sched)) return fail(CGRT_ERR_UNSUPPORTED, std::string(L.what()) + ": no kernel built for this variant");
    const int rc = sched ? launch_checked(e->sched, L.what(), s->device, gd, block, L.lds, st, L.dev, g, rgb, nhit, cnt)
                         : launch_checked(e->grid, L.what(), s->device, gd, block, L.lds, st, L.dev, g, rgb, nhit, cnt, sink);
    if (rc == CGRT_OK) s->eye_log.add(sched ? kEyeSched : kEyeGrid, L.k);
    return rc;
}

// A grid's rows, samples and stripes and the camera's lens: what an eye pass reads (traced: spp_total and max_depth too) and
// what cgrt_camera_rays does
static int check_grid_rows(const cgrt_camera *cam, const cgrt_grid *g, bool traced) {
    if (g->width <= 0 || g->height <= 0 || g->rows <= 0) return fail(CGRT_ERR_INVALID, "empty grid");
    if (g->spp <= 0 || (traced && g->spp_total <= 0) || g->sample_offset < 0) return fail(CGRT_ERR_INVALID, "bad sample range");
    if (traced && (g->max_depth < 1 || g->max_depth > kMaxDepth)) return fail(CGRT_ERR_INVALID, "max_depth must be 1..5");
    if (g->stripe_nranks > 1) {
        if (g->stripe_rows <= 0 || g->stripe_rows % kTileH != 0)
            return fail(CGRT_ERR_INVALID, "stripe_rows must be a positive multiple of 8");
        if (g->stripe_rank < 0 || g->stripe_rank >= g->stripe_nranks) return fail(CGRT_ERR_INVALID, "bad stripe_rank");
    } else if (g->row_offset < 0) {
        return fail(CGRT_ERR_INVALID, "bad row_offset");
    }
    if (!(cam->lens_radius >= 0)) return fail(CGRT_ERR_INVALID, "lens_radius must be >= 0");
    if (const char *bad = pose_error(cam, g)) return fail(CGRT_ERR_INVALID, bad);  // CGRT_GRID_POSED: cam is a cgrt_posed_camera's base
    return CGRT_OK;
}
static int check_grid(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *g) {
    if (!s || !cam || !g) return fail(CGRT_ERR_INVALID, "null argument");
    if (!s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    return check_grid_rows(cam, g, true);
}

// ---- cgrt_trace_grid's stages ----
// The plan whose scratch the handle holds.  A device short of memory gets a smaller deferred buffer (fewer heavy tiles, the
// same image) before it gets an error; every refused size is remembered (fit_heavy_tiles).
static int fit_scratch(const cgrt_scene *s, const FrameInputs &in, FramePlan &p) {
    p = frame_plan(in, fit_heavy_tiles(in, max_heavy_tiles(in), s->scratch_refused));
    while (s->scratch.need(p.scratch.total) != hipSuccess) {
        (void)hipGetLastError();
        if (!s->scratch_refused || p.scratch.total < s->scratch_refused) s->scratch_refused = p.scratch.total;
        if (p.kmax == 0) return fail(CGRT_ERR_DEVICE, "cannot allocate launch scratch (chunk sums / schedule / deferred Hitpoint values)");
        p = frame_plan(in, p.kmax / 2);
    }
    return CGRT_OK;
}

// What frame_plan needs of cgrt_trace_grid's launch L, as plain values
static FrameInputs frame_inputs(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const EyeLaunch &L, const EyeKnobs &kn) {
    const DeviceScene &d = s->dev;
    FrameInputs in{*grid, *cam, L.form == EyeForm::Sched, L.k.spill, L.k.stats, L.k.glass, L.k.nt, d.has_mesh != 0,
                   d.has_bezier != 0, d.prim_finish != 0, d.light_ok != 0, d.prim_obj, kn, s->mem_total, s->n_cu,
                   L.k.nt == 64 ? kBezWaves : (L.k.trees ? kSchedTreeWaves : 4)};
    in.image = L.form == EyeForm::Image;
    in.sph = L.k.sph;
    in.pair = L.k.pair;
    in.order_ok = s->order.ok;
    in.aux_stream = s->aux_stream != nullptr;
    in.all_spheres = d.all_spheres != 0;
    in.n_objs = d.n_objs;
    in.n_lds = d.n_lds;
    in.all_special = order_all_special(s->order.spheres, *cam);
    in.posed = L.k.pose;
    if (in.posed) in.posed_cam = *reinterpret_cast<const cgrt_posed_camera *>(cam);
    return in;
}

// Cost-aware scheduling ("classify -> probe -> plan -> render -> ordered sum"; DESIGN.md sections 4.6-4.7).  A frame's cost
// is concentrated in a few tiles (a glass mesh: one 32x8 tile ran 38 of the frame's 46 ms while four of the eight XCDs
// were idle after 6 ms), the hardware hands out workgroups in block-index order, and a tile is bound to one wave per
// 64 pixels.  So: (0) classify_kernel marks the LIGHT wave tiles (no primary ray can reach a mesh, a Bezier object or a
// reflecting / refracting sphere), which a lighter kernel variant renders on a second stream; (1) the full variant traces
// ONE sample of every other wave tile (16x4 pixels) storing nothing but the shader-clock ticks it took; (2) plan_kernel
// marks as HEAVY the tiles that alone would hold a wave slot for more than 1/heavy_div of the frame's ideal duration,
// orders them heaviest first, and lists the remaining tiles with something to render, costliest first; (3) the render
// launch serves the heavy tiles through a queue of (pixel, sample) units that any lane of any wave may take, and the
// other tiles through a queue of tiles, with persistent workgroups serving both (GridParams); (4) deferred_sum_kernel
// adds the heavy tiles' Hitpoint values in the reference's order.  The image does not depend on any of this -- every
// Hitpoint value is added to its pixel in sample order, emission order within a sample --: identical bits and counters;
// the probe costs 1/spp of the frame and the whole scheme is skipped below 4 samples per pixel or on request
// (CGRT_GRID_NO_REORDER); eye_launch decides it.  Here (0) to (2); g: the frame's GridParams before the scratch is placed.
static int probe_and_plan(const cgrt_scene *s, const EyeLaunch &L, const EyeKnobs &kn, const FramePlan &p, const GridParams &g,
                          unsigned char *scratch, hipStream_t st, float *rgb, uint32_t *nhit, unsigned long long *cnt) {
    const ScratchLayout &at = p.scratch;
    unsigned char *light = at.light.in<unsigned char>(scratch);  // nullptr: no light split
    if (light)
        hipLaunchKernelGGL(classify_kernel, dim3((unsigned)((p.n_wt + 255) / 256)), dim3(256), 0, st, s->dev, g, light, (int)p.n_wt);
    GridParams gp = g;  // the probe: this launch's first sample, natural order, one workgroup per tile, nothing stored
    gp.spp = gp.chunks = gp.chunk_spp = 1;
    gp.probe = 1;
    gp.cost = at.cost.in<uint32_t>(scratch);
    gp.light = light;  // light tiles are not probed (plan_kernel counts them as zero); their cost entries stay unwritten
    int rc = launch_eye(L, false, s, gp, dim3((unsigned)p.tile_blocks), st, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (light) {
        // The light tiles: the variant without tree / Bezier / pending-ray code on the second stream, beside everything that
        // follows here.  It needs nothing but the classification and starts as soon as the probe is through, beside the
        // plan (one workgroup, 0.1-0.3 ms).  Started before the probe it perturbs the measured costs and delays the
        // probe's workgroups: C3 14.4 -> 14.1 ms but C4 (spp 64) 33.6 -> 35.3 ms.
        GridParams gl = g;
        gl.light = light;
        gl.light_mode = 1;
        gl.xcd_tiles = 0;
        HIP_TRY(hipEventRecord(s->ev_fork, st));
        HIP_TRY(hipStreamWaitEvent(s->aux_stream, s->ev_fork, 0));
        if ((rc = launch_eye(light_launch(s->dev, L.k.dof, kn), false, s, gl,
                             dim3((unsigned)tile_grid_blocks(g.W, g.rows, false)), s->aux_stream, rgb, nhit, cnt)))
            return rc;
        HIP_TRY(hipEventRecord(s->ev_join, s->aux_stream));
    }
    const int tw = L.k.nt == 64 ? 1 : kTileW / kWaveTileW, th = L.k.nt == 64 ? 1 : kTileH / kWaveTileH;  // wave tiles per tile
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(1024), 0, st, gp.cost, light, (int)p.n_wt, (unsigned)p.kmax, p.plan_div,
                       at.plan.in<uint32_t>(scratch), at.order.in<uint32_t>(scratch), at.hidx.in<int32_t>(scratch),
                       at.border.in<uint32_t>(scratch), p.wtiles_x, p.wtiles_y, tw, th);
    return CGRT_OK;
}

// The probe of the relay's start order by cost, between the two host steps of cgrt_tile_order.hpp (cost_start_begin,
// cost_start_rank): the START twin of the launch's own kernel, which the frame then runs too, over entries [0, plan[3]) of the
// list (kOrderFull: the workgroups beyond leave at once) with the first probe_spp samples of every pixel from sample 0, the
// launch's seed and depth, no relay, no lens table.
static EyeLaunch start_twin(EyeLaunch L) {
    L.k.start = true;
    return L;
}
// ... and of a launch with a lens table: the twin whose full and parking bodies read it (of the plain or of the START variant)
static EyeLaunch table_twin(EyeLaunch L) {
    L.k.ltab = true;
    return L;
}
static int relay_cost_start(const cgrt_scene *s, const EyeLaunch &L, const FramePlan &p, GridParams &g, hipStream_t st) {
    CostStart c;
    if (int rc = cost_start_begin(s->order, p.relay, g, st, c)) return rc;
    if (!c.wcost) return CGRT_OK;
    if (!c.have_cost) {
        GridParams gp = g;
        gp.probe = 2;
        gp.cost = c.wcost;
        gp.spp = gp.chunk_spp = p.relay.probe_spp;
        gp.sample_offset = 0;
        gp.accumulate = 0;
        gp.tile_order = kOrderFull;
        gp.relay = nullptr;
        gp.relay_k = 0;
        gp.relay_start_at = gp.relay_boost_at = 0;
        // (L is the launch's kernel without a lens table: the probe draws its lens points by the loop -- its samples start at 0
        // whatever the launch's offset, and the table is mostly being written beside it; the counts are the same either way)
        gp.lens_table = nullptr;
        gp.lens_table_cap = gp.lens_table_spp = 0;
        if (int rc = launch_eye(start_twin(L), false, s, gp, dim3((unsigned)p.grid_dim), st, nullptr, nullptr, nullptr)) return rc;
    }
    return cost_start_rank(s->order, p, c, g, st);
}

// The heavy units' primary rays against the mesh, as a walk-only kernel with lane refill (cgrt_primwalk.hpp): a chip's worth
// of persistent workgroups at 4 waves per SIMD
static int primary_walk(const cgrt_scene *s, const EyeLaunch &L, const GridParams &g, hipStream_t st, unsigned long long *cnt) {
    PrimWalkArgs pw;
    pw.len = const_cast<double *>(g.prim_len);
    pw.tri = const_cast<int32_t *>(g.prim_tri);
    pw.obj = s->dev.prim_obj;
    pw.tree = s->host.objs[(size_t)s->dev.prim_obj].tree;
    pw.finish = g.prim_done;
    pw.pad_ = 0;
    pw.counters = cnt;
    const size_t staged = (size_t)(pw.finish ? s->dev.n_objs : pw.obj + 1);  // all objects when it finishes units
    const int rc = launch_checked(L.k.dof ? &primary_walk_kernel<true> : &primary_walk_kernel<false>, "primary_walk_kernel", s->device,
                                  dim3((unsigned)s->n_cu * 4), dim3(kThreads), primary_walk_lds(staged), st, s->dev, g, pw);
    if (rc == CGRT_OK) {
        EyeFlags walk{};  // (its one template flag)
        walk.dof = L.k.dof;
        s->eye_log.add(kEyePrimaryWalk, walk);
    }
    return rc;
}

// development aid: CGRT_TIMELINE_FILE=path makes a launch synchronous and dumps, per workgroup, when and where it ran
// (GridParams::timeline), behind a header {workgroups, threads per workgroup, chunks, xcd_tiles} (tools/timeline_probe.py)
static int write_timeline(const char *file, const DevBuf &tl, size_t n_blocks, const GridParams &g, int nt, hipStream_t st) {
    std::vector<unsigned long long> rec(n_blocks * 4);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(rec.data(), tl.p, rec.size() * 8, hipMemcpyDeviceToHost));
    if (FILE *f = std::fopen(file, "wb")) {
        // (a relaying launch: relay_k << 32 | extent << 40 | order << 41 | relay_cap in the xcd_tiles word, which is 0 for every
        // tile-order launch)
        const unsigned long long form = (unsigned long long)g.relay_k | (unsigned long long)g.relay_extent << 8 | (unsigned long long)g.relay_order << 9;
        const unsigned long long head[4] = {n_blocks, (unsigned long long)nt, (unsigned long long)g.chunks,
                                            g.relay_k > 1 ? (form << 32 | (unsigned long long)g.relay_cap) : (unsigned long long)g.xcd_tiles};
        std::fwrite(head, 8, 4, f);
        std::fwrite(rec.data(), 8, rec.size(), f);
        std::fclose(f);
    }
    return CGRT_OK;
}
// development aid: CGRT_PLAN_DUMP=1 makes a scheduled launch synchronous and prints what the planner decided
static int dump_plan(const FramePlan &p, const GridParams &g, hipStream_t st) {
    uint32_t pl[8] = {0};
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(pl, g.plan, sizeof(pl), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "cgrt plan: wave tiles %zu, heavy %u (capacity %zu), cost threshold %u, tile-queue entries %u, items per tile %d, prim walk %s\n",
                 p.n_wt, pl[0], p.kmax, pl[1], pl[3], g.items_per_tile, g.prim_len ? "on" : "off");
    return CGRT_OK;
}

extern "C" {

int cgrt_trace_grid_variant(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, char *name, size_t cap) {
    int rc = check_grid(s, cam, grid);
    if (rc) return rc;
    if (!name || cap == 0) return fail(CGRT_ERR_INVALID, "null name buffer");
    ON_DEVICE(s->device);
    // CGRT_GRID_HITPOINTS: the Hitpoint capture's launch
    const EyeLaunch L = eye_launch(s, cam, grid, eye_knobs(), (grid->flags & CGRT_GRID_HITPOINTS) != 0);
    const EyeFlags &k = L.k;
    const bool sched = L.form == EyeForm::Sched;
    if (!eye_kernels(k)) return fail(CGRT_ERR_UNSUPPORTED, std::string(L.what()) + ": no kernel built for this variant");
    std::snprintf(name, cap, "trace_grid_%skernel<TREES=%d,BEZ=%d,DOF=%d,GLASS=%d,SPH=%d,STATS=%d,%s%sNT=%d%s%s>", sched ? "sched_" : "",
                  (int)k.trees, (int)k.bez, (int)k.dof, (int)k.glass, (int)k.sph, (int)k.stats,
                  sched ? "" : (k.hps ? "HPS=1," : "HPS=0,"), k.pair ? "PAIR=1," : "", k.nt, k.spill ? ",SPILL=1" : "", k.pose ? ",POSE=1" : "");
    return CGRT_OK;
}

int cgrt_trace_grid(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, float *rgb, uint32_t *nhit,
                    uint64_t *counters, void *stream) {
    int rc = check_grid(s, cam, grid);
    if (rc) return rc;
    if (!rgb) return fail(CGRT_ERR_INVALID, "null rgb");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto *cnt = reinterpret_cast<unsigned long long *>(counters);
    // launch on the scene's device whatever the caller's current device is (one host thread may drive several GPUs)
    ON_DEVICE(s->device);
    const EyeKnobs kn = eye_knobs();
    s->eye_log.clear();
    const EyeLaunch L0 = eye_launch(s, cam, grid, kn, false);
    if (L0.k.pose && (rc = check_eye(L0, s->device))) return rc;  // (not every form has a POSE kernel: refused before anything is launched)
    const FrameInputs in = frame_inputs(s, cam, grid, L0, kn);
    FramePlan p;
    if ((rc = fit_scratch(s, in, p))) return rc;
    GridParams g = frame_params(in, p);
    unsigned char *scratch = reinterpret_cast<unsigned char *>(s->scratch.p);
    if (p.heavy_blocks > 0 && (rc = probe_and_plan(s, L0, kn, p, g, scratch, st, rgb, nhit, cnt))) return rc;
    p.scratch.place(g, scratch, nhit != nullptr);
    size_t n_blocks = (size_t)p.heavy_blocks + p.grid_dim;
    TileOrderGuard guard(s->order, s->relay);
    LensTableGuard lens(s->lens, st);
    bool tabled = false;  // the launch reads the handle's lens table
    EyeLaunch L = L0;
    if (p.order.on) {  // the tiles that see a mirror or glass sphere first; where the plan says so, their samples relayed
        const Capturing capturing = stream_capturing(st);
        if ((rc = order_tiles(s->order, s->dev, p, g, kn.no_order_reuse, capturing, st))) return rc;
        // the lens draws of classes 0-2, ahead of the probe and the frame, which then run the kernel's table-reading twin
        // (written only beside the cost probe, unless the plan says always; a launch without a table runs the kernels without one)
        const bool beside_probe = p.relay.relays() && p.relay.start == kRelayStartCost && cost_probe_due(s->order, p.relay, g);
        if (p.order.lens_table_cap > 0 && (tabled = lens_table_prepare(s->lens, s->order, p, g, kn.no_order_reuse, beside_probe, capturing, st, s->aux_stream)))
            L = table_twin(L0);
        if (p.relay.relays() && relay_prepare(s->relay, p.relay, g, capturing, st)) {
            guard.relayed = &p.relay;
            if (p.relay.start == kRelayStartCost && (rc = relay_cost_start(s, L0, p, g, st))) return rc;
            // (with the promoted form's table: the promoted tiles' extra chunks too, as many as the boost area holds)
            n_blocks = p.relay.grid(p.grid_dim, g.relay_boost_at != 0);
        }
        if ((rc = lens_table_join(s->lens, st))) return rc;  // the frame reads the table
    }
    DevBuf timeline;
    if (kn.timeline_file) {
        HIP_TRY(timeline.alloc(n_blocks * 32));
        HIP_TRY(hipMemsetAsync(timeline.p, 0, n_blocks * 32, st));
        g.timeline = timeline.as<unsigned long long>();
    }
    if (p.heavy_blocks > 0) {  // (3) heavy workgroups in front, the tile workgroups behind them, one launch
        if (L.k.pose) hipLaunchKernelGGL(pixel_const_kernel<true>, dim3((unsigned)p.kmax), dim3(64), 0, st, g);
        else hipLaunchKernelGGL(pixel_const_kernel<false>, dim3((unsigned)p.kmax), dim3(64), 0, st, g);
        if (g.prim_len && (rc = primary_walk(s, L, g, st, cnt))) return rc;
        if ((rc = launch_eye(L, true, s, g, dim3((unsigned)n_blocks), st, rgb, nhit, cnt))) return rc;
    } else if (p.order.class3 == TileOrderPlan::SecondLaunch) {
        // The list's class 0-2 entries by this launch, its class-3 entries by the terminal-diffuse variant on the second stream,
        // started behind it (fork / join events, lowest priority: the arrangement of the light-tile launch).  Where class 3
        // begins is known on the device only: both launches span the list, workgroups beyond their part leave at once.
        const EyeLaunch DL = diffuse_launch(s->dev, L.k.dof);
        if ((rc = check_eye(DL, s->device))) return rc;  // before the main launch goes out with only its part of the list
        GridParams gd = g;
        g.tile_order = kOrderFull;
        gd.tile_order = kOrderDiffuse;
        HIP_TRY(hipEventRecord(s->ev_fork, st));
        if ((rc = launch_eye(L, false, s, g, dim3((unsigned)n_blocks), st, rgb, nhit, cnt))) return rc;
        HIP_TRY(hipStreamWaitEvent(s->aux_stream, s->ev_fork, 0));
        if ((rc = launch_eye(DL, false, s, gd, dim3((unsigned)n_blocks), s->aux_stream, rgb, nhit, cnt))) return rc;
        HIP_TRY(hipEventRecord(s->ev_join, s->aux_stream));
    } else {
        // The pair variant in tile order: the list's class-3 workgroups take the terminal-diffuse body inside this launch
        if (p.order.class3 == TileOrderPlan::InKernel) g.tile_order = kOrderAllDiffuse;
        // (a launch with a start table runs the variant that reads it: the twin of L's, the kernel its probe ran)
        if ((rc = launch_eye(g.relay_start_at ? start_twin(L) : L, false, s, g, dim3((unsigned)n_blocks), st, rgb, nhit, cnt))) return rc;
    }
    if (p.chunks > 1)
        hipLaunchKernelGGL(finalize_chunks_kernel, dim3((unsigned)(((size_t)g.rows * g.W + 255) / 256)), dim3(256), 0, st, g, rgb, nhit);
    if (p.heavy_blocks > 0) hipLaunchKernelGGL(deferred_sum_kernel, dim3((unsigned)p.kmax), dim3(64), 0, st, g, rgb, nhit);  // (4)
    if (g.light || p.order.class3 == TileOrderPlan::SecondLaunch) HIP_TRY(hipStreamWaitEvent(st, s->ev_join, 0));  // the caller's stream continues when both launches are done
    const hipError_t launch_err = hipGetLastError();
    if (g.timeline && launch_err == hipSuccess && (rc = write_timeline(kn.timeline_file, timeline, n_blocks, g, L.k.nt, st))) return rc;
    if (launch_err != hipSuccess) return fail(CGRT_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(launch_err));
    if ((rc = guard.commit(g, st))) return rc;
    if ((rc = lens.commit(tabled))) return rc;
    return kn.plan_dump && g.plan && !g.tile_order ? dump_plan(p, g, st) : CGRT_OK;
}

// what the last cgrt_trace_grid on the handle did (cgrt_tile_order.hpp)
#define NEED_COMMITTED(s, args_ok)                                           \
    if (!(s) || !(args_ok)) return fail(CGRT_ERR_INVALID, "null argument"); \
    if (!(s)->committed) return fail(CGRT_ERR_INVALID, "scene not committed")

int cgrt_scene_last_tile_order(const cgrt_scene *s, uint32_t *plan5, uint32_t *list, uint8_t *cls, int64_t cap, int64_t *n_tiles) {
    NEED_COMMITTED(s, n_tiles);
    ON_DEVICE(s->device);
    return last_tile_order(s->order, plan5, list, cls, cap, n_tiles);
}
int cgrt_scene_last_sphere_masks(const cgrt_scene *s, uint32_t *masks, int64_t cap, int64_t *n_wave_tiles) {
    NEED_COMMITTED(s, n_wave_tiles);
    ON_DEVICE(s->device);
    return last_sphere_masks(s->order, masks, cap, n_wave_tiles);
}
int cgrt_scene_last_sure_tiles(const cgrt_scene *s, uint8_t *sure, int64_t cap, int64_t *n_wave_tiles) {
    NEED_COMMITTED(s, n_wave_tiles);
    ON_DEVICE(s->device);
    return last_sure_tiles(s->order, sure, cap, n_wave_tiles);
}
int cgrt_scene_last_tile_order_reused(const cgrt_scene *s, int32_t *reused) {
    NEED_COMMITTED(s, reused);
    *reused = s->order.reused ? 1 : 0;
    return CGRT_OK;
}
int cgrt_scene_last_diffuse_tiles(const cgrt_scene *s, int64_t *n_tiles) {
    NEED_COMMITTED(s, n_tiles);
    ON_DEVICE(s->device);
    return last_class3_tiles(s->order, TileOrderPlan::SecondLaunch, n_tiles);
}
int cgrt_scene_last_inkernel_diffuse_tiles(const cgrt_scene *s, int64_t *n_tiles) {
    NEED_COMMITTED(s, n_tiles);
    ON_DEVICE(s->device);
    return last_class3_tiles(s->order, TileOrderPlan::InKernel, n_tiles);
}
int cgrt_scene_last_lens_stage(const cgrt_scene *s, int64_t *lds_tiles, int64_t *area_tiles) {
    NEED_COMMITTED(s, lds_tiles && area_tiles);
    ON_DEVICE(s->device);
    return last_lens_stage(s->order, lds_tiles, area_tiles);
}
int cgrt_scene_last_lens_table(const cgrt_scene *s, int64_t *entries, int64_t *capacity, int32_t *reused) {
    NEED_COMMITTED(s, entries && capacity && reused);
    ON_DEVICE(s->device);
    return last_lens_table(s->order, s->lens, entries, capacity, reused);
}
int cgrt_scene_inside_spheres(const cgrt_scene *s, int32_t *index, uint32_t *mask, double *rin2, int32_t cap, int32_t *n) {
    NEED_COMMITTED(s, n && (cap <= 0 || (index && mask && rin2)));
    const InsideTrait &t = s->dev.inside;
    *n = t.n;
    for (int k = 0; k < t.n && k < cap; k++) index[k] = t.idx[k], mask[k] = t.mask[k], rin2[k] = t.rin2[k];
    return CGRT_OK;
}
int cgrt_scene_last_sample_relay(const cgrt_scene *s, int64_t *tiles, int32_t *chunks, int64_t *parked_values) {
    NEED_COMMITTED(s, tiles && chunks && parked_values);
    ON_DEVICE(s->device);
    return last_sample_relay(s->order, s->relay, tiles, chunks, parked_values);
}
int cgrt_scene_last_relay_form(const cgrt_scene *s, int32_t *mirror, int32_t *order) {
    NEED_COMMITTED(s, mirror && order);
    last_relay_form(s->order, s->relay, mirror, order);
    return CGRT_OK;
}

int cgrt_scene_last_relay_start(const cgrt_scene *s, uint32_t *start, int64_t start_cap, uint32_t *wcost, int64_t cost_cap, int64_t *t,
                                int64_t *n_wave_tiles, int32_t *reused) {
    NEED_COMMITTED(s, t && n_wave_tiles && reused);
    ON_DEVICE(s->device);
    return last_relay_start(s->order, s->relay, start, start_cap, wcost, cost_cap, t, n_wave_tiles, reused);
}

int cgrt_scene_last_relay_boost(const cgrt_scene *s, int64_t *promoted, int32_t *k_boost, int64_t *boost_cap, uint64_t *cost_sum, int32_t *num,
                                int32_t *den, int32_t *wg_slots, uint32_t *bslot, int64_t slot_cap) {
    NEED_COMMITTED(s, promoted && k_boost && boost_cap && cost_sum && num && den && wg_slots);
    ON_DEVICE(s->device);
    return last_relay_boost(s->order, s->relay, promoted, k_boost, boost_cap, cost_sum, num, den, wg_slots, bslot, slot_cap);
}

int cgrt_scene_last_eye_launches(const cgrt_scene *s, int32_t *rows, int64_t cap, int64_t *n) {
    NEED_COMMITTED(s, n && (cap <= 0 || rows));
    const EyeLaunchLog &log = s->eye_log;
    *n = log.n;
    for (int i = 0; i < log.n && i < cap; i++) log.row(i, rows + (size_t)i * kEyeLogCols);
    return log.overflow ? fail(CGRT_ERR_LIMIT, "eye pass: more launches than the handle's record holds") : CGRT_OK;
}

int cgrt_trace_grid_diffuse_variant(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, char *name, size_t cap) {
    int rc = check_grid(s, cam, grid);
    if (rc) return rc;
    if (!name || cap == 0) return fail(CGRT_ERR_INVALID, "null name buffer");
    ON_DEVICE(s->device);
    const EyeKnobs kn = eye_knobs();
    const EyeLaunch L = eye_launch(s, cam, grid, kn, false);
    name[0] = 0;
    if (frame_plan(frame_inputs(s, cam, grid, L, kn), 0).order.class3 == TileOrderPlan::SecondLaunch)
        diffuse_name(diffuse_launch(s->dev, L.k.dof), name, cap);
    return CGRT_OK;
}

}  // extern "C"


// Row e: global row h of the frame = local row (stripe / nshares) * S + h % S of share stripe % nshares (the inverse of
// global_row()); one workgroup column per 256 floats of a row, blockIdx.y = the row.  Rows of absent shares are zeroed.
__global__ void unpermute_stripes_kernel(const float *__restrict__ shares, int n_present, int nshares, int row_floats, int S,
                                         int rows_local, float *__restrict__ frame) {
    const int h = blockIdx.y, x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= row_floats) return;
    const int stripe = h / S, share = stripe % nshares, j = (stripe / nshares) * S + h % S;
    float v = 0.f;
    if (share < n_present && j < rows_local) v = shares[((size_t)share * rows_local + (size_t)j) * row_floats + x];
    frame[(size_t)h * row_floats + x] = v;
}

// What both Hitpoint captures end with: wait for the kernel, read how many records it produced (*count; 0 on failure) and hand
// the buffer over (*d_rec_out, unless cap == 0)
static int capture_finish(const char *what, DevBuf &b_rec, DevBuf &b_cnt, uint64_t cap, double **d_rec_out, uint64_t *count) {
    *count = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(CGRT_ERR_DEVICE, std::string(what) + hipGetErrorString(e));
    unsigned long long n = 0;
    if (hipMemcpy(&n, b_cnt.p, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return fail(CGRT_ERR_DEVICE, "hitpoint count copy");
    *count = n;
    if (cap && d_rec_out) *d_rec_out = reinterpret_cast<double *>(b_rec.release());
    return CGRT_OK;
}
// and what both host entry points do with a capture's outcome: the count, the first `cap` records to the host, the buffer freed
static int hitpoints_to_host(int rc, double *d_rec, uint64_t n, double *hp10, uint64_t cap, uint64_t *count) {
    if (rc == CGRT_OK) {
        *count = n;
        const uint64_t m = n < cap ? n : cap;
        if (m && hipMemcpy(hp10, d_rec, (size_t)m * 10 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(CGRT_ERR_DEVICE, "hitpoint copy");
    }
    if (d_rec) (void)hipFree(d_rec);
    return rc;
}

// Eye pass with Hitpoint capture into a device buffer of `cap` records (10 doubles each); *count = hitpoints produced.
// *d_rec_out is hipMalloc'ed here (caller frees) unless cap == 0.
static int hitpoints_device(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, uint64_t cap,
                            double **d_rec_out, uint64_t *count) {
    s->eye_log.clear();
    GridParams g = grid_params(cam, grid);  // capture keeps one workgroup per tile
    g.accumulate = 0;
    g.xcd_tiles = (s->dev.has_mesh && !s->dev.has_bezier) ? 1 : 0;
    const size_t npx = (size_t)grid->rows * grid->width;
    DevBuf b_rgb, b_rec, b_cnt;
    HIP_TRY(b_rgb.alloc(npx * 3 * sizeof(float)));
    HIP_TRY(b_rec.alloc((cap ? cap : 1) * 10 * sizeof(double)));
    HIP_TRY(b_cnt.alloc(sizeof(unsigned long long)));
    float *d_rgb = b_rgb.as<float>();
    double *d_rec = b_rec.as<double>();
    unsigned long long *d_cnt = b_cnt.as<unsigned long long>();
    HIP_TRY(hipMemset(d_cnt, 0, sizeof(unsigned long long)));
    const EyeLaunch L = eye_launch(s, cam, grid, eye_knobs(), true);
    int rc = launch_eye(L, false, s, g, dim3((unsigned)tile_grid_blocks(g.W, g.rows, g.xcd_tiles != 0)), 0, d_rgb, nullptr,
                        nullptr, HitpointSink{d_rec, d_cnt, (unsigned long long)cap});
    if (rc) return rc;
    return capture_finish("hitpoint kernel: ", b_rec, b_cnt, cap, d_rec_out, count);
}

// caller-supplied rays: the ray-list kernels' table, launch path, checks and entry points
#include "cgrt_rays_plan.h"
#include "cgrt_ray_queries.hpp"
// grid AOVs: the first-hit feature buffers of a frame (kernel, plan, entry points)
#include "cgrt_aov.hpp"

extern "C" {

int cgrt_trace_grid_hitpoints(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, double *hp10,
                              uint64_t cap, uint64_t *count) {
    int rc = check_grid(s, cam, grid);
    if (rc) return rc;
    if (!count || (cap > 0 && !hp10)) return fail(CGRT_ERR_INVALID, "null output");
    ON_DEVICE(s->device);
    double *d_rec = nullptr;
    uint64_t n = 0;
    rc = hitpoints_device(s, cam, grid, cap, &d_rec, &n);
    return hitpoints_to_host(rc, d_rec, n, hp10, cap, count);
}

int cgrt_unpermute_stripes(const float *shares, int n_present, int nshares, int width, int height, int stripe_rows,
                           int rows_local, int channels, float *frame, void *stream) {
    if (!shares || !frame || width <= 0 || height <= 0 || channels <= 0 || nshares < 1 || n_present < 1 || n_present > nshares ||
        stripe_rows <= 0 || rows_local <= 0 || rows_local % stripe_rows)
        return fail(CGRT_ERR_INVALID, "cgrt_unpermute_stripes: bad argument");
    const int row_floats = width * channels;
    const dim3 grid((unsigned)((row_floats + 255) / 256), (unsigned)height);
    hipLaunchKernelGGL(unpermute_stripes_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), shares, n_present, nshares,
                       row_floats, stripe_rows, rows_local, frame);
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

int cgrt_trace_grid_host(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, float *rgb,
                         uint32_t *nhit, uint64_t *counters) {
    int rc = check_grid(s, cam, grid);
    if (rc) return rc;
    if (!rgb) return fail(CGRT_ERR_INVALID, "null rgb");
    ON_DEVICE(s->device);
    const size_t npx = (size_t)grid->rows * grid->width;
    HostStage hs;
    float *d_rgb = hs.out(rgb, npx * 3 * sizeof(float), true);
    uint32_t *d_nhit = hs.out_always(nhit, npx * sizeof(uint32_t), true);
    uint64_t *d_cnt = hs.out_always(counters, CGRT_NCOUNTERS * sizeof(uint64_t), true);
    if ((rc = hs.error())) return rc;
    return hs.finish(cgrt_trace_grid(s, cam, grid, d_rgb, d_nhit, d_cnt, nullptr));
}

int cgrt_intersect_rays(const cgrt_scene *s, int obj, const double *org3, const double *dir3, const uint64_t *keys,
                        int n, int32_t *hit, double *len, double *normal3) {
    if (!s || !s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    if (obj < 0 || obj >= s->dev.n_objs || n < 0 || !org3 || !dir3 || !hit || !len || !normal3)
        return fail(CGRT_ERR_INVALID, "bad argument");
    if (n == 0) return CGRT_OK;
    ON_DEVICE(s->device);
    HostStage hs;
    const double *d_o = hs.in(org3, (size_t)n * 24), *d_d = hs.in(dir3, (size_t)n * 24);
    const unsigned long long *d_keys = reinterpret_cast<const unsigned long long *>(hs.in(keys, (size_t)n * 8));
    int32_t *d_hit = hs.out(hit, (size_t)n * 4);
    double *d_len = hs.out(len, (size_t)n * 8), *d_n = hs.out(normal3, (size_t)n * 24);
    if (const int rc = hs.error()) return rc;
    hipLaunchKernelGGL(intersect_rays_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, s->dev, obj, d_o, d_d, d_keys, n,
                       d_hit, d_len, d_n);
    HIP_TRY(hipGetLastError());
    return hs.finish(CGRT_OK);
}

int cgrt_surface_colors(const cgrt_scene *s, int obj, const double *points3, int n, double *colors3) {
    if (!s || !s->committed) return fail(CGRT_ERR_INVALID, "scene not committed");
    if (obj < 0 || obj >= s->dev.n_objs || n < 0 || (n > 0 && (!points3 || !colors3))) return fail(CGRT_ERR_INVALID, "bad argument");
    if (n == 0) return CGRT_OK;
    ON_DEVICE(s->device);
    HostStage hs;
    const double *d_p = hs.in(points3, (size_t)n * 24);
    double *d_c = hs.out(colors3, (size_t)n * 24);
    if (const int rc = hs.error()) return rc;
    hipLaunchKernelGGL(surface_colors_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, s->dev, obj, d_p, n, d_c);
    HIP_TRY(hipGetLastError());
    return hs.finish(CGRT_OK);
}

// The arguments the two host tables share, checked: the items and the grid's tile arithmetic
static int relay_host_args(bool others_ok, int32_t k, int32_t chunk_spp, int32_t spp, int64_t cap, int32_t extent, int64_t n01, int64_t n012, int64_t n_tiles,
                           const uint32_t *list, const uint32_t *wcost, int32_t width, int32_t rows, RelayStartArgs &a) {
    if (!others_ok || !list || !wcost || k < 2 || k > kRelayMaxChunks || chunk_spp <= 0 || spp <= 0 || cap < 0 || width <= 0 || rows <= 0 ||
        n01 < 0 || n01 > n012 || n012 > n_tiles || (size_t)n_tiles >= kRelayStartMaxTiles || (extent != kRelayGlass && extent != kRelayMirror))
        return fail(CGRT_ERR_INVALID, "bad argument");
    const uint32_t tiles_y = (uint32_t)((rows + kTileH - 1) / kTileH);
    a.tiles_x = (uint32_t)((width + kTileW - 1) / kTileW);
    a.wtiles_x = (uint32_t)((width + kWaveTileW - 1) / kWaveTileW);
    a.wtiles_y = (uint32_t)((rows + kWaveTileH - 1) / kWaveTileH);
    if ((int64_t)a.tiles_x * tiles_y != n_tiles) return fail(CGRT_ERR_INVALID, "n_tiles is not the grid's tile count");
    for (int64_t e = 0; e < n012; e++)
        if (list[e] >= (uint32_t)n_tiles) return fail(CGRT_ERR_INVALID, "list names a tile beyond the grid");
    a.r = RelayItems{(uint32_t)k, (uint32_t)n01, (uint32_t)n012, (uint32_t)n_tiles, (uint32_t)std::min<int64_t>(cap, n_tiles), extent, chunk_spp, spp};
    return CGRT_OK;
}

int cgrt_relay_start_host(int32_t k, int32_t chunk_spp, int32_t spp, int64_t cap, int32_t extent, int64_t n01, int64_t n012, int64_t n_tiles,
                          const uint32_t *list, const uint32_t *wcost, int32_t width, int32_t rows, uint32_t *start, int64_t start_cap,
                          int64_t *t) {
    RelayStartArgs a;
    if (int rc = relay_host_args(t != nullptr, k, chunk_spp, spp, cap, extent, n01, n012, n_tiles, list, wcost, width, rows, a)) return rc;
    *t = (int64_t)relay_items_total(a.r);
    if (!start || start_cap < *t || *t == 0) return CGRT_OK;
    std::vector<uint64_t> weight((size_t)*t);
    relay_start_table(a.r, list, wcost, a.tiles_x, a.wtiles_x, a.wtiles_y, weight.data(), start);
    return CGRT_OK;
}

int cgrt_relay_boost_host(int32_t k, int32_t chunk_spp, int32_t spp, int64_t cap, int32_t extent, int64_t n01, int64_t n012, int64_t n_tiles,
                          const uint32_t *list, const uint32_t *wcost, int32_t width, int32_t rows, int32_t k_boost, int32_t boost_chunk_spp,
                          int64_t boost_cap, int32_t num, int32_t den, int32_t wg_slots, uint32_t *start, int64_t start_cap, uint32_t *bslot,
                          int64_t slot_cap, int64_t *t, int64_t *promoted, uint64_t *cost_sum) {
    const bool boost_ok = t && promoted && cost_sum && k_boost >= k && k_boost <= kRelayMaxChunks && boost_chunk_spp > 0 && boost_cap >= 0 && num >= 0 &&
                          (uint32_t)num <= kRelayBoostMaxTerm && den >= 1 && (uint32_t)den <= kRelayBoostMaxTerm && wg_slots >= 1;
    RelayStartArgs a;
    if (int rc = relay_host_args(boost_ok, k, chunk_spp, spp, cap, extent, n01, n012, n_tiles, list, wcost, width, rows, a)) return rc;
    const RelayItems &r = a.r;
    const RelayBoost b{(uint32_t)k_boost, (uint32_t)std::min<int64_t>(boost_cap, n_tiles), boost_chunk_spp, (uint32_t)num, (uint32_t)den, (uint32_t)wg_slots};
    const size_t n_split = relay_split_entries(r.n01, r.n012, r.cap, r.extent);
    const size_t most = relay_items_total(r) + relay_boost_extra(k, k_boost, std::min<size_t>(b.cap, n_split));
    std::vector<uint64_t> weight(most + 1);
    std::vector<uint32_t> table(most + 1), slots(n_split + 1);
    const RelayBoosted out = relay_boost_table(r, b, list, wcost, a.tiles_x, a.wtiles_x, a.wtiles_y, slots.data(), weight.data(), table.data());
    *t = (int64_t)out.items;
    *promoted = (int64_t)out.promoted;
    *cost_sum = out.S;
    if (start && start_cap >= *t) std::copy(table.begin(), table.begin() + out.items, start);
    if (bslot && slot_cap >= (int64_t)n_split) std::copy(slots.begin(), slots.begin() + n_split, bslot);
    return CGRT_OK;
}

int cgrt_lens_samples(uint64_t seed, const int64_t *pixel, const int32_t *sample, int n, double radius, double *out3) {
    if (n < 0 || (n > 0 && (!pixel || !sample || !out3))) return fail(CGRT_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; i++) {
        Stream rs(stream_key(seed, (uint64_t)pixel[i], (uint64_t)sample[i], 0));
        double sx, sy;
        while (true) {
            double ux, uy;
            rs.pair(ux, uy);
            sx = ux * 2.0 - 1;
            sy = uy * 2.0 - 1;
            if (sx * sx + sy * sy < 1) break;
        }
        out3[3 * i] = sx * radius;
        out3[3 * i + 1] = sy * radius;
        out3[3 * i + 2] = 0 * radius;
    }
    return CGRT_OK;
}

int cgrt_math_probe(int device, int op, const double *in, int64_t n, double *out) {
    if (op != CGRT_PROBE_SQRT && op != CGRT_PROBE_NORMALIZED && op != CGRT_PROBE_SPHERE_LEN && op != CGRT_PROBE_SPHERE_LEN_PAIR)
        return fail(CGRT_ERR_INVALID, "cgrt_math_probe: unknown op");
    if (!in || !out) return fail(CGRT_ERR_INVALID, "cgrt_math_probe: null buffer");
    if (n < 0) return fail(CGRT_ERR_INVALID, "cgrt_math_probe: negative n");
    if (n > ((int64_t)1 << 28)) return fail(CGRT_ERR_LIMIT, "cgrt_math_probe: more than 2^28 elements");
    if (n == 0) return CGRT_OK;
    const size_t n_in = op == CGRT_PROBE_SQRT ? 1 : (op == CGRT_PROBE_NORMALIZED ? 3 : (op == CGRT_PROBE_SPHERE_LEN ? 10 : 14)),
                 n_out = op == CGRT_PROBE_NORMALIZED ? 3 : (op == CGRT_PROBE_SPHERE_LEN_PAIR ? 2 : 1);
    ON_DEVICE(device);
    HostStage hs;
    const double *d_in = hs.in(in, (size_t)n * n_in * sizeof(double));
    double *d_out = hs.out(out, (size_t)n * n_out * sizeof(double));
    if (const int rc = hs.error()) return rc;
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, d_in, (long long)n, d_out);
    HIP_TRY(hipGetLastError());
    return hs.finish(CGRT_OK);
}

int cgrt_inside_probe(const cgrt_scene *s, int op, const double *rays, int64_t n, double *out) {
    NEED_COMMITTED(s, rays && out);
    if (op != CGRT_PROBE_INSIDE_LOOP) return fail(CGRT_ERR_INVALID, "cgrt_inside_probe: unknown op");
    if (n < 0) return fail(CGRT_ERR_INVALID, "cgrt_inside_probe: negative n");
    if (n > ((int64_t)1 << 28)) return fail(CGRT_ERR_LIMIT, "cgrt_inside_probe: more than 2^28 elements");
    const DeviceScene &d = s->dev;
    if (!d.all_spheres || d.n_objs < 1 || d.n_objs != d.n_lds)
        return fail(CGRT_ERR_UNSUPPORTED, "cgrt_inside_probe: the pair loop serves sphere-only scenes whose list is resident");
    if (n == 0) return CGRT_OK;
    ON_DEVICE(s->device);
    HostStage hs;
    const double *d_in = hs.in(rays, (size_t)n * 6 * sizeof(double));
    double *d_out = hs.out(out, (size_t)n * 5 * sizeof(double));
    if (const int rc = hs.error()) return rc;
    hipLaunchKernelGGL(inside_loop_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, inside_paying(d), d_in, (long long)n, d_out);
    HIP_TRY(hipGetLastError());
    return hs.finish(CGRT_OK);
}

}  // extern "C"

// the photon pass, the session and the image output
#include "cgrt_ppm_plan.h"
#include "cgrt_hp_order.h"
#include "cgrt_ppm_table.hpp"
#include "cgrt_photon_trace.hpp"
#include "cgrt_ppm_apply.hpp"
#include "cgrt_photon_session.hpp"
#include "cgrt_ppm_session.hpp"
#include "cgrt_sppm.hpp"
#include "cgrt_output.hpp"

#ifdef CGRT_UTIL
// development aid (make exp NAME=util DEFS=-DCGRT_UTIL; tools/util_probe.py): lane-utilisation probes, see UTILP in cgrt_device_math.hpp
extern "C" void cgrt_util_dump(unsigned long long *out) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_util), sizeof(unsigned long long) * 64);
    unsigned long long z[64] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_util), z, sizeof(z));
}
#endif
