// Photon paths: the built-in emitter, photon_trace_kernel (one lane per photon, a diffuse hit = an event) and its launch, and
// the emitter and event probes of the C ABI (cgrt_photon_emit, cgrt_photon_emit_host, cgrt_photon_events, cgrt_photon_ray_events).
#include <climits>

namespace {

#ifndef CGRT_PHOTON_WAVES
#define CGRT_PHOTON_WAVES 4
#endif
constexpr int kPhotonWaves = CGRT_PHOTON_WAVES;  // waves per SIMD photon_trace_kernel<false> is compiled for
constexpr double kPiRef = 3.14159265358979;  // main.cpp:26

// sampling.h:11-29 on the photon's sequential stream
__device__ __forceinline__ V3 sample_sphere(Stream &rs) {
    while (true) {
        const double x = rs.u01() * 2.0 - 1, y = rs.u01() * 2.0 - 1, z = rs.u01() * 2.0 - 1;
        if (x * x + y * y + z * z <= 1) return normalized(mk(x, y, z));
    }
}

// ---- the built-in emitter, main.cpp:240-246 --------------------------------------------------------------------------
// What photon `index` of cgrt_photons starts with: its origin (the light, jittered in x and z), a direction uniform over the
// sphere (sampling.h:11-20 by rejection), the flux power * 4 PI in each channel, and the stream its bounces go on drawing from
// (rs.n = the draws the emission consumed: 2 + 3 per attempt at the direction).  ONE function is photon_trace_kernel's
// emission, cgrt_photon_emit's kernel and cgrt_photon_emit_host's loop: the device's normalized() and the host's sqrt and
// division are correctly rounded, the rest is plain IEEE arithmetic without contraction, so all three give the same bits
// (as camera_ray does for cgrt_camera_rays / _host).
struct EmittedPhoton {
    double o[3], d[3], flux[3];
};
__host__ __device__ __forceinline__ EmittedPhoton photon_emit(const EmitArgs &ea, Stream &rs) {
    EmittedPhoton e;
    const double a = rs.u01() * (2 * ea.jitter) - ea.jitter;
    const double b = rs.u01() * (2 * ea.jitter) - ea.jitter;
    e.o[0] = ea.light[0] + a;
    e.o[1] = ea.light[1] + 0;
    e.o[2] = ea.light[2] + b;
    while (true) {
        double x = rs.u01() * 2.0 - 1, y = rs.u01() * 2.0 - 1, z = rs.u01() * 2.0 - 1;
        if (x * x + y * y + z * z <= 1) {
            camera_normalize(x, y, z);  // vec3.h:36-44 (cgrt_rays.hpp: normalized() on the device)
            e.d[0] = x; e.d[1] = y; e.d[2] = z;
            break;
        }
    }
    e.flux[0] = e.flux[1] = e.flux[2] = ea.power * (kPiRef * 4.0);
    return e;
}
__host__ __device__ __forceinline__ uint64_t photon_key(uint64_t seed, uint64_t index) { return stream_key(seed, index, 0, 0x70686f74ull); }

// Component j of lane's triple in an [n][3] array of doubles, read so that a wave reads whole lines: the wave's 64 triples are
// 192 consecutive doubles (1536 B = twelve 128-byte lines when the array is line-aligned), fetched as three loads of 64
// consecutive doubles -- every load instruction covers four whole lines, where a lane reading its own triple would touch all
// twelve lines three times, a third of each -- and handed to their lanes by three cross-lane reads per component.  `a` points at
// the wave's first triple, nd = 3 * (photons of this wave that exist); called by all 64 lanes.
__device__ __forceinline__ V3 wave_load3(const double *__restrict__ a, int nd, int lane) {
    double r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] = (64 * k + lane < nd) ? a[64 * k + lane] : 0.0;
    double c[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int e = 3 * lane + j, src = e & 63, k = e >> 6;
        const double v0 = __shfl(r[0], src), v1 = __shfl(r[1], src), v2 = __shfl(r[2], src);
        c[j] = k == 0 ? v0 : (k == 1 ? v1 : v2);
    }
    return mk(c[0], c[1], c[2]);
}

// whether photon_trace_kernel<false> keeps the wide walk's first stack entries in LDS: 32 KiB per workgroup, taken only
// while four workgroups (its 4 waves/SIMD) still fit a CU's 160 KiB beside the object list
__host__ __device__ inline bool photon_lds_stack(const DeviceScene &sc) { return sc.has_wide && sc.n_objs <= 56; }
// 1. photon paths.  events: count*kSegStride records of 9 doubles; valid: same count of bytes.
// RAYS: the photons' starts come from the caller's arrays (cgrt_ppm_session_add_photon_rays) instead of the built-in emitter;
// a compile-time choice, so neither form carries the other's code or a branch for it.
template <bool BEZ, bool SPILL = false, bool RAYS = false>
__global__ __launch_bounds__(kThreads, BEZ ? 2 : kPhotonWaves) void photon_trace_kernel(DeviceScene sc, PhotonArgs pa, double *__restrict__ events,
                                                                   unsigned char *__restrict__ valid, PhotonRayArgs ra) {
    // dynamic LDS: the object list, then a staging record per wave (SPILL), a BezLds per wave (BEZ; the Newton starts continue the
    // photon's own stream) or, with neither, the first entries of the 4-wide walk's stack where photon_lds_stack asks for them
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const WgLdsPtrs lds = wg_lds_carve(wg_lds(wg_ask_photon(BEZ, SPILL), (size_t)sc.n_lds, 0, photon_lds_stack(sc)), lds_raw);
    ObjRec *const lobjs = lds.lobjs;
    const LdsAux aux = lds.aux;
    wg_stage16<kThreads>(lobjs, sc.objs, sc.n_lds * (int)(sizeof(ObjRec) / 16));
    __syncthreads();
    const int p = blockIdx.x * kThreads + threadIdx.x;
    bool alive = p < pa.count;
    Stream rs(photon_key(pa.seed, (uint64_t)(pa.first + (alive ? p : 0))));
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1), flux = mk(0, 0, 0);
    if (RAYS) {
        // all 64 lanes take part in the loads (the cross-lane reads need them); a wave beyond the batch has nothing to read
        const int lane = threadIdx.x & 63, wave_first = p - lane;
        const int nd = 3 * (pa.count - wave_first < 64 ? pa.count - wave_first : 64);
        if (nd > 0) {  // wave-uniform
            o = wave_load3(ra.org + 3 * (size_t)wave_first, nd, lane);
            d = wave_load3(ra.dir + 3 * (size_t)wave_first, nd, lane);
            flux = wave_load3(ra.flux + 3 * (size_t)wave_first, nd, lane);
        }
        if (alive) {
            if (ra.keys) rs.key = ra.keys[p];  // (uniform: a kernel argument)
            if (ra.draws) rs.n = ra.draws[p];
            alive = !(d.x == 0 && d.y == 0 && d.z == 0);  // emitted, goes nowhere: counted by the host, never traced
        }
        if (!alive) {  // an inactive lane rides along with what the built-in form gives it
            o = mk(0, 0, 0);
            d = mk(0, 0, 1);
            flux = mk(0, 0, 0);
        }
    } else if (alive) {  // main.cpp:240-246
        EmitArgs ea;
        ea.light[0] = pa.light[0]; ea.light[1] = pa.light[1]; ea.light[2] = pa.light[2];
        ea.jitter = pa.jitter; ea.power = pa.power; ea.seed = pa.seed;
        const EmittedPhoton e = photon_emit(ea, rs);
        o = mk(e.o[0], e.o[1], e.o[2]);
        d = mk(e.d[0], e.d[1], e.d[2]);
        flux = mk(e.flux[0], e.flux[1], e.flux[2]);
    }
    uint32_t dn = 0, dt = 0;
    for (int seg = 0; seg < pa.max_depth; seg++) {
        if (__ballot(alive) == 0ull) break;
        RayKey rk{rs.key, 1, true, rs.n};
        const SceneHit hit = intersect_scene<true, BEZ, false, false, SPILL>(lobjs, sc.n_lds, sc.n_objs, sc, o, d, rk, alive, aux, dn, dt);
        if (BEZ) rs.n = rk.n0;
        if (!alive) continue;
        if (hit.id < 0) {
            alive = false;
            continue;
        }
        const ObjMat ob = load_mat<SPILL>(lobjs, sc.n_lds, sc.objs, hit.id);
        const V3 P = o + d * hit.t;
        V3 n = hit.n;
        const V3 n_old = n;
        bool into = true;
        if (dot(n, d) > 0) {
            n = -n;
            into = false;
        }
        V3 f = ob.col;
        if (ob.kind == KIND_PLANE && ob.tex >= 0) {
            V3 c;
            if (texture_color(sc.texs[ob.tex], sc.texels, P, c)) f = c;
        }
        const double pmax = (f.x > f.y && f.x > f.z) ? f.x : (f.y > f.z ? f.y : f.z);  // util.h:16-27, main.cpp:79
        const double refl = ob.refl, transp = ob.transp;
        if (refl < kEps && transp < kEps) {
            // diffuse: record the event the serial loop of main.cpp:103-125 would process now
            const size_t slot = (size_t)p * kSegStride + seg;
            double *e = events + 9 * slot;
            e[0] = P.x; e[1] = P.y; e[2] = P.z;
            e[3] = n.x; e[4] = n.y; e[5] = n.z;
            e[6] = flux.x; e[7] = flux.y; e[8] = flux.z;
            valid[slot] = 1;
            V3 nd;
            while (true) {  // uniform_sampling_halfsphere, sampling.h:22-29
                nd = sample_sphere(rs);
                if (dot(nd, n) > 0) break;
            }
            o = P;  // main.cpp:127: no epsilon offset here
            d = nd;
            flux = mulv(f, flux) * (1.0 / pmax);
        } else if (transp < kEps) {
            const V3 nd = d - n * 2.0 * dot(n, d);  // main.cpp:131-134
            o = P + n * kEps;
            d = nd;
            flux = mulv(f, flux) * refl;
        } else {
            const double nc = 1.0, nt = 1.33;  // main.cpp:140-164
            const double nnt = into ? nc / nt : nt / nc;
            const double ddn = dot(d, n);
            const V3 refl_dir = d - n_old * 2.0 * dot(n_old, d);
            const double cos2t = 1 - nnt * nnt * (1 - ddn * ddn);
            if (cos2t < 0) {
                o = P + n * kEps;
                d = refl_dir;
            } else {
                const V3 refr_dir = normalized(d * nnt - n_old * ((into ? 1 : -1) * (ddn * nnt + sqrt(cos2t))));
                if (rs.u01() < 0.5) {  // Russian roulette; the photon's flux is untouched by glass
                    o = P + n * kEps;
                    d = refl_dir;
                } else {
                    o = P - n * kEps;
                    d = refr_dir;
                }
            }
        }
    }
}

// cgrt_photon_emit: one lane per photon, no scene.  Any output may be null.
__global__ __launch_bounds__(256) void photon_emit_kernel(EmitArgs ea, long long first, long long count, double *__restrict__ org,
                                                          double *__restrict__ dir, double *__restrict__ flux,
                                                          unsigned long long *__restrict__ keys, unsigned int *__restrict__ draws) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    Stream rs(photon_key(ea.seed, (uint64_t)(first + i)));
    const EmittedPhoton e = photon_emit(ea, rs);
    for (int k = 0; k < 3; k++) {
        if (org) org[3 * i + k] = e.o[k];
        if (dir) dir[3 * i + k] = e.d[k];
        if (flux) flux[3 * i + k] = e.flux[k];
    }
    if (keys) keys[i] = rs.key;
    if (draws) draws[i] = rs.n;
}

// ra: null for the built-in emitter, else the caller's photons of this batch (the RAYS instantiations)
int launch_photon_trace(const cgrt_scene *s, const PhotonArgs &pa, double *events, unsigned char *valid, hipStream_t st = 0,
                        const PhotonRayArgs *ra = nullptr) {
    const DeviceScene &d = s->dev;
    // more objects than the LDS list holds: the variants that read the rest from the uploaded array
    const bool spill = d.n_objs > d.n_lds, bez = d.has_bezier != 0;
    const auto fn = ra ? (spill ? (bez ? &photon_trace_kernel<true, true, true> : &photon_trace_kernel<false, true, true>)
                                : (bez ? &photon_trace_kernel<true, false, true> : &photon_trace_kernel<false, false, true>))
                       : (spill ? (bez ? &photon_trace_kernel<true, true> : &photon_trace_kernel<false, true>)
                                : (bez ? &photon_trace_kernel<true> : &photon_trace_kernel<false>));
    return launch_checked(fn, spill ? "photon_trace_kernel, SPILL" : "photon_trace_kernel", s->device,
                          dim3((pa.count + kThreads - 1) / kThreads), dim3(kThreads),
                          photon_lds((size_t)d.n_lds, spill, bez, photon_lds_stack(d)), st, d, pa, events, valid,
                          ra ? *ra : PhotonRayArgs{});
}

}  // namespace

// What both event probes do: allocate and clear the slots of batch `pa`, trace it, synchronise and copy the slots back.  pr: the
// batch's photons are the caller's (HOST arrays, uploaded here); null: the built-in emitter's.
static int photon_events(const cgrt_scene *s, const PhotonArgs &pa, const cgrt_photon_rays *pr, double *events9, uint8_t *valid) {
    ON_DEVICE(s->device);
    const size_t n = (size_t)pa.count, nslots = n * kSegStride;
    DevBuf ev, va, b_o, b_d, b_f, b_k, b_n;
    HIP_TRY(ev.alloc(nslots * 9 * sizeof(double)));
    HIP_TRY(va.alloc(nslots));
    HIP_TRY(hipMemset(ev.p, 0, nslots * 9 * sizeof(double)));
    HIP_TRY(hipMemset(va.p, 0, nslots));
    PhotonRayArgs ra{};
    if (pr) {
        HIP_TRY(b_o.alloc(n * 24)); HIP_TRY(b_d.alloc(n * 24)); HIP_TRY(b_f.alloc(n * 24));
        HIP_TRY(hipMemcpy(b_o.p, pr->org3, n * 24, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b_d.p, pr->dir3, n * 24, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b_f.p, pr->flux3, n * 24, hipMemcpyHostToDevice));
        ra.org = b_o.as<double>(); ra.dir = b_d.as<double>(); ra.flux = b_f.as<double>();
        if (pr->keys) {
            HIP_TRY(b_k.alloc(n * 8));
            HIP_TRY(hipMemcpy(b_k.p, pr->keys, n * 8, hipMemcpyHostToDevice));
            ra.keys = b_k.as<unsigned long long>();
        }
        if (pr->draws) {
            HIP_TRY(b_n.alloc(n * 4));
            HIP_TRY(hipMemcpy(b_n.p, pr->draws, n * 4, hipMemcpyHostToDevice));
            ra.draws = b_n.as<unsigned int>();
        }
    }
    if (const int rc = launch_photon_trace(s, pa, ev.as<double>(), va.as<unsigned char>(), 0, pr ? &ra : nullptr)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(events9, ev.p, nslots * 9 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, va.p, nslots, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

// verification probe: the diffuse hits of photons [first, first+count) -- count*8 slots of 9 doubles {P, n, flux}
// (slot = (photon-first)*8 + path segment) and one validity byte per slot, HOST buffers
extern "C" int cgrt_photon_events(const cgrt_scene *s, const cgrt_photons *ph, int max_depth, int64_t first, int32_t count,
                                  double *events9, uint8_t *valid) {
    if (!s || !s->committed || !ph || !events9 || !valid || count <= 0 || count > (1 << 20) || max_depth < 1 ||
        max_depth > kMaxDepth)
        return fail(CGRT_ERR_INVALID, "bad argument");
    return photon_events(s, photon_args(*ph, first, count, max_depth), nullptr, events9, valid);
}
// ---- caller-supplied photons: argument checks, the built-in emitter as a producer, the probe -------------------------------
constexpr long long kMaxPhotonRays = 1ll << 36;
// what can be said without a device or a session (so the refusals are the same wherever the struct arrives)
static int check_photon_rays(const cgrt_photon_rays *pr) {
    if (!pr) return fail(CGRT_ERR_INVALID, "null cgrt_photon_rays");
    if (pr->n < 0) return fail(CGRT_ERR_INVALID, "negative photon count");
    if (pr->n > kMaxPhotonRays) return fail(CGRT_ERR_LIMIT, "more than 2^36 photons in one call");
    if (pr->n > 0 && (!pr->org3 || !pr->dir3 || !pr->flux3)) return fail(CGRT_ERR_INVALID, "null org3 / dir3 / flux3");
    return CGRT_OK;
}
static int check_emit(const cgrt_photons *ph, int64_t first, int64_t count) {
    if (!ph) return fail(CGRT_ERR_INVALID, "null cgrt_photons");
    if (first < 0 || count < 0) return fail(CGRT_ERR_INVALID, "negative photon index or count");
    if (count > kMaxPhotonRays) return fail(CGRT_ERR_LIMIT, "more than 2^36 photons in one call");
    if (first > LLONG_MAX - count) return fail(CGRT_ERR_INVALID, "photon index out of range");
    return CGRT_OK;
}

extern "C" int cgrt_photon_emit(const cgrt_photons *ph, int64_t first, int64_t count, double *org3, double *dir3, double *flux3,
                                uint64_t *keys, uint32_t *draws, void *stream) {
    if (const int rc = check_emit(ph, first, count)) return rc;
    if (count == 0) return CGRT_OK;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const EmitArgs ea = emit_args(ph);
    // 2^36 photons are 2^28 workgroups: launched in pieces of at most 2^30 photons (a grid's x extent is below 2^31)
    for (long long k0 = 0; k0 < count; k0 += 1ll << 30) {
        const long long m = count - k0 < (1ll << 30) ? count - k0 : (1ll << 30);
        hipLaunchKernelGGL(photon_emit_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, ea, (long long)first + k0, m,
                           org3 ? org3 + 3 * k0 : nullptr, dir3 ? dir3 + 3 * k0 : nullptr, flux3 ? flux3 + 3 * k0 : nullptr,
                           keys ? reinterpret_cast<unsigned long long *>(keys) + k0 : nullptr, draws ? draws + k0 : nullptr);
    }
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

extern "C" int cgrt_photon_emit_host(const cgrt_photons *ph, int64_t first, int64_t count, double *org3, double *dir3,
                                     double *flux3, uint64_t *keys, uint32_t *draws) {
    if (const int rc = check_emit(ph, first, count)) return rc;
    const EmitArgs ea = emit_args(ph);
    for (int64_t i = 0; i < count; i++) {
        Stream rs(photon_key(ea.seed, (uint64_t)(first + i)));
        const EmittedPhoton e = photon_emit(ea, rs);
        for (int k = 0; k < 3; k++) {
            if (org3) org3[3 * i + k] = e.o[k];
            if (dir3) dir3[3 * i + k] = e.d[k];
            if (flux3) flux3[3 * i + k] = e.flux[k];
        }
        if (keys) keys[i] = rs.key;
        if (draws) draws[i] = rs.n;
    }
    return CGRT_OK;
}

// cgrt_photon_events for caller-supplied photons (HOST arrays): the RAYS instantiation; of a cgrt_photons only the seed counts
extern "C" int cgrt_photon_ray_events(const cgrt_scene *s, const cgrt_photon_rays *pr, uint64_t seed, int64_t first_index,
                                      int max_depth, double *events9, uint8_t *valid) {
    if (const int rc = check_photon_rays(pr)) return rc;
    if (!s || !s->committed || !events9 || !valid || pr->n < 1 || pr->n > (1 << 20) || first_index < 0 || max_depth < 1 ||
        max_depth > kMaxDepth)
        return fail(CGRT_ERR_INVALID, "bad argument");
    cgrt_photons ph{};
    ph.seed = seed;
    return photon_events(s, photon_args(ph, first_index, (int)pr->n, max_depth), pr, events9, valid);
}
