// Caller-supplied rays: trace_rays_kernel (cgrt_trace_rays) and camera_rays_kernel (cgrt_camera_rays).  Part of libcgrt.so
// (cgrt_hip.hip).  The work items are rays from a buffer; nothing of the eye pass's tile geometry is used.
#ifndef CGRT_RAYS_HPP
#define CGRT_RAYS_HPP
#include "cgrt_eye.hpp"
#include "cgrt_ray_wave.hpp"

// Kernel arguments of trace_rays_kernel (cgrt_rays / cgrt_ray_results of cgrt.h; every output pointer may be nullptr)
struct RayParams {
    RayInput in;
    int32_t max_depth, pad_;
    double *acc;
    uint32_t *nhit;
    int32_t *hit_obj;
    double *hit_t, *hit_normal;
    unsigned int *queue;  // head of the block queue (block = 64 consecutive rays), zeroed before the launch
};
// Where capture_rays_kernel puts the Hitpoints (cgrt_trace_rays_hitpoints, the eye stage of cgrt_ppm_session_create_rays):
// records of 10 doubles {hf, P, n, label} as HitpointSink's (cgrt_eye.hpp), label = (ray index << 4) | position of the
// Hitpoint in the ray tree's emission order.  *count is advanced for every Hitpoint, records beyond cap are dropped.
struct RaySink {
    double *rec;
    unsigned long long *count;
    unsigned long long cap;
    const long long *pixel;  // nullptr, or per ray: a ray whose entry is negative belongs to no texel and is not traced
};

// One step of trace() behind the scene walk (main.cpp:64-157) for a ray that hit object hit.id: the expressions of
// trace_grid_body (cgrt_eye.hpp), in its order -- that order is the parity contract (fp64, no contraction, sqrt_cr,
// normalized).  trace_grid_body keeps its own copy (DESIGN.md section 4.17 names the tests that pin each).
struct RayState {
    V3 o, d, adj;
    int32_t depth_left;
    uint32_t path;
};
enum RayStep {
    RAY_END = 0,      // absorbed: a mirror or glass hit at the depth limit (main.cpp:46)
    RAY_HITPOINT = 1, // diffuse: `hf` is the Hitpoint's f * adj (main.cpp:88); the ray ends
    RAY_CONTINUE = 2, // `r` is the reflected child
    RAY_SPLIT = 3     // `r` is the reflected child and `pe` the refracted one, to be traced after r's subtree
};
struct RaySurface {  // where the step happened: what a Hitpoint stores beside its value (main.cpp:89-90)
    V3 P, n;         // o + d * t, and the normal after the flip of main.cpp:73-76
};
template <bool GLASS, bool SPILL>
__device__ __forceinline__ RayStep shade_step(const DeviceScene &sc, const ObjRec *__restrict__ lobjs, const SceneHit &hit,
                                              RayState &r, V3 &hf, Pending &pe, RaySurface &at) {
    const ObjMat ob = load_mat<SPILL>(lobjs, sc.n_lds, sc.objs, hit.id);
    const V3 o = r.o, d = r.d;
    const V3 P = o + d * hit.t;  // main.cpp:68
    V3 n = hit.n;
    const V3 n_old = n;
    bool into = true;
    if (dot(n, d) > 0) {  // main.cpp:73-76
        n = -n;
        into = false;
    }
    V3 f = ob.col;  // getSurfaceColor
    if (ob.kind == KIND_PLANE && ob.tex >= 0) {
        V3 c;
        if (texture_color(sc.texs[ob.tex], sc.texels, P, c)) f = c;  // objects.h:533-539
    }
    const double refl = ob.refl, transp = ob.transp;
    if (refl < kEps && transp < kEps) {
        hf = mulv(f, r.adj);  // main.cpp:85-100
        at.P = P;
        at.n = n;
        return RAY_HITPOINT;
    }
    if (!(r.depth_left > 1)) return RAY_END;
    if (transp < kEps) {
        // mirror, main.cpp:129-134
        const V3 nd = d - n * 2.0 * dot(n, d);
        r.adj = mulv(f, r.adj) * refl;
        r.o = P + n * kEps;
        r.d = nd;
        r.depth_left--;
        r.path = r.path * 2;
        return RAY_CONTINUE;
    }
    if (!GLASS) return RAY_END;  // (not instantiated for scenes with a transparent object at max_depth > 1)
    // glass, main.cpp:135-157
    RayStep step = RAY_CONTINUE;
    const double nc = 1.0, nt = 1.33;
    const double nnt = into ? nc / nt : nt / nc;
    const double ddn = dot(d, n);
    const V3 refl_dir = d - n_old * 2.0 * dot(n_old, d);
    const double cos2t = 1 - nnt * nnt * (1 - ddn * ddn);
    if (cos2t < 0) {
        // total internal reflection keeps adj (main.cpp:144)
        r.o = P + n * kEps;
        r.d = refl_dir;
    } else {
        const V3 refr_dir = normalized(d * nnt - n_old * ((into ? 1 : -1) * (ddn * nnt + sqrt_cr(cos2t))));
        const double a = nt - nc, b = nt + nc, R0 = a * a / (b * b);
        const double c = 1 - (into ? -ddn : dot(refr_dir, n_old));
        const double Re = R0 + (1 - R0) * c * c * c * c * c;
        const V3 fa = mulv(f, r.adj);
        pe.o = P - n * kEps;
        pe.d = refr_dir;
        pe.adj = fa * (1 - Re);
        pe.depth_left = r.depth_left - 1;
        pe.path = r.path * 2 + 1;
        r.o = P + n * kEps;
        r.d = refl_dir;
        r.adj = fa * Re;
        step = RAY_SPLIT;
    }
    r.depth_left--;
    r.path = r.path * 2;
    return step;
}

// Persistent workgroups of NT threads.  A wave draws blocks of 64 consecutive rays from one queue counter (lane 0's atomic, the
// next block's already in flight while the current one is traced); a lane whose ray tree is finished stores that ray's results
// and takes the next ray of the wave's block at once, and the wave moves on to its next block while other lanes still finish
// rays of the old one: lanes idle only when the queue is empty.  A ray's Hitpoint values are added in the lane in emission
// order (reflect subtree, then refract), so its result does not depend on which lane or wave traced it, nor on what the other
// lanes were doing.
// FIRST: nearest-hit query -- one scene walk per ray, no shading, no pending-ray code.
// CAPTURE: every Hitpoint is also appended to `sink` (capture_rays_kernel below); false compiles all of that away.
// Dynamic LDS: wg_ask_trace's layout (cgrt_wg_lds.h), as the eye pass.
template <bool TREES, bool BEZ, bool GLASS, bool SPH, bool STATS, bool SPILL, bool FIRST, int NT, bool CAPTURE>
__device__ __forceinline__ void trace_rays_body(const DeviceScene &sc, const RayParams &rp, unsigned long long *wc, const RaySink &sink) {
    static_assert(!(FIRST && GLASS), "a nearest-hit query has no pending rays");
    static_assert(!(CAPTURE && (FIRST || STATS)), "Hitpoints come from the full trace; the capture counts nothing");
    constexpr size_t level_bytes = pending_level_bytes(NT);

    extern __shared__ __align__(16) unsigned char lds_raw[];
    const WgLdsPtrs lds = ray_wg_begin<NT, TREES, BEZ, GLASS, SPILL>(sc, lds_raw);
    ObjRec *const lobjs = lds.lobjs;
    const LdsAux aux = lds.aux;

    const int lane = threadIdx.x & 63;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const unsigned n_blocks = (unsigned)((rp.in.n + 63) >> 6);

    // RayBlocks (cgrt_ray_wave.hpp) written out: through the struct a nearest-hit variant's occupancy moved.
    // The wave's block: rays [ray_next, ray_end) are still to be handed out (wave-uniform)
    long long ray_next = 0, ray_end = 0;
    bool queue_empty = false;
    unsigned block_ahead = 0;
    if (lane == 0) block_ahead = atomicAdd(rp.queue, 1u);

    // the lane's ray tree
    long long my_ray = 0;  // index of the ray whose tree this lane is tracing
    bool open = false;     // its sums are still to be stored
    bool primary = false;  // the next walk is the ray's own: it supplies hit_obj / hit_t / hit_normal
    bool have = false;
    uint64_t key = 0;
    RayState r;
    r.o = mk(0, 0, 0);
    r.d = mk(0, 0, 1);
    r.adj = mk(1, 1, 1);
    r.depth_left = 0;
    r.path = 1;
    double acc_r = 0, acc_g = 0, acc_b = 0;
    uint32_t ray_hits = 0;
    uint32_t my_hits = 0, my_rays = 0, my_nodes = 0, my_tris = 0, wave_iters = 0;

    Pending deep[2];  // third stack level (scratch)
    Pending sib;      // refracted sibling of a leaf-level glass hit (registers)
    bool sib_valid = false;
    unsigned char *lslot = lds.pending;  // level L, field f of this thread: lslot + L*level_bytes + (f*NT + tid)*8
    int sp = 0;

    while (true) {
        const bool want = !have;
        const unsigned long long m = __ballot(want);
        if (m != 0ull) {
            if (!FIRST && want && open) {  // the finished ray's sums
                if (rp.acc) st3(rp.acc + 3 * my_ray, mk(acc_r, acc_g, acc_b));
                if (rp.nhit) rp.nhit[my_ray] = ray_hits;
                open = false;
            }
            if (ray_next >= ray_end && !queue_empty) {
                // the block fetched ahead, and the request for the one after it
                const unsigned blk = (unsigned)__builtin_amdgcn_readfirstlane((int)block_ahead);
                if (lane == 0) block_ahead = atomicAdd(rp.queue, 1u);
                if (blk >= n_blocks) {
                    queue_empty = true;
                } else {
                    ray_next = (long long)blk << 6;
                    ray_end = ray_next + 64 < rp.in.n ? ray_next + 64 : rp.in.n;
                }
            }
            const long long u = ray_next + (long long)__popcll(m & lanes_below);
            ray_next += (long long)__popcll(m);  // lanes that drew beyond ray_end draw again from the next block
            if (want && u < ray_end) {
                r.o = ld3(rp.in.org + 3 * u);
                r.d = ld3(rp.in.dir + 3 * u);
                bool skip = ray_is_none(r.d);
                if (CAPTURE && sink.pixel) skip = skip || sink.pixel[u] < 0;
                if (skip) {
                    // not a ray (cgrt_camera_rays' padding rows; a ray without a texel): the results of a miss, nothing counted
                    if (!FIRST && rp.acc) st3(rp.acc + 3 * u, mk(0, 0, 0));
                    if (!FIRST && rp.nhit) rp.nhit[u] = 0u;
                    if (rp.hit_obj) rp.hit_obj[u] = -1;
                    if (rp.hit_t) rp.hit_t[u] = 0.0;
                    if (rp.hit_normal) st3(rp.hit_normal + 3 * u, mk(0, 0, 0));
                } else {
                    my_ray = u;
                    key = ray_default_key(rp.in, u);
                    r.adj = mk(1, 1, 1);
                    r.depth_left = rp.max_depth;
                    r.path = 1;
                    acc_r = acc_g = acc_b = 0;
                    ray_hits = 0;
                    primary = true;
                    open = true;
                    have = true;
                }
            }
        }
        if (__ballot(have) == 0ull) {
            if (queue_empty && ray_next >= ray_end) break;  // nothing left anywhere
            continue;  // drew nothing traceable (block boundary, padding rays)
        }
        wave_iters++;
        // All 64 lanes enter the scene walk together (lanes without a ray carry on == false)
        RayKey rk{key, r.path, false, 0u};
        const SceneHit hit = intersect_scene<TREES, BEZ, SPH, STATS, SPILL, /*PRE*/ false, /*HFONLY*/ false>(
            lobjs, sc.n_lds, sc.n_objs, sc, r.o, r.d, rk, have, aux, my_nodes, my_tris);
        if (have) {
            my_rays++;
            have = false;
            if (FIRST || primary) {
                primary = false;
                const bool is_hit = hit.id >= 0;
                if (rp.hit_obj) rp.hit_obj[my_ray] = is_hit ? hit.id : -1;
                if (rp.hit_t) rp.hit_t[my_ray] = is_hit ? hit.t : 0.0;
                if (rp.hit_normal) {  // (not st3 of a selected V3: DESIGN.md section 4.21)
                    double *q = rp.hit_normal + 3 * my_ray;
                    q[0] = is_hit ? hit.n.x : 0.0;
                    q[1] = is_hit ? hit.n.y : 0.0;
                    q[2] = is_hit ? hit.n.z : 0.0;
                }
            }
            if (!FIRST) {
                if (hit.id >= 0) {
                    V3 hf;
                    Pending pe;
                    RaySurface at;
                    const RayStep step = shade_step<GLASS, SPILL>(sc, lobjs, hit, r, hf, pe, at);
                    if (step == RAY_HITPOINT) {
                        if (CAPTURE) {
                            // one atomic per wave, as trace_grid_body's capture: the lanes that are at a Hitpoint together take
                            // consecutive places behind the count their first lane fetched
                            const unsigned long long here = __ballot(true);
                            const int lead = (int)__ffsll((long long)here) - 1;
                            unsigned long long base = 0ull;
                            if (lane == lead) base = atomicAdd(sink.count, (unsigned long long)__popcll(here));
                            base = (unsigned long long)__shfl((long long)base, lead);
                            const unsigned long long k = base + (unsigned long long)__popcll(here & lanes_below);
                            if (k < sink.cap) {
                                double *q = sink.rec + 10 * k;
                                q[0] = hf.x; q[1] = hf.y; q[2] = hf.z;
                                q[3] = at.P.x; q[4] = at.P.y; q[5] = at.P.z;
                                q[6] = at.n.x; q[7] = at.n.y; q[8] = at.n.z;
                                q[9] = (double)(((unsigned long long)my_ray << 4) | (unsigned long long)ray_hits);  // ray < 2^36
                            }
                        }
                        acc_r += hf.x;
                        acc_g += hf.y;
                        acc_b += hf.z;
                        ray_hits++;
                        my_hits++;
                    } else if (step != RAY_END) {
                        have = true;
                        if (GLASS && step == RAY_SPLIT) {
                            if (pe.depth_left == 1) {  // the children are leaves of the recursion: consumed right after the reflected one
                                sib = pe;
                                sib_valid = true;
                            } else {
                                if (sp < kLdsLevels) {
                                    double *q = reinterpret_cast<double *>(lslot + sp * level_bytes) + threadIdx.x;
                                    q[0 * NT] = pe.o.x; q[1 * NT] = pe.o.y; q[2 * NT] = pe.o.z;
                                    q[3 * NT] = pe.d.x; q[4 * NT] = pe.d.y; q[5 * NT] = pe.d.z;
                                    q[6 * NT] = pe.adj.x; q[7 * NT] = pe.adj.y; q[8 * NT] = pe.adj.z;
                                    // depth_left <= 4 and path < 32: one word
                                    reinterpret_cast<uint32_t *>(lslot + sp * level_bytes + kPendDoubles * NT * sizeof(double))[threadIdx.x] =
                                        ((uint32_t)pe.depth_left << 8) | pe.path;
                                } else {
                                    deep[sp - kLdsLevels] = pe;
                                }
                                sp++;
                            }
                        }
                    }
                }
                if (GLASS && !have && sib_valid) {
                    r.o = sib.o;
                    r.d = sib.d;
                    r.adj = sib.adj;
                    r.depth_left = sib.depth_left;
                    r.path = sib.path;
                    sib_valid = false;
                    have = true;
                }
                if (GLASS && !have && sp > 0) {
                    --sp;
                    if (sp < kLdsLevels) {
                        const double *q = reinterpret_cast<const double *>(lslot + sp * level_bytes) + threadIdx.x;
                        r.o = mk(q[0 * NT], q[1 * NT], q[2 * NT]);
                        r.d = mk(q[3 * NT], q[4 * NT], q[5 * NT]);
                        r.adj = mk(q[6 * NT], q[7 * NT], q[8 * NT]);
                        const uint32_t meta =
                            reinterpret_cast<const uint32_t *>(lslot + sp * level_bytes + kPendDoubles * NT * sizeof(double))[threadIdx.x];
                        r.depth_left = (int)(meta >> 8);
                        r.path = meta & 0xffu;
                    } else {
                        const Pending &pe = deep[sp - kLdsLevels];
                        r.o = pe.o;
                        r.d = pe.d;
                        r.adj = pe.adj;
                        r.depth_left = pe.depth_left;
                        r.path = pe.path;
                    }
                    have = true;
                }
            }
        }
    }  // ray loop

    ray_counters_flush<STATS, true>(wc, lane, my_rays, my_hits, my_nodes, my_tris, wave_iters);
}

template <bool TREES, bool BEZ, bool GLASS, bool SPH, bool STATS, bool SPILL, bool FIRST, int NT>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kTreeWaves : 4)) void trace_rays_kernel(DeviceScene sc, RayParams rp,
                                                                                               unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long wg_cnt[CGRT_NCOUNTERS];
    unsigned long long *wc = wg_counters_begin(wg_cnt, counters);
    trace_rays_body<TREES, BEZ, GLASS, SPH, STATS, SPILL, FIRST, NT, false>(sc, rp, wc, RaySink{nullptr, nullptr, 0ull, nullptr});
    wg_counters_end(wg_cnt, counters);
}
// The capture form: the full trace of every ray that has a texel, its Hitpoints appended to `sink`; rp's result pointers are
// null and nothing is counted.  Same LDS layout and occupancy as trace_rays_kernel<..., STATS=false, FIRST=false, NT>.
template <bool TREES, bool BEZ, bool GLASS, bool SPH, bool SPILL, int NT>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kTreeWaves : 4)) void capture_rays_kernel(DeviceScene sc, RayParams rp, RaySink sink) {
    trace_rays_body<TREES, BEZ, GLASS, SPH, false, SPILL, false, NT, true>(sc, rp, nullptr, sink);
}

// hit_normal3 of rays whose nearest object is an OPAQUE mesh walked in its 4-wide form: the scene walk prunes such a mesh by
// distance and orients the normal as for an odd improvement count (tree_intersect_wide: counter = 1; nothing trace() computes
// depends on the sign, main.cpp:73-76).  The array promises the normal intersect() returned, so this pass -- launched behind
// trace_rays_kernel only when hit_normal3 is asked for and the scene has such a mesh -- recounts the improvements without
// pruning (tree_count_wide) and turns the normal where the reference's count is even.  One thread per ray.
__global__ __launch_bounds__(256) void ray_normal_sign_kernel(DeviceScene sc, RayParams rp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rp.in.n) return;
    const int id = rp.hit_obj[i];
    if (id < 0) return;
    const ObjRec &ob = sc.objs[id];
    if (ob.kind != KIND_MESH || !(ob.transp < kEps) || ob.aux == 2) return;  // (objtype 2 fixes the sign itself, objects.h:434-436)
    const TreeRec T = sc.trees[ob.tree];
    if (!T.tri_level || T.nwide == 0) return;
    const V3 o = ld3(rp.in.org + 3 * i), d = ld3(rp.in.dir + 3 * i);
    const V3 inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
    const Ray32 r32 = make_ray32(o, inv, T.bmax);
    const int c = tree_count_wide(sc.wnodes + T.wnode_begin, sc.otris + T.otri_begin, sc.tris + T.tri_begin, o, d, r32);
    if (c > 0 && (c & 1) == 0) {
        double *q = rp.hit_normal + 3 * i;
        q[0] = -q[0];
        q[1] = -q[1];
        q[2] = -q[2];
    }
}

// ---- the primary rays of the eye pass, as a ray list --------------------------------------------------------------------
// What a (pixel, sample) of the grid starts with: set_pixel / start_sample of trace_grid_body (main.cpp:188-189,198,203-209).
// Host and device evaluate this one function; the device's normalized() and the host's sqrt and division are correctly
// rounded, the rest is plain IEEE arithmetic without contraction, so both give the same bits (tests/test_gpu_rays.py).
struct CameraRay {
    double o[3], d[3];
    uint64_t key;
};
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void camera_normalize(double &x, double &y, double &z) {
    const V3 v = normalized(mk(x, y, z));
    x = v.x;
    y = v.y;
    z = v.z;
}
#else
inline void camera_normalize(double &x, double &y, double &z) {  // vec3.h:36-44
    const double len = std::sqrt(x * x + y * y + z * z);
    if (len > 0) {
        const double r = 1 / len;
        x *= r;
        y *= r;
        z *= r;
    }
}
#endif
// local row j, column w, sample index `smp` (sample_offset included)
__host__ __device__ __forceinline__ CameraRay camera_ray(const GridParams &g, int j, int w, int smp) {
    CameraRay c;
    const int h = global_row(g, j);
    c.o[0] = g.cam[0];
    c.o[1] = g.cam[1];
    c.o[2] = g.cam[2];
    c.d[0] = c.d[1] = c.d[2] = 0.0;
    c.key = 0;
    if (h >= g.H) {  // a row beyond the image (stripe padding): dir = 0, not to be traced; the origin is the eye
        if (g.posed) pose_point(g, g.cam[0], g.cam[1], g.cam[2], c.o[0], c.o[1], c.o[2]);
        return c;
    }
    const double px = (2.0 * ((double)w / g.W) - 1) * g.half_width;
    const double py = (2.0 * ((double)h / g.H) - 1) * g.half_width * g.H / g.W;
    double dx = px - g.cam[0], dy = py - g.cam[1], dz = 0 - g.cam[2];
    camera_normalize(dx, dy, dz);
    c.key = sample_key(pixel_key(g.seed, (uint64_t)h * (uint64_t)g.W + (uint64_t)w), (uint64_t)smp);
    if (g.posed) {
        // A posed camera (pose_point, cgrt_frame.h, where the definition stands): the same points of the camera's frame, the ray
        // made of their images -- what set_pixel / start_sample of the POSE kernels do, expression for expression.
        double ex, ey, ez, tx, ty, tz;  // the ray's origin and the point it aims at, in the world
        if (g.lens_radius > 0) {
            const double pf = (g.focus_plane - g.cam[2]) / dz;
            pose_point(g, dx * pf + g.cam[0], dy * pf + g.cam[1], dz * pf + g.cam[2], tx, ty, tz);
            double sx, sy;
            lens_disc(c.key, sx, sy);
            pose_point(g, g.cam[0] + sx * g.lens_radius, g.cam[1] + sy * g.lens_radius, g.cam[2] + 0 * g.lens_radius, ex, ey, ez);
        } else {
            pose_point(g, px, py, 0, tx, ty, tz);
            pose_point(g, g.cam[0], g.cam[1], g.cam[2], ex, ey, ez);
        }
        c.o[0] = ex;
        c.o[1] = ey;
        c.o[2] = ez;
        dx = tx - ex;
        dy = ty - ey;
        dz = tz - ez;
        camera_normalize(dx, dy, dz);
        c.d[0] = dx;
        c.d[1] = dy;
        c.d[2] = dz;
        return c;
    }
    if (g.lens_radius > 0) {
        const double pf = (g.focus_plane - g.cam[2]) / dz;  // pof = pdir * pf + camorg
        const double fx = dx * pf + g.cam[0], fy = dy * pf + g.cam[1], fz = dz * pf + g.cam[2];
        double sx, sy;
        lens_disc(c.key, sx, sy);
        c.o[0] = g.cam[0] + sx * g.lens_radius;
        c.o[1] = g.cam[1] + sy * g.lens_radius;
        c.o[2] = g.cam[2] + 0 * g.lens_radius;
        dx = fx - c.o[0];
        dy = fy - c.o[1];
        dz = fz - c.o[2];
        camera_normalize(dx, dy, dz);
    }
    c.d[0] = dx;
    c.d[1] = dy;
    c.d[2] = dz;
    return c;
}

// one thread per (sample, local row, column): ray index = (k * rows + j) * W + w
__global__ __launch_bounds__(256) void camera_rays_kernel(GridParams g, double *__restrict__ org, double *__restrict__ dir,
                                                          unsigned long long *__restrict__ keys, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % g.W), j = (int)((i / g.W) % g.rows), k = (int)(i / ((long long)g.W * g.rows));
    const CameraRay c = camera_ray(g, j, w, g.sample_offset + k);
    if (org) {
        org[3 * i] = c.o[0];
        org[3 * i + 1] = c.o[1];
        org[3 * i + 2] = c.o[2];
    }
    if (dir) {
        dir[3 * i] = c.d[0];
        dir[3 * i + 1] = c.d[1];
        dir[3 * i + 2] = c.d[2];
    }
    if (keys) keys[i] = c.key;
}

#endif
