// Grid AOVs: aov_grid_kernel (cgrt_trace_grid_aov) -- per pixel the albedo, shading normal, depth, coverage and object id of
// the camera's first hit.  Part of libcgrt.so (cgrt_hip.hip).  The nearest-hit query of the camera's own rays without the ray
// list: the pixel is the lane (the eye pass's tiles and pixel <-> lane map), the ray comes from camera_ray() in registers, the
// sums stay in registers and the stores are the eye pass's; no queue and no atomics but the workgroup's counter flush.
// Calls the device functions of the other kernels (camera_ray, intersect_scene, surface_color) and changes none of them.
#ifndef CGRT_AOV_HPP
#define CGRT_AOV_HPP
#include "cgrt_aov_plan.h"
#include "cgrt_rays.hpp"

// Kernel arguments behind GridParams (cgrt_grid_aov of cgrt.h; every pointer may be nullptr)
struct AovParams {
    float *albedo, *normal, *depth;
    uint32_t *hits;
    int32_t *obj_id;
};

// The wave's 16x4 pixels of a [rows][W][3] array: the transposed store of trace_grid_body (cgrt_eye.hpp) -- lane l of pass k
// writes float k*64 + l of the wave tile, fetched from the lane that owns that pixel, so a store instruction covers 256
// contiguous bytes of a row.  All 64 lanes call it.  pad_too: rows beyond the image (stripe padding) are written as well.
__device__ __forceinline__ void aov_store3(const GridParams &g, float *__restrict__ dst3, int wx, int wy, int lane, float v0, float v1, float v2,
                                           bool pad_too) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int idx = k * 64 + lane;
        const int row = idx / (kWaveTileW * 3), c = idx % (kWaveTileW * 3);
        const int src = row * kWaveTileW + c / 3, ch = c % 3;
        const float a0 = __shfl(v0, src), a1 = __shfl(v1, src), a2 = __shfl(v2, src);
        const float v = ch == 0 ? a0 : (ch == 1 ? a1 : a2);
        const int jj = wy * kWaveTileH + row, ww = wx * kWaveTileW + c / 3;
        if (jj < g.rows && ww < g.W && (pad_too || global_row(g, jj) < g.H)) {
            float *dst = dst3 + ((size_t)jj * g.W + ww) * 3 + ch;
            *dst = g.accumulate ? *dst + v : v;  // progressive passes add into the fp32 frame
        }
    }
}

// One workgroup per tile (tile_of_block): 32x8 pixels at NT = 256, one 16x4 wave tile at NT = 64.  Per sample every lane of a
// wave enters the scene walk together -- intersect_scene and tree_hit want all 64 -- and the lanes whose pixel lies outside the
// image (right and top edge, stripe padding) ride along switched off: they make no ray, count nothing and store nothing.  A
// wave without any pixel of the image skips the loop.  Lens and pose are GridParams' runtime fields, as in camera_ray.
// Dynamic LDS: aov_ask's layout (cgrt_aov_plan.h), staged as trace_rays_body<FIRST> stages it.
template <bool TREES, bool BEZ, bool SPH, bool SPILL, int NT>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kTreeWaves : 4)) void aov_grid_kernel(DeviceScene sc, GridParams g, AovParams out,
                                                                                          unsigned long long *__restrict__ counters) {
    using TG = TileGeom<NT>;
    int tile_x, tile_y;
    if (!tile_of_block(g, (int)blockIdx.x, tile_x, tile_y, TG::W, TG::H)) return;  // whole workgroup, ahead of every barrier
    __shared__ unsigned long long wg_cnt[CGRT_NCOUNTERS];
    unsigned long long *wc = wg_counters_begin(wg_cnt, counters);

    extern __shared__ __align__(16) unsigned char lds_raw[];
    const WgLdsPtrs lds = ray_wg_begin<NT, TREES, BEZ, false, SPILL>(sc, lds_raw);  // aov_ask's layout, cgrt_aov_plan.h
    ObjRec *const lobjs = lds.lobjs;
    const LdsAux aux = lds.aux;

    // the lane's pixel: wave tile (wx, wy), lane & 15 across and lane >> 4 down, as set_pixel of trace_grid_body
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wtiles_x = (g.W + kWaveTileW - 1) / kWaveTileW, wtiles_y = (g.rows + kWaveTileH - 1) / kWaveTileH;
    const int wx = tile_x * (TG::W / kWaveTileW) + (NT == 256 ? (wave & 1) : 0);
    const int wy = tile_y * (TG::H / kWaveTileH) + (NT == 256 ? (wave >> 1) : 0);
    const bool have_tile = wx < wtiles_x && wy < wtiles_y;  // (wave-uniform)
    const int w = wx * kWaveTileW + (lane & 15), j = wy * kWaveTileH + (lane >> 4);
    const bool inside = have_tile && w < g.W && j < g.rows;  // the pixel is one of the arrays'
    const bool live = inside && global_row(g, j) < g.H;      // ... and of the image: it has rays

    double alb_r = 0, alb_g = 0, alb_b = 0, nrm_x = 0, nrm_y = 0, nrm_z = 0, dep = 0;
    uint32_t px_hits = 0;
    int32_t id0 = -1;
    uint32_t my_rays = 0, my_nodes = 0, my_tris = 0, wave_iters = 0;
    if (__ballot(live) != 0ull) {
        for (int k = 0; k < g.spp; k++) {
            // a lane without a ray carries a harmless one, switched off
            V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
            uint64_t key = 0;
            if (live) {
                const CameraRay c = camera_ray(g, j, w, g.sample_offset + k);
                o = mk(c.o[0], c.o[1], c.o[2]);
                d = mk(c.d[0], c.d[1], c.d[2]);
                key = c.key;
            }
            wave_iters++;
            RayKey rk{key, 1u, false, 0u};
            const SceneHit hit = intersect_scene<TREES, BEZ, SPH, /*STATS*/ false, SPILL, /*PRE*/ false, /*HFONLY*/ false>(
                lobjs, sc.n_lds, sc.n_objs, sc, o, d, rk, live, aux, my_nodes, my_tris);
            if (live) {
                my_rays++;
                if (hit.id >= 0) {
                    px_hits++;
                    if (k == 0) id0 = hit.id;
                    dep += hit.t;
                    if (out.albedo) {
                        const V3 c = surface_color(sc, sc.objs[hit.id], o + d * hit.t);  // cgrt_ray_hit_attributes' color3 at P (main.cpp:68)
                        alb_r += c.x;
                        alb_g += c.y;
                        alb_b += c.z;
                    }
                    if (out.normal) {
                        const V3 n = dot(hit.n, d) > 0 ? -hit.n : hit.n;  // the flip of shade_step (main.cpp:73-76)
                        nrm_x += n.x;
                        nrm_y += n.y;
                        nrm_z += n.z;
                    }
                }
            }
        }
    }

    // ---- stores.  Rows beyond the image get zeros and -1, or under ACCUMULATE nothing
    if (have_tile) {
        const bool pad_too = !g.accumulate;
        if (out.albedo)
            aov_store3(g, out.albedo, wx, wy, lane, (float)(alb_r * g.inv_spp_total), (float)(alb_g * g.inv_spp_total),
                       (float)(alb_b * g.inv_spp_total), pad_too);
        if (out.normal)
            aov_store3(g, out.normal, wx, wy, lane, (float)(nrm_x * g.inv_spp_total), (float)(nrm_y * g.inv_spp_total),
                       (float)(nrm_z * g.inv_spp_total), pad_too);
        if (inside && (pad_too || live)) {
            const size_t px = (size_t)j * g.W + w;
            if (out.depth) {
                const float v = (float)(dep * g.inv_spp_total);
                out.depth[px] = g.accumulate ? out.depth[px] + v : v;
            }
            if (out.hits) out.hits[px] = g.accumulate ? out.hits[px] + px_hits : px_hits;
            if (out.obj_id) out.obj_id[px] = id0;
        }
    }

    ray_counters_flush</*STATS*/ false, /*HITS*/ false>(wc, lane, my_rays, 0u, my_nodes, my_tris, wave_iters);
    wg_counters_end(wg_cnt, counters);
}

// ---- the dispatch table, the launch and the C entry points (cgrt_hip.hip has the handle, the checks and the checked launch) ----
using AovKernel = void (*)(DeviceScene, GridParams, AovParams, unsigned long long *);
struct AovKernels {
    int id;  // AovFlags::id()
    AovKernel fn;
};
#define CGRT_X(T, B, P, SP, NT) AovKernels{AovFlags{T != 0, B != 0, P != 0, SP != 0, NT}.id(), &aov_grid_kernel<T != 0, B != 0, P != 0, SP != 0, NT>},
static const AovKernels kAovKernels[] = {CGRT_AOV_VARIANTS(CGRT_X)};
#undef CGRT_X

static AovPlan aov_plan_for(const cgrt_scene *s, const cgrt_grid *grid) {
    const bool general = rays_general(s->dev);
    const AovKernels *g = general ? variant_row(kAovKernels, aov_flags(rays_general_flags(true))) : nullptr;
    return aov_plan(s->dev, grid->width, grid->rows,
                    AovDevice{general ? device_lds_bytes(s->device) : kLdsBytes,
                              g ? kernel_static_lds(reinterpret_cast<const void *>(g->fn)) : kStaticLdsAllowance});
}
// cgrt_trace_grid's argument checks (check_grid) on a copy whose max_depth passes them: the pass traces first hits only
static int check_aov(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, bool own_ok) {
    if (!s || !cam || !grid || !own_ok) return fail(CGRT_ERR_INVALID, "null argument");
    cgrt_grid g = *grid;
    g.max_depth = 1;
    return check_grid(s, cam, &g);
}
static bool aov_asks(const cgrt_grid_aov *o) { return o->albedo3 || o->normal3 || o->depth || o->hits || o->obj_id; }

extern "C" {

int cgrt_trace_grid_aov(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_grid_aov *out, uint64_t *counters,
                        void *stream) {
    int rc = check_aov(s, cam, grid, out != nullptr);
    if (rc) return rc;
    if (!aov_asks(out)) return CGRT_OK;
    ON_DEVICE(s->device);
    const AovPlan p = aov_plan_for(s, grid);
    const AovKernels *row = variant_row(kAovKernels, p.k);
    if (!row) return fail(CGRT_ERR_UNSUPPORTED, std::string(p.what()) + ": no kernel built for this variant");
    GridParams g = grid_params(cam, grid);
    g.xcd_tiles = p.xcd_tiles ? 1 : 0;
    const AovParams ap{out->albedo3, out->normal3, out->depth, out->hits, out->obj_id};
    if ((rc = launch_checked(row->fn, p.what(), s->device, dim3((unsigned)p.blocks), dim3((unsigned)p.k.nt), p.lds,
                             reinterpret_cast<hipStream_t>(stream), with_resident(s->dev, p.resident), g, ap,
                             reinterpret_cast<unsigned long long *>(counters))))
        return rc;
    HIP_TRY(hipGetLastError());
    return CGRT_OK;
}

int cgrt_trace_grid_aov_host(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, const cgrt_grid_aov *out, uint64_t *counters) {
    int rc = check_aov(s, cam, grid, out != nullptr);
    if (rc) return rc;
    if (!aov_asks(out)) {
        if (counters) std::memset(counters, 0, kCounterBytes);
        return CGRT_OK;
    }
    ON_DEVICE(s->device);
    const size_t npx = (size_t)grid->rows * grid->width;
    cgrt_grid fresh = *grid;  // the device buffers are this call's own: nothing to add to
    fresh.flags &= ~CGRT_GRID_ACCUMULATE;
    HostStage hs;
    cgrt_grid_aov dout{};
    dout.albedo3 = hs.out(out->albedo3, npx * 3 * sizeof(float));
    dout.normal3 = hs.out(out->normal3, npx * 3 * sizeof(float));
    dout.depth = hs.out(out->depth, npx * sizeof(float));
    dout.hits = hs.out(out->hits, npx * sizeof(uint32_t));
    dout.obj_id = hs.out(out->obj_id, npx * sizeof(int32_t));
    uint64_t *d_cnt = hs.out_always(counters, kCounterBytes, true);
    if ((rc = hs.error())) return rc;
    return hs.finish(cgrt_trace_grid_aov(s, cam, &fresh, &dout, d_cnt, nullptr));
}

int cgrt_trace_grid_aov_variant(const cgrt_scene *s, const cgrt_camera *cam, const cgrt_grid *grid, char *name, size_t cap) {
    int rc = check_aov(s, cam, grid, true);
    if (rc) return rc;
    if (!name || cap == 0) return fail(CGRT_ERR_INVALID, "null name buffer");
    ON_DEVICE(s->device);
    aov_plan_for(s, grid).name(name, cap);
    return CGRT_OK;
}

}  // extern "C"

#endif
