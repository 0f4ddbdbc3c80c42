// Occlusion queries for caller-supplied rays: occlusion_rays_kernel (cgrt_occlusion_rays).  Part of libcgrt.so (cgrt_hip.hip).
// "Is some object's intersect() length below tmax?" -- the lengths are those of the nearest-hit query (intersect_scene,
// cgrt_scene_walk.hpp), computed by the same functions; what differs is the walk: a lane that has found one blocker is done,
// takes no part in any later object, and the wave leaves the object list as soon as none of its lanes is still looking.
// Nothing of shading, pending rays or normals exists here.  DESIGN.md section 4.17, "Occlusion queries".
#ifndef CGRT_OCCLUSION_HPP
#define CGRT_OCCLUSION_HPP
#include "cgrt_rays.hpp"

// Kernel arguments of occlusion_rays_kernel (cgrt_rays / cgrt_occlusion of cgrt.h)
struct OccParams {
    RayInput in;
    const double *tmax;  // nullptr: kInf for every ray
    uint8_t *occluded;
    unsigned int *queue;  // head of the block queue (block = 64 consecutive rays), zeroed before the launch
    int32_t skip_transparent, pad_;
};

// =====================================================================================================
// any-hit forms of the tree walks (cgrt_traverse.hpp): the same boxes, the same triangle test, the same `len`; a walk
// ends at the first triangle it accepts with len < tmax (tmax <= kInf: a length that the leaf scans would not have kept,
// objects.h:278, is no hit here either)
// =====================================================================================================

// tree_intersect_wide with bound = tmax throughout: no child order, a lane stops at its first accepted triangle
template <bool STATS>
__device__ __forceinline__ bool tree_occluded_wide(const WideNodeRec *__restrict__ wn, const OTriRec *__restrict__ otris, V3 o, V3 d,
                                                   const Ray32 &r32, double tmax, uint32_t &n_node, uint32_t &n_tri, uint2 *lstack) {
    const float bound32 = __double2float_ru(tmax);  // >= tmax: an entry distance above it is above tmax
    // the stack holds references only where tree_intersect_wide keeps {ref, entry distance}: same depth, same LDS part
    int32_t stk[kWideStack];
    int sp = 0;
    const int nt = blockDim.x, tid = threadIdx.x;
    auto pop = [&]() -> int32_t {
        if (sp == 0) return kWideNone;
        --sp;
        return (lstack && sp < kWideLdsDepth) ? reinterpret_cast<const int32_t *>(lstack + sp * nt + tid)[0] : stk[sp];
    };
    int32_t nxt = ~0;  // the root
    while (true) {
        while (nxt < 0 && nxt != kWideNone) {  // inner nodes, all lanes together, until this lane stands on a leaf or has nothing left
            const float4 *q = reinterpret_cast<const float4 *>(wn + (~nxt));
            const float4 lox = q[0], loy = q[1], loz = q[2], hix = q[3], hiy = q[4], hiz = q[5];
            const int4 ref = reinterpret_cast<const int4 *>(q)[6];
            const float lx[4] = {lox.x, lox.y, lox.z, lox.w}, ly[4] = {loy.x, loy.y, loy.z, loy.w}, lz[4] = {loz.x, loz.y, loz.z, loz.w};
            const float hx[4] = {hix.x, hix.y, hix.z, hix.w}, hy[4] = {hiy.x, hiy.y, hiy.z, hiy.w}, hz[4] = {hiz.x, hiz.y, hiz.z, hiz.w};
            const int32_t rf[4] = {ref.x, ref.y, ref.z, ref.w};
            nxt = kWideNone;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float tn, tf;
                slab32(r32, lx[k], ly[k], lz[k], hx[k], hy[k], hz[k], tn, tf);
                if (STATS && rf[k] != kWideNone) n_node++;
                if ((rf[k] != kWideNone) && (tf > 0.f) && (tn <= tf) && !(tn > bound32)) {
                    if (nxt == kWideNone) {
                        nxt = rf[k];
                    } else {  // (cgrt_build.cpp bounds a wide tree's depth so that kWideStack cannot overflow)
                        if (lstack && sp < kWideLdsDepth) reinterpret_cast<int32_t *>(lstack + sp * nt + tid)[0] = rf[k];
                        else stk[sp] = rf[k];
                        sp++;
                    }
                }
            }
            if (nxt == kWideNone) nxt = pop();
        }
        if (nxt == kWideNone) break;
        const OTriRec *tp = otris + (nxt >> 4);
        const int cnt = nxt & 15;
        for (int k = 0; k < cnt; k++) {
            if (STATS) n_tri++;
            double len;
            if (tri_test(tp[k].t, o, d, len) && len < tmax) return true;
        }
        nxt = pop();
    }
    return false;
}

// hfield_intersect with bound = tmax: the ray's range is clipped to (0, tmax] once, the columns are visited as there, and the
// walk ends at the first accepted triangle
template <bool STATS>
__device__ __forceinline__ bool hfield_occluded(const HFieldRec &H, const HCellRec *__restrict__ cells, const HCellY *__restrict__ celly,
                                                V3 o, V3 d, V3 inv, double tmax, uint32_t &n_node, uint32_t &n_tri) {
    double ta = 0.0, tb = tmax;
    const double lo[3] = {H.x0 - kHfPad, H.ylo - kHfPad, H.z0 - kHfPad};
    const double hi[3] = {H.x0 + H.hx * H.nx + kHfPad, H.yhi + kHfPad, H.z0 + H.hz * H.nz + kHfPad};
    const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, ii[3] = {inv.x, inv.y, inv.z};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (dd[k] != 0.0) {
            const double t1 = (lo[k] - oo[k]) * ii[k], t2 = (hi[k] - oo[k]) * ii[k];
            ta = fmax(ta, fmin(t1, t2));
            tb = fmin(tb, fmax(t1, t2));
        } else if (oo[k] < lo[k] || oo[k] > hi[k]) {
            tb = -1.0;
        }
    }
    if (!(ta <= tb)) return false;
    const bool xmaj = fabs(d.x) * H.hz >= fabs(d.z) * H.hx;
    const double oM = xmaj ? o.x : o.z, dM = xmaj ? d.x : d.z, iM = xmaj ? inv.x : inv.z;
    const double om = xmaj ? o.z : o.x, dm = xmaj ? d.z : d.x;
    const double M0 = xmaj ? H.x0 : H.z0, hM = xmaj ? H.hx : H.hz, m0 = xmaj ? H.z0 : H.x0;
    const int nM = xmaj ? H.nx : H.nz, nm = xmaj ? H.nz : H.nx;
    const double ihM = xmaj ? H.ihx : H.ihz, ihm = xmaj ? H.ihz : H.ihx;
    const double Ma = oM + dM * ta, Mb = oM + dM * tb;
    int j0 = (int)floor((fmin(Ma, Mb) - kHfPad - M0) * ihM), j1 = (int)floor((fmax(Ma, Mb) + kHfPad - M0) * ihM);
    j0 = j0 < 0 ? 0 : j0;
    j1 = j1 > nM - 1 ? nM - 1 : j1;
    const int step = dM >= 0.0 ? 1 : -1;
    const int jn = j1 - j0 + 1;
    int j = step > 0 ? j0 : j1;
    for (int c = 0; c < jn; c++, j += step) {
        double s0 = ta, s1 = tb;
        if (dM != 0.0) {
            const double t1 = (M0 + hM * j - kHfPad - oM) * iM, t2 = (M0 + hM * (j + 1) + kHfPad - oM) * iM;
            s0 = fmax(s0, fmin(t1, t2));
            s1 = fmin(s1, fmax(t1, t2));
        }
        if (!(s0 <= s1)) continue;
        const double ma = om + dm * s0, mb = om + dm * s1;
        int i0 = (int)floor((fmin(ma, mb) - kHfPad - m0) * ihm), i1 = (int)floor((fmax(ma, mb) + kHfPad - m0) * ihm);
        i0 = i0 < 0 ? 0 : i0;
        i1 = i1 > nm - 1 ? nm - 1 : i1;
        const double ya = o.y + d.y * s0, yb = o.y + d.y * s1;
        const double ymin = fmin(ya, yb) - kHfPad, ymax = fmax(ya, yb) + kHfPad;
        for (int i = i0; i <= i1; i++) {
            const size_t ci = xmaj ? (size_t)i * H.nx + j : (size_t)j * H.nx + i;
            const HCellY cy = celly[ci];
            if (ymin > (double)cy.hi || ymax < (double)cy.lo) continue;
            if (STATS) n_node++;
            const HCellRec *cell = cells + ci;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (STATS) n_tri++;
                double len;
                if (tri_test(cell->t[q], o, d, len) && len < tmax) return true;
            }
        }
    }
    return false;
}

// tree_intersect_lq with its node gating unchanged -- a triangle is tested only if every box on its path and its own box
// pass the slab test, so the triangles that are REACHED are the query's -- and another stopping rule: a lane that has accepted
// a reached triangle with len < tmax walks no further node and drops its queued leaves.
template <bool STATS>
__device__ __forceinline__ bool tree_occluded_lq(const NodeRec *__restrict__ nodes, const TriRec *__restrict__ tris, int nnodes, V3 o,
                                                 V3 d, const Ray32 &r32, double tmax, uint32_t &n_node, uint32_t &n_tri,
                                                 const NodeRec *__restrict__ tboxes) {
    bool found = false;
    int i = 0;
    int lq0 = 0, lq1 = 0, lq2 = 0, lq3 = 0, nl = 0;  // queued leaves (NodeRec::leaf), oldest in lq0
    while (true) {
        for (int st = 0; st < kLqSteps; st++) {
            const bool can = i < nnodes && nl < 4;
            if (__ballot(can) == 0ull) break;
            if (can) {
                const float4 q0 = reinterpret_cast<const float4 *>(nodes + i)[0];  // lo.x lo.y lo.z hi.x
                const float4 q1 = reinterpret_cast<const float4 *>(nodes + i)[1];  // hi.y hi.z skip leaf
                if (STATS) n_node++;
                float tn, tf;
                slab32(r32, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tn, tf);
                const bool touch = (tf > 0.f) && (tn <= tf);
                const int leaf = __float_as_int(q1.w);
                if (!touch) {
                    i = __float_as_int(q1.z);
                } else {
                    i = i + 1;
                    if (leaf >= 0) {
                        if (nl == 0) lq0 = leaf;
                        else if (nl == 1) lq1 = leaf;
                        else if (nl == 2) lq2 = leaf;
                        else lq3 = leaf;
                        nl++;
                    }
                }
            }
        }
        const unsigned long long walkers = __ballot(i < nnodes && nl < 4);
        const unsigned long long holders = __ballot(nl > 0);
        if (walkers == 0ull && holders == 0ull) break;
        // (the lanes that still look: tree_intersect_lq's quorum, taken over them)
        if (walkers != 0ull && kLqDen * (int)__popcll(holders) < kLqNum * (int)__popcll(__ballot(!found))) continue;
        if (nl > 0) {
            const int leaf_begin = lq0 >> 4, leaf_cnt_tris = lq0 & 15;
            lq0 = lq1;
            lq1 = lq2;
            lq2 = lq3;
            nl--;
            const TriRec *tp = tris + leaf_begin;
            const NodeRec *bp = tboxes + leaf_begin;
            unsigned cand = 0;
            for (int k = 0; k < leaf_cnt_tris; k++) {
                const float4 q0 = reinterpret_cast<const float4 *>(bp + k)[0];  // lo.x lo.y lo.z hi.x
                const float2 q1 = reinterpret_cast<const float2 *>(bp + k)[2];  // hi.y hi.z
                float tn, tf;
                slab32(r32, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tn, tf);
                if ((tf > 0.f) && (tn <= tf)) cand |= 1u << k;
            }
            while (cand != 0u) {
                const int k = __ffs((int)cand) - 1;
                cand &= cand - 1u;
                if (STATS) n_tri++;
                double len;
                if (tri_test(tp[k], o, d, len) && len < tmax) {
                    found = true;
                    i = nnodes;
                    nl = 0;
                    break;
                }
            }
        }
    }
    return found;
}

// tree_hit's dispatch (cgrt_scene_walk.hpp) over the any-hit forms; `on` = this lane is still looking and has a ray for this tree
template <bool STATS>
__device__ __forceinline__ bool tree_occluded(const DeviceScene &sc, const LdsAux &aux, int tr, bool opaque, double tmax, bool on, V3 o,
                                              V3 d, V3 inv, uint32_t &n_node, uint32_t &n_tri) {
    const TreeRec T = load_uniform(sc.trees + tr);
    if (!on) return false;
    if (opaque && T.hfield >= 0) {
        const HFieldRec H = load_uniform(sc.hfields + T.hfield);
        return hfield_occluded<STATS>(H, sc.hcells + H.cell_begin, sc.hcell_y + H.cell_begin, o, d, inv, tmax, n_node, n_tri);
    }
    const bool cached = aux.lnodes != nullptr && tr == sc.cached_tree;
    const Ray32 r32 = make_ray32(o, inv, T.bmax);
    const NodeRec *nodes = sc.nodes + T.node_begin;
    const TriRec *tris = sc.tris + T.tri_begin;
    if (opaque) {
        if (T.tri_level) {
            if (T.nwide == 0) return false;
            return tree_occluded_wide<STATS>(sc.wnodes + T.wnode_begin, sc.otris + T.otri_begin, o, d, r32, tmax, n_node, n_tri, aux.wstack);
        }
        // an opaque owner whose stackless hierarchy is walked as it is (CGRT_TREE=ref; a bump floor without a grid): the pruned
        // nearest-hit walk bounded by tmax -- rare enough not to carry a fourth any-hit form
        const TreeHit h = cached ? tree_intersect<STATS, true>(aux.lnodes, tris, T.nnodes, o, d, r32, tmax, n_node, n_tri)
                                 : tree_intersect<STATS, true>(nodes, tris, T.nnodes, o, d, r32, tmax, n_node, n_tri);
        return h.counter > 0 && h.len < tmax;
    }
    const NodeRec *tb = sc.tboxes + T.tbox_begin;
    if (cached) return tree_occluded_lq<STATS>(aux.lnodes, tris, T.nnodes, o, d, r32, tmax, n_node, n_tri, tb);
    return tree_occluded_lq<STATS>(nodes, tris, T.nnodes, o, d, r32, tmax, n_node, n_tri, tb);
}

// =====================================================================================================
// the walk over the object list
// =====================================================================================================
// Returns, per lane, whether some occluder's length is below tmax (tmax <= kInf, not NaN, for a lane that is `on`).  All lanes of the
// wave call it.  `skip` (wave-uniform): objects whose transparency is >= kEps are no occluders.
// The order of the objects is free for a boolean, so the cheap kinds go first: spheres and the planes' own distances (pass A),
// then the trees -- bump floors and meshes -- (pass B), then the Bezier objects in list order (pass C).  Each Bezier object's
// solve draws from the stream purpose_key(key, (1 << 16) | (object + 1)) at position 0, as in the query's walk of a caller's ray.
// Objects beyond the LDS list (SPILL) are read as intersect_scene reads them.
template <bool TREES, bool BEZ, bool SPH, bool STATS, bool SPILL>
__device__ __forceinline__ bool occluded_scene(const ObjRec *__restrict__ objs, int n_lds, int n_objs, const DeviceScene &sc, V3 o, V3 d,
                                               uint64_t key, bool on, double tmax, bool skip, const LdsAux &aux, uint32_t &n_node,
                                               uint32_t &n_tri) {
    bool done = false;
    if (SPH) {
        int i_single = 0;
        if (!SPILL) {  // the pair form
            for (int i = 0; i + 1 < n_lds; i += 2) {
                double lenA, lenB;
                const ObjRec &A = objs[i], &B = objs[i + 1];
                sphere_len_pair(ld3(A.a), A.s0, ld3(B.a), B.s0, o, d, lenA, lenB);
                const bool useA = !(skip && !(A.transp < kEps)), useB = !(skip && !(B.transp < kEps));  // (wave-uniform)
                done = done || (useA && lenA < tmax) || (useB && lenB < tmax);
                if (__ballot(on && !done) == 0ull) return on && done;
            }
            i_single = n_lds & ~1;
        }
        for (int i = i_single; i < n_lds; i++) {
            if (skip && !(objs[i].transp < kEps)) continue;
            done = done || sphere_len(objs[i], o, d) < tmax;
            if (__ballot(on && !done) == 0ull) return on && done;
        }
        for (int i = n_lds; SPILL && i < n_objs; i++) {
            if (skip && !(load_uniform(&sc.objs[i].transp) < kEps)) continue;
            const ObjHead h = load_uniform(reinterpret_cast<const ObjHead *>(sc.objs + i));
            done = done || sphere_len(mk(h.a[0], h.a[1], h.a[2]), h.s0, o, d) < tmax;
            if (__ballot(on && !done) == 0ull) return on && done;
        }
        return on && done;
    }
    const int n_all = SPILL ? n_objs : n_lds;
    // stages object i (>= n_lds) in this wave's LDS slot, as intersect_scene does
    auto staged = [&](int i) -> const ObjRec * {
        if (!SPILL || i < n_lds) return objs + i;
        if ((threadIdx.x & 63) < 8)
            reinterpret_cast<uint4 *>(aux.spill)[threadIdx.x & 63] = reinterpret_cast<const uint4 *>(sc.objs + i)[threadIdx.x & 63];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        return aux.spill;
    };
    auto kind_of = [&](int i) -> int {
        if (!SPILL || i < n_lds) return __builtin_amdgcn_readfirstlane(objs[i].kind);
        return load_uniform(&sc.objs[i].kind);
    };

    // ---- pass A: spheres and planes --------------------------------------------------------------------------------------
    // The run of axis-aligned planes (plane_run): a lane that is sure of the run's smallest positive distance needs nothing else
    // of the run -- some plane of it is below tmax exactly when that one is.
    bool run_sure = false;
    int run_begin = 0, run_end = 0;
    if (sc.prun_end > 0 && sc.prun_end <= n_lds) {  // (wave-uniform)
        bool usable = true;
        for (int j = sc.prun_begin; skip && j < sc.prun_end; j++) usable = usable && objs[j].transp < kEps;
        if (__builtin_amdgcn_readfirstlane((int)usable) != 0) {
            run_begin = sc.prun_begin;
            run_end = sc.prun_end;
            const PlaneRunHit ph = plane_run(objs, run_begin, run_end, o, d);
            run_sure = !ph.unsure;
            if (run_sure && ph.id >= 0 && ph.len > 0 && ph.len < tmax) done = true;
            if (__ballot(on && !done) == 0ull) return on && done;
        }
    }
    const bool run_skip = __ballot(on && !done && !run_sure) == 0ull;
    for (int i = 0; i < n_all; i++) {
        if (i >= run_begin && i < run_end && run_skip) continue;
        const int kind = kind_of(i);
        if (kind != KIND_SPHERE && kind != KIND_PLANE) continue;
        const ObjRec &ob = *staged(i);
        if (skip && __builtin_amdgcn_readfirstlane((int)(ob.transp < kEps)) == 0) continue;
        if (kind == KIND_SPHERE) {
            done = done || sphere_len(ob, o, d) < tmax;
        } else {
            // the plane's own distance; a bump hit can only be nearer (objects.h:514), so a plane below tmax needs no tree
            const double len = plane_len(ob, ld3(ob.b), o, d);
            const bool mine = !(i >= run_begin && i < run_end && run_sure);
            done = done || (mine && len > 0 && len < tmax);
        }
        if (__ballot(on && !done) == 0ull) return on && done;
    }

    // ---- pass B: trees ---------------------------------------------------------------------------------------------------
    if (TREES && sc.has_mesh != 0) {
        V3 inv = mk(0, 0, 0);
        bool inv_ready = false;  // wave-uniform
        for (int i = 0; i < n_all; i++) {
            const int kind = kind_of(i);
            if (kind != KIND_PLANE && kind != KIND_MESH) continue;
            if (kind == KIND_PLANE && i < n_lds && __builtin_amdgcn_readfirstlane(objs[i].tree) < 0) continue;
            const ObjRec &ob = *staged(i);
            const int tr = __builtin_amdgcn_readfirstlane(ob.tree);
            if (tr < 0) continue;
            const bool opaque = __builtin_amdgcn_readfirstlane((int)(ob.transp < kEps)) != 0;
            if (skip && !opaque) continue;
            bool want;
            if (kind == KIND_PLANE) {
                // the bump tree is consulted when the plane is hit (objects.h:508-513); the plane itself is at or beyond tmax
                // here, so a bump triangle below tmax is nearer than the plane
                const double len = plane_len(ob, ld3(ob.b), o, d);
                want = on && !done && len > 0;
            } else {
                want = on && !done && mesh_may_hit(ob, o, d);
            }
            want = want && tmax > 0;  // an accepted triangle's length is det2 / det1 of one sign: never below zero
            if (__ballot(want) == 0ull) continue;
            if (!inv_ready) {
                inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
                inv_ready = true;
            }
            const bool h = tree_occluded<STATS>(sc, aux, tr, opaque, tmax, want, o, d, inv, n_node, n_tri);
            done = done || (want && h);
            if (__ballot(on && !done) == 0ull) return on && done;
        }
    }

    // ---- pass C: Bezier objects, in list order ---------------------------------------------------------------------------
    if (BEZ && sc.has_bezier != 0) {
        for (int i = 0; i < n_all; i++) {
            if (kind_of(i) != KIND_BEZIER) continue;
            const ObjRec &ob = *staged(i);
            if (skip && __builtin_amdgcn_readfirstlane((int)(ob.transp < kEps)) == 0) continue;
            const int bi = __builtin_amdgcn_readfirstlane(ob.aux);
            const uint64_t bkey = purpose_key(key, ((uint64_t)1 << 16) | (uint64_t)(i + 1));
            double len = 0;
            V3 nrm = mk(0, 0, 0);
            uint32_t n0 = 0u;
            const bool bh = bezier_wave(sc.beziers[bi], ld3(ob.a), ob.b[0], on && !done, o, d, bkey, n0, len, nrm, aux.bl,
                                        sc.bez_slabs ? sc.bez_slabs + (size_t)bi * kBezSlabs : nullptr);
            done = done || (bh && len < tmax);
            if (__ballot(on && !done) == 0ull) return on && done;
        }
    }
    return on && done;
}

// Persistent workgroups of NT threads, as trace_rays_body: a wave draws blocks of 64 consecutive rays from one queue counter
// (lane 0's atomic, the next block's already in flight while the current one is walked).  A ray is one walk, so lane k of the
// wave takes ray k of the block and the block's 64 results leave as one coalesced store of bytes.
// Dynamic LDS: wg_ask_trace's layout without pending rays (cgrt_wg_lds.h), that of trace_rays_kernel<..., FIRST>.
template <bool TREES, bool BEZ, bool SPH, bool STATS, bool SPILL, int NT>
__global__ __launch_bounds__(NT, BEZ ? kBezWaves : (TREES ? kTreeWaves : 4)) void occlusion_rays_kernel(DeviceScene sc, OccParams rp,
                                                                                                    unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long wg_cnt[CGRT_NCOUNTERS];
    unsigned long long *wc = wg_counters_begin(wg_cnt, counters);

    extern __shared__ __align__(16) unsigned char lds_raw[];
    const WgLdsPtrs lds = ray_wg_begin<NT, TREES, BEZ, false, SPILL>(sc, lds_raw);
    ObjRec *const lobjs = lds.lobjs;
    const LdsAux aux = lds.aux;

    const int lane = threadIdx.x & 63;
    const unsigned n_blocks = (unsigned)((rp.in.n + 63) >> 6);
    const bool skip = rp.skip_transparent != 0;
    uint32_t my_rays = 0, my_nodes = 0, my_tris = 0, wave_iters = 0;
    // Lane k takes ray k of a block, so of RayBlocks (cgrt_ray_wave.hpp) only the fetch-ahead is left, and a wave that finds the
    // queue empty asks for nothing more: written out
    unsigned block_ahead = 0;
    if (lane == 0) block_ahead = atomicAdd(rp.queue, 1u);
    while (true) {
        const unsigned blk = (unsigned)__builtin_amdgcn_readfirstlane((int)block_ahead);
        if (blk >= n_blocks) break;
        if (lane == 0) block_ahead = atomicAdd(rp.queue, 1u);
        const long long u = ((long long)blk << 6) + lane;
        const bool in = u < rp.in.n;
        V3 o = mk(0, 0, 0), d = mk(0, 0, 0);
        double tmax = kInf;
        uint64_t key = 0;
        if (in) {
            o = ld3(rp.in.org + 3 * u);
            d = ld3(rp.in.dir + 3 * u);
            if (rp.tmax) tmax = rp.tmax[u];
        }
        const bool ray = in && !ray_is_none(d);  // nothing counted
        // A NaN tmax admits nothing and is answered without a walk.  tmax <= 0 is walked: Sphere::intersect and the Bezier cap
        // can return a length below zero (a ray that starts on a sphere's surface within rounding), which the query keeps
        const bool on = ray && tmax == tmax;
        if (BEZ && on) key = ray_default_key(rp.in, u);
        tmax = fmin(tmax, kInf);
        if (ray) my_rays++;
        bool occ = false;
        if (__ballot(on) != 0ull) {
            wave_iters++;
            occ = occluded_scene<TREES, BEZ, SPH, STATS, SPILL>(lobjs, sc.n_lds, sc.n_objs, sc, o, d, key, on, tmax, skip, aux, my_nodes,
                                                                 my_tris);
        }
        if (in) rp.occluded[u] = occ ? (uint8_t)1 : (uint8_t)0;
    }

    ray_counters_flush<STATS, false>(wc, lane, my_rays, 0u, my_nodes, my_tris, wave_iters);
    wg_counters_end(wg_cnt, counters);
}

#endif
