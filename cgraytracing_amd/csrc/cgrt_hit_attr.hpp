// Hit attributes of caller-supplied rays: ray_hit_attributes_kernel (cgrt_ray_hit_attributes).  Part of libcgrt.so
// (cgrt_hip.hip).  A pass of its own behind the nearest-hit query, in the shape of ray_normal_sign_kernel: the scene walk
// drops the winning triangle on purpose (SceneHit has no room for it and the eye kernels' registers are measured), so the
// callers who ask get it from a re-walk of the winning object alone, and no existing kernel's code generation changes.
#ifndef CGRT_HIT_ATTR_HPP
#define CGRT_HIT_ATTR_HPP
#include "cgrt_rays.hpp"

// Kernel arguments (cgrt_hit_attributes of cgrt.h; every output pointer may be nullptr)
struct HitAttrParams {
    long long n;
    const double *org, *dir;
    const int32_t *hit_obj;
    const double *hit_t;
    int32_t *prim;
    double *uv, *color, *material;
    const int32_t *tri_ids;  // per record of sc.tris: the triangle's index in its tree's construction order (with prim)
};

// One thread per ray.  The object record comes from sc.objs (HBM / L2): there is no LDS list, so a scene beyond the
// LDS-resident count is served by the same code.  prim / uv: the lanes of a wave hold different objects, and tree_hit() wants
// a wave-uniform tree that all 64 lanes enter together -- so the wave serves ONE tree at a time: ballot the lanes that
// still need a walk, take the first one's tree, walk with on = (my tree is that tree), repeat until no lane is left.  No
// lane returns before that loop (a lane beyond n, a miss or a sphere just never asks for a walk).
// The walk is the scene walk's own (tree_hit), bounded by hit_t: an opaque owner prunes at it and visits little, a transparent
// owner's walk is unpruned and costs what the query's cost.  Both meet every triangle that returns exactly hit_t and decide
// between several of them by the comparison the scene walk used, so the triangle is the one whose normal the query gave.
// h.tri is, for every walk, an index into the tree's tris[] (tree_intersect / _lq: leaf_begin + k; wide: OTriRec::k; height
// field: HCellRec::k): leaf order in a host-built tree, construction order in a device-built one -- tri_ids maps either.
// No LDS: the node cache and the wide walk's LDS stack are null (the stack lives in scratch), as in the function-level probes.
__global__ __launch_bounds__(256) void ray_hit_attributes_kernel(DeviceScene sc, HitAttrParams hp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < hp.n;
    const long long ii = live ? i : 0;  // (n > 0)
    const int id = live ? hp.hit_obj[ii] : -1;
    const bool hit = id >= 0 && id < sc.n_objs;
    const double t = hit ? hp.hit_t[ii] : 0.0;
    const V3 o = ld3(hp.org + 3 * ii), d = ld3(hp.dir + 3 * ii);
    const bool want_tri = hp.prim != nullptr || hp.uv != nullptr;  // (wave-uniform)
    V3 col = mk(0, 0, 0);
    double refl = 0.0, transp = 0.0;
    int tree = -1;
    bool opaque = false;
    if (hit) {
        const ObjRec &ob = sc.objs[id];
        refl = ob.refl;
        transp = ob.transp;
        if (hp.color) col = surface_color(sc, ob, o + d * t);  // P of main.cpp:68
        if (want_tri && (ob.kind == KIND_MESH || ob.kind == KIND_PLANE)) {
            tree = ob.tree;
            opaque = ob.transp < kEps;
        }
    }
    int prim = -1;
    double u = 0.0, v = 0.0;
    if (want_tri) {
        const V3 inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
        LdsAux aux;
        aux.bl = nullptr;
        aux.lnodes = nullptr;
        uint32_t n_node = 0, n_tri = 0;
        bool need = tree >= 0;
        unsigned long long m;
        while ((m = __ballot(need)) != 0ull) {
            const int lead = (int)__ffsll((long long)m) - 1;
            const int tr = __builtin_amdgcn_readfirstlane(__shfl(tree, lead));
            const bool op = __builtin_amdgcn_readfirstlane(__shfl((int)opaque, lead)) != 0;
            const bool on = need && tree == tr && opaque == op;
            const TreeHit h = tree_hit<false>(sc, aux, tr, op, t, on, o, d, inv, n_node, n_tri);
            if (on) {
                need = false;
                if (h.counter > 0 && h.len == t) {
                    const long long at = (long long)load_uniform(&sc.trees[tr].tri_begin) + h.tri;
                    prim = hp.tri_ids ? hp.tri_ids[at] : h.tri;
                    // Triangle::intersect's own quotients (objects.h:101-105), determinants as tri_test spells them
                    const TriRec &T = sc.tris[at];
                    const V3 pa = ld3(T.pa), e1 = ld3(T.e1), e2 = ld3(T.e2);
                    const V3 s = pa - o;
                    const double det1 = det3(d, e1, e2);
                    u = det3(d, s, e2) / det1;
                    v = det3(d, e1, s) / det1;
                }
            }
        }
    }
    if (!live) return;
    if (hp.prim) hp.prim[i] = prim;
    if (hp.uv) {
        hp.uv[2 * i] = u;
        hp.uv[2 * i + 1] = v;
    }
    if (hp.color) {
        double *q = hp.color + 3 * i;
        q[0] = col.x;
        q[1] = col.y;
        q[2] = col.z;
    }
    if (hp.material) {
        hp.material[2 * i] = refl;
        hp.material[2 * i + 1] = transp;
    }
}

#endif
