// The plan of a mesh refit in plain C++ (no HIP): what cgrt_scene_refit_mesh's kernels (cgrt_refit.hpp) need to recompute the
// boxes of a committed 4-wide hierarchy bottom-up without touching its topology.  Built once per mesh by the first refit from
// the tree's wide nodes and its triangle order, and kept on the handle like the hit-attribute table; a scene that never refits
// pays nothing.  cgrt_scene_refit_plan_host exposes it; tests/test_refit_host.py and tests/native/refit_plan.cpp check it on the
// CPU.
//
// Per wide node: its parent, the slot of the parent whose reference is ~node, and the number of arrivals that complete it --
// one per inner child (the thread that finishes the child writes the child's union into the slot and arrives), plus one for
// the node's own thread, which fits the leaf slots.  Per position j of the hierarchy's triangle order (otris[j]): the
// construction index of the triangle, which is where the caller's tri9 holds it, and the record of tris[] that carries the same
// triangle.  OTriRec::k is that record for either build: a device-built tree keeps tris[] in construction order and k is the
// construction index; a host-built tree keeps tris[] in the reference's leaf order, k is the leaf-order index and
// HostTree::leaf_ids maps it to construction order (what cgrt_ray_queries.hpp's need_tri_ids derives its table from).
//
// The builder also VALIDATES what the kernels will index by: every reference in range, every node but the root referenced
// once, every leaf range inside the triangle order, both maps permutations.  A plan that fails is refused; no kernel runs.
#ifndef CGRT_REFIT_PLAN_H
#define CGRT_REFIT_PLAN_H
#include <cstdint>
#include <vector>

#include "cgrt_types.h"

struct RefitPlan {
    std::vector<int32_t> parent, slot, arrivals;  // per wide node; the root: parent -1, slot 0
    std::vector<int32_t> src, rec;                // per position of the triangle order: construction index, record of tris[]
    int32_t cover_first = 0, n_cover = 0;         // the mesh's spheres in cover[]: [cover_first, cover_first + n_cover)
};

// wide: the tree's nwide nodes, root first; otri_k[j]: OTriRec::k of position j (ntri of them); leaf_ids: leaf-order index ->
// construction index of a host-built tree, nullptr for a device-built one.  Returns nullptr, or what is wrong with the tree.
inline const char *refit_plan(const cgrt::WideNodeRec *wide, int32_t nwide, const int32_t *otri_k, int32_t ntri, const int32_t *leaf_ids,
                              RefitPlan &out) {
    out.parent.assign((size_t)nwide, -1);
    out.slot.assign((size_t)nwide, 0);
    out.arrivals.assign((size_t)nwide, 1);
    out.src.assign((size_t)ntri, -1);
    out.rec.assign((size_t)ntri, -1);
    if (nwide <= 0 || ntri <= 0) return "refit plan: the tree has no 4-wide hierarchy";
    std::vector<uint8_t> referenced((size_t)nwide, 0), covered((size_t)ntri, 0);
    for (int32_t i = 0; i < nwide; i++)
        for (int k = 0; k < 4; k++) {
            const int32_t r = wide[i].ref[k];
            if (r == cgrt::kWideNone) continue;
            if (r >= 0) {  // a leaf: (first position << 4) | count
                const int64_t first = r >> 4, cnt = r & 15;
                if (cnt < 1 || first + cnt > ntri) return "refit plan: a leaf lies outside the triangle order";
                for (int64_t j = first; j < first + cnt; j++)
                    if (covered[(size_t)j]++) return "refit plan: a triangle lies in two leaves";
                continue;
            }
            const int32_t c = ~r;
            if (c <= 0 || c >= nwide) return "refit plan: a child reference lies outside the tree";
            if (referenced[(size_t)c]++) return "refit plan: a node has two parents";
            out.parent[(size_t)c] = i;
            out.slot[(size_t)c] = k;
            out.arrivals[(size_t)i]++;
        }
    for (int32_t i = 1; i < nwide; i++)
        if (!referenced[(size_t)i]) return "refit plan: a node has no parent";
    // every node hangs below the root: following the parents from any node ends at node 0 within nwide steps
    {
        std::vector<uint8_t> rooted((size_t)nwide, 0);
        rooted[0] = 1;
        std::vector<int32_t> path;
        for (int32_t i = 1; i < nwide; i++) {
            path.clear();
            int32_t n = i;
            while (!rooted[(size_t)n]) {
                if ((int32_t)path.size() > nwide) return "refit plan: the parents form a cycle";
                path.push_back(n);
                n = out.parent[(size_t)n];
            }
            for (int32_t p : path) rooted[(size_t)p] = 1;
        }
    }
    std::vector<uint8_t> seen_src((size_t)ntri, 0), seen_rec((size_t)ntri, 0);
    for (int32_t j = 0; j < ntri; j++) {
        if (!covered[(size_t)j]) return "refit plan: a triangle lies in no leaf";
        const int32_t k = otri_k[j];
        if (k < 0 || k >= ntri || seen_rec[(size_t)k]++) return "refit plan: the triangle order is no permutation";
        const int32_t c = leaf_ids ? leaf_ids[k] : k;
        if (c < 0 || c >= ntri || seen_src[(size_t)c]++) return "refit plan: the construction indices are no permutation";
        out.rec[(size_t)j] = k;
        out.src[(size_t)j] = c;
    }
    return nullptr;
}

#endif
