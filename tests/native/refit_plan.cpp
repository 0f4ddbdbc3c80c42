// The refit plan (cgrt_refit_plan.h) on host-built hierarchies (HostScene::add_mesh_triangles, cgrt_build.cpp): parents, slots,
// arrival counts and the two triangle maps against the wide nodes they were derived from, and the builder's refusals of trees
// a kernel must never index by.  CPU build under ASan + UBSan, driven by tests/test_refit_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "cgrt_build.h"
#include "cgrt_refit_plan.h"

using namespace cgrt;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

static double unit(uint64_t &state) {
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0;
}

static std::vector<double> soup(int n, uint64_t seed) {
    std::vector<double> t((size_t)n * 9);
    for (int i = 0; i < n; i++) {
        const double c[3] = {-6 + 12 * unit(seed), -14 + 12 * unit(seed), 24 + 12 * unit(seed)};
        for (int v = 0; v < 9; v++) t[(size_t)i * 9 + v] = c[v % 3] + (-1.5 + 3 * unit(seed));
    }
    return t;
}

static std::vector<int32_t> ks(const HostTree &T) {
    std::vector<int32_t> k;
    for (const OTriRec &o : T.otris) k.push_back(o.k);
    return k;
}

static void check_tree(const HostTree &T, int ntri) {
    RefitPlan p;
    const std::vector<int32_t> k = ks(T);
    const char *bad = refit_plan(T.wide.data(), (int32_t)T.wide.size(), k.data(), (int32_t)k.size(), T.leaf_ids.data(), p);
    CHECK(bad == nullptr);
    if (bad) {
        std::printf("  %s\n", bad);
        return;
    }
    const size_t nw = T.wide.size();
    CHECK(p.parent.size() == nw && p.slot.size() == nw && p.arrivals.size() == nw);
    CHECK((int)p.src.size() == ntri && (int)p.rec.size() == ntri);
    CHECK(p.parent[0] == -1);
    std::vector<int> kids(nw, 0), seen_src((size_t)ntri, 0);
    for (size_t i = 1; i < nw; i++) {
        CHECK(p.parent[i] >= 0 && (size_t)p.parent[i] < nw && p.slot[i] >= 0 && p.slot[i] < 4);
        CHECK(T.wide[(size_t)p.parent[i]].ref[p.slot[i]] == ~(int32_t)i);
        kids[(size_t)p.parent[i]]++;
    }
    for (size_t i = 0; i < nw; i++) CHECK(p.arrivals[i] == kids[i] + 1);
    for (int j = 0; j < ntri; j++) {
        CHECK(p.rec[(size_t)j] == T.otris[(size_t)j].k);
        CHECK(p.src[(size_t)j] == T.leaf_ids[(size_t)T.otris[(size_t)j].k]);
        seen_src[(size_t)p.src[(size_t)j]]++;
        // the triangle at position j IS triangle src[j] of the input
        const double *in = &T.tri9[9 * (size_t)p.src[(size_t)j]];
        CHECK(std::memcmp(T.otris[(size_t)j].t.pa, in, 3 * sizeof(double)) == 0);
    }
    for (int c = 0; c < ntri; c++) CHECK(seen_src[(size_t)c] == 1);
}

int main() {
    const double grey[3] = {0.5, 0.5, 0.5};
    for (int n : {1, 2, 4, 5, 17, 333, 5000}) {
        HostScene H;
        const std::vector<double> t = soup(n, 100 + (uint64_t)n);
        const int obj = H.add_mesh_triangles(t.data(), n, grey, 0.0, 0.0, 0);
        CHECK(obj == 0 && H.trees.size() == 1);
        const HostTree &T = H.trees[0];
        CHECK(T.tri_level && !T.wide.empty() && (int)T.otris.size() == n);
        CHECK(T.cover_first == 0 && T.cover_n >= 1 && (size_t)T.cover_n * 4 == H.cover.size());
        check_tree(T, n);
    }
    {   // two meshes: the second one's cover spheres lie behind the first one's
        HostScene H;
        const std::vector<double> a = soup(300, 1), b = soup(700, 2);
        H.add_mesh_triangles(a.data(), 300, grey, 0.0, 0.0, 0);
        H.add_mesh_triangles(b.data(), 700, grey, 0.0, 0.0, 0);
        CHECK(H.trees[1].cover_first == (size_t)H.trees[0].cover_n);
        CHECK((size_t)(H.trees[0].cover_n + H.trees[1].cover_n) * 4 == H.cover.size());
        check_tree(H.trees[1], 700);
    }
    {   // trees no kernel may index by
        HostScene H;
        const std::vector<double> t = soup(200, 9);
        H.add_mesh_triangles(t.data(), 200, grey, 0.0, 0.0, 0);
        const HostTree &T = H.trees[0];
        const std::vector<int32_t> k = ks(T);
        const int32_t nw = (int32_t)T.wide.size(), n = 200;
        RefitPlan p;
        CHECK(refit_plan(T.wide.data(), 0, k.data(), n, T.leaf_ids.data(), p) != nullptr);
        std::vector<WideNodeRec> w = T.wide;
        int leaf_node = -1, leaf_slot = -1, inner_node = -1, inner_slot = -1;
        for (int32_t i = 0; i < nw; i++)
            for (int s = 0; s < 4; s++) {
                if (w[(size_t)i].ref[s] >= 0 && leaf_node < 0) leaf_node = i, leaf_slot = s;
                if (w[(size_t)i].ref[s] < 0 && w[(size_t)i].ref[s] != kWideNone && inner_node < 0) inner_node = i, inner_slot = s;
            }
        CHECK(leaf_node >= 0 && inner_node >= 0);
        w[(size_t)leaf_node].ref[leaf_slot] = (int32_t)(((uint32_t)(n - 1) << 4) | 3u);  // runs past the last triangle
        CHECK(refit_plan(w.data(), nw, k.data(), n, T.leaf_ids.data(), p) != nullptr);
        w = T.wide;
        w[(size_t)inner_node].ref[inner_slot] = ~nw;  // a child beyond the tree
        CHECK(refit_plan(w.data(), nw, k.data(), n, T.leaf_ids.data(), p) != nullptr);
        w = T.wide;
        w[(size_t)inner_node].ref[inner_slot] = ~0;  // the root as a child
        CHECK(refit_plan(w.data(), nw, k.data(), n, T.leaf_ids.data(), p) != nullptr);
        w = T.wide;
        w[(size_t)inner_node].ref[inner_slot] = kWideNone;  // an orphaned subtree
        CHECK(refit_plan(w.data(), nw, k.data(), n, T.leaf_ids.data(), p) != nullptr);
        std::vector<int32_t> k2 = k;
        k2[0] = k2[1];  // no permutation
        CHECK(refit_plan(T.wide.data(), nw, k2.data(), n, T.leaf_ids.data(), p) != nullptr);
        k2 = k;
        k2[0] = n;
        CHECK(refit_plan(T.wide.data(), nw, k2.data(), n, T.leaf_ids.data(), p) != nullptr);
        std::vector<int32_t> ids = T.leaf_ids;
        ids[5] = -1;
        CHECK(refit_plan(T.wide.data(), nw, k.data(), n, ids.data(), p) != nullptr);
        CHECK(refit_plan(T.wide.data(), nw, k.data(), n, T.leaf_ids.data(), p) == nullptr);
    }
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
