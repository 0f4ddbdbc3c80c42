// A workgroup's dynamic LDS (cgrt_wg_lds.h: wg_lds and the asks of the kernel families) for every kernel variant that is
// compiled, against byte counts written out from the record sizes: region order, alignment, sizes, the total, the general
// variant's resident limits and HFONLY's empty tree regions.  CPU build under ASan + UBSan, driven by tests/test_wg_lds_host.py.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "cgrt_variants.h"

static int g_failed = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        if (a_ != b_) {                                                                                         \
            std::printf("FAIL %s:%d: %s == %lld, expected %s == %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
            g_failed++;                                                                                         \
        }                                                                                                       \
    } while (0)

// The flag tuples of the compiled kernels: the two lists of cgrt_variants.h, expanded (the capture and occlusion kernels take
// their trace_rays_kernel's flags and LDS)
struct Eye { int T, B, D, G, P, S, H, NT, SP, HF, DF, PR, ST, LT, SCHED; };
#define X(...) {__VA_ARGS__},
static const Eye kEye[] = {CGRT_EYE_VARIANTS(X)};
struct Rays { int T, B, G, P, S, SP, F, NT; };
static const Rays kRays[] = {CGRT_RAY_VARIANTS(X)};
#undef X
static EyeFlags eye_flags(const Eye &e) {
    return {e.T != 0, e.B != 0, e.D != 0, e.G != 0, e.P != 0, e.S != 0, e.H != 0, e.SP != 0, e.HF != 0, e.NT, e.DF != 0, e.PR != 0, e.ST != 0, e.LT != 0};
}
static const int kCounts[] = {0, 1, 255, 257, 600, 727, 768};

// regions in the documented order, each 16-byte aligned, of the given sizes (so disjoint), the total the end of the last one
static void check_regions(const WgLds &l, long long pending, long long objs, long long staging, long long bez, long long nodes, long long wstack) {
    const size_t at[] = {l.pending, l.objs, l.staging, l.bez, l.nodes, l.wstack, l.total};
    const long long size[] = {pending, objs, staging, bez, nodes, wstack};
    CHECK_EQ(l.pending, 0);
    for (int i = 0; i < 6; i++) {
        CHECK_EQ(at[i] % 16, 0);
        CHECK_EQ((long long)at[i + 1] - (long long)at[i], size[i]);
    }
    CHECK_EQ(l.total, pending + objs + staging + bez + nodes + wstack);
}

// a trace_grid / trace_rays variant (HF: eye pass only) over the object counts, with and without a 255-node cached tree and a wide tree
static void check_trace(int T, int B, int G, int SP, int HF, int NT) {
    const WgLdsAsk a = wg_ask_trace(NT, T != 0, B != 0, G != 0, SP != 0, HF != 0);
    for (int n : kCounts)
        for (int nodes : {0, 255})
            for (int wide = 0; wide < 2; wide++) {
                const WgLds l = wg_lds(a, (size_t)n, (size_t)nodes, wide != 0);
                const long long waves = NT / 64;
                const long long pending = G ? (NT == 256 ? 38912 : 38912 / 4) : 0;
                const long long tree_nodes = (T && !HF) ? nodes * 32 : 0;
                const long long wstack = (T && !HF && !G && !B && wide) ? 32768 : 0;
                check_regions(l, pending, n * 128, SP ? waves * 128 : 0, B ? waves * 7872 : 0, tree_nodes, wstack);
                CHECK_EQ(l.total, pending + (n + (SP ? waves : 0)) * 128 + (B ? waves * 7872 : 0) + tree_nodes + wstack);
                CHECK_EQ(l.level_bytes, NT * (9 * 8 + 4));
                if (HF) {  // no node and no wide-stack region, whatever the scene
                    CHECK_EQ(l.wstack, l.nodes);
                    CHECK_EQ(l.total, l.wstack);
                    CHECK_EQ(l.has.nodes || l.has.wstack, 0);
                }
                CHECK_EQ(l.has.wstack, wstack != 0);
                CHECK_EQ(l.has.nodes, tree_nodes != 0);  // no cached tree: no node region to stage into
                // the scene overload reads the same numbers; a scene without a cached tree has no nodes whatever cached_nodes says
                cgrt::DeviceScene sc{};
                sc.n_lds = n;
                sc.cached_tree = nodes ? 3 : -1;
                sc.cached_nodes = nodes ? nodes : 77;
                sc.has_wide = wide;
                CHECK_EQ(wg_lds(a, sc).total, l.total);
                CHECK_EQ(wg_lds(a, sc).wstack, l.wstack);
                CHECK_EQ(wg_lds(a, sc).has.nodes, tree_nodes != 0);
            }
}

// largest resident count with which the variant fits a workgroup's 163 840 B beside `st` static bytes
static int resident_limit(const WgLdsAsk &a, int nodes, int st) {
    int r = 0;
    while (wg_lds(a, (size_t)(r + 1), (size_t)nodes, false).total + st <= 163840) r++;
    return r;
}

int main() {
    for (const Eye &e : kEye) check_trace(e.T, e.B, e.G, e.SP, e.HF, e.NT);
    for (const Rays &r : kRays) check_trace(r.T, r.B, r.G, r.SP, 0, r.NT);
    // a START or LTAB twin is its PAIR parent with another body: the parent is compiled too, and the twin's LDS is the parent's
    int twins = 0;
    for (const Eye &e : kEye) {
        if (!e.ST && !e.LT) continue;
        twins++;
        CHECK_EQ(e.PR, 1);
        Eye parent = e;
        parent.ST = parent.LT = 0;
        int found = 0;
        for (const Eye &p : kEye) found += eye_flags(p).id() == eye_flags(parent).id();
        CHECK_EQ(found, 1);
        for (int n : kCounts)
            for (int nodes : {0, 255})
                for (int wide = 0; wide < 2; wide++)
                    CHECK_EQ(eye_lds(eye_flags(e), (size_t)n, (size_t)nodes, wide != 0), eye_lds(eye_flags(parent), (size_t)n, (size_t)nodes, wide != 0));
    }
    CHECK_EQ(twins, 4);
    // an HFONLY variant of any other shape has no tree regions either
    for (int G = 0; G < 2; G++)
        for (int B = 0; B < 2; B++) check_trace(1, B, G, 0, 1, B ? 64 : 256);
    // photon_trace_kernel<BEZ, SPILL, RAYS> (RAYS changes nothing in LDS); `wide` is photon_lds_stack's answer
    for (int bez = 0; bez < 2; bez++)
        for (int spill = 0; spill < 2; spill++)
            for (int n : kCounts)
                for (int wide = 0; wide < 2; wide++) {
                    const WgLds l = wg_lds(wg_ask_photon(bez != 0, spill != 0), (size_t)n, 0, wide != 0);
                    const long long wstack = (!bez && !spill && wide) ? 32768 : 0;
                    check_regions(l, 0, n * 128, spill ? 4 * 128 : 0, bez ? 4 * 7872 : 0, 0, wstack);
                    CHECK_EQ(l.total, (n + (spill ? 4 : 0)) * 128 + (bez ? 4 * 7872 : 0) + wstack);
                }
    // primary_walk_kernel: the objects it stages, then the stack
    for (int n : kCounts) {
        const WgLds l = wg_lds(wg_ask_primary_walk(), (size_t)n, 0, true);
        check_regions(l, 0, n * 128, 0, 0, 0, 32768);
        CHECK_EQ(l.total, n * 128 + 32768);
    }
    // the general variant (trees, Bezier, pending rays; 336 B static): 727 resident objects, 663 beside a 255-node tree; four
    // fewer beside one staging record per wave
    CHECK_EQ(resident_limit(wg_ask_trace(256, true, true, true, false, false), 0, 336), 727);
    CHECK_EQ(resident_limit(wg_ask_trace(256, true, true, true, false, false), 255, 336), 663);
    CHECK_EQ(resident_limit(wg_ask_trace(256, true, true, true, true, false), 0, 336), 723);
    CHECK_EQ(resident_limit(wg_ask_trace(256, true, true, true, true, false), 255, 336), 659);
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
