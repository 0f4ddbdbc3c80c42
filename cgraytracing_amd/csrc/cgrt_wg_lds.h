// A workgroup's dynamic LDS in plain C++ (no HIP): which regions a kernel variant asks for, where each begins and how many
// bytes the launch must request.  The host (the launch plans of cgrt_hip.hip) and the kernels (wg_lds_carve,
// cgrt_scene_walk.hpp) both take their numbers from wg_lds() below; tests/native/wg_lds.cpp checks it on the CPU.
// trace_grid_body (cgrt_eye.hpp) alone writes the same regions out by hand.
//
// Regions, in this order, each 16-byte aligned (every record size is a multiple of 16):
//   pending-ray levels | resident objects | one staging record per wave | one BezLds per wave | node cache | wide-walk stack
#ifndef CGRT_WG_LDS_H
#define CGRT_WG_LDS_H
#include "cgrt_rng.hpp"  // CGRT_HD
#include "cgrt_types.h"

// Pending refracted rays (main.cpp:157) of a lane, newest last (trace_grid_body, cgrt_eye.hpp; trace_rays_body, cgrt_rays.hpp):
//   * a glass hit whose children are leaves of the recursion keeps the refracted child in REGISTERS (it is consumed right
//     after the reflected child, before any other push) -- in a full glass tree that is 8 of the 15 pushes;
//   * the first two other levels live in LDS: per level 9 doubles + one packed (depth, path) word per thread,
//     layout [level][field][thread] (conflict-free), 2 x 19 456 B = 38 912 B per workgroup of 256;
//   * a third level (three nested glass hits with all siblings waiting) spills to scratch memory.
// The output needs no LDS (each wave transposes its 16x4 tile with lane shuffles), so stack + objs stays under 40 KiB and
// FOUR workgroups fit a CU's 160 KiB: occupancy 4 waves/SIMD instead of 3, worth ~10 % on C2.
static constexpr int kPendDoubles = 9;
static constexpr int kLdsLevels = 2;
// one LDS level of a workgroup of `threads`: [field][thread], then the packed words
CGRT_HD constexpr size_t pending_level_bytes(int threads) { return (size_t)threads * (kPendDoubles * sizeof(double) + sizeof(uint32_t)); }
static constexpr size_t kBezLdsBytes = 7872;  // sizeof(BezLds) (cgrt_bezier.hpp; tied to the type in cgrt_hip.hip)

// What a kernel variant asks for
struct WgLdsAsk {
    int threads;   // workgroup size (waves = threads / 64)
    bool pending;  // the pending-ray levels
    bool staging;  // one ObjRec per wave for objects beyond the resident list (SPILL)
    bool bez;      // one BezLds per wave
    bool nodes;    // the cached tree's nodes, where the scene has one
    bool wstack;   // the first kWideLdsDepth entries of the 4-wide walk's stack, where the launch says the walk runs
};
// trace_grid_kernel / trace_grid_sched_kernel and trace_rays_kernel / capture_rays_kernel (HFONLY false).  Glass and Bezier
// variants' LDS is spoken for: no wide-walk stack.  HFONLY walks height fields only: neither node cache nor stack.
CGRT_HD constexpr WgLdsAsk wg_ask_trace(int nt, bool trees, bool bez, bool glass, bool spill, bool hfonly) {
    return {nt, glass, spill, bez, trees && !hfonly, trees && !hfonly && !glass && !bez};
}
// photon_trace_kernel: the stack only without Bezier objects and without SPILL (whose launch keeps four workgroups a CU)
CGRT_HD constexpr WgLdsAsk wg_ask_photon(bool bez, bool spill) { return {256, false, spill, bez, false, !bez && !spill}; }
// primary_walk_kernel: the objects it stages and the stack
CGRT_HD constexpr WgLdsAsk wg_ask_primary_walk() { return {256, false, false, false, false, true}; }

// Byte offsets of the regions from the start of the dynamic LDS; a region the launch does not have is empty (its offset is
// that of the next one).  `total` is what the launch requests.
struct WgLds {
    WgLdsAsk has;                 // the regions this launch has: the ask, narrowed by the launch's numbers
    size_t pending, level_bytes;  // level L, field f of thread t: pending + L * level_bytes + (f * threads + t) * 8
    size_t objs, staging, bez, nodes, wstack, total;
};
// resident: objects staged in the list; cached_nodes: nodes of the scene's cached tree (0: none); wide: the launch wants the
// wide walk's stack in LDS (eye pass and ray kernels: the scene has a wide tree; photon kernel: photon_lds_stack; primary
// walk: always)
CGRT_HD constexpr WgLds wg_lds(const WgLdsAsk &a, size_t resident, size_t cached_nodes, bool wide) {
    const size_t waves = (size_t)a.threads / 64;
    WgLds l{};
    l.has = a;
    l.has.nodes = a.nodes && cached_nodes > 0;
    l.has.wstack = a.wstack && wide;
    l.pending = 0;
    l.level_bytes = pending_level_bytes(a.threads);
    l.objs = l.pending + (a.pending ? (size_t)kLdsLevels * l.level_bytes : 0);
    l.staging = l.objs + resident * sizeof(cgrt::ObjRec);
    l.bez = l.staging + (a.staging ? waves * sizeof(cgrt::ObjRec) : 0);
    l.nodes = l.bez + (a.bez ? waves * kBezLdsBytes : 0);
    l.wstack = l.nodes + (a.nodes ? cached_nodes * sizeof(cgrt::NodeRec) : 0);
    l.total = l.wstack + (l.has.wstack ? (size_t)a.threads * cgrt::kWideLdsDepth * 8 : 0);
    return l;
}
// ... for the launch's copy of the scene: what the eye pass's and the ray kernels' bodies and their launch plans both call
CGRT_HD constexpr WgLds wg_lds(const WgLdsAsk &a, const cgrt::DeviceScene &sc) {
    return wg_lds(a, (size_t)sc.n_lds, sc.cached_tree >= 0 ? (size_t)sc.cached_nodes : 0, sc.has_wide != 0);
}

#endif
