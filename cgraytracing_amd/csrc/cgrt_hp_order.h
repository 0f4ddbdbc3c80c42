// The order of caller-supplied Hitpoint records (cgrt_ppm_session_create_hitpoints) in plain C++ (no HIP): which records are
// kept, the total sort key of a record's place in its ray's tree, and the widths of the table build's three sort passes.
// PpmTable::build_hitpoints (cgrt_ppm_table.hpp) and its kernels use these; tests/native/hp_order.cpp checks them on the CPU.
#ifndef CGRT_HP_ORDER_H
#define CGRT_HP_ORDER_H
#include <cstdint>

#include "cgrt_wavefront_plan.h"  // wavefront_sort_key, wavefront_path_bits, CGRT_HD

static constexpr int kHpPathLenBits = 5;                                    // a path has 0..30 bits behind its leading 1
static constexpr int kHpPathKeyBits = kWavefrontPathBits + kHpPathLenBits;  // 35
static constexpr long long kHpMaxRay = 1ll << 36;                           // ray ids are 0 .. 2^36 - 1
static constexpr int kHpTexelBits = 32;                                     // (bucket << 32) | texel, texel < 2^31

// path in [1, 2^31): a place in a ray's tree (root 1, children 2p and 2p + 1)
CGRT_HD bool hp_path_ok(uint32_t path) { return path != 0u && path < (1u << 31); }
CGRT_HD bool hp_ray_ok(long long ray) { return ray >= 0 && ray < kHpMaxRay; }

// A total order of paths: the bit strings behind the leading 1 compared lexicographically (reflected, bit 0, before refracted,
// bit 1), a prefix before its extensions.  wavefront_sort_key's left alignment orders strings of which none is a prefix of
// another; the bit count below it puts "0" before "00".  Distinct paths have distinct keys, all below 2^35.
CGRT_HD uint64_t hp_path_key(uint32_t path) {
    return (wavefront_sort_key(0u, path) << kHpPathLenBits) | (uint64_t)wavefront_path_bits(path);
}

// bits of a radix pass whose keys are 0 .. max_key
CGRT_HD int hp_key_bits(uint64_t max_key) {
    int b = 1;
    while (b < 64 && (max_key >> b) != 0) b++;
    return b;
}

#endif
