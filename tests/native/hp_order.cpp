// The order of caller-supplied Hitpoint records (cgrt_hp_order.h) on the CPU: hp_path_key against a comparison of the paths'
// bit strings written out here (lexicographic, a prefix first) over every path with up to 10 bits behind its leading 1 and a
// few hundred random longer ones; distinct paths have distinct keys; the key's upper 30 bits are wavefront_sort_key(0, path);
// keys stay below 2^35; the validity limits and the radix passes' widths.
// CPU build under ASan + UBSan, driven by tests/test_hp_order_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "cgrt_hp_order.h"

static int g_failed = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (g_failed++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                  \
    } while (0)

// the bits of `path` behind its leading 1, most significant first, as text
static std::string bits_of(uint32_t path) {
    int top = 31;
    while (!((path >> top) & 1u)) top--;
    std::string s;
    for (int b = top - 1; b >= 0; b--) s.push_back(((path >> b) & 1u) ? '1' : '0');
    return s;
}
// -1, 0, 1: a before b in emission order (std::string compares lexicographically and puts a prefix before its extensions)
static int cmp_paths(uint32_t a, uint32_t b) {
    const std::string sa = bits_of(a), sb = bits_of(b);
    return sa < sb ? -1 : sa == sb ? 0 : 1;
}
static int cmp_keys(uint32_t a, uint32_t b) {
    const uint64_t ka = hp_path_key(a), kb = hp_path_key(b);
    return ka < kb ? -1 : ka == kb ? 0 : 1;
}

int main() {
    std::vector<uint32_t> paths;
    for (uint32_t p = 1; p < (1u << 11); p++) paths.push_back(p);  // every path of 0 .. 10 bits behind the leading 1
    std::mt19937_64 rng(20240607);
    for (int k = 0; k < 300; k++) paths.push_back((1u << 30) | (uint32_t)(rng() & ((1u << 30) - 1u)));  // 30 bits
    for (int k = 0; k < 300; k++) {  // any length 11 .. 30
        const int ln = 11 + (int)(rng() % 20);
        paths.push_back((1u << ln) | (uint32_t)(rng() & ((1ull << ln) - 1ull)));
    }
    paths.push_back((1u << 31) - 1u);  // the longest, all refracted
    paths.push_back(1u << 30);         // the longest, all reflected

    for (uint32_t p : paths) {
        const uint64_t k = hp_path_key(p);
        CHECK(k < (1ull << kHpPathKeyBits));
        CHECK(kHpPathKeyBits == 35);
        CHECK((k >> kHpPathLenBits) == wavefront_sort_key(0u, p));
        CHECK((int)(k & ((1u << kHpPathLenBits) - 1u)) == (int)bits_of(p).size());
        CHECK(hp_path_ok(p));
    }
    // every pair of the short paths and of the random ones: the keys compare as the bit strings do
    long long pairs = 0;
    for (size_t i = 0; i < paths.size(); i++)
        for (size_t j = (i < 2047 ? 0 : 2047); j < paths.size(); j++) {
            if (i < 2047 && j >= 2047 && (i % 7) != 0) continue;  // short against long: a seventh of the short ones
            CHECK(cmp_keys(paths[i], paths[j]) == cmp_paths(paths[i], paths[j]));
            pairs++;
        }
    // distinct paths, distinct keys; sorting by key is sorting by the bit strings
    std::vector<uint32_t> uniq(paths);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<uint64_t> keys;
    for (uint32_t p : uniq) keys.push_back(hp_path_key(p));
    std::sort(keys.begin(), keys.end());
    CHECK(std::adjacent_find(keys.begin(), keys.end()) == keys.end());
    std::vector<uint32_t> by_key(uniq), by_bits(uniq);
    std::sort(by_key.begin(), by_key.end(), [](uint32_t a, uint32_t b) { return hp_path_key(a) < hp_path_key(b); });
    std::sort(by_bits.begin(), by_bits.end(), [](uint32_t a, uint32_t b) { return cmp_paths(a, b) < 0; });
    CHECK(by_key == by_bits);
    // the cases the left alignment alone cannot tell apart
    CHECK(hp_path_key(1u) < hp_path_key(2u));   // "" before "0"
    CHECK(hp_path_key(2u) < hp_path_key(4u));   // "0" before "00"
    CHECK(hp_path_key(4u) < hp_path_key(5u));   // "00" before "01"
    CHECK(hp_path_key(5u) < hp_path_key(3u));   // "01" before "1": reflected subtree before the refracted one
    CHECK(wavefront_sort_key(0u, 2u) == wavefront_sort_key(0u, 4u));
    // which records are kept
    CHECK(!hp_path_ok(0u) && hp_path_ok(1u) && hp_path_ok((1u << 31) - 1u) && !hp_path_ok(1u << 31) && !hp_path_ok(0xFFFFFFFFu));
    CHECK(!hp_ray_ok(-1) && hp_ray_ok(0) && hp_ray_ok(kHpMaxRay - 1) && !hp_ray_ok(kHpMaxRay) && kHpMaxRay == (1ll << 36));
    // the passes' widths: keys 0 .. max_key fit hp_key_bits(max_key) bits, and no fewer
    for (int b = 1; b <= 37; b++) {
        CHECK(hp_key_bits((1ull << b) - 1ull) == b);
        CHECK(hp_key_bits(1ull << b) == b + 1);
    }
    CHECK(hp_key_bits(0) == 1 && hp_key_bits(1) == 1 && hp_key_bits(1000001) == 20 && hp_key_bits(1ull << 20) == 21);
    CHECK(kHpTexelBits + hp_key_bits(1ull << 20) <= 64 && hp_key_bits((uint64_t)kHpMaxRay) == 37);
    std::printf("%zu paths, %lld pairs compared\n", paths.size(), pairs);
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
