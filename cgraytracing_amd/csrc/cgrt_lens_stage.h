// Lens points staged ahead of the sample loop, in plain C++ (no HIP): the per-lane stager and where a lane's staged draws lie.
// The thin-lens terminal-diffuse body inside the PAIR launch (trace_grid_body, cgrt_eye.hpp) runs it on the device;
// tests/native/lens_stage.cpp runs the same functions on the CPU, 64 lanes at a time.
//
// lens_disc (cgrt_eye.hpp) draws a sample's lens point by rejection: attempt j of sample s of a pixel takes the two draws of
//     z = fin64(sample_key(k_pix, s) + (j + 1) G),
// accepts when (sx, sy) = (2 ux - 1, 2 uy - 1) lies inside the unit circle (probability pi / 4, 1.27 attempts a lane) and
// retries otherwise.  A wave runs that loop in lockstep at the pace of its unluckiest lane: 3.6 rounds when all 64 lanes start
// a sample.  z is a pure function of (pixel, sample, attempt), whoever computes it and whenever, so a lane may find the
// accepted z of its next `count` samples ahead of their use, on its own (sample, attempt) stream, and keep the 8 bytes; the
// sample loop rebuilds (sx, sy) from z with lens_disc's own expressions: the same bits.
//
// Staging a batch takes two phases:
//   A  no divergence: for every sample of the batch the lane computes sample_key and attempt 1 (lens_stage_first); it keeps z
//      when the attempt is accepted, else the attempt's counter, and notes the sample in its reject word;
//   B  while any lane of the wave has a bit left: a lane with rejects retries its lowest rejected sample (lens_stage_retry)
//      and keeps z or the new counter; a lane that accepts clears the bit.
// Rounds a sample: 1 + 0.69 at batches of 16, 1 + 0.55 at 32 (tests/native/lens_stage.cpp measures both).
#ifndef CGRT_LENS_STAGE_H
#define CGRT_LENS_STAGE_H
#include <stddef.h>
#include <stdint.h>

#include "cgrt_rng.hpp"

// Samples a lane stages at a time in LDS; the reject word has a bit for each
static constexpr int kLensBatch = 16;
static_assert(kLensBatch <= 32, "a lane's reject word is 32 bits");
// The per-lane LDS slots: slot b of thread t of `threads` at (b * threads + t) * 8 bytes from the region's start (the lanes of
// a wave contiguous: conflict-free 8-byte accesses), kLensBatch slots a thread
CGRT_HD constexpr size_t lens_slot_at(int b, int t, int threads) { return ((size_t)b * (size_t)threads + (size_t)t) * sizeof(uint64_t); }
CGRT_HD constexpr size_t lens_batch_lds(int threads) { return (size_t)kLensBatch * (size_t)threads * sizeof(uint64_t); }

// lens_disc's expressions on one attempt's draw: the point, and whether the attempt is accepted
CGRT_HD void lens_point(uint64_t z, double &sx, double &sy) {
    const double ux = cgrt::div_rand_max((uint32_t)(z >> 33)), uy = cgrt::div_rand_max((uint32_t)((z >> 2) & 0x7fffffffu));
    sx = ux * 2.0 - 1;
    sy = uy * 2.0 - 1;
}
CGRT_HD bool lens_accepts(uint64_t z) {
    double sx, sy;
    lens_point(z, sx, sy);
    return sx * sx + sy * sy < 1;
}

// What a lane keeps for a sample it is staging: the accepted draw z (done), or the counter of the last rejected attempt
struct LensSlot {
    uint64_t v;
    bool done;
};
// Phase A: attempt 1 of sample `sample` (the launch's sample_offset included) of the pixel with key k_pix
CGRT_HD LensSlot lens_stage_first(uint64_t k_pix, uint64_t sample) {
    const uint64_t ctr = cgrt::sample_key(k_pix, sample) + cgrt::kGolden;
    const uint64_t z = cgrt::fin64(ctr);
    const bool ok = lens_accepts(z);
    return LensSlot{ok ? z : ctr, ok};
}
// Phase B: the next attempt of a sample whose last attempt, at counter ctr, was rejected
CGRT_HD LensSlot lens_stage_retry(uint64_t ctr) {
    ctr += cgrt::kGolden;
    const uint64_t z = cgrt::fin64(ctr);
    const bool ok = lens_accepts(z);
    return LensSlot{ok ? z : ctr, ok};
}

#endif
