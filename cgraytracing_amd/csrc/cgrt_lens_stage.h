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

// The lens table (device memory on the scene handle; the full and the parking body of the thin-lens PAIR variants, classes 0-2 of
// the tile order, which have neither LDS nor registers to spare for a stager): lens_table_kernel (cgrt_eye.hpp), a small kernel
// ahead of the frame, finds the accepted draw of every (pixel, sample) of the launch by the two phases above over batches of up to
// kLensTableBatch samples and leaves it in table[entry][sample][thread] -- uint64_t, a workgroup's threads contiguous; entry = the
// tile-order list entry, sample = the launch's sample number (sample_offset goes into the draw, not into the index), thread = the
// body's threadIdx.x, so the pixel mapping is the body's own.  A body that reads the table needs neither the pixel key nor
// sample_key nor the rejection loop.  The table holds the list's first `cap` entries; a workgroup beyond them keeps the per-sample
// loop (workgroup-uniform).  The draws depend on seed, sample_offset, spp and the pixel set, their place on the order list: the
// table is kept with the tile order and reused while all of these stand (cgrt_tile_order.hpp).
static constexpr int kLensTableBatch = 32;
static_assert(kLensTableBatch <= 32, "a thread's reject word is 32 bits");
static constexpr size_t kLensTableBudget = (size_t)256 << 20;  // default budget in bytes (knob CGRT_LENS_TABLE_BYTES)
CGRT_HD constexpr size_t lens_table_entry_bytes(int spp, int threads) { return (size_t)spp * (size_t)threads * sizeof(uint64_t); }
// the byte offset of table[entry][sample][t]
CGRT_HD constexpr size_t lens_table_at(size_t entry, int sample, int t, int spp, int threads) {
    return entry * lens_table_entry_bytes(spp, threads) + ((size_t)sample * (size_t)threads + (size_t)t) * sizeof(uint64_t);
}
// entries the table holds: as many of the list's n_tiles entries as the budget pays for
CGRT_HD constexpr size_t lens_table_cap(size_t n_tiles, int spp, int threads, size_t budget) {
    return budget / lens_table_entry_bytes(spp, threads) < n_tiles ? budget / lens_table_entry_bytes(spp, threads) : n_tiles;
}
CGRT_HD constexpr size_t lens_table_bytes(size_t cap, int spp, int threads) { return cap * lens_table_entry_bytes(spp, threads); }

// lens_table_kernel's per-thread routine for one batch: samples first .. first + count - 1 (sample_offset included in `first`),
// count <= kLensTableBatch, of the pixel with key k_pix, written to row[b * stride].  Phase A (lens_table_first) returns the
// thread's reject word; a thread with no live pixel writes 0 and rejects nothing.  Phase B: while any thread of the wave has a bit
// left, each of those runs lens_table_retry on its lowest rejected sample.
CGRT_HD uint32_t lens_table_first(uint64_t k_pix, uint64_t first, int count, bool live, uint64_t *row, size_t stride) {
    uint32_t rejected = 0u;
    for (int b = 0; b < count; b++) {
        const LensSlot a = lens_stage_first(k_pix, first + (uint64_t)b);
        row[(size_t)b * stride] = live ? a.v : 0ull;
        rejected |= a.done ? 0u : (1u << b);
    }
    return live ? rejected : 0u;
}
CGRT_HD uint32_t lens_table_retry(uint32_t rejected, uint64_t *row, size_t stride) {  // rejected != 0
    const int b = __builtin_ctz(rejected);
    const LensSlot a = lens_stage_retry(row[(size_t)b * stride]);
    row[(size_t)b * stride] = a.v;
    return a.done ? rejected & (rejected - 1u) : rejected;
}

#endif
