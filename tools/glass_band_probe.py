#!/usr/bin/env python3
"""Development aid (not a test): C2's longest workgroup inside the frame and alone on the chip.

  python tools/glass_band_probe.py [--out band.json] [--frames N]
  python tools/glass_band_probe.py --band-only ROW_OFFSET [--frames N]      (the program of a rocprofv3 --pmc run)

Without --band-only: takes the timeline of one C2 frame (CGRT_TIMELINE_FILE, as tools/timeline_probe.py), finds the workgroup
that ran longest and its tile, then renders the 8-row band that holds that tile alone -- same camera, same frame, rows=8,
row_offset = 8 * tile_y -- N times between device events, and once more with the timeline on.  The band's 60 workgroups have
a CU each and their four waves a SIMD each, so the band's longest workgroup is that tile's standalone time and the band's
counters are those of waves that share their SIMD with nobody.  Prints and writes: the frame's span, its longest workgroup
and when class 3 ended; the band's time per launch and its longest workgroup.
With --band-only: renders that band N times and nothing else."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

W, H, SPP, DEPTH, SEED = 1920, 1080, 64, 5, 12345


def timeline(sc, cam, **kw):
    """One launch with the timeline on: per workgroup that ran its start and end in microseconds, its tile (the record holds the
    16x4 wave tile of its first wave: two by two to a 32x8 tile), its rays and its index in the launch; and the launch's result."""
    tf = tempfile.mktemp(suffix=".tl")
    os.environ["CGRT_TIMELINE_FILE"] = tf
    r = sc.trace_grid_host(W, H, SPP, cam, DEPTH, SEED, **kw)
    del os.environ["CGRT_TIMELINE_FILE"]
    raw = np.fromfile(tf, dtype=np.uint64)
    os.unlink(tf)
    tl = raw[4:].reshape(int(raw[0]), 4)
    blk = np.nonzero(tl[:, 1] > 0)[0]
    tl = tl[blk]
    t0 = tl[:, 0].astype(np.int64)
    a, b = (t0 - t0.min()) / 100.0, (tl[:, 1].astype(np.int64) - t0.min()) / 100.0
    tx = (tl[:, 3] & np.uint64(0xffff)).astype(int) // 2
    ty = ((tl[:, 3] >> np.uint64(16)) & np.uint64(0xffff)).astype(int) // 2
    rays = (tl[:, 3] >> np.uint64(32)).astype(np.int64)
    # a launch that relays samples (cgrt_relay.h) left relay_k << 32 | relay_cap in the header: its first relay_k * n_split
    # workgroups are (entry i // relay_k, chunk i % relay_k), n_split = min(plan[2], relay_cap); blk becomes the order's entry
    relay_k, relay_cap = int(raw[3]) >> 32, int(raw[3]) & 0xffffffff
    order = sc.last_tile_order()
    if relay_k > 1 and order is not None:
        n_split = min(int(order["plan"][2]), relay_cap)
        blk = np.where(blk < relay_k * n_split, blk // relay_k, blk - (relay_k - 1) * n_split)
    return a, b, tx, ty, rays, blk, r


def band_frames(sc, cam, row_offset, frames):
    """ms per launch of the band between device events."""
    import torch
    out = torch.zeros((8, W, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    kw = dict(rows=8, row_offset=row_offset, out=out, nhit=False, counters=cnt)
    sc.trace_grid(W, H, SPP, cam, DEPTH, SEED, **kw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sc.trace_grid(W, H, SPP, cam, DEPTH, SEED, **kw)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    argv = sys.argv[1:]
    frames = int(argv[argv.index("--frames") + 1]) if "--frames" in argv else 5
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    import cgraytracing_amd as cg
    import scenes
    cam = scenes.cam_dof()
    sc = cg.Scene(scenes.scene_c2())
    if "--band-only" in argv:
        ro = int(argv[argv.index("--band-only") + 1])
        ms = band_frames(sc, cam, ro, frames)
        print(json.dumps({"row_offset": ro, "band_ms": [round(m, 4) for m in ms]}))
        sc.close()
        return
    sc.trace_grid_host(W, H, 1, cam, DEPTH, SEED)  # warm-up
    a, b, tx, ty, rays, blk, r = timeline(sc, cam)
    order = sc.last_tile_order()
    dur = b - a
    i = int(np.argmax(dur))
    top = np.sort(dur)[::-1]
    doc = {"workload": "c2 %dx%d spp %d" % (W, H, SPP), "kernel": sc.kernel_variant(W, H, SPP, cam, DEPTH),
           "frame": {"span_us": round(float(b.max()), 1), "workgroups": int(len(dur)), "rays": int(r["nrays"]),
                     "longest_us": round(float(dur[i]), 1), "longest_start_us": round(float(a[i]), 1), "longest_tile": [int(tx[i]), int(ty[i])],
                     "longest_rays": int(rays[i]), "five_longest_us": [round(float(x), 1) for x in top[:5]],
                     "p99_us": round(float(np.percentile(dur, 99)), 1)}}
    if order is not None:
        is3 = blk >= int(order["plan"][3])  # blk: the order's entry a workgroup rendered; class 3 begins at plan[3]
        doc["frame"]["class_bounds"] = [int(x) for x in order["plan"]]
        doc["frame"]["class3_last_end_us"] = round(float(b[is3].max()), 1) if is3.any() else None
        doc["frame"]["class012_last_end_us"] = round(float(b[~is3].max()), 1) if (~is3).any() else None
    ro = 8 * int(ty[i])
    ms = band_frames(sc, cam, ro, frames)
    ba, bb, btx, bty, brays, _, br = timeline(sc, cam, rows=8, row_offset=ro)
    bdur = bb - ba
    j = int(np.argmax(bdur))
    doc["band"] = {"rows": 8, "row_offset": ro, "ms_per_launch": [round(m, 4) for m in ms], "workgroups": int(len(bdur)),
                   "rays": int(br["nrays"]), "span_us": round(float(bb.max()), 1), "longest_us": round(float(bdur[j]), 1),
                   "longest_tile": [int(btx[j]), int(bty[j])], "longest_rays": int(brays[j]),
                   "same_tile_us": [round(float(x), 1) for x in bdur[btx == tx[i]]]}
    doc["in_frame_over_standalone"] = round(float(dur[i]) / float(bdur[btx == tx[i]].max()), 3) if (btx == tx[i]).any() else None
    sc.close()
    print(json.dumps(doc, indent=1))
    if out:
        json.dump(doc, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
