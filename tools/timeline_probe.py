#!/usr/bin/env python3
"""Development aid (not a test): when and where every workgroup of one trace_grid launch ran.

  python tools/timeline_probe.py c3|c4|c2|c5band [--spp N] [--split] [--natural] [--relay on|off] [--mirror on|off]
                                 [--order chunks_first|mirror_first|interleaved] [--start list|cost] [--out tl.json]

Sets CGRT_TIMELINE_FILE so that libcgrt.so records, per workgroup, {start, end} on the 100 MHz wall clock, the hardware
id (XCC, SE, CU) and the rays it traced, then prints: launch span, concurrency over time (resident workgroups in 20 time
bins), the distribution of workgroup durations, the share of the span during which fewer than half of the slots were in
use ("tail"), and per-XCD finish times."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "c3"
    spp = int(sys.argv[sys.argv.index("--spp") + 1]) if "--spp" in sys.argv else None
    split = "--split" in sys.argv
    natural = "--natural" in sys.argv  # CGRT_GRID_NO_REORDER
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    relay = {"on": True, "off": False}[sys.argv[sys.argv.index("--relay") + 1]] if "--relay" in sys.argv else None  # sample_relay
    form = {}  # relay_mirror / relay_order
    if "--mirror" in sys.argv:
        form["relay_mirror"] = {"on": True, "off": False}[sys.argv[sys.argv.index("--mirror") + 1]]
    if "--order" in sys.argv:
        form["relay_order"] = sys.argv[sys.argv.index("--order") + 1]
    if "--start" in sys.argv:  # relay_start
        form["relay_start"] = sys.argv[sys.argv.index("--start") + 1]
    import cgraytracing_amd as cg
    import scenes
    cam = scenes.cam_dof()
    rows, row_offset = None, 0
    if which == "c3":
        objs, W, H, s0 = scenes.scene_c3(True), 2048, 2048, 64
    elif which == "c4":
        objs, W, H, s0 = scenes.scene_dragon(), 4096, 4096, 64
    elif which == "c2":
        objs, W, H, s0 = scenes.scene_c2(), 1920, 1080, 64
    else:
        objs, W, H, s0 = scenes.scene_c5(scenes.stone_texture()), 8192, 8192, 16
        rows, row_offset = 256, 3000
    spp = spp or s0
    sc = cg.Scene(objs)
    sc.trace_grid_host(W, H, 1, cam, 5, 12345, rows=rows, row_offset=row_offset)  # warm-up
    tf = tempfile.mktemp(suffix=".tl")
    os.environ["CGRT_TIMELINE_FILE"] = tf
    r = sc.trace_grid_host(W, H, spp, cam, 5, 12345, rows=rows, row_offset=row_offset, split_samples=split, reorder=not natural,
                           **dict({} if relay is None else {"sample_relay": relay}, **form))
    del os.environ["CGRT_TIMELINE_FILE"]
    tile_order = sc.last_tile_order() if hasattr(sc, "last_tile_order") else None  # image-order launches of sphere scenes
    relayed = sc.last_sample_relay() if hasattr(sc, "last_sample_relay") else None
    relay_form = sc.last_relay_form() if hasattr(sc, "last_relay_form") else None
    relay_start = sc.last_relay_start() if hasattr(sc, "last_relay_start") else None  # the start table by cost, where the launch had one
    sc.close()
    raw = np.fromfile(tf, dtype=np.uint64)
    os.unlink(tf)
    nblk, nthr, chunks, xcd_tiles = [int(x) for x in raw[:4]]
    # a launch that relays samples (cgrt_relay.h) writes (relay_k | extent << 8 | order << 9) << 32 | relay_cap there (its tiles
    # are row-major: xcd_tiles 0)
    relay_k, relay_extent, relay_order, relay_cap, xcd_tiles = ((xcd_tiles >> 32) & 255, (xcd_tiles >> 40) & 1, (xcd_tiles >> 41) & 3,
                                                                 xcd_tiles & 0xffffffff, 0) if xcd_tiles >> 32 else (1, 0, 0, 0, xcd_tiles)
    tl = raw[4:].reshape(nblk, 4)
    ran = tl[:, 1] > 0
    t0 = tl[ran, 0].astype(np.int64)
    t1 = tl[ran, 1].astype(np.int64)
    base = t0.min()
    a, b = (t0 - base) / 100.0, (t1 - base) / 100.0  # microseconds
    span = b.max()
    dur = b - a
    xcc = ((tl[ran, 2] >> np.uint64(32)) & np.uint64(15)).astype(int)
    hw = (tl[ran, 2] & np.uint64(0xffffffff)).astype(np.int64)
    cu = (hw >> 8) & 15
    se = (hw >> 13) & 3
    rays = (tl[ran, 3] >> np.uint64(32)).astype(np.int64)
    bins = 20
    edges = np.linspace(0, span, bins + 1)
    conc = [float(np.minimum(b, edges[i + 1]).clip(min=0).__sub__(np.maximum(a, edges[i])).clip(min=0).sum() / (edges[i + 1] - edges[i]))
            for i in range(bins)]
    order = np.argsort(dur)[::-1]
    doc = {
        "workload": "%s %dx%d spp %d%s%s" % (which, W, rows or H, spp, " split-samples" if split else "", " image order" if natural else " cost order"),
        "workgroups": int(ran.sum()), "threads": nthr, "chunks": chunks, "xcd_tiles": xcd_tiles, "rays": int(r["nrays"]),
        "span_us": round(span, 1),
        "resident_workgroups_by_time_bin": [round(c, 1) for c in conc],
        "workgroup_us": {"mean": round(float(dur.mean()), 1), "p50": round(float(np.percentile(dur, 50)), 1),
                         "p90": round(float(np.percentile(dur, 90)), 1), "p99": round(float(np.percentile(dur, 99)), 1),
                         "max": round(float(dur.max()), 1)},
        "sum_workgroup_us": round(float(dur.sum()), 1),
        "mean_resident_workgroups": round(float(dur.sum() / span), 1),
        "heaviest": [{"us": round(float(dur[i]), 1), "start_us": round(float(a[i]), 1), "rays": int(rays[i]), "xcc": int(xcc[i]),
                      "se": int(se[i]), "cu": int(cu[i])} for i in order[:8]],
        "xcc_finish_us": {str(x): round(float(b[xcc == x].max()), 1) for x in sorted(set(xcc.tolist()))},
        "xcc_busy_us": {str(x): round(float(dur[xcc == x].sum()), 1) for x in sorted(set(xcc.tolist()))},
        "dur_weighted_by_rays_corr": round(float(np.corrcoef(dur, rays)[0, 1]), 3),
    }
    idx = np.nonzero(ran)[0]
    last = np.argsort(b)[::-1][:12]
    doc["last_to_finish"] = [{"block": int(idx[i]), "start_us": round(float(a[i]), 1), "end_us": round(float(b[i]), 1), "rays": int(rays[i])}
                             for i in last]
    late = b > 0.8 * span
    doc["finishing_in_last_fifth"] = {"workgroups": int(late.sum()), "mean_us": round(float(dur[late].mean()), 1) if late.any() else 0,
                                      "started_after_half": int((late & (a > 0.5 * span)).sum())}
    half = 0.5 * max(conc)
    doc["fraction_of_span_below_half_peak_concurrency"] = round(sum(1 for c in conc if c < half) / bins, 2)
    if tile_order is not None and nblk == len(tile_order["list"]) + (relay_k - 1) * relay_cap:
        # workgroup i rendered tile list[i]; plan[c] = workgroups of classes < c (classes 0-2: tiles that may see a glass / mirror sphere).
        # With the relay: relay_block_ordered (cgrt_relay.h), written out for arrays; workgroups beyond the list left at once and
        # have no record.
        plan = [int(x) for x in tile_order["plan"]]
        blk = np.nonzero(ran)[0].astype(np.int64)
        n01, n012 = plan[2], plan[3]
        n_split = min(n012 if relay_extent else n01, relay_cap) if relay_k > 1 else 0
        k = relay_k
        s_a = min(n_split, n01)
        s_m = n_split - s_a
        n_a, n_m = n01 + (k - 1) * s_a, n012 - n01 + (k - 1) * s_m
        t = n_a + n_m
        if relay_order == 2:
            q = blk * n_m // max(t, 1)
            mirror = blk * n_m - q * t + n_m >= t
            i = np.where(mirror, q, blk - q)
        elif relay_order == 1:
            mirror = blk < n_m
            i = np.where(mirror, blk, blk - n_m)
        else:
            mirror = blk >= n_a
            i = np.where(mirror, blk - n_a, blk)
        first, s_of = np.where(mirror, n01, 0), np.where(mirror, s_m, s_a)
        split_blk = (blk < t) & (i < k * s_of)
        chunk = np.where(split_blk, i % k, 0)
        in_table = blk < t
        blk = np.where(blk >= t, n012 + blk - t, np.where(split_blk, first + i // k, first + i - (k - 1) * s_of))  # the entry
        if relay_start is not None and relay_start["t"] == t:
            # the workgroups of classes 0-2 went through the start table (cgrt_relay.h): word = entry << 2 | chunk
            word = relay_start["start"].astype(np.int64)[np.minimum(np.nonzero(ran)[0], t - 1)]
            blk = np.where(in_table, word >> 2, blk)
            chunk = np.where(in_table, word & 3, chunk)
            split_blk = in_table & (blk < n_split)
            # an item's weight (tile cost x samples) against what its workgroup took: Spearman's rank correlation
            tx, wtx, wty = (W + 31) // 32, (W + 15) // 16, ((rows or H) + 3) // 4
            wc = relay_start["wcost"].reshape(wty, wtx).astype(np.int64)
            tiles = tile_order["list"].astype(np.int64)[np.minimum(blk, plan[4] - 1)]
            cost = np.zeros(len(blk), np.int64)
            for dy in range(2):
                for dx in range(2):
                    wy, wx = 2 * (tiles // tx) + dy, 2 * (tiles % tx) + dx
                    cost = np.maximum(cost, np.where((wy < wty) & (wx < wtx), wc[np.minimum(wy, wty - 1), np.minimum(wx, wtx - 1)], 0))
            cs = -(-spp // k)
            weight = cost * np.where(split_blk, np.minimum((chunk + 1) * cs, spp) - chunk * cs, spp)
            def ranks(v):
                o = np.argsort(v, kind="stable")
                r = np.empty(len(v))
                r[o] = np.arange(len(v))
                u, inv = np.unique(v, return_inverse=True)  # ties: the mean rank
                return (np.bincount(inv, weights=r) / np.bincount(inv))[inv]
            doc["cost_start"] = {"items": int(in_table.sum()), "reused": relay_start["reused"], "largest_wave_cost": int(wc.max()),
                                 "spearman_weight_vs_workgroup_us": round(float(np.corrcoef(ranks(weight[in_table]), ranks(dur[in_table]))[0, 1]), 4),
                                 "first_workgroups_us": [round(float(x), 1) for x in dur[in_table][:8]],
                                 "last_workgroups_us": [round(float(x), 1) for x in dur[in_table][-8:]]}
        if relay_k > 1:
            ent_rays = np.bincount(blk, weights=rays, minlength=plan[4])
            heavy = int(np.argmax(ent_rays))  # the entry with the most rays: the glass sphere's centre tile
            doc["sample_relay"] = {"chunks": relay_k, "capacity_tiles": relay_cap, "split_tiles": n_split, "last": relayed, "form": relay_form,
                                   "workgroups_launched": nblk, "workgroups_beyond_the_list": int(nblk - ran.sum()),
                                   "split_workgroup_us": {"mean": round(float(dur[split_blk].mean()), 1), "max": round(float(dur[split_blk].max()), 1)} if split_blk.any() else None,
                                   "heaviest_entry": {"entry": heavy, "tile": int(tile_order["list"][heavy]), "rays": int(ent_rays[heavy]),
                                                      "workgroups": [{"chunk": int(chunk[i]), "start_us": round(float(a[i]), 1), "end_us": round(float(b[i]), 1),
                                                                      "rays": int(rays[i])} for i in np.nonzero(blk == heavy)[0]]}}
        c0, c3 = blk < plan[1], blk >= plan[3]
        doc["tile_order"] = {"class_bounds": plan,
                             "class0_last_start_us": round(float(a[c0].max()), 1) if c0.any() else None,
                             "class012_last_start_us": round(float(a[~c3].max()), 1) if (~c3).any() else None,
                             "class3_first_start_us": round(float(a[c3].min()), 1) if c3.any() else None,
                             "class3_last_end_us": round(float(b[c3].max()), 1) if c3.any() else None,
                             "class012_last_end_us": round(float(b[~c3].max()), 1) if (~c3).any() else None}
        # per class (class 2: its split and its unsplit workgroups apart): first start, last start, last end
        def span_of(sel):
            return {"workgroups": int(sel.sum()), "first_start_us": round(float(a[sel].min()), 1), "last_start_us": round(float(a[sel].max()), 1),
                    "last_end_us": round(float(b[sel].max()), 1), "mean_us": round(float(dur[sel].mean()), 1),
                    "max_us": round(float(dur[sel].max()), 1)} if sel.any() else None
        cls = np.searchsorted(np.asarray(plan[1:4]), blk, side="right")
        doc["tile_order"]["classes"] = {"class0": span_of(cls == 0), "class1": span_of(cls == 1), "class2_split": span_of((cls == 2) & split_blk),
                                        "class2_unsplit": span_of((cls == 2) & ~split_blk), "class3": span_of(cls == 3)}
        end012, end3 = doc["tile_order"]["class012_last_end_us"], doc["tile_order"]["class3_last_end_us"]
        doc["tile_order"]["classes_0_2_end_no_later_than_class_3"] = bool(end012 is not None and end3 is not None and end012 <= end3)
    print(json.dumps(doc, indent=1))
    if out:
        json.dump(doc, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
