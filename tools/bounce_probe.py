"""Times Scene.bounce (one step of trace() per ray) against the nearest-hit query Scene.trace_rays(want=("hit",)) on the same
rays, and the compacted wavefront loop in torch to depth 5 against one full Scene.trace_rays: the primary rays of the bench
frame (1920x1080, one thin-lens sample per pixel), C2 and the dragon scene.  Writes profiles/bounce_bench.json (or the path
given).

    python tools/bounce_probe.py [out.json]

Per form: 3 warm-ups, then 20 runs, each between two device events; the median, least and largest run are reported.  The
expectation to hold the numbers against: a bounce call costs the nearest-hit walk plus its stores (up to 37 doubles a ray); the
wavefront loop costs more than the fused recursion -- that is the price of the seam between the levels."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes
from cgraytracing_amd import _capi

WARM, RUNS = 3, 20
ALL = ("step", "hit", "pos", "normal", "value", "children")


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def wavefront(sc, org, dirs, keys, depth):
    """The compacted loop: per level one bounce call, torch.nonzero and five gathers; returns the rays traced per level"""
    adj = path = None
    rays = []
    for level in range(1, depth + 1):
        res = sc.bounce(org, dirs, adj, path, keys, want=("step", "value", "children"))
        rays.append(org.shape[0])
        if level == depth:
            break
        keep = torch.nonzero(res["child_path"] != 0).flatten()
        org, dirs, adj, path, keys = (res[k][keep] for k in ("child_org", "child_dir", "child_adj", "child_path", "child_keys"))
        if org.shape[0] == 0:
            break
    return rays


def probe(name, objs, cam, W=1920, H=1080, depth=5):
    sc = cg.Scene(objs)
    org, dirs, keys = sc.camera_rays(W, H, 1, cam)
    n = org.shape[0]
    dev = org.device
    hit = dict(hit_obj=torch.empty(n, dtype=torch.int32, device=dev), hit_t=torch.empty(n, dtype=torch.float64, device=dev),
               hit_normal=torch.empty((n, 3), dtype=torch.float64, device=dev))
    out = {k: v for k, v in sc.bounce(org, dirs, keys=keys, want=ALL).items() if k != "counters"}
    full = dict(acc=torch.empty((n, 3), dtype=torch.float64, device=dev), nhit=torch.empty(n, dtype=torch.int32, device=dev))
    first = sc.bounce(org, dirs, keys=keys, want=("step",))
    torch.cuda.synchronize()
    steps = np.bincount(first["step"].cpu().numpy(), minlength=4).tolist()
    rec = dict(name=name, width=W, height=H, rays=n, first_level_steps=dict(zip(("none", "hitpoint", "reflect", "split"), steps)),
               bounce_variant=sc.bounce_variant(), query_variant=sc.rays_variant(1, want=("hit",)), full_variant=sc.rays_variant(depth))
    rec["rays_per_level"] = wavefront(sc, org, dirs, keys, depth)
    rec["time"] = {
        "nearest_hit_query": timed(lambda: sc.trace_rays(org, dirs, keys, want=("hit",), out=hit, sign_pass=False)),
        "bounce_all_outputs": timed(lambda: sc.bounce(org, dirs, keys=keys, want=ALL, out=out)),
        "bounce_step_and_children": timed(lambda: sc.bounce(org, dirs, keys=keys, want=("step", "children"), out=out)),
        "bounce_step_only": timed(lambda: sc.bounce(org, dirs, keys=keys, want=("step",), out=out)),
        "full_trace_depth_%d" % depth: timed(lambda: sc.trace_rays(org, dirs, keys, max_depth=depth, want=("acc", "nhit"), out=full)),
        "wavefront_loop_depth_%d" % depth: timed(lambda: wavefront(sc, org, dirs, keys, depth)),
    }
    t = rec["time"]
    rec["bounce_all_over_query"] = t["bounce_all_outputs"]["median_ms"] / t["nearest_hit_query"]["median_ms"]
    rec["bounce_children_over_query"] = t["bounce_step_and_children"]["median_ms"] / t["nearest_hit_query"]["median_ms"]
    rec["wavefront_over_full_trace"] = t["wavefront_loop_depth_%d" % depth]["median_ms"] / t["full_trace_depth_%d" % depth]["median_ms"]
    rec["output_bytes_all"] = int(sum(v.numel() * v.element_size() for v in out.values()))
    sc.close()
    print(json.dumps(rec))
    return rec


def main(path=os.path.join(ROOT, "profiles", "bounce_bench.json")):
    recs = [probe("c2_spheres", scenes.scene_c2(), scenes.cam_dof()), probe("dragon", scenes.scene_dragon(), scenes.cam_dof())]
    doc = dict(device=torch.cuda.get_device_name(0), method="device events around each run, %d warm-ups, median of %d runs per form" % (WARM, RUNS),
               configurations=recs)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:2])
