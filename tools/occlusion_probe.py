"""Times Scene.occluded (the any-hit kernel) against the nearest-hit query Scene.trace_rays(want=("hit",)) on the same rays:
the shadow rays of a 1920x1080 frame at one sample per pixel towards the reference's light.  Writes
profiles/occlusion_bench.json (or the path given).

    python tools/occlusion_probe.py [out.json]

Per scene: the camera's rays are traced, every hit sends one shadow ray (origin moved 1e-4 along the normal turned against the
camera ray, direction towards the light, tmax = the distance to the light; a camera ray that hits nothing sends none: its
direction is zero).  Timed: 3 warm-ups, then 9 windows of 4 launches each per form, the forms ALTERNATING window by window
(device events around a window); median, least and largest window per launch are reported, so a difference can be held against
the spread.  Node and triangle tests are those of one launch with STATS."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes

LIGHT = (0.0, 19.999, 20.0)
WARM, WINDOWS, PER_WINDOW = 3, 9, 4


def timed_alternating(fns):
    """{name: fn} -> {name: dict(median_ms, min_ms, max_ms, all_ms)} per launch"""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_WINDOW):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / PER_WINDOW)
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), all_ms=[round(x, 4) for x in v])
            for k, v in ms.items()}


def shadow_rays(sc, cam, W, H):
    org, dirs, _ = sc.camera_rays(W, H, 1, cam)
    hit = sc.trace_rays(org, dirs, want=("hit",))
    seen = hit["hit_obj"] >= 0
    n = hit["hit_normal"]
    n = torch.where((n * dirs).sum(dim=1, keepdim=True) > 0, -n, n)
    P = org + dirs * hit["hit_t"][:, None] + n * 1e-4
    to_light = torch.tensor(LIGHT, dtype=torch.float64, device=org.device) - P
    dist = to_light.norm(dim=1)
    L = to_light / dist[:, None]
    L[~seen] = 0.0
    return P.contiguous(), L.contiguous(), dist.contiguous(), int(seen.sum().item())


def probe(name, objs, cam, W=1920, H=1080):
    sc = cg.Scene(objs)
    P, L, dist, n_rays = shadow_rays(sc, cam, W, H)
    n = P.shape[0]
    dev = P.device
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    hit = dict(hit_obj=torch.empty(n, dtype=torch.int32, device=dev), hit_t=torch.empty(n, dtype=torch.float64, device=dev),
               hit_normal=torch.empty((n, 3), dtype=torch.float64, device=dev))
    rec = dict(name=name, width=W, height=H, shadow_rays=n_rays, occlusion_variant=sc.occlusion_variant(),
               query_variant=sc.rays_variant(1, want=("hit",)))
    rec["time"] = timed_alternating({
        "occluded": lambda: sc.occluded(P, L, dist, out=occ),
        "occluded_skip_transparent": lambda: sc.occluded(P, L, dist, skip_transparent=True, out=occ),
        "nearest_hit_query": lambda: sc.trace_rays(P, L, want=("hit",), out=hit, sign_pass=False),
    })
    t = rec["time"]
    rec["speedup_median"] = t["nearest_hit_query"]["median_ms"] / t["occluded"]["median_ms"]
    rec["faster_beyond_spread"] = bool(t["occluded"]["max_ms"] < t["nearest_hit_query"]["min_ms"])
    # the answers, and what each form tested
    a = sc.occluded(P, L, dist, stats=True)
    s = sc.occluded(P, L, dist, skip_transparent=True, stats=True)
    q = sc.trace_rays(P, L, want=("hit",), stats=True, sign_pass=False)
    torch.cuda.synchronize()
    same = torch.equal(a["occluded"], ((q["hit_obj"] >= 0) & (q["hit_t"] < dist)).to(torch.uint8))
    rec["equal_to_query_and_compare"] = bool(same)
    rec["occluded_rays"] = int(a["occluded"].sum().item())
    rec["occluded_rays_skip_transparent"] = int(s["occluded"].sum().item())
    for key, c in (("occluded", a["counters"]), ("occluded_skip_transparent", s["counters"]), ("nearest_hit_query", q["counters"])):
        c = c.cpu().numpy()
        rec["tests_" + key] = dict(node=int(c[3]), triangle=int(c[4]), rays=int(c[0]), wave_iters=int(c[2]))
    sc.close()
    print(json.dumps(rec))
    return rec


def main(path=os.path.join(ROOT, "profiles", "occlusion_bench.json")):
    recs = [probe("c2_spheres", scenes.scene_c2(), scenes.cam_dof()),
            probe("c3_glass_bunny", scenes.scene_c3(True), scenes.cam_dof()),
            probe("dragon", scenes.scene_dragon(), scenes.cam_pinhole())]
    doc = dict(device=torch.cuda.get_device_name(0),
               method="device events around windows of %d launches, %d warm-ups, %d windows per form, forms alternating" % (PER_WINDOW, WARM, WINDOWS),
               light=LIGHT, configurations=recs)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:2])
