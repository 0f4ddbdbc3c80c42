"""Times Scene.trace_grid_aov (all five buffers) against the composed path it replaces -- camera_rays, the nearest-hit trace_rays
without its sign pass, hit_attributes' colour and the fold per pixel in torch -- and, for scale, trace_grid at the same sample
count.  Writes profiles/aov_probe.json (or the path given).

    python tools/aov_probe.py [out.json]

Per frame and path: median and best of 7 timed runs after 3 warm-ups (device events around one run each), one process; the
composed path's stages on their own; the peak of torch's device allocations over one run of each path (the ray list, the
per-ray results and the fold's temporaries against five frame buffers).  The two paths' buffers are compared bit for bit at
every frame before anything is timed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes

NAMES = ("albedo", "normal", "depth", "hits", "obj_id")


def timed(fn, warm=3, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), best_ms=float(min(ms)), all_ms=[round(x, 4) for x in ms])


def peak_bytes(fn):
    """torch's peak device allocation over one run of fn, above what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    return int(peak)


def fold(W, spp, dirs, hit, col):
    """The contract's fold: the normal turned against the ray, fp64 sums per pixel in sample order from +0.0, one rounding."""
    rows = dirs.shape[0] // (spp * W)
    d = dirs.view(spp, rows, W, 3)
    ids, t = hit["hit_obj"].view(spp, rows, W), hit["hit_t"].view(spp, rows, W)
    n, c = hit["hit_normal"].view(spp, rows, W, 3), col["color"].view(spp, rows, W, 3)
    alb = torch.zeros((rows, W, 3), dtype=torch.float64, device=dirs.device)
    nrm, dep = torch.zeros_like(alb), torch.zeros((rows, W), dtype=torch.float64, device=dirs.device)
    hits = torch.zeros((rows, W), dtype=torch.int32, device=dirs.device)
    zero = torch.zeros((), dtype=torch.float64, device=dirs.device)
    for k in range(spp):
        is_hit = ids[k] >= 0
        nd = (n[k, ..., 0] * d[k, ..., 0] + n[k, ..., 1] * d[k, ..., 1]) + n[k, ..., 2] * d[k, ..., 2]
        m = torch.where((nd > 0)[..., None], -n[k], n[k])
        alb += torch.where(is_hit[..., None], c[k], zero)
        nrm += torch.where(is_hit[..., None], m, zero)
        dep += torch.where(is_hit, t[k], zero)
        hits += is_hit.to(torch.int32)
    inv = 1.0 / spp
    return dict(albedo=(alb * inv).float(), normal=(nrm * inv).float(), depth=(dep * inv).float(), hits=hits,
                obj_id=torch.where(ids[0] >= 0, ids[0], torch.full_like(ids[0], -1)))


def probe(name, objs, cam, W, H, spp, depth=5):
    sc = cg.Scene(objs)
    rec = dict(name=name, width=W, height=H, spp=spp, rays=W * H * spp, aov_variant=sc.aov_variant(W, H, cam),
               query_variant=sc.rays_variant(1, want=("hit",)), grid_variant=sc.kernel_variant(W, H, spp, cam, depth))

    def composed():
        org, dirs, keys = sc.camera_rays(W, H, spp, cam)
        hit = sc.trace_rays(org, dirs, keys, want=("hit",), sign_pass=False)
        col = sc.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=("color",))
        return fold(W, spp, dirs, hit, col)

    # the same buffers, bit for bit, before anything is timed
    got, want = sc.trace_grid_aov(W, H, spp, cam), composed()
    torch.cuda.synchronize()
    rec["equal_bit_for_bit"] = {k: bool(torch.equal(got[k], want[k])) for k in NAMES}
    assert all(rec["equal_bit_for_bit"].values()), rec["equal_bit_for_bit"]
    del want

    out = {k: got[k] for k in NAMES}
    cnt = got["counters"]
    rec["aov"] = timed(lambda: sc.trace_grid_aov(W, H, spp, cam, out=out, counters=cnt))
    rec["composed"] = timed(composed)
    rgb, nhit, gcnt = sc.trace_grid(W, H, spp, cam, depth)
    rec["trace_grid"] = timed(lambda: sc.trace_grid(W, H, spp, cam, depth, out=rgb, nhit=nhit, counters=gcnt))
    # the composed path's stages, each on the buffers of the one before
    org, dirs, keys = sc.camera_rays(W, H, spp, cam)
    hit = sc.trace_rays(org, dirs, keys, want=("hit",), sign_pass=False)
    col = sc.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=("color",))
    hout = {k: hit[k] for k in ("hit_obj", "hit_t", "hit_normal")}
    rec["composed_stages"] = dict(
        camera_rays=timed(lambda: sc.camera_rays(W, H, spp, cam)),
        trace_rays_query=timed(lambda: sc.trace_rays(org, dirs, keys, want=("hit",), sign_pass=False, out=hout, counters=hit["counters"])),
        hit_attributes_color=timed(lambda: sc.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=("color",), out=col)),
        torch_fold=timed(lambda: fold(W, spp, dirs, hit, col)))
    del org, dirs, keys, hit, col, hout
    rec["peak_device_bytes"] = dict(aov=peak_bytes(lambda: sc.trace_grid_aov(W, H, spp, cam)), composed=peak_bytes(composed))
    rec["ratio_composed_to_aov"] = rec["composed"]["median_ms"] / rec["aov"]["median_ms"]
    rec["ratio_aov_to_trace_grid"] = rec["aov"]["median_ms"] / rec["trace_grid"]["median_ms"]
    rec["aov_no_slower_than_composed"] = rec["aov"]["median_ms"] <= rec["composed"]["median_ms"]
    sc.close()
    print(json.dumps(rec))
    return rec


def main(path=os.path.join(ROOT, "profiles", "aov_probe.json")):
    recs = [probe("c2_1920x1080_dof_spp1", scenes.scene_c2(), scenes.cam_dof(), 1920, 1080, 1),
            probe("c2_1920x1080_dof_spp64", scenes.scene_c2(), scenes.cam_dof(), 1920, 1080, 64),
            probe("dragon_1024_spp16", scenes.scene_dragon(), scenes.cam_pinhole(), 1024, 1024, 16)]
    doc = dict(device=torch.cuda.get_device_name(0), method="device events around single runs: 3 warm-ups, 7 timed, one process",
               frames=recs)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)
    assert all(r["aov_no_slower_than_composed"] for r in recs), "the AOV launch is slower than the composed path on some frame"


if __name__ == "__main__":
    main(*sys.argv[1:2])
