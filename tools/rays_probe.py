"""Times Scene.trace_rays against Scene.trace_grid at one sample per pixel (the nearest existing launch: one image-order pass,
which neither reads 96 B of ray nor writes per-ray results).  Writes profiles/rays_probe.json (or the path given).

    python tools/rays_probe.py [out.json]

Per configuration: median and best of 7 timed launches after 3 warm-ups (device events around one launch each); the same rays
in a random permutation (incoherent waves); the nearest-hit query.  Bytes per ray are what the call moves through HBM at the
least: 48 B origin and direction (+8 B key) in, the result arrays out."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes


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


def probe(name, objs, cam, W, H, depth=5, permuted=False):
    sc = cg.Scene(objs)
    rec = dict(name=name, width=W, height=H, rays=W * H, max_depth=depth, grid_variant=sc.kernel_variant(W, H, 1, cam, depth),
               rays_variant=sc.rays_variant(depth), query_variant=sc.rays_variant(depth, want=("hit",)))
    out, nhit, cnt = sc.trace_grid(W, H, 1, cam, depth)
    rec["trace_grid_spp1"] = timed(lambda: sc.trace_grid(W, H, 1, cam, depth, out=out, nhit=nhit, counters=cnt))
    org, dirs, keys = sc.camera_rays(W, H, 1, cam)
    rec["camera_rays"] = timed(lambda: sc.camera_rays(W, H, 1, cam))
    n = org.shape[0]
    dev = org.device
    full = dict(acc=torch.empty((n, 3), dtype=torch.float64, device=dev), nhit=torch.empty(n, dtype=torch.int32, device=dev))
    hit = dict(hit_obj=torch.empty(n, dtype=torch.int32, device=dev), hit_t=torch.empty(n, dtype=torch.float64, device=dev),
               hit_normal=torch.empty((n, 3), dtype=torch.float64, device=dev))
    rec["trace_rays_full"] = timed(lambda: sc.trace_rays(org, dirs, keys, depth, want=("acc", "nhit"), out=full, counters=cnt))
    rec["trace_rays_full"]["hbm_bytes_per_ray"] = 56 + 28
    rec["trace_rays_query"] = timed(lambda: sc.trace_rays(org, dirs, keys, depth, want=("hit",), out=hit, counters=cnt))
    rec["trace_rays_query"]["hbm_bytes_per_ray"] = 56 + 36
    if "TREES=1" in rec["query_variant"]:  # what the pass that signs an opaque mesh's normals costs (0 where there is none)
        rec["trace_rays_query_no_sign_pass"] = timed(lambda: sc.trace_rays(org, dirs, keys, depth, want=("hit",), out=hit, counters=cnt,
                                                                          sign_pass=False))
    rec["ratio_full_to_grid"] = rec["trace_rays_full"]["median_ms"] / rec["trace_grid_spp1"]["median_ms"]
    if permuted:
        perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        po, pd, pk = org[perm].contiguous(), dirs[perm].contiguous(), keys[perm].contiguous()
        rec["trace_rays_full_permuted"] = timed(lambda: sc.trace_rays(po, pd, pk, depth, want=("acc", "nhit"), out=full, counters=cnt))
        rec["ratio_permuted_to_ordered"] = rec["trace_rays_full_permuted"]["median_ms"] / rec["trace_rays_full"]["median_ms"]
    cnt.zero_()
    sc.trace_rays(org, dirs, keys, depth, want=("acc", "nhit"), out=full, counters=cnt)
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    rec["traced_rays"], rec["lane_utilisation"] = int(c[0]), float(c[0]) / max(1.0, 64.0 * float(c[2]))
    sc.close()
    print(json.dumps(rec))
    return rec


def main(path=os.path.join(ROOT, "profiles", "rays_probe.json")):
    recs = [probe("c2_1920x1080_dof", scenes.scene_c2(), scenes.cam_dof(), 1920, 1080, permuted=True),
            probe("dragon_1024", scenes.scene_dragon(), scenes.cam_pinhole(), 1024, 1024),
            probe("c3_glass_bunny_1024", scenes.scene_c3(True), scenes.cam_dof(), 1024, 1024)]
    doc = dict(device=torch.cuda.get_device_name(0), method="device events around single launches: 3 warm-ups, 7 timed",
               configurations=recs)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)


def kernel_stats(db, path=os.path.join(ROOT, "profiles", "rays_probe_kernels.json")):
    """python tools/rays_probe.py --kernels RESULTS.db: the kernel times of a `rocprofv3 --kernel-trace --stats -- python
    tools/rays_probe.py` run (its rocpd database), per kernel of this library: calls, mean and least duration."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, count(*), avg(end - start) / 1000.0, min(end - start) / 1000.0 from kernels "
                                       "group by name order by 3 desc").fetchall()
    keep = [dict(kernel=n, calls=c, mean_us=round(a, 1), min_us=round(m, 1)) for n, c, a, m in rows
            if any(k in n for k in ("trace_rays_kernel", "trace_grid_kernel", "ray_normal_sign_kernel", "camera_rays_kernel"))]
    json.dump(dict(source="rocprofv3 --kernel-trace --stats -- python tools/rays_probe.py", kernels=keep), open(path, "w"), indent=1)
    for k in keep:
        print("%9.1f us  x%-3d %s" % (k["mean_us"], k["calls"], k["kernel"][:120]))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--kernels"]:
        kernel_stats(*sys.argv[2:4])
    else:
        main(*sys.argv[1:2])
