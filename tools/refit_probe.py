#!/usr/bin/env python3
"""Refit measurement (not a test): what cgrt_scene_refit_mesh costs and what it saves, on one MI355X.
  python tools/refit_probe.py [out.json]
For the dragon (100 000 triangles) and the opaque bunny, each twisted about its vertical axis -- mildly and strongly --:
  1. one refit, stream-timed (an event pair per refit, the median of REPS after WARM warm-up refits), and the first refit of
     the mesh, which builds the plan, by the host clock around a synchronise (with the library's own ms_plan);
  2. what a user does without it, in the same run: destroy + add + commit of the twisted mesh under the host build and under
     CGRT_BUILD_DEVICE (host clock around a synchronise, first and best of three);
  3. the frame time at 1024 x 1024, spp 16, after the refit against the frame time after a fresh build of the same pose in the
     same build mode -- the price of keeping a topology that was built for another pose -- and whether the frames are equal."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cgraytracing_amd as cg
import scenes

WARM, REPS = 5, 41
W = H = 1024
SPP = 16


def twist(tris, turns):
    """tris [n,9] on the device: every vertex turned about the vertical axis through the mesh's centre by an angle that grows
    with its height, `turns` radians from the lowest vertex to the highest."""
    p = tris.reshape(-1, 3)
    lo, hi = p.min(0).values, p.max(0).values
    c = 0.5 * (lo + hi)
    a = turns * (p[:, 1] - lo[1]) / (hi[1] - lo[1])
    x, z = p[:, 0] - c[0], p[:, 2] - c[2]
    q = torch.stack([c[0] + torch.cos(a) * x + torch.sin(a) * z, p[:, 1], c[2] - torch.sin(a) * x + torch.cos(a) * z], 1)
    return q.reshape(-1, 9).contiguous()


def frame_ms(sc, cam, reps=3):
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    sc.trace_grid(W, H, SPP, cam, 5, 12345, out=out, nhit=False, counters=cnt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        sc.trace_grid(W, H, SPP, cam, 5, 12345, out=out, nhit=False, counters=cnt)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def refit_ms(sc, obj, poses):
    """Median stream time of one refit, alternating the poses so that every refit moves the mesh."""
    for k in range(WARM):
        sc.refit_mesh(obj, poses[k % len(poses)])
    torch.cuda.synchronize()
    ms = []
    for k in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sc.refit_mesh(obj, poses[k % len(poses)])
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    for k in range(REPS):  # the enqueue alone, by the host clock: what the calling thread pays
        sc.refit_mesh(obj, poses[k % len(poses)])
    host = (time.perf_counter() - t0) * 1e3 / REPS
    torch.cuda.synchronize()
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": REPS,
            "host_enqueue_mean": round(host, 4)}


def main():
    cam = scenes.cam_dof()
    torch.zeros(1, device="cuda")
    meshes = {
        "dragon (100 000 triangles) + 5 planes": (scenes.dragon_tris(), lambda t: scenes.planes() + [scenes.TriangleMesh.from_triangles(t, (0.25, 0.25, 0.5), 0.0, 0.0, 1)]),
        "opaque bunny + 5 planes": (scenes.bunny_tris(), lambda t: scenes.planes(scenes.chessboard_texture(False)) + [scenes.TriangleMesh.from_triangles(t, (1.0, 1.0, 1.0))]),
    }
    res = {}
    for name, (tris, mk) in meshes.items():
        rest = torch.as_tensor(np.ascontiguousarray(tris), device="cuda")
        poses = {"mild twist (0.5 rad)": twist(rest, 0.5), "strong twist (3 rad)": twist(rest, 3.0)}
        host_poses = {k: v.cpu().numpy() for k, v in poses.items()}
        obj = len(mk(tris)) - 1
        rec = {"triangles": int(len(tris))}
        for mode in ("host", "device"):
            m = {}
            sc = cg.Scene(mk(tris), build=mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.refit_mesh(obj, poses["mild twist (0.5 rad)"])
            torch.cuda.synchronize()
            m["first_refit_with_plan_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            m["ms_plan"] = round(sc.refit_info(obj)["ms_plan"], 3)
            m["wide_nodes"] = sc.refit_info(obj)["nwide"]
            m["refit_ms"] = refit_ms(sc, obj, list(poses.values()))
            for pose, t in poses.items():
                sc.refit_mesh(obj, t)
                ms_refit, f_refit = frame_ms(sc, cam)
                walls = []
                for k in range(3):  # what a user does today: destroy, add, commit
                    t0 = time.perf_counter()
                    fresh = cg.Scene(mk(host_poses[pose]), build=mode)
                    torch.cuda.synchronize()
                    walls.append((time.perf_counter() - t0) * 1e3)
                    if k < 2:
                        fresh.close()
                ms_fresh, f_fresh = frame_ms(fresh, cam)
                fresh.close()
                m[pose] = {"destroy_add_commit_ms": {"first": round(walls[0], 3), "best_of_3": round(min(walls), 3)},
                           "frame_ms_after_refit": round(ms_refit, 3), "frame_ms_after_fresh_build": round(ms_fresh, 3),
                           "frame_time_ratio_refit_over_fresh": round(ms_refit / ms_fresh, 4),
                           "frames_bit_equal": bool(torch.equal(f_refit, f_fresh)),
                           "frames_linf": float((f_refit - f_fresh).abs().max()),
                           "pixels_not_bit_equal": int((f_refit != f_fresh).any(dim=2).sum())}
            sc.close()
            rec["build=" + mode] = m
        res[name] = rec
        print(name, json.dumps(rec), flush=True)
    out = {"what": "tools/refit_probe.py on one MI355X: cgrt_scene_refit_mesh against destroy + add + commit; frames %dx%d spp %d" % (W, H, SPP),
           "host_cpus": os.cpu_count(), "cases": res}
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
