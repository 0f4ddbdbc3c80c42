#!/usr/bin/env python3
"""Rebuild measurement (not a test): what cgrt_scene_rebuild_mesh costs against destroy + add + commit, and what the tree cost
says about frame time, on one MI355X.
  python tools/rebuild_probe.py [out.json] [--parent parent_commit.json]
  python tools/rebuild_probe.py --commit-only [out.json]
For the dragon (100 000 triangles) and the opaque bunny, device-built, each twisted about its vertical axis mildly and strongly
(tools/refit_probe.py's poses):
  1. the rebuild by the host clock around the call (it ends in a synchronise): the first one, which allocates the scratch, then
     the median and min-max of REPS after WARM warm-ups, alternating the poses, with levels, read-backs and scratch bytes;
  2. in the same loop, alternating with the rebuilds: destroy + add + commit of the same pose under CGRT_BUILD_DEVICE (host
     clock around a synchronise), and the commit's own cgrt_build_info.ms_device_build;
  3. frames at 1024 x 1024, spp 16, after a refit, after a rebuild and after a fresh commit of each pose, with mesh_cost: the
     frame-time ratio beside the cost ratio.
--commit-only does step 2's commits alone (no rebuild call), so that the figure can be taken with another checkout's package:
CGRT_PROBE_PACKAGE_ROOT names the directory that holds the cgraytracing_amd to import.  --parent merges such a file."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("CGRT_PROBE_PACKAGE_ROOT", ROOT))
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cgraytracing_amd as cg
import scenes

WARM, REPS = 3, 21
W = H = 1024
SPP = 16


def twist(tris, turns):
    """tools/refit_probe.py's: every vertex turned about the vertical axis through the mesh's centre by an angle that grows with
    its height, `turns` radians from the lowest vertex to the highest."""
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


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": len(ms)}


def commit(mk, host_pose):
    """destroy + add + commit under CGRT_BUILD_DEVICE: (wall ms, ms_device_build, the scene)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh = cg.Scene(mk(host_pose), build="device")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, fresh.build_info()["ms_device_build"], fresh


def meshes():
    return {
        "dragon (100 000 triangles) + 5 planes": (scenes.dragon_tris(), lambda t: scenes.planes() + [scenes.TriangleMesh.from_triangles(t, (0.25, 0.25, 0.5), 0.0, 0.0, 1)]),
        "opaque bunny + 5 planes": (scenes.bunny_tris(), lambda t: scenes.planes(scenes.chessboard_texture(False)) + [scenes.TriangleMesh.from_triangles(t, (1.0, 1.0, 1.0))]),
    }


def poses_of(tris):
    rest = torch.as_tensor(np.ascontiguousarray(tris), device="cuda")
    poses = {"mild twist (0.5 rad)": twist(rest, 0.5), "strong twist (3 rad)": twist(rest, 3.0)}
    return poses, {k: v.cpu().numpy() for k, v in poses.items()}


def commit_only():
    res = {}
    for name, (tris, mk) in meshes().items():
        _, host_poses = poses_of(tris)
        hp = list(host_poses.values())
        walls, builds = [], []
        for k in range(WARM + REPS):
            wall, build, fresh = commit(mk, hp[k % 2])
            fresh.close()
            if k >= WARM:
                walls.append(wall)
                builds.append(build)
        res[name] = {"destroy_add_commit_ms": stats(walls), "ms_device_build": stats(builds)}
        print(name, json.dumps(res[name]), flush=True)
    return res


def main(argv):
    torch.zeros(1, device="cuda")
    if "--commit-only" in argv:
        argv.remove("--commit-only")
        out = {"what": "tools/rebuild_probe.py --commit-only: destroy + add + commit under CGRT_BUILD_DEVICE", "cases": commit_only()}
        if argv:
            json.dump(out, open(argv[0], "w"), indent=1)
        return
    parent = None
    if "--parent" in argv:
        at = argv.index("--parent")
        parent = json.load(open(argv[at + 1]))
        del argv[at:at + 2]
    cam = scenes.cam_dof()
    total = lambda c: c["node_cost"] + c["tri_cost"]
    res = {}
    for name, (tris, mk) in meshes().items():
        poses, host_poses = poses_of(tris)
        pl, hp = list(poses.values()), list(host_poses.values())
        obj = len(mk(tris)) - 1
        rec = {"triangles": int(len(tris))}
        sc = cg.Scene(mk(tris), build="device")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.rebuild_mesh(obj, pl[0])
        rec["first_rebuild_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        rebuilds, walls, builds = [], [], []
        for k in range(WARM + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.rebuild_mesh(obj, pl[k % 2])
            ms = (time.perf_counter() - t0) * 1e3
            wall, build, fresh = commit(mk, hp[k % 2])
            fresh.close()
            if k >= WARM:
                rebuilds.append(ms)
                walls.append(wall)
                builds.append(build)
        inf = sc.rebuild_info(obj)
        rec["rebuild_ms"] = stats(rebuilds)
        rec["rebuild_info"] = {k: inf[k] for k in ("nwide", "stack_need", "balanced", "levels", "readbacks", "scratch_bytes")}
        rec["destroy_add_commit_ms"] = stats(walls)
        rec["ms_device_build"] = stats(builds)
        if parent and name in parent.get("cases", {}):
            rec["parent_commit"] = parent["cases"][name]
        rec["rebuild_below_commit"] = bool(rec["rebuild_ms"]["median"] < rec["destroy_add_commit_ms"]["median"])
        sc.close()
        for pose, t in poses.items():
            sc = cg.Scene(mk(tris), build="device")  # the topology of the rest pose
            sc.refit_mesh(obj, t)
            ms_refit, f_refit = frame_ms(sc, cam)
            f_refit = f_refit.clone()
            c_refit = sc.mesh_cost(obj)
            sc.rebuild_mesh(obj, t)
            ms_rebuilt, f_rebuilt = frame_ms(sc, cam)
            f_rebuilt = f_rebuilt.clone()
            c_rebuilt = sc.mesh_cost(obj)
            sc.close()
            _, _, fresh = commit(mk, host_poses[pose])
            ms_fresh, f_fresh = frame_ms(fresh, cam)
            c_fresh = fresh.mesh_cost(obj)
            fresh.close()
            rec[pose] = {"frame_ms_after_refit": round(ms_refit, 3), "frame_ms_after_rebuild": round(ms_rebuilt, 3),
                         "frame_ms_after_fresh_commit": round(ms_fresh, 3),
                         "frame_time_ratio_refit_over_fresh": round(ms_refit / ms_fresh, 4),
                         "frame_time_ratio_rebuilt_over_fresh": round(ms_rebuilt / ms_fresh, 4),
                         "cost_after_refit": c_refit, "cost_after_rebuild": c_rebuilt, "cost_after_fresh_commit": c_fresh,
                         "cost_ratio_refit_over_fresh": round(total(c_refit) / total(c_fresh), 4),
                         "cost_ratio_rebuilt_over_fresh": round(total(c_rebuilt) / total(c_fresh), 6),
                         "frames_bit_equal": bool(torch.equal(f_refit, f_fresh) and torch.equal(f_rebuilt, f_fresh)),
                         "pixels_not_bit_equal_refit": int((f_refit != f_fresh).any(dim=2).sum()),
                         "pixels_not_bit_equal_rebuilt": int((f_rebuilt != f_fresh).any(dim=2).sum())}
        res[name] = rec
        print(name, json.dumps(rec), flush=True)
    out = {"what": "tools/rebuild_probe.py on one MI355X: cgrt_scene_rebuild_mesh against destroy + add + commit under CGRT_BUILD_DEVICE; "
                   "frames %dx%d spp %d" % (W, H, SPP), "host_cpus": os.cpu_count(), "cases": res}
    if argv:
        json.dump(out, open(argv[0], "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
