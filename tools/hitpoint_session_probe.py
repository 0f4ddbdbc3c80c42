"""Table-build time of a hitpoint session against a ray session on the same rays (profiles/hitpoint_session.json).

C2, camera rays of a W x H frame: the ray session (Scene.ppm_session_rays) traces them itself and builds its table from 10-double
labelled records; the hitpoint session (Scene.ppm_session_hitpoints) builds its table from the depth-5 wavefront's records.
Both report ms_table (device events around the table build, cgrt_ppm_session_get_info).  The two are created in turn, `reps`
times after a warm-up of each; no photon is traced.  The sessions are also compared: same hp_count, and after a few photons the
same image.

    python tools/hitpoint_session_probe.py [out.json] [W] [H] [reps]
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes


def main(out=None, W=768, H=432, reps=9):
    W, H, reps = int(W), int(H), int(reps)
    sc = cg.Scene(scenes.scene_c2())
    org, dirs, keys = sc.camera_rays(W, H, 1, scenes.cam_dof(), 12345)
    count = sc.wavefront(org, dirs, keys, max_depth=5, want=())["hp_count"]
    wf = sc.wavefront(org, dirs, keys, max_depth=5, want=("hp",), hp_cap=count)
    torch.cuda.synchronize()

    def ray_session(nph=0):
        return sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=1, nphotons=nph)

    def hp_session(nph=0):
        return sc.ppm_session_hitpoints(wf["hp9"], wf["hp_ray"], wf["hp_path"], width=W, rows=H, spp=1, nphotons=nph)

    with ray_session(20000) as a, hp_session(20000) as b:  # warm-up, and the two are the same session
        same = bool(np.array_equal(a.image(), b.image()) and a.info()["hp_count"] == b.info()["hp_count"] == count)
    ms = dict(ray=[], hitpoints=[])
    for _ in range(reps):
        for name, make in (("ray", ray_session), ("hitpoints", hp_session)):
            with make() as ses:
                ms[name].append(ses.info()["ms_table"])
    sc.close()
    res = dict(scene="C2", width=W, height=H, rays=int(org.shape[0]), hitpoints=int(count), eye_depth=5, reps=reps,
               device=torch.cuda.get_device_name(0), same_session=same,
               ms_table_ray_session=dict(median=float(np.median(ms["ray"])), min=min(ms["ray"]), all=ms["ray"]),
               ms_table_hitpoint_session=dict(median=float(np.median(ms["hitpoints"])), min=min(ms["hitpoints"]), all=ms["hitpoints"]),
               note="device events around PpmTable::build (cgrt_ppm_session_info.ms_table), sessions created in turn after one "
                    "warm-up each; the hitpoint build includes its read-back of the kept count and its allocations")
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main(*sys.argv[1:5])
