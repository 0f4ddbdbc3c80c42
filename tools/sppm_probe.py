"""Measurement driver (not a test): stochastic progressive photon mapping (cgrt_sppm_session) of C2 under the thin lens at
1920x1080 -- 16 passes of spp 1 with 1 M photons each -- beside one classic cgrt_ppm_session of the same sample and photon
budget (spp 16, 16 M photons).

Records per pass the device ms of the eye, table, photon and update stages, the pass's wall time (what is left of it beside the
stages is the host's share: allocating and freeing the pass's table among it) and device_bytes; for the classic session its
stage times and device_bytes.  The claim the numbers are for: the SPPM session's memory does not depend on the passes, the
classic session's grows with spp.

    python tools/sppm_probe.py [--passes 16] [--photons 1000000] [--out profiles/sppm_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cgraytracing_amd as cg
import scenes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--photons", type=int, default=1000000, help="per pass")
    ap.add_argument("--no-classic", action="store_true", help="skip the cgrt_ppm_session run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sppm_probe.json"))
    args = ap.parse_args()
    W, H, P, M = args.width, args.height, args.passes, args.photons
    cam = scenes.cam_dof()
    sc = cg.Scene(scenes.scene_c2())
    with sc.sppm_session(64, 48, 1, cam) as w:  # warm-up (module load, allocator)
        w.add_passes(2, 1000)
        w.image()
    doc = {"workload": "C2, thin lens, %dx%d: %d passes of spp 1 with %d photons each" % (W, H, P, M), "passes": []}
    t_all = time.perf_counter()
    with sc.sppm_session(W, H, 1, cam) as ses:
        for k in range(P):
            t0 = time.perf_counter()
            ses.add_passes(1, M)
            wall = (time.perf_counter() - t0) * 1e3
            inf = ses.info()
            stages = inf["ms_eye"] + inf["ms_table"] + inf["ms_photons"] + inf["ms_update"]
            rec = {"pass": k + 1, "ms_eye": round(inf["ms_eye"], 3), "ms_table": round(inf["ms_table"], 3),
                   "ms_photons": round(inf["ms_photons"], 3), "ms_update": round(inf["ms_update"], 3), "wall_ms": round(wall, 3),
                   "wall_minus_stages_ms": round(wall - stages, 3), "hp_count": inf["hp_count"], "device_bytes": inf["device_bytes"]}
            doc["passes"].append(rec)
            print(json.dumps(rec), flush=True)
        t0 = time.perf_counter()
        ses.rgb8()
        doc["sppm"] = {"total_wall_ms": round((time.perf_counter() - t_all) * 1e3, 2), "image_wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                       "n_events": inf["n_events"], "n_pairs": inf["n_pairs"], "n_batch_halvings": inf["n_batch_halvings"],
                       "device_bytes_min": min(r["device_bytes"] for r in doc["passes"]),
                       "device_bytes_max": max(r["device_bytes"] for r in doc["passes"])}
    if not args.no_classic:
        t0 = time.perf_counter()
        with sc.ppm_session(W, H, P, cam, 5, 12345) as ses:
            ses.add_photons(P * M)
            inf = ses.info()
            doc["classic"] = {"spp": P, "photons": P * M, "wall_ms": round((time.perf_counter() - t0) * 1e3, 2),
                              "ms_eye": round(inf["ms_eye"], 3), "ms_table": round(inf["ms_table"], 3),
                              "ms_photons": round(inf["ms_photons"], 3), "hp_count": inf["hp_count"],
                              "device_bytes": inf["device_bytes"]}
        print(json.dumps(doc["classic"]), flush=True)
    sc.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["sppm"]))


if __name__ == "__main__":
    main()
