"""Measurement driver (not a test): resumable photon mapping (cgrt_ppm_session) against the one-shot cgrt_ppm_render in the
reference's committed configuration (tests/measure_ppm.py's scene: 1024x768, spp 1, planes + stone bump floor + dragon,
20 480 000 photons).

Records the one-shot wall time and stage times; the session fed as 1 x N, 20 x N/20 and 200 x N/200 photons, each with and
without lookahead, with a device checkpoint image after every call (the interactive pattern); the host and device
checkpoint times against the one-shot's ms_gather.  Every session's final image (and rgb8) must equal the one-shot's bit for
bit, or the probe exits 1.

    python tools/ppm_session_probe.py [--photons N] [--out profiles/ppm_session.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import cgraytracing_amd as cg
import scenes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=20480000)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--splits", default="1,20,200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppm_session.json"))
    args = ap.parse_args()
    import torch

    W, H, N = args.width, args.height, args.photons
    objs = scenes.planes(scenes.stone_texture()) + [
        scenes.TriangleMesh.from_triangles(scenes.dragon_tris(), (0.25, 0.25, 0.5), 0.0, 0.0, 1)]
    cam = scenes.cam_pinhole()
    sc = cg.Scene(objs)
    sc.ppm_render(64, 48, 1, cam, 5, 12345, nphotons=1000)  # warm-up (module load, allocator)
    with sc.ppm_session(64, 48, 1, cam, 5, 12345, nphotons=1000) as w:
        w.image_tensor()
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    one = sc.ppm_render(W, H, 1, cam, 5, 12345, nphotons=N, want_rgb8=True)
    one_wall = time.perf_counter() - t0
    doc = {"workload": "committed scene %dx%d spp 1, %d photons" % (W, H, N),
           "one_shot": {"wall_ms": round(one_wall * 1e3, 2), "stage_ms": {k: round(v, 3) for k, v in one["ms"].items()},
                        "hitpoints": one["count"], "n_events": one["n_events"], "n_pairs": one["n_pairs"]},
           "sessions": []}
    ok = True
    dev = torch.device("cuda", sc.device)
    for parts in [int(x) for x in args.splits.split(",")]:
        for lookahead in (True, False):
            img_t = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
            rgb_t = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            t0 = time.perf_counter()
            ses = sc.ppm_session(W, H, 1, cam, 5, 12345, lookahead=lookahead)
            create_ms = (time.perf_counter() - t0) * 1e3
            add_wall, add_dev, dev_img_wall, dev_img_ms = [], [], [], []
            for p in range(parts):
                n = N * (p + 1) // parts - ses.photons_done
                t0 = time.perf_counter()
                ses.add_photons(n)
                add_wall.append((time.perf_counter() - t0) * 1e3)
                add_dev.append(ses.info()["ms_last_add"])
                t0 = time.perf_counter()
                ses.image_tensor(out=img_t, rgb8_out=rgb_t)
                torch.cuda.current_stream(dev).synchronize()
                dev_img_wall.append((time.perf_counter() - t0) * 1e3)
                dev_img_ms.append(ses.info()["ms_last_image"])
            host_ms = []
            for _ in range(5):
                t0 = time.perf_counter()
                img = ses.image()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            host_gather_ms = ses.info()["ms_last_image"]
            rgb8 = ses.rgb8()
            inf = ses.info()
            same = (np.array_equal(img, one["image"]) and np.array_equal(rgb8, one["rgb8"]) and
                    np.array_equal(img_t.cpu().numpy(), one["image"]) and np.array_equal(rgb_t.cpu().numpy(), one["rgb8"]) and
                    inf["n_events"] == one["n_events"])
            ok = ok and same
            ses.close()
            rec = {"calls": parts, "photons_per_call": N // parts, "lookahead": lookahead, "create_wall_ms": round(create_ms, 2),
                   "ms_eye": round(inf["ms_eye"], 3), "ms_table": round(inf["ms_table"], 3),
                   "photon_stage_wall_ms": round(sum(add_wall), 2), "photon_stage_device_ms": round(inf["ms_photons"], 2),
                   "photon_stage_vs_one_shot": round(sum(add_wall) / one["ms"]["photons"], 3),
                   "add_wall_ms_median": round(float(np.median(add_wall)), 3),
                   "checkpoint_device_gather_ms_median": round(float(np.median(dev_img_ms)), 4),
                   "checkpoint_device_wall_ms_median": round(float(np.median(dev_img_wall)), 4),
                   "checkpoint_host_wall_ms_median": round(float(np.median(host_ms)), 3),
                   "checkpoint_host_gather_ms": round(host_gather_ms, 4),
                   "n_batch_halvings": inf["n_batch_halvings"], "n_pairs": inf["n_pairs"],
                   "device_bytes": inf["device_bytes"], "bit_identical_to_one_shot": bool(same)}
            doc["sessions"].append(rec)
            print(json.dumps(rec), flush=True)
    sc.close()
    doc["all_bit_identical"] = bool(ok)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["one_shot"]))
    if not ok:
        print("FAIL: a session's image differs from the one-shot render", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
