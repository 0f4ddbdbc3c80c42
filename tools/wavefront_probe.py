"""Times Scene.wavefront (the depth loop on the device) against what it replaces -- the torch loop over Scene.bounce with its
compaction, its carried root index and the emission-order sum -- and, at depth 5, against the full trace Scene.trace_rays:
C2 at 1920x1080 with one thin-lens sample per pixel and the glass bunny at 1024x1024, depths 5, 8 and 12.  Writes
profiles/wavefront_trace_bench.json (or the path given).

    python tools/wavefront_probe.py [out.json] [--resources table.json]

Per form: 2 warm-ups, then 5 runs, the forms taking turns, each run between two host clock readings with the device idle before and after (both loops
synchronise with the host, so device events would miss their round trips); the median, least and largest run are reported.
The step kernel's registers come from the compiler's report as tools/resource_table.py reads it (--resources: a table it wrote
before; else it is run here, which compiles the device code once more).  The expectation to hold the numbers against:
Scene.wavefront does strictly less memory traffic and fewer synchronisations than the torch loop, so it must not be slower at any
depth; at depth 5 the register-resident tree of trace_rays is expected to win."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes
from cgraytracing_amd import _capi

WARM, RUNS = 2, 5
DEPTHS = (5, 8, 12)


def timed(forms):
    """forms: name -> callable.  The forms take turns, run by run, so that what else the machine does meets them alike."""
    for fn in forms.values():
        for _ in range(WARM):
            fn()
    ms = {name: [] for name in forms}
    for _ in range(RUNS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v))) for name, v in ms.items()}


def torch_loop(sc, org, dirs, keys, depth):
    """The loop of tests/test_gpu_bounce.py on the device as far as torch goes: per level one bounce call, the Hitpoints'
    (root, path, value) gathered, torch.nonzero and six gathers for the children; then the emission-order sum -- a sort by
    (root, left-aligned path) and one masked add per position within a root, fp64 from 0.  Returns (acc, nhit, rays per level)."""
    n = org.shape[0]
    dev = org.device
    root = torch.arange(n, device=dev)
    adj = path = None
    hp_root, hp_path, hp_value, rays = [], [], [], []
    for level in range(1, depth + 1):
        res = sc.bounce(org, dirs, adj, path, keys, want=("step", "value", "children"))
        rays.append(int(res["counters"][_capi.CNT_RAYS].item()))
        hp = torch.nonzero(res["step"] == _capi.STEP_HITPOINT).flatten()
        hp_root.append(root[hp])
        hp_path.append(path[hp].long() if path is not None else torch.ones(hp.numel(), dtype=torch.int64, device=dev))
        hp_value.append(res["value"][hp])
        if level == depth:
            break
        keep = torch.nonzero(res["child_path"] != 0).flatten()
        org, dirs, adj, path, keys = (res[k][keep] for k in ("child_org", "child_dir", "child_adj", "child_path", "child_keys"))
        root = torch.cat([root, root])[keep]
        if org.shape[0] == 0:
            break
    r, p, v = torch.cat(hp_root), torch.cat(hp_path), torch.cat(hp_value)
    bits = torch.zeros_like(p)
    for b in range(1, 32):
        bits += (p >> b) > 0
    order = torch.argsort((r << 30) | ((p - (torch.ones_like(bits) << bits)) << (30 - bits)))
    r, v = r[order], v[order]
    nhit = torch.bincount(r, minlength=n)
    starts = torch.cumsum(nhit, 0) - nhit
    seq = torch.arange(r.numel(), device=dev) - starts[r]
    acc = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    for k in range(int(nhit.max().item()) if r.numel() else 0):
        sel = torch.nonzero(seq == k).flatten()
        acc[r[sel]] += v[sel]  # each root at most once per k
    return acc, nhit.int(), rays


def step_kernel_resources(table, variant_w, variant_b):
    rows = {k["kernel"]: k for k in table["kernels"]}
    pick = lambda r: None if r is None else {k: r[k] for k in ("vgprs", "vgpr_spills", "scratch_bytes_per_lane", "occupancy_waves_per_simd")}
    return dict(wavefront_step_kernel=pick(rows.get(variant_w)), bounce_rays_kernel=pick(rows.get(variant_b)))


def probe(name, objs, cam, W, H, table):
    sc = cg.Scene(objs)
    org, dirs, keys = sc.camera_rays(W, H, 1, cam)
    n = org.shape[0]
    dev = org.device
    out = dict(acc=torch.empty((n, 3), dtype=torch.float64, device=dev), nhit=torch.empty(n, dtype=torch.int32, device=dev))
    full = dict(acc=torch.empty((n, 3), dtype=torch.float64, device=dev), nhit=torch.empty(n, dtype=torch.int32, device=dev))
    rec = dict(name=name, width=W, height=H, rays=n, step_variant=sc.wavefront_variant(), bounce_variant=sc.bounce_variant(), depths={})
    rec["registers"] = step_kernel_resources(table, rec["step_variant"], rec["bounce_variant"])
    for depth in DEPTHS:
        res = sc.wavefront(org, dirs, keys, max_depth=depth, out=out)
        acc, nhit, rays = torch_loop(sc, org, dirs, keys, depth)
        torch.cuda.synchronize()
        d = dict(rays_per_level=res["rays_per_level"], hitpoints=res["hp_count"], slices=res["slices"], halvings=res["halvings"],
                 equals_torch_loop=bool(torch.equal(out["acc"], acc) and torch.equal(out["nhit"], nhit) and rays == res["rays_per_level"]))
        forms = {"wavefront": lambda: sc.wavefront(org, dirs, keys, max_depth=depth, out=out),
                 "torch_loop": lambda: torch_loop(sc, org, dirs, keys, depth)}
        if depth == 5:
            sc.trace_rays(org, dirs, keys, max_depth=5, want=("acc", "nhit"), out=full)
            torch.cuda.synchronize()
            d["equals_trace_rays"] = bool(torch.equal(out["acc"], full["acc"]) and torch.equal(out["nhit"], full["nhit"]))
            forms["trace_rays"] = lambda: sc.trace_rays(org, dirs, keys, max_depth=5, want=("acc", "nhit"), out=full)
        d["time"] = timed(forms)
        d["wavefront_over_torch_loop"] = d["time"]["wavefront"]["median_ms"] / d["time"]["torch_loop"]["median_ms"]
        if depth == 5:
            d["wavefront_over_trace_rays"] = d["time"]["wavefront"]["median_ms"] / d["time"]["trace_rays"]["median_ms"]
        rec["depths"][str(depth)] = d
        print(json.dumps({name: {depth: d}}), flush=True)
    sc.close()
    return rec


def main(argv):
    path = os.path.join(ROOT, "profiles", "wavefront_trace_bench.json")
    table = None
    args = list(argv)
    if "--resources" in args:
        i = args.index("--resources")
        table = json.load(open(args[i + 1]))
        del args[i:i + 2]
    if args:
        path = args[0]
    if table is None:
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "resource_table.py"), "--out", os.path.join(tmp, "t.json")],
                                  stdout=subprocess.DEVNULL)
            table = json.load(open(os.path.join(tmp, "t.json")))
    recs = [probe("c2_spheres", scenes.scene_c2(), scenes.cam_dof(), 1920, 1080, table),
            probe("c3_glass_bunny", scenes.scene_c3(True), scenes.cam_dof(), 1024, 1024, table)]
    doc = dict(device=torch.cuda.get_device_name(0),
               method="host clock around each run with the device idle before and after, %d warm-ups, median of %d runs per form" % (WARM, RUNS),
               registers_from=table["command"], configurations=recs)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
