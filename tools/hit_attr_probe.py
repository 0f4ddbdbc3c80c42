"""Times Scene.hit_attributes beside the nearest-hit query it follows, on the three frames of DESIGN.md section 4.17's table.
Writes profiles/hit_attributes_probe.json (or the path given).

    python tools/hit_attr_probe.py [out.json]

Per frame: the camera's primary rays at one sample per pixel; median and best of 7 timed launches after 3 warm-ups (device
events around one launch each, as tools/rays_probe.py) of the query and of the attribute pass with all four arrays, with
prim + uv only (the tree re-walk) and with color + material only (no walk).  Nothing here is a pass/fail threshold."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch

import cgraytracing_amd as cg
import scenes
from rays_probe import timed


def probe(name, objs, cam, W, H):
    sc = cg.Scene(objs)
    org, dirs, keys = sc.camera_rays(W, H, 1, cam)
    n, dev = org.shape[0], org.device
    hit = dict(hit_obj=torch.empty(n, dtype=torch.int32, device=dev), hit_t=torch.empty(n, dtype=torch.float64, device=dev),
               hit_normal=torch.empty((n, 3), dtype=torch.float64, device=dev))
    out = dict(prim=torch.empty(n, dtype=torch.int32, device=dev), uv=torch.empty((n, 2), dtype=torch.float64, device=dev),
               color=torch.empty((n, 3), dtype=torch.float64, device=dev), material=torch.empty((n, 2), dtype=torch.float64, device=dev))
    rec = dict(name=name, width=W, height=H, rays=n, query_variant=sc.rays_variant(5, want=("hit",)))
    rec["trace_rays_query"] = timed(lambda: sc.trace_rays(org, dirs, keys, want=("hit",), out=hit))
    attrs = lambda want: sc.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=want, out=out)
    rec["hit_attributes_all"] = timed(lambda: attrs(("prim", "uv", "color", "material")))
    rec["hit_attributes_prim_uv"] = timed(lambda: attrs(("prim", "uv")))
    rec["hit_attributes_color_material"] = timed(lambda: attrs(("color", "material")))
    torch.cuda.synchronize()
    rec["rays_with_a_triangle"] = int((out["prim"] >= 0).sum().item())
    rec["ratio_all_to_query"] = rec["hit_attributes_all"]["median_ms"] / rec["trace_rays_query"]["median_ms"]
    sc.close()
    print(json.dumps(rec))
    return rec


def main(path=os.path.join(ROOT, "profiles", "hit_attributes_probe.json")):
    recs = [probe("c2_1920x1080_dof", scenes.scene_c2(), scenes.cam_dof(), 1920, 1080),
            probe("dragon_1024", scenes.scene_dragon(), scenes.cam_pinhole(), 1024, 1024),
            probe("c3_glass_bunny_1024", scenes.scene_c3(True), scenes.cam_dof(), 1024, 1024)]
    doc = dict(device=torch.cuda.get_device_name(0), method="device events around single launches: 3 warm-ups, 7 timed",
               configurations=recs)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:2])
