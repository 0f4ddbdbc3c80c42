"""Times the posed camera (CGRT_GRID_POSED) in the grid kernels against the built-in camera and against the ray-list route.
Writes profiles/posed_camera_probe.json (or the path given).

    python tools/posed_probe.py [out.json]

One MI355X, device events around one frame each, 3 warm-ups, the median of 7 (as tools/rays_probe.py).  Frames: C2 at
1920 x 1080 under the thin lens at 1 and 64 samples per pixel, the dragon at 1024 x 1024 pinhole at 4 samples.  Per frame:
  (a) the built-in camera, default launch
  (b) the built-in camera with CGRT_GRID_NO_TILE_ORDER (the form a posed launch runs)
  (c) the identity pose
  (d) the look-at view of examples/lookat_grid.py
  (e) the same look-at view through camera_rays + trace_rays, one sample per slice (what fits without a frame-sized ray
      buffer per sample), the samples averaged in torch
(c) against (b) is the pose's own cost; (d) against (e) is what the feature buys; (a) against (c) is what the tile order in the
camera's frame would have to win back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch

import cgraytracing_amd as cg
import scenes
from rays_probe import timed

IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
EYE, TARGET, FOV = (17.0, 8.0, 2.0), (-2.0, -13.0, 30.0), 70.0


def probe(name, objs, cam, W, H, spp, depth=5):
    sc = cg.Scene(objs)
    ident = cg.Camera(cam.cam, cam.half_width, cam.focus_plane, cam.lens_radius, pose=IDENTITY)
    look = cg.Camera.look_at(EYE, TARGET, (0.0, 1.0, 0.0), FOV, focus_distance=30.0, lens_radius=0.5 if cam.lens_radius > 0 else 0.0)
    rec = dict(name=name, width=W, height=H, spp=spp, max_depth=depth, variant_builtin=sc.kernel_variant(W, H, spp, cam, depth),
               variant_posed=sc.kernel_variant(W, H, spp, look, depth), rays_variant=sc.rays_variant(depth))
    out, nhit, cnt = sc.trace_grid(W, H, spp, cam, depth)

    def frame(camera, **kw):
        return timed(lambda: sc.trace_grid(W, H, spp, camera, depth, out=out, nhit=nhit, counters=cnt, **kw))

    rec["a_builtin_default"] = frame(cam)
    rec["b_builtin_no_tile_order"] = frame(cam, tile_order=False)
    rec["c_identity_pose"] = frame(ident)
    rec["d_look_at_grid"] = frame(look)
    n = W * H
    dev = out.device
    res = dict(acc=torch.empty((n, 3), dtype=torch.float64, device=dev))
    total = torch.zeros((n, 3), dtype=torch.float64, device=dev)

    def ray_route():  # a sample per slice: 56 B of ray buffer and 24 B of result per pixel at a time
        total.zero_()
        for k in range(spp):
            org, dirs, keys = sc.camera_rays(W, H, 1, look, sample_offset=k)
            sc.trace_rays(org, dirs, keys, depth, want=("acc",), out=res, counters=cnt)
            total.add_(res["acc"])
        return (total * (1.0 / spp)).to(torch.float32)

    rec["e_look_at_ray_list"] = timed(ray_route)
    rec["e_look_at_ray_list"]["slices"] = spp
    m = lambda k: rec[k]["median_ms"]  # noqa: E731
    rec["pose_cost_c_over_b"] = m("c_identity_pose") / m("b_builtin_no_tile_order")
    rec["gain_e_over_d"] = m("e_look_at_ray_list") / m("d_look_at_grid")
    rec["follow_up_c_over_a"] = m("c_identity_pose") / m("a_builtin_default")
    # the two routes render the same frame: sample sums in fp64, the grid's in sample order inside the kernel
    img = ray_route().reshape(H, W, 3)
    sc.trace_grid(W, H, spp, look, depth, out=out, nhit=nhit, counters=cnt)
    torch.cuda.synchronize()
    rec["max_abs_difference_d_e"] = float((out - img).abs().max().item())
    sc.close()
    print(json.dumps(rec))
    return rec


def main(path=os.path.join(ROOT, "profiles", "posed_camera_probe.json")):
    recs = [probe("c2_1920x1080_dof_spp1", scenes.scene_c2(), scenes.cam_dof(), 1920, 1080, 1),
            probe("c2_1920x1080_dof_spp64", scenes.scene_c2(), scenes.cam_dof(), 1920, 1080, 64),
            probe("dragon_1024_pinhole_spp4", scenes.scene_dragon(), scenes.cam_pinhole(), 1024, 1024, 4)]
    doc = dict(device=torch.cuda.get_device_name(0), method="device events around one frame each: 3 warm-ups, median of 7",
               configurations=recs)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:2])
