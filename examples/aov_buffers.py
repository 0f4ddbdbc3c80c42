"""A frame's feature buffers: C2 under the thin lens as albedo, normal and depth images, from one launch.

What a denoiser takes as guides, a compositor as mattes and a picker as its answer -- per pixel the first hit's surface colour,
its normal turned against the ray, its distance, how many samples hit and which object the first sample hit -- comes from
Scene.trace_grid_aov: the camera's rays are made and traced in registers, one pixel a lane, and only the five frame buffers
reach memory.

    python examples/aov_buffers.py [prefix]        # writes prefix_albedo.png, prefix_normal.png, prefix_depth.png

The normal image is 0.5 + 0.5 n of the averaged normal; the depth image is near / mean hit depth (white = near), the mean
taken over the samples that hit: depth * spp / hits.  The mirror and the glass sphere show their own white albedo -- AOVs
"behind" a reflection or refraction are not made.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes  # the test scenes: C2 = five wall spheres, a diffuse, a mirror and a glass sphere


def main(prefix="aov", W=960, H=540, spp=16):
    sc = cg.Scene(scenes.scene_c2())
    cam = scenes.cam_dof()
    res = sc.trace_grid_aov(W, H, spp, cam)
    torch.cuda.synchronize()
    variant = sc.aov_variant(W, H, cam)
    sc.close()
    albedo, normal, depth = (res[k].cpu().numpy().astype(np.float64) for k in ("albedo", "normal", "depth"))
    hits, obj_id = res["hits"].cpu().numpy(), res["obj_id"].cpu().numpy()
    mean_depth = depth * spp / np.maximum(hits, 1)
    near = float(mean_depth[hits > 0].min())
    shade = np.where(hits > 0, near / np.maximum(mean_depth, near), 0.0)
    # (tonemap_rgb8 applies the reference's gamma and flips the rows: row 0 of a frame is its bottom row)
    cg.write_png(prefix + "_albedo.png", cg.tonemap_rgb8(albedo))
    cg.write_png(prefix + "_normal.png", cg.tonemap_rgb8(0.5 + 0.5 * normal))
    cg.write_png(prefix + "_depth.png", cg.tonemap_rgb8(np.repeat(shade[..., None], 3, axis=2)))
    seen = sorted(int(i) for i in np.unique(obj_id))
    print("%s_{albedo,normal,depth}.png: %dx%d, %d samples per pixel, %d rays, objects first seen %s, coverage %.4f (%s)" %
          (prefix, W, H, spp, int(res["counters"][0].item()), seen, float(hits.sum()) / (spp * W * H), variant))
    return dict(rays=int(res["counters"][0].item()), objects=seen)


if __name__ == "__main__":
    main(*sys.argv[1:2])
