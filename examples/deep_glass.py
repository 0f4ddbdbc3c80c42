"""C2's glass sphere past depth 5: Scene.wavefront traces camera rays to any depth inside the library.

The full trace (Scene.trace_rays) keeps a fixed stack of pending rays and stops at depth 5; a glass sphere's ray tree does not.
Scene.wavefront runs the depth loop over the bounce step on the device -- ray queues in device memory, the Hitpoints parked
with their place in the tree and summed in trace()'s emission order -- up to depth 31.  This example renders the C2 frame at
depth 5 (bit for bit trace_rays' image; check=True asserts it) and at depth 12, writes both PNGs and the difference image
(scaled by 8: what the rays beyond depth 5 add), and prints the rays per level.

    python examples/deep_glass.py [prefix]      ->  prefix_depth5.png, prefix_depth12.png, prefix_diff.png
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes  # the test scenes: C2's walls, diffuse, mirror and glass spheres


def main(prefix="deep_glass", W=640, H=360, spp=2, depths=(5, 12), check=False):
    sc = cg.Scene(scenes.scene_c2())
    org, dirs, keys = sc.camera_rays(W, H, spp, scenes.cam_dof(), 12345)
    info, images = dict(variant=sc.wavefront_variant()), {}
    for depth in depths:
        res = sc.wavefront(org, dirs, keys, max_depth=depth, want=("acc", "nhit"))
        acc = res["acc"].cpu().numpy()
        images[depth] = acc.reshape(spp, H, W, 3).mean(axis=0)  # row 0 = bottom, like trace_grid
        info[depth] = dict(rays=res["rays_per_level"], levels=res["levels"], hitpoints=res["hp_count"], slices=res["slices"])
        if check and depth <= 5:  # the same rays through the fused recursion
            full = sc.trace_rays(org, dirs, keys, max_depth=depth, want=("acc", "nhit"))
            torch.cuda.synchronize()
            info[depth]["equals_trace_rays"] = bool(torch.equal(res["acc"], full["acc"]) and torch.equal(res["nhit"], full["nhit"]))
            assert info[depth]["equals_trace_rays"], "Scene.wavefront and trace_rays differ"
        cg.write_png("%s_depth%d.png" % (prefix, depth), cg.tonemap_rgb8(images[depth]))
        print("depth %2d: rays per level %s, %d Hitpoints, %d slice(s)" % (depth, res["rays_per_level"], res["hp_count"], res["slices"]))
    sc.close()
    lo, hi = min(depths), max(depths)
    diff = np.abs(images[hi] - images[lo])
    info["max_diff"] = float(diff.max())
    cg.write_png("%s_diff.png" % prefix, cg.tonemap_rgb8(np.minimum(diff * 8.0, 1.0)))
    print("%s_*.png: %dx%d, %d samples per pixel, depth %d against %d: largest difference %.4g (%s)" %
          (prefix, W, H, spp, hi, lo, info["max_diff"], info["variant"]))
    return info


if __name__ == "__main__":
    main(*sys.argv[1:2])
