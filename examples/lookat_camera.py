"""A look-at camera over Scene.trace_rays: the C2 room seen from the side.

The library's own camera looks along +z from a point in front of the image plane z = 0.  Here the rays are built in torch from
eye / target / up / field of view, traced as a ray list, and the per-ray sums reshaped into an image:

    python examples/lookat_camera.py [out.png]

A turntable, a fisheye or a cube-map face differs only in the few lines that make `dirs`.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes  # the test scenes: C2 = a room of wall spheres with a diffuse, a mirror and a glass sphere


def lookat_rays(eye, target, up, fov_deg, W, H, spp, device, seed=1):
    """[spp*H*W, 3] origins and unit directions of a pinhole camera at `eye` looking at `target`; row 0 is the bottom row, as in
    trace_grid's images.  Each sample is jittered inside its pixel."""
    f64 = dict(dtype=torch.float64, device=device)
    eye, target, up = (torch.tensor(v, **f64) for v in (eye, target, up))
    fwd = torch.nn.functional.normalize(target - eye, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(up, fwd), dim=0)
    upv = torch.linalg.cross(fwd, right)
    g = torch.Generator(device=device).manual_seed(seed)
    jit = torch.rand((spp, H, W, 2), generator=g, **f64)
    x = (torch.arange(W, **f64)[None, None, :] + jit[..., 0]) / W * 2 - 1
    y = (torch.arange(H, **f64)[None, :, None] + jit[..., 1]) / H * 2 - 1
    t = float(np.tan(np.radians(fov_deg) / 2))
    d = fwd + x[..., None] * (t * right) + y[..., None] * (t * H / W * upv)
    dirs = torch.nn.functional.normalize(d, dim=-1).reshape(-1, 3).contiguous()
    return eye.expand_as(dirs).contiguous(), dirs


def main(out="lookat.png", W=640, H=360, spp=16):
    sc = cg.Scene(scenes.scene_c2())
    dev = torch.device("cuda", sc.device)
    org, dirs = lookat_rays(eye=(17.0, 8.0, 2.0), target=(-2.0, -13.0, 30.0), up=(0.0, 1.0, 0.0), fov_deg=70, W=W, H=H, spp=spp,
                            device=dev)
    res = sc.trace_rays(org, dirs, want=("acc",))
    image = res["acc"].reshape(spp, H, W, 3).mean(dim=0)  # row 0 = bottom, like trace_grid
    torch.cuda.synchronize()
    rays = int(res["counters"][0].item())
    sc.close()
    cg.write_png(out, cg.tonemap_rgb8(image.cpu().numpy()))
    print("%s: %dx%d, %d samples per pixel, %d rays traced" % (out, W, H, spp, rays))


if __name__ == "__main__":
    main(*sys.argv[1:2])
