"""The look-at camera of lookat_camera.py, photon-mapped: Scene.ppm_session_rays.

lookat_camera.py traces a side view of the C2 room and shows the eye pass's sums (the un-lit f * adj).  Here the same rays open a
photon-mapping session: their Hitpoints go into the hash table, photons from the ceiling light are added in a few steps, and
the gathered, tone-mapped image is written as a PNG:

    python examples/lookat_ppm.py [out.png]

Ray i = sample * (W * H) + texel belongs to texel i % (W * H), which is what ppm_session_rays assumes without a `pixel` tensor.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch

import cgraytracing_amd as cg
import scenes
from lookat_camera import lookat_rays


def render(W=320, H=180, spp=2, steps=4, photons_per_step=50000):
    """(rgb8 [H, W, 3] uint8, top row first; info dict of the session)"""
    with cg.Scene(scenes.scene_c2()) as sc:
        dev = torch.device("cuda", sc.device)
        org, dirs = lookat_rays(eye=(17.0, 8.0, 2.0), target=(-2.0, -13.0, 30.0), up=(0.0, 1.0, 0.0), fov_deg=70, W=W, H=H, spp=spp,
                                device=dev)
        with sc.ppm_session_rays(org, dirs, width=W, rows=H, spp=spp) as ses:
            for _ in range(steps):
                ses.add_photons(photons_per_step)  # ses.rgb8() after any step is a preview
            return ses.rgb8(), ses.info()


def main(out="lookat_ppm.png", **kw):
    rgb8, info = render(**kw)
    cg.write_png(out, rgb8)
    print("%s: %dx%d, %d Hitpoints, %d photons" % (out, rgb8.shape[1], rgb8.shape[0], info["hp_count"], info["photons_done"]))
    return rgb8


if __name__ == "__main__":
    main(*sys.argv[1:2])
