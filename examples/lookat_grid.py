"""The view of examples/lookat_camera.py through the grid kernels: the C2 room seen from the side with a posed camera.

    python examples/lookat_grid.py [out.png]

Camera.look_at places the camera's frame in the world and Scene.trace_grid starts its primary rays from it (CGRT_GRID_POSED): no
ray buffer, the grid kernels' per-pixel fp64 sum in the reference's order, and everything else a grid launch can do -- here 64
thin-lens samples per pixel in one launch, then the same view continued as a photon-mapping session, whose image is written.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch

import cgraytracing_amd as cg
import scenes  # the test scenes: C2 = a room of wall spheres with a diffuse, a mirror and a glass sphere

EYE, TARGET, FOV = (17.0, 8.0, 2.0), (-2.0, -13.0, 30.0), 70.0


def main(out="lookat_grid.png", W=1920, H=1080, spp=64, ppm_spp=1, photons=200000):
    """Returns (the eye pass's image [H, W, 3] float32, the session's image [H, W, 3] float64, its rgb8 as written)."""
    # sharp where the view's centre ray meets the glass sphere's neighbourhood; a lens a third of the built-in camera's
    cam = cg.Camera.look_at(EYE, TARGET, up=(0.0, 1.0, 0.0), fov_x_deg=FOV, focus_distance=30.0, lens_radius=0.5)
    with cg.Scene(scenes.scene_c2()) as sc:
        rgb, nhit, cnt = sc.trace_grid(W, H, spp, cam)
        torch.cuda.synchronize()
        eye_image = rgb.cpu().numpy()
        rays = int(cnt[0].item())
        variant = sc.kernel_variant(W, H, spp, cam)
        # the same view as a progressive photon-mapping render: the grid's Hitpoint capture, photons added in two steps
        with sc.ppm_session(W, H, ppm_spp, cam) as ses:
            ses.add_photons(photons // 2)
            ses.add_photons(photons - photons // 2)
            image, rgb8 = ses.image(), ses.rgb8()
    cg.write_png(out, rgb8)
    print("%s: %dx%d, %d samples per pixel, %d rays traced by %s; photon map: %d photons" % (out, W, H, spp, rays, variant, photons))
    return eye_image, image, rgb8


if __name__ == "__main__":
    main(*sys.argv[1:2])
