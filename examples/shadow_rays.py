"""Direct lighting with shadow rays, shaded in torch from Scene.occluded: the glass bunny and a pyramid under a point light.

The library's own image comes from photon mapping.  Here a nearest-hit query tells what every camera ray sees, hit_attributes
gives the surface colour there, and one SHADOW RAY per hit asks whether anything opaque lies between the hit point and the
light -- Scene.occluded, an any-hit query: it stops at the first blocker instead of finding the nearest one.

    python examples/shadow_rays.py [out.png]

The shadow ray starts at the hit point, moved a little along the normal turned against the camera ray, points at the light
and ends there (tmax = the distance to the light).  skip_transparent=True: glass casts no shadow, so the bunny's is missing
and the pyramid's is not.  The camera is examples/lookat_camera.py's.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch

import cgraytracing_amd as cg
import scenes  # the test scenes: the room's planes, the pyramid and the bunny
from cgraytracing_amd.scene import TriangleMesh
from lookat_camera import lookat_rays

LIGHT = (0.0, 15.0, 20.0)


def main(out="shadow_rays.png", W=640, H=360, spp=4):
    objs = scenes.scene_c3(True) + [TriangleMesh.from_triangles(scenes.pyramid_tris(1.0, (-9.0, -5.0, 24.0)), (0.9, 0.6, 0.3))]
    sc = cg.Scene(objs)
    dev = torch.device("cuda", sc.device)
    org, dirs = lookat_rays(eye=(14.0, 4.0, 2.0), target=(-3.0, -13.0, 32.0), up=(0.0, 1.0, 0.0), fov_deg=65, W=W, H=H, spp=spp,
                            device=dev)
    hit = sc.trace_rays(org, dirs, want=("hit",))
    color = sc.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=("color",))["color"]
    seen = hit["hit_obj"] >= 0
    # the normal turned against the camera ray, the hit point moved off the surface along it
    n = hit["hit_normal"]
    n = torch.where((n * dirs).sum(dim=1, keepdim=True) > 0, -n, n)
    P = org + dirs * hit["hit_t"][:, None] + n * 1e-4
    to_light = torch.tensor(LIGHT, dtype=torch.float64, device=dev) - P
    dist = to_light.norm(dim=1)
    L = to_light / dist[:, None]
    L[~seen] = 0.0  # a direction of zero marks a ray that is not traced
    shadow = sc.occluded(P.contiguous(), L.contiguous(), tmax=dist.contiguous(), skip_transparent=True)
    lit = seen & (shadow["occluded"] == 0)
    lambert = (n * L).sum(dim=1).clamp(min=0.0) * lit
    image = (color * (0.08 + 0.92 * lambert[:, None])).reshape(spp, H, W, 3).mean(dim=0)  # row 0 = bottom, like trace_grid
    torch.cuda.synchronize()
    n_shadow, n_blocked = int(shadow["counters"][0].item()), int(shadow["occluded"].sum().item())
    variant = sc.occlusion_variant()
    sc.close()
    cg.write_png(out, cg.tonemap_rgb8(image.cpu().numpy()))
    print("%s: %dx%d, %d samples per pixel, %d shadow rays, %d blocked (%s)" % (out, W, H, spp, n_shadow, n_blocked, variant))
    return dict(shadow_rays=n_shadow, blocked=n_blocked)


if __name__ == "__main__":
    main(*sys.argv[1:2])
