"""Per-vertex colours on meshes, shaded in torch from Scene.hit_attributes: the pyramid and the bunny in the room.

The library shades with one flat colour per mesh.  Here a nearest-hit query tells which object every ray hits, hit_attributes
adds the triangle (`prim`, in the order the triangles were given) and the point on it (`uv`), and the colour is interpolated in
torch from a per-vertex table: (1-u-v)*c_a + u*c_b + v*c_c.  Everything that is not a mesh takes the library's own
getSurfaceColor (`color`: the chessboard on the floor, the walls' flat colours):

    python examples/vertex_colors.py [out.png]

The camera is examples/lookat_camera.py's.  UV-mapped textures and smooth normals are the same gather with other tables.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes  # the test scenes: the room's planes, the pyramid and the bunny
from cgraytracing_amd.scene import TriangleMesh
from lookat_camera import lookat_rays


def vertex_colors(tri9):
    """[ntri, 3 vertices, 3] colours from the vertex positions: a vertex shared by several triangles gets one colour."""
    v = tri9.reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    return 0.1 + 0.9 * (v - lo) / (hi - lo)


def main(out="vertex_colors.png", W=640, H=360, spp=4):
    pyramid, bunny = scenes.pyramid_tris(1.0, (-9.0, -5.0, 24.0)), scenes.bunny_tris()
    objs = scenes.planes(scenes.chessboard_texture(False)) + [
        TriangleMesh.from_triangles(pyramid, (1.0, 1.0, 1.0)), TriangleMesh.from_triangles(bunny, (1.0, 1.0, 1.0))]
    meshes = {5: pyramid, 6: bunny}  # position in objs -> the triangles as given
    sc = cg.Scene(objs)
    dev = torch.device("cuda", sc.device)
    org, dirs = lookat_rays(eye=(14.0, 4.0, 2.0), target=(-3.0, -13.0, 32.0), up=(0.0, 1.0, 0.0), fov_deg=65, W=W, H=H, spp=spp,
                            device=dev)
    hit = sc.trace_rays(org, dirs, want=("hit",))
    attr = sc.hit_attributes(org, dirs, hit["hit_obj"], hit["hit_t"], want=("prim", "uv", "color"))
    rgb = attr["color"].clone()
    u, v = attr["uv"][:, 0:1], attr["uv"][:, 1:2]
    for obj, tri9 in meshes.items():
        table = torch.from_numpy(vertex_colors(tri9)).to(dev)  # [ntri, 3, 3]
        on = (hit["hit_obj"] == obj) & (attr["prim"] >= 0)
        c = table[attr["prim"][on].long()]
        rgb[on] = (1 - u[on] - v[on]) * c[:, 0] + u[on] * c[:, 1] + v[on] * c[:, 2]
    # a headlight: the cosine between the ray and the normal the query returned
    cos = (hit["hit_normal"] * dirs).sum(dim=1, keepdim=True).abs()
    image = (rgb * (0.25 + 0.75 * cos)).reshape(spp, H, W, 3).mean(dim=0)  # row 0 = bottom, like trace_grid
    torch.cuda.synchronize()
    n_mesh = int(sum(((hit["hit_obj"] == k) & (attr["prim"] >= 0)).sum().item() for k in meshes))
    sc.close()
    cg.write_png(out, cg.tonemap_rgb8(image.cpu().numpy()))
    print("%s: %dx%d, %d samples per pixel, %d of %d rays shaded from vertex colours" % (out, W, H, spp, n_mesh, len(org)))


if __name__ == "__main__":
    main(*sys.argv[1:2])
