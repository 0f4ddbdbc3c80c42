"""A mesh that moves between frames: the dragon twisted about its vertical axis, refitted on the device.

The scene is committed ONCE.  Every frame makes the new vertices in torch on the GPU, hands them to Scene.refit_mesh -- the
hierarchy keeps its topology, its boxes, the triangle records and the mesh's bounding and cover spheres are recomputed by
kernels on the same stream, with no copy through the host -- and renders through trace_grid:

    python examples/deforming_mesh.py OUT [frames] [mesh] [--rebuild-at RATIO]

writes OUT_00.png, OUT_01.png, ... (mesh: dragon or bunny).  Destroying, adding and committing the scene per frame would give
the same pictures and cost the build every time (README, "Refit").

--rebuild-at RATIO (off by default): after each refit the hierarchy's surface-area cost (Scene.mesh_cost) is compared with its
value after the last build; once it exceeds RATIO times that, the mesh is rebuilt in place (Scene.rebuild_mesh) for the pose.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes  # the test scenes' meshes: the reference's dragon and low-poly bunny


def twist(tris, turns):
    """tris [n,9] on the device: every vertex turned about the vertical axis through the mesh's centre by an angle that grows
    with its height, `turns` radians from the lowest vertex to the highest."""
    p = tris.reshape(-1, 3)
    lo, hi = p.min(0).values, p.max(0).values
    c = 0.5 * (lo + hi)
    a = turns * (p[:, 1] - lo[1]) / (hi[1] - lo[1])
    x, z = p[:, 0] - c[0], p[:, 2] - c[2]
    q = torch.stack([c[0] + torch.cos(a) * x + torch.sin(a) * z, p[:, 1], c[2] - torch.sin(a) * x + torch.cos(a) * z], 1)
    return q.reshape(-1, 9).contiguous()


def main(out="deforming", frames=6, mesh="dragon", W=512, H=384, spp=8, rebuild_at=None):
    frames = int(frames)
    if mesh == "dragon":
        tris, colour, kind = scenes.dragon_tris(), (0.25, 0.25, 0.5), 1
    else:
        tris, colour, kind = scenes.bunny_tris(), (0.9, 0.9, 0.9), 0
    objs = scenes.planes() + [scenes.TriangleMesh.from_triangles(tris, colour, 0.0, 0.0, kind)]
    obj = len(objs) - 1
    sc = cg.Scene(objs, build="device")
    rest = torch.as_tensor(np.ascontiguousarray(tris), device=torch.device("cuda", sc.device))
    cam = scenes.cam_dof()
    total = lambda c: c["node_cost"] + c["tri_cost"]
    built = total(sc.mesh_cost(obj)) if rebuild_at else 0.0
    for f in range(frames):
        pose = twist(rest, 2.5 * np.sin(2 * np.pi * f / max(frames, 1)))
        sc.refit_mesh(obj, pose)  # asynchronous on torch's current stream, as is the frame behind it
        if rebuild_at:
            cost = total(sc.mesh_cost(obj))
            if cost > rebuild_at * built:
                sc.rebuild_mesh(obj, pose)  # synchronises the stream
                built = total(sc.mesh_cost(obj))
                print("frame %d: cost %.1f after the refit, rebuilt: %.1f" % (f, cost, built))
        image, _, _ = sc.trace_grid(W, H, spp, cam, 5, 12345)
        path = "%s_%02d.png" % (out, f)
        cg.write_png(path, cg.tonemap_rgb8(image.double().cpu().numpy()))  # (.cpu() waits for the stream: `pose` may go now)
        print(path)
    inf = sc.refit_info(obj)
    print("%d refits of %d triangles (%d wide nodes); the plan took %.2f ms, once" % (inf["refits"], inf["ntris"], inf["nwide"], inf["ms_plan"]))
    if rebuild_at:
        print("%d rebuilds at cost ratio %.2f" % (sc.rebuild_info(obj)["rebuilds"], rebuild_at))
    sc.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    ratio = None
    if "--rebuild-at" in args:
        at = args.index("--rebuild-at")
        ratio = float(args[at + 1])
        del args[at:at + 2]
    main(*args[:3], rebuild_at=ratio)
