"""A wavefront tracer in torch over Scene.bounce: C2's spheres to depth 8, the glass tinted by the length of the path inside it.

The library's full trace (Scene.trace_rays) stops at depth 5 and knows the reference's materials only.  Scene.bounce is one
step of it for any rays: the nearest hit, then what trace() does there -- a Hitpoint's value f * adj, or the child rays with
their throughput.  The depth loop is the caller's, so between two levels it may do what the library cannot.  Here:

  * the children are compacted (absent children are rows of zeros) and each carries the index of its camera ray;
  * the loop runs to depth 8;
  * a ray that has crossed the glass hands its children exp(-sigma * t) of its throughput, per colour channel, t being the
    length of its segment inside the glass (Beer-Lambert): the refracted child leaves the glass with it, the reflected one
    turns back into the glass and will be attenuated again.  Whether a ray is inside is a flag the loop keeps: a refracted
    child changes sides, a reflected one does not;
  * the Hitpoint values of a camera ray are added in the order trace() emits them (depth first, the reflected subtree before
    the refracted one: the paths compared as bit strings behind their leading 1), so the sum does not depend on how the GPU
    scheduled anything.  With sigma = 0 and depth 5 it is trace_rays' sum bit for bit (check=True asserts that).

    python examples/wavefront_tinted_glass.py [out.png]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np
import torch

import cgraytracing_amd as cg
import scenes  # the test scenes: C2's walls, diffuse, mirror and glass spheres
from cgraytracing_amd import _capi

SIGMA = (0.10, 0.02, 0.06)  # absorption per unit length inside the glass: a green tint


def emission_sum(root, path, value, n):
    """Per camera ray the sum of its Hitpoints' values in trace()'s emission order (numpy, fp64, starting from 0)."""
    path = path.astype(np.int64)
    bits = np.zeros(len(path), np.int64)  # bits behind the leading 1
    for b in range(1, 32):
        bits += (path >> b) > 0
    order = np.lexsort(((path - (np.int64(1) << bits)) << (32 - bits), root))  # Hitpoints are leaves: no path prefixes another
    root, value = root[order], value[order]
    first = np.r_[True, root[1:] != root[:-1]] if len(root) else np.zeros(0, bool)
    starts = np.nonzero(first)[0]
    seq = np.arange(len(root)) - np.repeat(starts, np.diff(np.r_[starts, len(root)]))
    acc = np.zeros((n, 3))
    for k in range(int(seq.max()) + 1 if len(seq) else 0):
        sel = seq == k
        acc[root[sel]] += value[sel]
    return acc


def main(out="wavefront_tinted_glass.png", W=640, H=360, spp=2, depth=8, sigma=SIGMA, check=False):
    objs = scenes.scene_c2()
    sc = cg.Scene(objs)
    dev = torch.device("cuda", sc.device)
    sig = torch.tensor([sigma] * 3 if np.isscalar(sigma) else sigma, dtype=torch.float64, device=dev)
    org, dirs, keys = sc.camera_rays(W, H, spp, scenes.cam_dof(), 12345)
    n = org.shape[0]
    roots = (org, dirs, keys)
    root = torch.arange(n, device=dev)
    inside = torch.zeros(n, dtype=torch.bool, device=dev)
    adj = path = None
    hp_root, hp_path, hp_value, rays, tinted = [], [], [], [], 0
    for level in range(1, depth + 1):
        m = org.shape[0]
        res = sc.bounce(org, dirs, adj, path, keys, want=("step", "hit_t", "value", "children"))
        rays.append(int(res["counters"][_capi.CNT_RAYS].item()))
        hp = torch.nonzero(res["step"] == _capi.STEP_HITPOINT).flatten()
        hp_root.append(root[hp])
        hp_path.append(path[hp] if path is not None else torch.ones(hp.numel(), dtype=torch.int32, device=dev))
        hp_value.append(res["value"][hp])
        if level == depth:
            break
        # Beer-Lambert: both children of a ray that ran inside the glass (row i and row m + i)
        fade = torch.where(inside[:, None], torch.exp(-sig[None, :] * res["hit_t"][:, None]), torch.ones((m, 3), dtype=torch.float64, device=dev))
        child_adj = res["child_adj"] * torch.cat([fade, fade])
        child_inside = torch.cat([inside, ~inside])  # the reflected child stays on its side, the refracted one changes it
        keep = torch.nonzero(res["child_path"] != 0).flatten()
        tinted += int((inside[keep % m]).sum().item())
        org, dirs, adj, path, keys = (t[keep].contiguous() for t in (res["child_org"], res["child_dir"], child_adj, res["child_path"], res["child_keys"]))
        root, inside = torch.cat([root, root])[keep], child_inside[keep]
        if org.shape[0] == 0:
            break
    acc = emission_sum(torch.cat(hp_root).cpu().numpy(), torch.cat(hp_path).cpu().numpy(), torch.cat(hp_value).cpu().numpy(), n)
    info = dict(levels=len(rays), rays=rays, tinted=tinted, hitpoints=int(sum(t.numel() for t in hp_root)))
    if check:  # the seam costs nothing in bits: the same rays through the fused recursion
        full = sc.trace_rays(*roots, max_depth=depth, want=("acc",))["acc"].cpu().numpy()
        info["equals_trace_rays"] = bool(np.array_equal(acc, full))
        assert info["equals_trace_rays"], "the wavefront loop and trace_rays differ"
    variant = sc.bounce_variant()
    sc.close()
    image = acc.reshape(spp, H, W, 3).mean(axis=0)  # row 0 = bottom, like trace_grid
    cg.write_png(out, cg.tonemap_rgb8(image))
    print("%s: %dx%d, %d samples per pixel, rays per level %s, %d Hitpoints, %d children tinted (%s)" %
          (out, W, H, spp, rays, info["hitpoints"], tinted, variant))
    return info


if __name__ == "__main__":
    main(*sys.argv[1:2])
