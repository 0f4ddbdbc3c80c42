"""C2's glass sphere photon-mapped past eye depth 5: Scene.ppm_session_wavefront starts a photon-mapping session from the
Hitpoint records of a wavefront trace of any depth.

A grid or ray session (Scene.ppm_session, Scene.ppm_session_rays) gets its Hitpoints from the library's full trace, which stops
at depth 5; a glass sphere's ray tree does not.  Scene.wavefront traces the camera rays to depth 12 and returns every Hitpoint
with its ray and its place in the ray's tree; Scene.ppm_session_hitpoints builds the photon pass's table from those records.
This example photon-maps the C2 frame at eye depth 5 (bit for bit Scene.ppm_session_rays' image; check=True asserts it) and at
eye depth 12 with the same photons, writes both PNGs and the difference image (scaled by 8: the light that the Hitpoints beyond
depth 5 gather), and prints the Hitpoint counts.

    python examples/deep_glass_ppm.py [prefix]      ->  prefix_depth5.png, prefix_depth12.png, prefix_diff.png
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import numpy as np

import cgraytracing_amd as cg
import scenes  # the test scenes: C2's walls, diffuse, mirror and glass spheres


def main(prefix="deep_glass_ppm", W=640, H=360, spp=2, photons=2000000, depths=(5, 12), check=False):
    sc = cg.Scene(scenes.scene_c2())
    org, dirs, keys = sc.camera_rays(W, H, spp, scenes.cam_dof(), 12345)
    info, images = {}, {}
    for depth in depths:
        ses, wf = sc.ppm_session_wavefront(org, dirs, keys, width=W, rows=H, spp=spp, eye_depth=depth, nphotons=photons)
        with ses:
            images[depth] = ses.image()  # row 0 = bottom
            rgb8 = ses.rgb8()
            inf = ses.info()
            most = int(ses.hitpoints()[:, 1].max()) + 1 if inf["hp_count"] else 0  # column 1: the rank within the ray
        info[depth] = dict(hitpoints=inf["hp_count"], most_per_ray=most, levels=wf["levels"], events=inf["n_events"], ms_table=inf["ms_table"])
        if check and depth <= 5:  # the same rays through the library's own eye stage
            with sc.ppm_session_rays(org, dirs, keys, width=W, rows=H, spp=spp, max_depth=depth, nphotons=photons) as ref:
                info[depth]["equals_ray_session"] = bool(np.array_equal(ref.image(), images[depth]) and np.array_equal(ref.rgb8(), rgb8))
            assert info[depth]["equals_ray_session"], "the hitpoint session and ppm_session_rays differ"
        cg.write_png("%s_depth%d.png" % (prefix, depth), rgb8)
        print("eye depth %2d: %d Hitpoints (at most %d on one ray, %d levels), %d photon hits" %
              (depth, inf["hp_count"], most, wf["levels"], inf["n_events"]))
    sc.close()
    lo, hi = min(depths), max(depths)
    diff = np.abs(images[hi] - images[lo])
    info["max_diff"] = float(diff.max())
    cg.write_png("%s_diff.png" % prefix, cg.tonemap_rgb8(np.minimum(diff * 8.0, 1.0)))
    print("%s_*.png: %dx%d, %d samples per pixel, %d photons, eye depth %d against %d: largest difference %.4g" %
          (prefix, W, H, spp, photons, hi, lo, info["max_diff"]))
    return info


if __name__ == "__main__":
    main(*sys.argv[1:2])
