"""Depth of field that converges: stochastic progressive photon mapping (Scene.sppm_session) of C2 under the thin lens.

A PpmSession keeps the Hitpoints of one fixed sample set, so more photons sharpen each Hitpoint's estimate and never the lens
blur.  Here every pass traces ONE fresh lens sample per pixel and a fresh photon batch, the statistics (N, R2, tau) belong to
the pixel, and the session's memory is one pass's Hitpoints plus the pixels whatever the number of passes:

    python examples/sppm_dof.py [out_prefix]

writes <out_prefix>_001.png, _008.png and _064.png -- the image after 1, 8 and 64 passes -- and prints the session's
device_bytes at each of them.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import cgraytracing_amd as cg
import scenes


def main(prefix="sppm_dof", W=480, H=270, passes=64, photons_per_pass=100000, checkpoints=(1, 8, 64)):
    """{passes: (rgb8 [H, W, 3] uint8 top row first, info dict)} at the checkpoints"""
    out = {}
    with cg.Scene(scenes.scene_c2()) as sc, sc.sppm_session(W, H, 1, scenes.cam_dof()) as ses:
        for k in range(1, passes + 1):
            ses.add_passes(1, photons_per_pass)
            if k in checkpoints:
                rgb8, info = ses.rgb8(), ses.info()
                out[k] = (rgb8, info)
                if prefix:
                    cg.write_png("%s_%03d.png" % (prefix, k), rgb8)
                print("%3d passes, %9d photons, %7d Hitpoints in the last pass, device_bytes %d" %
                      (k, info["photons_done"], info["hp_count"], info["device_bytes"]))
    return out


if __name__ == "__main__":
    main(*sys.argv[1:2])
