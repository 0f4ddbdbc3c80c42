"""Two lights the library does not know: a spot light and a coloured point light, over PpmSession.add_photon_rays.

The photon mapper's own emitter is the reference's single ceiling lamp (a jittered point light, white, uniform over the sphere).
Here the photons are made in torch instead -- a cone pointing down from the ceiling and a blue point light near the floor --
and handed to the session of examples/lookat_ppm.py's look-at camera, which traces them like its own:

    python examples/spot_light_ppm.py [out.png]

A photon is an origin, a unit direction and a flux; past its start it bounces as the reference's photons do.  An area light, a
light in a fixture or an importance-sampled emitter differs only in the few lines that make `org`, `dirs` and `flux`.
"""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch

import cgraytracing_amd as cg
import scenes
from lookat_camera import lookat_rays

# power: what a point light sending these photons over the whole sphere would have; the cone packs it into 0.59 sr
SPOT = dict(pos=(0.0, 15.0, 28.0), half_angle_deg=25.0, power=60.0, colour=(1.0, 1.0, 1.0))   # a cone about -y
POINT = dict(pos=(-14.0, -10.0, 10.0), power=25.0, colour=(0.25, 0.45, 1.0))                  # uniform over the sphere


def eye_rays(W, H, spp, device):
    """the look-at camera of lookat_ppm.py"""
    return lookat_rays(eye=(17.0, 8.0, 2.0), target=(-2.0, -13.0, 30.0), up=(0.0, 1.0, 0.0), fov_deg=70, W=W, H=H, spp=spp,
                       device=device)


def two_light_photons(n, device, seed=3):
    """n photons, the two lights interleaved (even indices: the spot, odd: the point light), as (org, dirs, flux) float64 [n,3].

    The final gather divides every Hitpoint's flux by ALL n photons of the session (main.cpp:256), whichever light sent them.  A
    light that sends n_i of the n photons therefore gives each of them the flux power_i * 4 PI * (n / n_i): the reference's
    power * 4 PI (main.cpp:246) for a light that has the session to itself, scaled up by the share of the photons it does not
    get.  Interleaving keeps both lights' contributions growing together when the photons arrive in several calls."""
    f64 = dict(dtype=torch.float64, device=device)
    g = torch.Generator(device=device).manual_seed(seed)
    u = torch.rand((n, 2), generator=g, **f64)
    is_spot = torch.arange(n, device=device) % 2 == 0
    # cos(theta) uniform in [cos(half angle), 1] is uniform over the cone's cap; in [-1, 1] over the whole sphere
    lo = torch.where(is_spot, torch.tensor(math.cos(math.radians(SPOT["half_angle_deg"])), **f64), torch.tensor(-1.0, **f64))
    cos_t = lo + (1 - lo) * u[:, 0]
    sin_t = torch.sqrt(1 - cos_t * cos_t)
    phi = 2 * math.pi * u[:, 1]
    dirs = torch.stack([sin_t * torch.cos(phi), -cos_t, sin_t * torch.sin(phi)], dim=1)  # the cone's axis is -y
    dirs = torch.nn.functional.normalize(dirs, dim=1).contiguous()
    org = torch.where(is_spot[:, None], torch.tensor(SPOT["pos"], **f64), torch.tensor(POINT["pos"], **f64)).contiguous()
    n_spot = int(is_spot.sum().item())
    w_spot = SPOT["power"] * 4 * math.pi * (n / max(n_spot, 1))
    w_point = POINT["power"] * 4 * math.pi * (n / max(n - n_spot, 1))
    flux = torch.where(is_spot[:, None], w_spot * torch.tensor(SPOT["colour"], **f64),
                       w_point * torch.tensor(POINT["colour"], **f64)).contiguous()
    return org, dirs, flux


def render(W=320, H=180, spp=2, photons=400000, steps=4):
    """(rgb8 [H, W, 3] uint8, top row first; info dict of the session)"""
    with cg.Scene(scenes.scene_c2()) as sc:
        dev = torch.device("cuda", sc.device)
        org, dirs = eye_rays(W, H, spp, dev)
        p_org, p_dirs, p_flux = two_light_photons(photons, dev)
        with sc.ppm_session_rays(org, dirs, width=W, rows=H, spp=spp) as ses:
            step = (photons + steps - 1) // steps
            for a in range(0, photons, step):  # ses.rgb8() after any step is a preview: it is normalised by the photons so far
                ses.add_photon_rays(p_org[a:a + step], p_dirs[a:a + step], p_flux[a:a + step])
            return ses.rgb8(), ses.info()


def main(out="spot_light_ppm.png", **kw):
    rgb8, info = render(**kw)
    cg.write_png(out, rgb8)
    print("%s: %dx%d, %d Hitpoints, %d photons" % (out, rgb8.shape[1], rgb8.shape[0], info["hp_count"], info["photons_done"]))
    return rgb8


if __name__ == "__main__":
    main(*sys.argv[1:2])
