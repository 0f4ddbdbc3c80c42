"""GPU: lens points staged ahead of the sample loop (CGRT_GRID_NO_LENS_STAGE, lens_stage=False; cgrt_lens_stage.h).

The thin-lens terminal-diffuse body inside the main launch finds the accepted lens draws of a wave's next 16 samples ahead of
their use -- attempt 1 of every sample without divergence, then the rejected ones, every lane on its own (sample, attempt)
stream -- and keeps them in LDS, instead of one rejection loop per sample at the pace of the wave's unluckiest lane.  Attempt j
of sample s is a pure function of (pixel, s, j), so the points are the same bits: every launch here runs staged and with
lens_stage=False on one handle and is compared bit for bit -- rgb, per-pixel nhit and every counter -- and the read-back names
the form that ran.  The scene is C2."""
import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32

pytestmark = pytest.mark.gpu

SEED = 12345
NONE = dict(lds_tiles=0, area_tiles=0)


def _launch(sc, W, H, spp, cam, stage, stream=None, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, 5, SEED, counters=cnt, lens_stage=stage, stream=stream, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "nhit", "counters")):
        assert np.array_equal(x, y), "%s: %s differs between staged and per-sample lens points" % (what, name)


def _both(sc, W, H, spp, cam, staged=True, **kw):
    """The launch staged and unstaged; staged: whether the first is expected to stage (its class-3 tiles, all of them)."""
    what = "%dx%d spp %d %r" % (W, H, spp, kw)
    on = _launch(sc, W, H, spp, cam, True, **kw)
    did, class3 = sc.last_lens_stage(), sc.last_inkernel_diffuse_tiles()
    if staged:
        assert class3 > 0, what + ": no tile took the terminal-diffuse body inside the launch"
        assert did == dict(lds_tiles=class3, area_tiles=0), (what, did, class3)
    else:
        assert did == NONE, (what, did)
    off = _launch(sc, W, H, spp, cam, False, **kw)
    assert sc.last_lens_stage() == NONE, what
    _same(on, off, what)
    return on


@pytest.fixture(scope="module")
def c2(gpu_ready):
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield sc
    sc.close()


@pytest.mark.parametrize("spp", [1, 5, 16, 17, 33, 64])
def test_sample_counts_around_the_batch(c2, orc, spp):
    got = _both(c2, 96, 54, spp, scenes.cam_dof())
    if spp in (5, 17):
        o = BackendScene(orc, scenes.scene_c2())
        want = o.trace_grid(scenes.cam_dof(), 96, 54, spp, 5, SEED)
        o.close()
        assert int(got[2][0]) == want["nrays"] and np.array_equal(got[1], want["nhit"])
        assert float(np.abs(got[0] - to_acc32(want["acc_sum"], spp)).max()) <= 1e-6


@pytest.mark.parametrize("spp,relay", [(32, True), (33, True), (64, True), (64, 4)])
def test_beside_the_sample_relay(c2, spp, relay):
    """The relayed tiles' chunk workgroups, the parking body included, run beside the staging class-3 workgroups."""
    _both(c2, 96, 54, spp, scenes.cam_dof(), sample_relay=relay)
    assert c2.last_sample_relay()["chunks"] == (4 if relay == 4 else 2)
    _both(c2, 96, 54, spp, scenes.cam_dof(), sample_relay=relay, relay_mirror=True, relay_order="interleaved")


def test_sample_offset_partial_tiles_and_stripes(c2):
    _both(c2, 96, 54, 20, scenes.cam_dof(), sample_offset=3, spp_total=64)
    _both(c2, 200, 52, 17, scenes.cam_dof())                               # partial tiles: lanes that are not live
    _both(c2, 200, 117, 18, scenes.cam_dof(), rows=56, stripe=(8, 1, 2))   # rows beyond the image


def test_nothing_is_staged_without_a_lens_or_in_the_second_launch(c2):
    _both(c2, 96, 54, 17, scenes.cam_pinhole(), staged=False)
    for spp in (5, 17, 64):
        _both(c2, 96, 54, spp, scenes.cam_dof(), staged=False, diffuse_tiles=True)  # the two-launch form draws sample by sample
        assert c2.last_diffuse_tiles() > 0
    _both(c2, 96, 54, 17, scenes.cam_dof(), staged=False, sphere_pairs=False)       # the full body renders class 3
    _both(c2, 96, 54, 17, scenes.cam_dof(), staged=False, tile_order=False)


def test_two_streams_on_one_handle(c2):
    import torch
    cam = scenes.cam_dof()
    want = _launch(c2, 96, 54, 33, cam, False)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for st in (s1, s2):
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        st.wait_stream(torch.cuda.current_stream())
        rgb, nhit, _ = c2.trace_grid(96, 54, 33, cam, 5, SEED, counters=cnt, stream=st.cuda_stream)
        outs.append((rgb, nhit, cnt))
    torch.cuda.synchronize()
    assert c2.last_lens_stage()["lds_tiles"] > 0
    for k, (rgb, nhit, cnt) in enumerate(outs):
        _same((rgb.cpu().numpy(), nhit.cpu().numpy().view(np.uint32), cnt.cpu().numpy()), want, "stream %d" % k)
