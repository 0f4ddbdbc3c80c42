"""GPU: the tile order of image-order launches (CGRT_GRID_NO_TILE_ORDER, tile_order_kernel).

An image-order launch over a scene of spheres and planes with reflecting or refracting spheres starts the tiles that may see
such a sphere first.  Only the workgroup that renders a tile changes, so every launch here is compared bit for bit -- rgb, nhit
and the counters -- with the same launch in row-major order (tile_order=False), and with the CPU oracle where the parity tests
compare this scene with it.  The order itself is read back (Scene.last_tile_order): a permutation of the tiles, classes
contiguous and ascending, row-major inside a class."""
import numpy as np
import pytest

import scenes
from backends import BackendScene, to_acc32
from cgraytracing_amd.scene import Sphere

pytestmark = pytest.mark.gpu

W0, H0 = 200, 117  # neither a multiple of 32 nor of 8


def _launch(sc, W, H, spp, cam, tile_order, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgb, nhit, _ = sc.trace_grid(W, H, spp, cam, 5, 12345, counters=cnt, tile_order=tile_order, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()


def _check_order(order, tiles_x, tiles_y):
    n = tiles_x * tiles_y
    plan, lst, cls = order["plan"], order["list"], order["cls"]
    assert len(lst) == n and np.array_equal(np.sort(lst), np.arange(n, dtype=np.uint32)), "not a permutation of the tiles"
    assert plan[0] == 0 and plan[4] == n and np.all(np.diff(plan.astype(np.int64)) >= 0)
    assert cls.max() <= 3
    for c in range(4):
        part = lst[plan[c]:plan[c + 1]]
        assert np.all(cls[part] == c), "class %d is not contiguous at its place" % c
        assert np.all(np.diff(part.astype(np.int64)) > 0), "class %d is not row-major" % c


def _both(objs, W, H, spp, cam, expect_order=True, **kw):
    """The launch with and without the order: identical bits; returns the ordered launch's results and its order."""
    import cgraytracing_amd as cg
    sc = cg.Scene(objs)
    try:
        assert "trace_grid_kernel<" in sc.kernel_variant(W, H, spp, cam, 5, rows=kw.get("rows"), stripe=kw.get("stripe"))  # not scheduled
        on = _launch(sc, W, H, spp, cam, True, **kw)
        order = sc.last_tile_order()
        off = _launch(sc, W, H, spp, cam, False, **kw)
        assert sc.last_tile_order() is None, "tile_order=False still ran the ordering kernel"
    finally:
        sc.close()
    for a, b, what in zip(on, off, ("rgb", "nhit", "counters")):
        assert np.array_equal(a, b), "%s differs between the ordered and the row-major launch" % what
    if expect_order:
        rows = kw.get("rows") or H
        assert order is not None, "the launch ran no ordering kernel"
        _check_order(order, (W + 31) // 32, (rows + 7) // 8)
    else:
        assert order is None, "a scene without reflecting or refracting spheres took the extra launch"
    return on, order


def _vs_oracle(orc, objs, cam, W, H, spp, got):
    rgb, nhit, cnt = got
    o = BackendScene(orc, objs)
    want = o.trace_grid(cam, W, H, spp, 5, 12345)
    o.close()
    assert int(cnt[0]) == want["nrays"]
    assert np.array_equal(nhit, want["nhit"])
    assert float(np.abs(rgb - to_acc32(want["acc_sum"], spp)).max()) <= 1e-6


@pytest.mark.parametrize("lens", ["pinhole", "thin_lens"])
@pytest.mark.parametrize("spp", [1, 64])
def test_c2_ordered_equals_row_major_and_oracle(gpu_ready, orc, lens, spp):
    cam = scenes.cam_pinhole() if lens == "pinhole" else scenes.cam_dof()
    objs = scenes.scene_c2()
    got, order = _both(objs, W0, H0, spp, cam)
    _vs_oracle(orc, objs, cam, W0, H0, spp, got)
    # the glass sphere (index 7) is seen: some tile has its centre on it, and the mirror's tiles follow the glass ones
    assert order["plan"][1] > 0 and order["plan"][2] > order["plan"][1] and order["plan"][3] > order["plan"][2]
    assert order["plan"][3] < order["plan"][4]


def test_c2_full_size_classes(gpu_ready):
    """The benchmark's frame, 8 100 tiles.  The two special spheres' discs cover about an eighth of it (radius 7 at 37 and 42
    units from the camera, the image plane 20 units wide at 10 units: discs of ~180 and ~160 pixels radius), so with the lens
    blur and the cone margins classes 0-2 stay below a quarter of the tiles."""
    _, order = _both(scenes.scene_c2(), 1920, 1080, 1, scenes.cam_dof())
    assert order["plan"][4] == 8100 and 0 < order["plan"][1] < order["plan"][3] < 8100 // 4


def test_striped_launch(gpu_ready):
    """Block-cyclic stripes, the last ones reaching beyond the image (rows beyond it are rendered as nothing)."""
    H = 117
    for rank in range(2):
        _both(scenes.scene_c2(), W0, H, 8, scenes.cam_dof(), rows=64, stripe=(16, rank, 2))
    _both(scenes.scene_c2(), W0, H, 8, scenes.cam_dof(), rows=40, row_offset=50)


def test_progressive_accumulate(gpu_ready):
    import torch
    import cgraytracing_amd as cg
    cam, spp_total, pass_spp = scenes.cam_dof(), 8, 2
    sc = cg.Scene(scenes.scene_c2())
    frames = []
    try:
        for tile_order in (True, False):
            out = torch.zeros((H0, W0, 3), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
            for k in range(spp_total // pass_spp):
                _, nhit, _ = sc.trace_grid(W0, H0, pass_spp, cam, 5, 12345, sample_offset=k * pass_spp, spp_total=spp_total, out=out,
                                           counters=cnt, accumulate=True, tile_order=tile_order)
            torch.cuda.synchronize()
            assert (sc.last_tile_order() is not None) == tile_order
            frames.append((out.cpu().numpy().copy(), nhit.cpu().numpy().copy(), cnt.cpu().numpy().copy()))
    finally:
        sc.close()
    for a, b in zip(*frames):
        assert np.array_equal(a, b)


def test_two_glass_spheres_one_behind_the_other(gpu_ready, orc):
    objs = scenes.wall_spheres() + [Sphere((-2.0, -8.0, 22), 5, (1.0, 1.0, 1.0), 0.8, 0.5),
                                    Sphere((1.0, -6.0, 45), 9, (0.9, 1.0, 0.9), 0.8, 0.5)]
    cam = scenes.cam_dof()
    got, order = _both(objs, W0, H0, 16, cam)
    _vs_oracle(orc, objs, cam, W0, H0, 16, got)
    assert order["plan"][1] > 0 and order["plan"][2] == order["plan"][3]  # no sphere that only reflects: class 2 is empty


def test_camera_inside_a_grown_bound(gpu_ready, orc):
    """The glass sphere reaches the lens plane (thin lens) or holds the camera (pinhole): every tile is doubtful."""
    for cam, centre, r in ((scenes.cam_dof(), (3.0, -2.0, -3.0), 7.0), (scenes.cam_pinhole(), (0.5, 0.5, -9.0), 3.0)):
        objs = scenes.wall_spheres() + [Sphere(centre, r, (1.0, 1.0, 1.0), 0.8, 0.5)]
        got, order = _both(objs, W0, H0, 4, cam)
        _vs_oracle(orc, objs, cam, W0, H0, 4, got)
        assert order["plan"][2] == order["plan"][4], "every tile may see the glass sphere: classes 0 and 1 hold them all"


def test_diffuse_only_scene_takes_no_extra_launch(gpu_ready):
    _both(scenes.scene_c1(), W0, H0, 8, scenes.cam_dof(), expect_order=False)


def test_row_major_launch_between_two_relayed_ones(gpu_ready):
    """One handle: a relayed, masked launch with class 3 inside the kernel, then a row-major launch, then the first again.  Every
    read-back of the row-major launch says "none", and the third launch reports what the first did -- from the order the buffer
    still holds, which the launch between them did not touch -- with the same bits."""
    import cgraytracing_amd as cg
    cam = scenes.cam_dof()
    sc = cg.Scene(scenes.scene_c2())

    def report():
        return dict(order=sc.last_tile_order(), masks=sc.last_sphere_masks(), reused=sc.last_tile_order_reused(),
                    relay=sc.last_sample_relay(), form=sc.last_relay_form(), diffuse=sc.last_diffuse_tiles(),
                    inkernel=sc.last_inkernel_diffuse_tiles())
    try:
        first, did = _launch(sc, W0, H0, 32, cam, True, sample_relay=True), report()
        _launch(sc, W0, H0, 4, cam, False)
        none = report()
        again, did_again = _launch(sc, W0, H0, 32, cam, True, sample_relay=True), report()
    finally:
        sc.close()
    _check_order(did["order"], 7, 15)
    assert did["masks"] is not None and len(did["masks"]) == 13 * 30
    assert did["relay"]["tiles"] == did["order"]["plan"][2] > 0 and did["relay"]["chunks"] == 2 and did["relay"]["parked_values"] > 0
    assert did["form"] == dict(mirror=False, order="chunks_first")
    assert did["diffuse"] == 0 and did["inkernel"] == did["order"]["plan"][4] - did["order"]["plan"][3] > 0
    assert not did["reused"]
    assert none == dict(order=None, masks=None, reused=False, relay=dict(tiles=0, chunks=0, parked_values=0), form=None, diffuse=0,
                        inkernel=0)
    assert did_again["reused"]
    for k in ("plan", "list", "cls"):
        assert np.array_equal(did_again["order"][k], did["order"][k])
    assert np.array_equal(did_again["masks"], did["masks"])
    assert all(did_again[k] == did[k] for k in ("relay", "form", "diffuse", "inkernel"))
    for a, b, what in zip(first, again, ("rgb", "nhit", "counters")):
        assert np.array_equal(a, b), "%s differs between the first launch and its repeat" % what
