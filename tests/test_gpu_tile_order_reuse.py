"""GPU: the tile order (and the sphere masks) kept across launches with the same inputs (cgrt_scene_last_tile_order_reused).

tile_order_kernel reads the camera, the frame geometry (width, height, rows, row offset, stripe) and the committed scene.  A
launch that finds the handle's buffer holding the result for exactly those runs no ordering kernel.  Every launch here equals
the same launch without any order (tile_order=False) bit for bit -- rgb, nhit, counters -- and the flag tells which way it went."""
import numpy as np
import pytest

import scenes
from cgraytracing_amd.scene import Camera, Sphere

pytestmark = pytest.mark.gpu

W, H, SPP = 200, 117, 4


def _launch(sc, cam, tile_order=True, W=W, H=H, seed=12345, stream=None, **kw):
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    if stream is None:
        rgb, nhit, _ = sc.trace_grid(W, H, SPP, cam, 5, seed, counters=cnt, tile_order=tile_order, **kw)
    else:
        with torch.cuda.stream(stream):
            rgb, nhit, _ = sc.trace_grid(W, H, SPP, cam, 5, seed, counters=cnt, tile_order=tile_order, **kw)
    reused = sc.last_tile_order_reused()
    torch.cuda.synchronize()
    return (rgb.cpu().numpy().copy(), nhit.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy()), reused


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "nhit", "counters")):
        assert np.array_equal(x, y), "%s: %s differs" % (what, name)


@pytest.fixture(scope="module")
def row_major(gpu_ready):
    """The launches without any order, on a handle of their own (they neither use nor disturb a stored order)."""
    import cgraytracing_amd as cg
    sc = cg.Scene(scenes.scene_c2())
    yield lambda cam, **kw: _launch(sc, cam, tile_order=False, **kw)[0]
    sc.close()


def test_same_view_reuses_the_order_and_another_view_does_not(gpu_ready, row_major):
    import cgraytracing_amd as cg
    a, b = scenes.cam_dof(), Camera(cam=(3.0, 2.0, -10.0), lens_radius=1.5)
    with cg.Scene(scenes.scene_c2()) as sc:
        flags = []
        for cam, kw in ((a, {}), (b, {}), (a, {}), (a, dict(seed=999, sample_offset=7, spp_total=64))):
            got, reused = _launch(sc, cam, **kw)
            flags.append(reused)
            assert sc.last_tile_order() is not None and sc.last_sphere_masks() is not None
            _same(got, row_major(cam, **kw), "camera %r %r" % (tuple(cam.cam), kw))
        assert flags == [False, False, False, True]
        # a launch without the order neither reuses nor forgets it
        _, reused = _launch(sc, a, tile_order=False)
        assert not reused
        assert _launch(sc, a)[1]
        # the masks are part of what is kept: without them the buffer's contents are another result
        got, reused = _launch(sc, a, sphere_masks=False)
        assert not reused and sc.last_sphere_masks() is None
        _same(got, row_major(a), "sphere_masks=False")
        got, reused = _launch(sc, a)
        assert not reused and sc.last_sphere_masks() is not None
        _same(got, row_major(a), "masks again")


def test_each_geometry_field_alone_misses(gpu_ready, row_major):
    import cgraytracing_amd as cg
    cam = scenes.cam_dof()
    base = dict(W=W, rows=56, stripe=(8, 0, 2))
    with cg.Scene(scenes.scene_c2()) as sc:
        assert not _launch(sc, cam, **base)[1]
        assert _launch(sc, cam, **base)[1]
        for change in (dict(W=W - 8), dict(rows=48), dict(stripe=(8, 1, 2))):
            kw = dict(base, **change)
            got, reused = _launch(sc, cam, **kw)
            assert not reused, change
            _same(got, row_major(cam, **kw), repr(change))
            got, reused = _launch(sc, cam, **kw)
            assert reused, change
            _same(got, row_major(cam, **kw), repr(change) + " again")
            assert not _launch(sc, cam, **base)[1]


def test_a_new_scene_does_not_see_the_old_list(gpu_ready):
    import cgraytracing_amd as cg
    cam = scenes.cam_dof()
    objs = scenes.scene_c2()
    with cg.Scene(objs) as sc:
        _launch(sc, cam)
        before = sc.last_tile_order()
    moved = objs[:7] + [Sphere((9.0, 8.0, 25), 7, (1.0, 1.0, 1.0), 0.8, 0.5)]  # the glass sphere, up and to the right
    with cg.Scene(moved) as sc, cg.Scene(moved) as ref:
        got, reused = _launch(sc, cam)
        assert not reused
        after = sc.last_tile_order()
        assert not np.array_equal(before["list"], after["list"])
        _same(got, _launch(ref, cam, tile_order=False)[0], "moved sphere")


def test_two_streams_with_the_same_key(gpu_ready, row_major):
    import torch
    import cgraytracing_amd as cg
    cam = scenes.cam_dof()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with cg.Scene(scenes.scene_c2()) as sc:
        first, r1 = _launch(sc, cam, stream=s1, W=1920, H=1080)
        # not synchronised in between: the second launch, on another stream, waits for the first one's ordering kernel
        cnt = [torch.zeros(8, dtype=torch.int64, device="cuda") for _ in range(2)]
        with torch.cuda.stream(s1):
            a = sc.trace_grid(W, H, SPP, cam, 5, 12345, counters=cnt[0])
            ra = sc.last_tile_order_reused()
        with torch.cuda.stream(s2):
            b = sc.trace_grid(W, H, SPP, cam, 5, 12345, counters=cnt[1])
            rb = sc.last_tile_order_reused()
        torch.cuda.synchronize()
        assert (r1, ra, rb) == (False, False, True)
        want = row_major(cam)
        for (rgb, nhit, _), c in ((a, cnt[0]), (b, cnt[1])):
            _same((rgb.cpu().numpy(), nhit.cpu().numpy().view(np.uint32), c.cpu().numpy()), want, "two streams")
