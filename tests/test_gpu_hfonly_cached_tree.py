"""GPU: the light tiles' HFONLY launch on a scene that has a cached tree, against the CPU oracle.

The HFONLY variant of trace_grid_kernel walks height fields only; its launch reserves neither the node cache nor the wide
walk's stack (cgrt_wg_lds.h: wg_ask_trace), and its body must stage no nodes.  Before the layout was shared the body staged
the cached tree's nodes behind the object list whatever the variant, beyond what an HFONLY launch had asked for."""
import numpy as np
import pytest

import scenes
from backends import BackendScene
from test_gpu_object_counts import FORCE_REORDER, SEED, H, W, _eye_exact

pytestmark = pytest.mark.gpu

N_OBJS = 12


@pytest.fixture(scope="module")
def room(gpu_ready, orc):
    """The kind "C" room of test_gpu_object_counts.py (five planes with the opaque stone bump floor, a small pyramid, spheres up
    to a dozen objects) with the pyramid made of GLASS: an opaque mesh is walked in its 4-wide form and leaves no node array
    (cached_tree = -1, tests/native/commit_layout.cpp), a transparent one keeps its nodes, and a tree of at most 256 nodes is
    the scene's cached tree."""
    pyramid = scenes.TriangleMesh.from_triangles(scenes.pyramid_tris(0.6, (-6.0, -13.0, 36.0)), (0.6, 0.7, 0.9), 0.8, 0.5)
    objs = scenes.room_with_objects(N_OBJS, 300 + N_OBJS, mesh=pyramid, floor_tex=scenes.stone_small_texture(True))
    o = BackendScene(orc, objs)
    want = {name: o.trace_grid(cam, W, H, 4, 5, SEED) for name, cam in (("pinhole", scenes.cam_pinhole()), ("lens", scenes.cam_dof()))}
    o.close()
    return objs, want


@pytest.mark.parametrize("camera", ["pinhole", "lens"])
def test_hfonly_light_launch_beside_a_cached_tree(room, camera):
    """64x48, spp 4, scheduled: rays, per-pixel Hitpoint counts and the image equal the oracle's, bit for bit.

    How it is established that the HFONLY light launch runs here: the scene's traits on the host (scene_traits of
    cgrt_build.cpp, evaluated for a room with a glass pyramid and an opaque bump floor) are light_ok = light_trees =
    light_hf_only = 1 and cached_tree >= 0 -- every plane diffuse, the floor's tree a height field, the pyramid's nodes the
    cached tree --; a scheduled frame of a light_ok scene issues light_launch, which takes the HFONLY variant whenever
    light_hf_only is set (cgrt_hip.hip), over every tile, and the tiles away from the pyramid and the mirror and glass spheres
    are its to render.  The scheduled form itself is asserted below."""
    import cgraytracing_amd as cg
    objs, want = room
    cam = scenes.cam_pinhole() if camera == "pinhole" else scenes.cam_dof()
    with cg.Scene(objs) as sc:
        v = sc.kernel_variant(W, H, 4, cam, flags=FORCE_REORDER)
        assert v.startswith("trace_grid_sched_kernel<TREES=1,BEZ=0,") and "GLASS=1" in v, v
        got = sc.trace_grid_host(W, H, 4, cam, 5, SEED, force_reorder=True)
    assert np.isfinite(got["rgb"]).all()
    _eye_exact(got, want[camera], 4, "glass pyramid over the bump floor, %s" % camera)
