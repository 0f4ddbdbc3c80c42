"""The ray-list kernels' draw from the block queue at its edges (RayBlocks, csrc/cgrt_ray_wave.hpp; occlusion's lane-k form).

A wave draws blocks of 64 consecutive rays; a lane without a ray takes the next ray of the wave's block, lanes that drew beyond
the block's end draw again, rays with dir = 0 are answered where they are drawn.  Nothing of a ray's result may depend on where
in the list it stands or on what its neighbours are.  So the kernel is compared with itself under another draw: a list padded
with dir = 0 rows against the compacted list of its real rays, bit for bit, for trace_rays (full trace and nearest-hit query),
occluded, bounce and wavefront.  Keys are always explicit, so a ray's result does not depend on its index.

n is the number of rows of patterns (a) and (b), and the number of real rays of pattern (c):
  (a) all n rays real;
  (b) every third of the n rows has dir = 0, so lanes draw past a block's end and draw again;
  (c) 64 consecutive dir = 0 rows, aligned to a block, among n real rays -- a block with nothing traceable, the `continue` path.
      Behind the last real ray where n is a multiple of 64 (the wave's last block is the empty one: the drained() exit), else
      as block n // 128 (the list's first block for n < 128).
CGRT_CNT_RAYS counts scene walks: it is the number of real rays for the one-walk queries (nearest hit, occluded, bounce) and for
the full trace and the wavefront trace at depth 1; at depth 5 those two are held to the compacted list's count."""
import numpy as np
import pytest

import scenes
from cgraytracing_amd import _capi

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 128, 129, 64 * 5 + 1)
SCENES = {
    "c2_spheres": scenes.scene_c2,                       # glass and mirror spheres: no trees, the SPH variants
    "glass_pyramid": lambda: scenes.scene_pyramid(True),  # planes and a small glass mesh: a tree variant
}
_N_MAX = max(COUNTS)


def _aimed_rays():
    """_N_MAX rays from around the eye into the room both scenes live in, unit directions, and a key each"""
    rng = np.random.default_rng(20240611)
    org = np.array([0.0, -5.0, -10.0]) + rng.uniform(-1.0, 1.0, (_N_MAX, 3))
    aim = np.stack([rng.uniform(-18, 18, _N_MAX), rng.uniform(-19.5, 5, _N_MAX), rng.uniform(20, 38, _N_MAX)], axis=1)
    d = aim - org
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    keys = rng.integers(1, 2 ** 62, _N_MAX, dtype=np.int64)
    return org, d, keys


ORG, DIRS, KEYS = _aimed_rays()


def _pattern(which, n):
    """real: bool per row of the padded list"""
    if which == "a":
        return np.ones(n, bool)
    if which == "b":
        return np.arange(n) % 3 != 2
    at = n if n % 64 == 0 else 64 * (n // 128)
    real = np.ones(n + 64, bool)
    real[at:at + 64] = False
    return real


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request, gpu_ready):
    import cgraytracing_amd as cg
    with cg.Scene(SCENES[request.param]()) as sc:
        yield request.param, sc


def _lists(real):
    """the padded list (dir = 0 and another origin in the rows that are none) and the compacted one, as device tensors"""
    import torch
    m = int(real.sum())
    org = np.full((len(real), 3), 7.0)
    dirs = np.zeros((len(real), 3))
    keys = np.full(len(real), 99, np.int64)
    org[real], dirs[real], keys[real] = ORG[:m], DIRS[:m], KEYS[:m]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return (dev(org), dev(dirs), dev(keys)), (dev(ORG[:m]), dev(DIRS[:m]), dev(KEYS[:m]))


def _np(res):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def _nrays(res):
    return int(res["counters"][_capi.CNT_RAYS])


def _same_rows(pad, cmp_, real, names, what):
    for k in names:
        assert np.array_equal(pad[k][real], cmp_[k]), (what, k)
        assert not pad[k][~real].any() or k == "hit_obj", (what, k, "a row that is none")
    if "hit_obj" in names:
        assert (pad["hit_obj"][~real] == -1).all(), (what, "hit_obj of a row that is none")


def _check_trace(sc, padded, compact, real, what):
    m = int(real.sum())
    for depth in (5, 1):
        pad, cmp_ = _np(sc.trace_rays(*padded, max_depth=depth)), _np(sc.trace_rays(*compact, max_depth=depth))
        _same_rows(pad, cmp_, real, ("acc", "nhit", "hit_obj", "hit_t", "hit_normal"), (what, "trace", depth))
        assert _nrays(pad) == _nrays(cmp_) >= m, (what, "trace", depth, _nrays(pad), _nrays(cmp_))
        assert int(pad["counters"][_capi.CNT_HITPOINTS]) == int(cmp_["counters"][_capi.CNT_HITPOINTS]) == int(cmp_["nhit"].sum())
        if depth == 1:
            assert _nrays(pad) == m, (what, "trace depth 1", _nrays(pad), m)
    pad, cmp_ = _np(sc.trace_rays(*padded, want=("hit",))), _np(sc.trace_rays(*compact, want=("hit",)))
    _same_rows(pad, cmp_, real, ("hit_obj", "hit_t", "hit_normal"), (what, "nearest hit"))
    assert _nrays(pad) == _nrays(cmp_) == m, (what, "nearest hit", _nrays(pad), m)
    return cmp_["hit_obj"]


def _check_occluded(sc, padded, compact, real, what):
    m = int(real.sum())
    pad, cmp_ = _np(sc.occluded(*padded[:2], keys=padded[2])), _np(sc.occluded(*compact[:2], keys=compact[2]))
    _same_rows(pad, cmp_, real, ("occluded",), (what, "occluded"))
    assert _nrays(pad) == _nrays(cmp_) == m, (what, "occluded", _nrays(pad), m)
    return cmp_["occluded"]


def _check_bounce(sc, padded, compact, real, what):
    m = int(real.sum())
    pad, cmp_ = _np(sc.bounce(*padded[:2], keys=padded[2])), _np(sc.bounce(*compact[:2], keys=compact[2]))
    _same_rows(pad, cmp_, real, ("step", "hit_obj", "hit_t", "pos", "normal", "value"), (what, "bounce"))
    real2 = np.r_[real, real]  # row i the reflected child of ray i, row n + i the refracted one
    _same_rows(pad, cmp_, real2, ("child_org", "child_dir", "child_adj", "child_path", "child_keys"), (what, "bounce children"))
    assert _nrays(pad) == _nrays(cmp_) == m, (what, "bounce", _nrays(pad), m)
    return cmp_["step"]


def _check_wavefront(sc, padded, compact, real, what):
    m = int(real.sum())
    index = np.nonzero(real)[0]
    for depth in (5, 1):
        kw = dict(max_depth=depth, want=("acc", "nhit", "hp"), hp_cap=32 * len(real))
        pad, cmp_ = _np(sc.wavefront(*padded, **kw)), _np(sc.wavefront(*compact, **kw))
        _same_rows(pad, cmp_, real, ("acc", "nhit"), (what, "wavefront", depth))
        assert pad["hp_count"] == cmp_["hp_count"] == len(pad["hp_ray"]) == int(cmp_["nhit"].view(np.uint32).sum()), (what, depth)
        assert np.array_equal(pad["hp_ray"], index[cmp_["hp_ray"]]), (what, "wavefront hp_ray", depth)
        for k in ("hp9", "hp_path"):
            assert np.array_equal(pad[k], cmp_[k]), (what, "wavefront", depth, k)
        assert _nrays(pad) == _nrays(cmp_) >= m and pad["rays_per_level"] == cmp_["rays_per_level"], (what, "wavefront", depth)
        assert pad["rays_per_level"][0] == m, (what, "wavefront level 1", pad["rays_per_level"], m)
        if depth == 1:
            assert _nrays(pad) == m, (what, "wavefront depth 1", _nrays(pad), m)


@pytest.mark.parametrize("n", COUNTS)
def test_padded_list_equals_compacted_list(scene, n):
    """Patterns (a), (b), (c) at n, each query: the padded list's results in the real rows are the compacted list's bit for bit,
    the rows that are none hold the query's miss (zeros, hit_obj -1), and CGRT_CNT_RAYS is as the module's docstring says."""
    name, sc = scene
    for which in "abc":
        real = _pattern(which, n)
        padded, compact = _lists(real)
        what = (name, n, which)
        hit_obj = _check_trace(sc, padded, compact, real, what)
        occ = _check_occluded(sc, padded, compact, real, what)
        step = _check_bounce(sc, padded, compact, real, what)
        _check_wavefront(sc, padded, compact, real, what)
        # condition, not measurement: the rays are aimed into a closed room, so each of them is answered by a walk
        assert (hit_obj >= 0).all() and (occ == 1).all() and (step != _capi.STEP_NONE).all(), what


def test_rays_reach_every_step(scene):
    """Condition on the aimed rays: in both scenes some end at a Hitpoint, some are reflected and some split at glass, so the
    comparisons above cover the stores of every kind of step."""
    name, sc = scene
    real = _pattern("a", _N_MAX)
    _, compact = _lists(real)
    step = _np(sc.bounce(*compact[:2], keys=compact[2]))["step"]
    want = (_capi.STEP_HITPOINT, _capi.STEP_REFLECT, _capi.STEP_SPLIT) if name == "c2_spheres" else (_capi.STEP_HITPOINT, _capi.STEP_SPLIT)
    for s in want:
        assert (step == s).sum() >= 4, (name, s, np.bincount(step, minlength=4))
