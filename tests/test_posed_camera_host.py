"""The posed camera (cgrt_posed_camera, CGRT_GRID_POSED, cgrt_look_at), the part that needs no GPU: the ABI, the identity frame
against the built-in camera bit for bit, the geometry of look-at views against numpy alone, the refusals, the launch plan of a
posed launch (tests/native/posed_plan.cpp under ASan + UBSan) and the compiler's resource rows of the kernels that were there
before, which adding POSE must not move."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import scenes
from cgraytracing_amd import _capi
from cgraytracing_amd.engine import camera_rays_host
from cgraytracing_amd.scene import Camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
# the cameras of tests/test_rays_host.py: on axis and two off axis, each with its lens and as a pinhole
CAMERAS = [
    ("dof", lambda: scenes.cam_dof()),
    ("off_axis_a", lambda: Camera(cam=(3.0, 2.0, -14.0), lens_radius=1.5)),
    ("off_axis_b", lambda: Camera(cam=(-4.5, 1.25, -8.0), focus_plane=17.0, lens_radius=0.7)),
]
GRIDS = [
    ("67x45_spp3", dict(spp=3)),
    ("striped", dict(spp=3, rows=16, stripe=(8, 2, 3))),
    ("band", dict(spp=3, rows=13, row_offset=20, sample_offset=4)),
]
# three look-at views: the example's, one from below and behind with a tilted hint, one straight down -y with an up hint of +z
VIEWS = [
    ("example", dict(eye=(17.0, 8.0, 2.0), target=(-2.0, -13.0, 30.0), up=(0.0, 1.0, 0.0), fov_x_deg=70.0)),
    ("tilted", dict(eye=(-6.5, -3.0, 41.0), target=(1.0, 2.5, 20.0), up=(0.3, 1.0, -0.2), fov_x_deg=38.0)),
    ("down", dict(eye=(2.0, 30.0, 25.0), target=(2.0, -13.0, 25.0), up=(0.0, 0.0, 1.0), fov_x_deg=100.0)),
]
ULP2 = 4 * 2.0 ** -53  # 2 ulp of 1.0


def _posed(cam, pose=IDENTITY, lens=None):
    return Camera(cam.cam, cam.half_width, cam.focus_plane, cam.lens_radius if lens is None else lens, pose=pose)


def _frame(cam):
    o, r, u, f = (np.asarray(v, np.float64) for v in cam.pose)
    return o, r, u, f


def _world(cam, p):
    """M(p) of cgrt.h for points p [n,3] of the camera's frame, in the documented order."""
    o, r, u, f = _frame(cam)
    return ((o[None, :] + r[None, :] * p[:, 0:1]) + u[None, :] * p[:, 1:2]) + f[None, :] * p[:, 2:3]


def _norm_err(d):
    x = d.astype(np.longdouble)
    return np.abs(np.sqrt((x * x).sum(axis=1)) - 1).astype(np.float64)


def _pixel_points(cam, W, H):
    """(px, py, 0) of every pixel in ray order of one sample (set_pixel's expressions)."""
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px = (2.0 * (w.reshape(-1).astype(np.float64) / W) - 1) * cam.half_width
    py = (2.0 * (h.reshape(-1).astype(np.float64) / H) - 1) * cam.half_width * H / W
    return np.stack([px, py, np.zeros_like(px)], axis=1)


def _off_line(p, org, d):
    """Distance of the points p from the rays (org, d), relative to their distance from the origins."""
    v = p - org
    along = (v * d).sum(axis=1)
    assert (along > 0).all()
    return np.linalg.norm(v - d * along[:, None], axis=1) / np.linalg.norm(v, axis=1)


def test_abi(tmp_path):
    """sizeof / offsetof as compile-time asserts of a strict C99 translation unit, which then calls cgrt_look_at and hands the
    posed camera's base to an entry that takes a cgrt_camera; the binding's struct has the same size and the flag the same bit."""
    assert C.sizeof(_capi.PosedCamera) == 144 and _capi.PosedCamera.base.offset == 0 and _capi.PosedCamera.origin.offset == 48
    assert C.sizeof(_capi.Camera) == 48 and C.sizeof(_capi.Grid) == 56
    assert _capi.GRID_POSED == 1 << 26
    assert "cgrt_look_at" in _capi.SIGNATURES and getattr(_capi.lib(), "cgrt_look_at") is not None
    src = os.path.join(ROOT, "tests", "native", "abi_posed_c99.c")
    obj = str(tmp_path / "abi_posed.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", obj])
    so = str(tmp_path / "libabi_posed.so")
    subprocess.check_call(["gcc", "-shared", "-o", so, obj, "-L", os.path.dirname(_capi.LIB_PATH), "-lcgrt",
                           "-Wl,-rpath," + os.path.dirname(_capi.LIB_PATH)])
    assert C.CDLL(so).cgrt_abi_posed_smoke() == 0


@pytest.mark.parametrize("grid_case", GRIDS, ids=lambda g: g[0])
@pytest.mark.parametrize("lens", [True, False], ids=["lens", "pinhole"])
@pytest.mark.parametrize("cam_case", CAMERAS, ids=lambda c: c[0])
def test_identity_pose_is_the_builtin_camera(cam_case, lens, grid_case):
    """cgrt_camera_rays_host with the identity pose against the call without the flag: origins, directions and keys equal."""
    cam = cam_case[1]()
    if not lens:
        cam = Camera(cam.cam, cam.half_width, cam.focus_plane, 0.0)
    kw = grid_case[1]
    a = camera_rays_host(67, 45, camera=cam, seed=SEED, **kw)
    b = camera_rays_host(67, 45, camera=_posed(cam), seed=SEED, **kw)
    for x, y, what in zip(a, b, ("origins", "directions", "keys")):
        assert np.array_equal(x, y), what
    assert np.any(b[1] != 0)


@pytest.mark.parametrize("view", VIEWS, ids=lambda v: v[0])
def test_look_at_geometry_against_numpy(view):
    """A 9 x 5 grid of a look-at view, against numpy alone.  Pinhole: every ray starts at the eye and passes through M(pix)
    within 1e-12 relative.  Thin lens: every ray starts in the lens disc's plane within lens_radius of the eye and passes through
    its pixel's focus point, which lies focus_distance along forward.  |dir| = 1 within 2 ulp.  The centre pixel pair brackets
    target - eye.  The rays, rotated back into the camera's frame, are the built-in camera's rays of `base` within 1e-12: the
    pose transforms rays, it does not change them."""
    W, H, spp = 9, 5, 4
    kw = view[1]
    eye, target = np.asarray(kw["eye"]), np.asarray(kw["target"])
    D = np.linalg.norm(target - eye)
    focus = 0.8 * D
    cam = Camera.look_at(focus_distance=focus, lens_radius=0.0, **kw)
    o, r, u, f = _frame(cam)
    # the frame: orthonormal, right-handed, looking at the target, right = normalize(up_hint x forward), up = forward x right
    R = np.stack([r, u, f], axis=1)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-15
    assert np.abs(f - (target - eye) / D).max() <= 1e-15
    want_r = np.cross(np.asarray(kw["up"]), f)
    assert np.abs(r - want_r / np.linalg.norm(want_r)).max() <= 1e-15 and np.abs(u - np.cross(f, r)).max() <= 1e-15
    assert np.dot(np.cross(r, u), f) > 0.999999
    assert abs(cam.half_width / -cam.cam[2] - np.tan(np.radians(kw["fov_x_deg"]) / 2)) <= 1e-14
    camv = np.asarray(cam.cam, np.float64)
    assert np.abs(_world(cam, camv[None, :])[0] - eye).max() <= 1e-12 * np.linalg.norm(eye)  # the eye maps to eye

    org, dirs, keys = camera_rays_host(W, H, 1, cam, SEED)
    pix = _world(cam, _pixel_points(cam, W, H))
    assert np.abs(org - eye[None, :]).max() <= 1e-12 * np.linalg.norm(eye)
    assert np.array_equal(org, np.tile(_world(cam, camv[None, :]), (W * H, 1)))  # ... and it is M(cam), bit for bit
    assert _off_line(pix, org, dirs).max() <= 1e-12
    assert _norm_err(dirs).max() <= ULP2
    # the centre pair: pixels (row 2, column 4) and (row 3, column 5) lie about the image's centre, point for point
    d = dirs.reshape(H, W, 3)
    lo, hi, t = d[2, 4], d[3, 5], (target - eye) / D
    assert np.dot(lo, r) < 0 < np.dot(hi, r) and np.dot(lo, u) < 0 < np.dot(hi, u) and np.dot(lo, f) > 0 and np.dot(hi, f) > 0
    mid = (lo + hi) / np.linalg.norm(lo + hi)
    assert np.abs(mid - t).max() <= 1e-12
    # row 0 is the bottom row: it looks below the centre
    assert np.dot(d[0, 4], u) < 0 < np.dot(d[H - 1, 4], u)

    # rotated back: the built-in camera's rays of the same base
    base = Camera(cam.cam, cam.half_width, cam.focus_plane, 0.0)
    org0, dirs0, keys0 = camera_rays_host(W, H, 1, base, SEED)
    assert np.array_equal(keys, keys0)
    assert np.abs((org - o[None, :]) @ R - org0).max() <= 1e-12 * D
    assert np.abs(dirs @ R - dirs0).max() <= 1e-12

    # thin lens
    lens_r = 0.75
    lcam = Camera(cam.cam, cam.half_width, cam.focus_plane, lens_r, pose=cam.pose)
    lorg, ldirs, lkeys = camera_rays_host(W, H, spp, lcam, SEED)
    lbase = Camera(cam.cam, cam.half_width, cam.focus_plane, lens_r)
    lorg0, ldirs0, lkeys0 = camera_rays_host(W, H, spp, lbase, SEED)
    assert np.array_equal(lkeys, lkeys0)
    off = lorg - eye[None, :]
    assert np.abs(off @ f).max() <= 1e-12 * D                       # in the lens disc's plane ...
    assert np.linalg.norm(off, axis=1).max() <= lens_r * (1 + 1e-12)   # ... within the lens
    assert np.linalg.norm(off, axis=1).max() > 0.5 * lens_r
    # the focus point of a pixel: on its pinhole ray, focus_distance along forward from the eye
    fp = eye[None, :] + dirs * (focus / (dirs @ f))[:, None]
    assert np.abs((fp - eye[None, :]) @ f - focus).max() <= 1e-12 * D
    assert _off_line(np.tile(fp, (spp, 1)), lorg, ldirs).max() <= 1e-12
    assert _norm_err(ldirs).max() <= ULP2
    assert np.abs((lorg - o[None, :]) @ R - lorg0).max() <= 1e-12 * D
    assert np.abs(ldirs @ R - ldirs0).max() <= 1e-12


def test_look_at_of_the_builtin_view_is_the_builtin_frame():
    """eye (0,0,-10), target 0, up +y, 90 degrees: origin 0 and the unit axes, the eye at (0,0,-10)."""
    cam = Camera.look_at((0.0, 0.0, -10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 90.0, focus_distance=30.0, lens_radius=1.5)
    assert cam.pose == IDENTITY
    assert tuple(cam.cam) == (0.0, 0.0, -10.0) and cam.focus_plane == 20.0 and cam.lens_radius == 1.5
    assert abs(cam.half_width - 10.0) <= 2e-15 * 10
    # with half_width set to the literal 10 the posed rays are the default camera's, bit for bit
    cam.half_width = 10.0
    for x, y in zip(camera_rays_host(67, 45, 3, cam, SEED), camera_rays_host(67, 45, 3, scenes.cam_dof(), SEED)):
        assert np.array_equal(x, y)


def _rays_rc(pc, flags=_capi.GRID_POSED):
    g = _capi.Grid(9, 5, 5, 0, 0, 0, 1, 1, 0, 1, 5, flags, SEED)
    org = np.zeros((45, 3))
    L = _capi.lib()
    rc = L.cgrt_camera_rays_host(C.byref(pc.base), C.byref(g), org.ctypes.data, None, None)
    return rc, L.cgrt_last_error().decode()


def _pc(right=(1, 0, 0), up=(0, 1, 0), forward=(0, 0, 1), origin=(0, 0, 0)):
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])  # noqa: E731
    return _capi.PosedCamera(_capi.Camera(d3((0, 0, -10)), 10.0, 20.0, 0.0), d3(origin), d3(right), d3(up), d3(forward))


def test_refusals():
    """CGRT_ERR_INVALID with a message: a basis scaled by 1 + 1e-6, two axes 1e-6 off orthogonal, a NaN; cgrt_look_at with eye
    == target, up parallel to the view, fov 0 or 180.  Accepted: a left-handed orthonormal basis (it mirrors the image), and
    anything at all behind the camera when the flag is not set."""
    INVALID = -1
    assert _rays_rc(_pc())[0] == 0
    s = 1 + 1e-6
    for what, pc in [("scaled basis", _pc((s, 0, 0), (0, s, 0), (0, 0, s))), ("one long axis", _pc(up=(0, s, 0))),
                     ("skewed", _pc(up=(1e-6, 1, 0))), ("skewed forward", _pc(forward=(0, 1e-6, 1))),
                     ("nan origin", _pc(origin=(0, float("nan"), 0))), ("nan axis", _pc(right=(float("nan"), 0, 0))),
                     ("inf", _pc(origin=(float("inf"), 0, 0))), ("zero axis", _pc(forward=(0, 0, 0)))]:
        rc, msg = _rays_rc(pc)
        assert rc == INVALID and "posed camera" in msg, (what, rc, msg)
        assert _rays_rc(pc, flags=0)[0] == 0, what  # without the flag the pose is not looked at
    # within the bound
    assert _rays_rc(_pc(up=(5e-10, 1, 0)))[0] == 0 and _rays_rc(_pc(right=(1 + 5e-10, 0, 0)))[0] == 0
    # left-handed: accepted, and the image is mirrored -- column w of the mirrored frame is column W - w of the other, about pixel W / 2
    rc, _ = _rays_rc(_pc(right=(-1, 0, 0)))
    assert rc == 0
    a = camera_rays_host(8, 4, 1, _posed(Camera(), IDENTITY), SEED)[1].reshape(4, 8, 3)
    b = camera_rays_host(8, 4, 1, _posed(Camera(), ((0, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 1))), SEED)[1].reshape(4, 8, 3)
    assert np.array_equal(b[:, 1:], a[:, :0:-1]) and not np.array_equal(b, a)
    # the Python layer raises what the library refuses
    with pytest.raises(_capi.CgrtError) as e:
        camera_rays_host(9, 5, 1, _posed(Camera(), ((0, 0, 0), (s, 0, 0), (0, 1, 0), (0, 0, 1))), SEED)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        Camera(pose=((0, 0, 0), (1, 0, 0), (0, 1, 0)))
    for what, kw in [("eye == target", dict(eye=(1, 2, 3), target=(1, 2, 3))), ("up parallel", dict(eye=(0, 0, 0), target=(0, 5, 0), up=(0, 1, 0))),
                     ("up antiparallel", dict(eye=(1, 1, 1), target=(3, 3, 3), up=(-2, -2, -2))), ("up zero", dict(eye=(0, 0, 0), target=(0, 0, 1), up=(0, 0, 0))),
                     ("fov 0", dict(eye=(0, 0, 0), target=(0, 0, 1), fov_x_deg=0.0)), ("fov 180", dict(eye=(0, 0, 0), target=(0, 0, 1), fov_x_deg=180.0)),
                     ("fov 200", dict(eye=(0, 0, 0), target=(0, 0, 1), fov_x_deg=200.0)), ("nan eye", dict(eye=(float("nan"), 0, 0), target=(0, 0, 1))),
                     ("focus 0", dict(eye=(0, 0, 0), target=(0, 0, 1), focus_distance=0.0)),
                     ("lens < 0", dict(eye=(0, 0, 0), target=(0, 0, 1), lens_radius=-1.0))]:
        with pytest.raises(_capi.CgrtError) as e:
            Camera.look_at(**kw)
        assert e.value.code == INVALID and "cgrt_look_at" in str(e.value), what
    assert _capi.lib().cgrt_look_at(None, None, None, 90.0, 1.0, 0.0, None) == INVALID


def test_posed_plan_under_sanitizers(tmp_path):
    """tests/native/posed_plan.cpp: pose_point on the identity frame, the validation's bounds, cgrt_look_at's frame, and for a
    sphere scene, a mesh scene and a Bezier scene the posed launch's plan (no tile order, relay, lens table, light split or
    primary walk; a compiled POSE kernel), every compiled POSE kernel reachable, the plan without the flag untouched."""
    exe = str(tmp_path / "posed_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "posed_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout


def test_cpp_host_layer(tmp_path):
    """include/cgrt_host.hpp from a plain C++14 program (tests/native/host_posed.cpp): the default RenderParams is the built-in
    camera without the flag; look_at and set_pose fill the posed camera that goes where a cgrt_camera goes."""
    exe = str(tmp_path / "host_posed")
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "host_posed.cpp"), "-L", lib_dir, "-lcgrt", "-Wl,-rpath," + lib_dir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok: 0 failed checks" in out.stdout, out.stdout + out.stderr


def test_posed_variants_list_and_resource_rows():
    """CGRT_EYE_POSED_VARIANTS is a list of its own with the columns of CGRT_EYE_VARIANTS, shorter than it; and the tracked
    resource tables (tools/resource_table.py, cross-compiled: the parent commit's kernels and this one's): every kernel the
    parent had has the same VGPRs, spilled VGPRs, scratch, static LDS and occupancy, and every POSE kernel has a row."""
    import variants

    plain, posed = variants._entries("CGRT_EYE_VARIANTS", 15), variants._entries("CGRT_EYE_POSED_VARIANTS", 15)
    assert len(plain) >= 40 and 0 < len(posed) < len(plain) and len(set(posed)) == len(posed)
    assert all(e[5] == 0 and e[9] == 0 and e[10] == 0 and e[11] == 0 and e[12] == 0 and e[13] == 0 for e in posed)  # no STATS, HFONLY, DIFF, PAIR, START, LTAB
    assert all(e[:14] in {v[:14] for v in plain} for e in posed)  # each is an existing variant's posed form (SCHED aside)
    cols = ("vgprs", "agprs", "vgpr_spills", "scratch_bytes_per_lane", "static_lds_bytes", "occupancy_waves_per_simd")
    tab = {}
    for name in ("posed_camera_parent_resources.json", "posed_camera_resources.json"):
        with open(os.path.join(ROOT, "profiles", name)) as fh:
            rows = json.load(fh)["kernels"]
        tab[name] = {r["kernel"]: tuple(r.get(c) for c in cols) for r in rows}
        assert len(tab[name]) == len(rows), "two kernels of one name in " + name
    before, after = tab["posed_camera_parent_resources.json"], tab["posed_camera_resources.json"]
    assert len(before) > 150
    # (camera_rays_kernel is the one kernel whose text changed on purpose: it gained the posed branch)
    moved = {k: (v, after.get(k)) for k, v in before.items() if after.get(k) != v and k != "camera_rays_kernel"}
    assert not moved, moved
    assert "camera_rays_kernel" in after
    new = set(after) - set(before)
    want = set()
    for (T, B, D, G, P, S, H, NT, SP, HF, DF, PR, ST, LT, SCHED) in posed:
        want.add("trace_grid_kernel<TREES=%d,BEZ=%d,DOF=%d,GLASS=%d,SPH=%d,STATS=%d,HPS=%d,NT=%d,SPILL=%d,HFONLY=%d,DIFF=%d,PAIR=%d,POSE=1>"
                 % (T, B, D, G, P, S, H, NT, SP, HF, DF, PR))
        if SCHED:
            want.add("trace_grid_sched_kernel<TREES=%d,BEZ=%d,DOF=%d,GLASS=%d,SPH=%d,STATS=%d,NT=%d,POSE=1>" % (T, B, D, G, P, S, NT))
    want.add("pixel_const_kernel<POSE=1>")
    assert new == want, new ^ want
