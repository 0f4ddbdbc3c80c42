"""Scene definitions used by tests, golden generation and bench.py.  Geometry and materials follow
SURVEY.md §8d, which in turn cites the (partly commented-out) scene code of main.cpp:281-376."""
from __future__ import annotations

import os

import numpy as np

from cgraytracing_amd.scene import Bezier, Camera, Plane, Sphere, Texture, TriangleMesh

HERE = os.path.dirname(os.path.abspath(__file__))
ASSETS = os.path.join(HERE, "golden", "assets")


def wall_spheres():
    # main.cpp:281-285
    return [
        Sphere((0.0, -10020, 0), 10000, (0.25, 0.25, 0.25), 0.0, 0.0),
        Sphere((10020, 0.0, 0), 10000, (0.25, 0.75, 0.25), 0.0, 0.0),
        Sphere((-10020, 0.0, 0), 10000, (0.75, 0.25, 0.25), 0.0, 0.0),
        Sphere((0.0, 0.0, 10040), 10000, (0.25, 0.25, 0.25), 0.0, 0.0),
        Sphere((0.0, 10020, 0), 10000, (0.25, 0.25, 0.25), 0.0, 0.0),
    ]


def scene_c1():
    """C1: six diffuse spheres (main.cpp:281-285,288)."""
    return wall_spheres() + [Sphere((-15.0, -20.0, 60), 10, (0.3, 0.3, 0.3), 0.0, 0.0)]


def scene_c2():
    """C2: walls + diffuse + mirror + glass spheres (materials main.cpp:288-290; centres per SURVEY §8d)."""
    return wall_spheres() + [
        Sphere((-15.0, -20.0, 60), 10, (0.3, 0.3, 0.3), 0.0, 0.0),
        Sphere((10.0, -13.0, 30), 7, (1.0, 1.0, 1.0), 0.8, 0.0),
        Sphere((-8.0, -13.0, 25), 7, (1.0, 1.0, 1.0), 0.8, 0.5),
    ]


def planes(floor_tex=None):
    # main.cpp:348-353
    return [
        Plane((0.0, -20, 0), (0, 1, 0), (0.15, 0.15, 0.15), 0.0, 0.0, floor_tex),
        Plane((20, 0.0, 0), (-1, 0, 0), (0.15, 0.50, 0.15), 0.0, 0.0),
        Plane((-20, 0.0, 0), (1, 0, 0), (0.50, 0.15, 0.15), 0.0, 0.0),
        Plane((0.0, 0.0, 40), (0, 0, -1), (0.15, 0.15, 0.15), 0.0, 0.0),
        Plane((0.0, 20, 0), (0, -1, 0), (0.15, 0.15, 0.15), 0.0, 0.0),
    ]


def load_asset(name):
    return np.load(os.path.join(ASSETS, name))


def chessboard_texture(bump=False):
    d = load_asset("chessboard_rgb.npz")["rgb"]
    return Texture(d, (0, 1, 0), (-21, 0, 0), 42, 40, bump)  # main.cpp:320 geometry


def stone_small_texture(bump=True):
    d = load_asset("stone_small_rgb.npz")["rgb"]
    return Texture(d, (0, 1, 0), (-21, 0, 0), 42, 40, bump)


def stone_texture(bump=True):
    """texture/stone.jpg at its full 1000x667 as the reference's stb decoder returns it, placed as main.cpp:320 does:
    Texture(tdata, (0,1,0), (-21,0,0), 42, 40, true).  As a bump map: 146 744 triangles, 32 767 nodes."""
    d = load_asset("stone_rgb.npz")["rgb"]
    return Texture(d, (0, 1, 0), (-21, 0, 0), 42, 40, bump)


def procedural_stone(rows=667, cols=1000, seed=7):
    """Seeded stand-in of texture/stone.jpg's size (kept for fuzz-style tests; the configurations use stone_texture())."""
    rng = np.random.default_rng(seed)
    base = rng.random((rows // 8 + 2, cols // 8 + 2))
    up = np.kron(base, np.ones((8, 8)))[:rows, :cols]
    fine = rng.random((rows, cols))
    g = np.clip(0.25 + 0.5 * up + 0.25 * fine, 0, 1)
    rgb = np.stack([g * 200 + 20, g * 190 + 20, g * 170 + 20], -1).astype(np.uint8)
    return np.ascontiguousarray(rgb)


def bunny_tris():
    """model/lowpolybunny.txt through the type-0 loader transform a=10, b=(0,-15,40) (main.cpp:293)."""
    return load_asset("bunny_tris.npz")["tris"]


def scene_c3(glass=True):
    """C3: 5 planes (chessboard floor) + glass bunny (main.cpp:293,348-353)."""
    floor = chessboard_texture(False)
    m = TriangleMesh.from_triangles(bunny_tris(), (1.0, 1.0, 1.0), 0.8 if glass else 0.0, 0.5 if glass else 0.0)
    return planes(floor) + [m]


def pyramid_tris(a=1.0, b=(0.0, -5.0, 30.0)):
    """The 6-triangle square pyramid of model/tri.txt (type-1 file, 5 vertices), transformed."""
    v = np.array([[5, 0, 5], [5, 0, -5], [-5, 0, 5], [-5, 0, -5], [0, -10, 0]], np.float64)
    f = np.array([[1, 2, 5], [1, 3, 5], [2, 4, 5], [3, 4, 5], [1, 2, 4], [1, 3, 4]]) - 1
    v = v * np.array([1, 1, -1.0]) * a + np.asarray(b, np.float64)
    return v[f].reshape(-1, 9)


def scene_pyramid(glass=False):
    m = TriangleMesh.from_triangles(pyramid_tris(1.0, (0.0, -5.0, 30.0)), (0.6, 0.7, 0.9),
                                    0.8 if glass else 0.0, 0.5 if glass else 0.0)
    return planes() + [m]


def procedural_mesh(n_u=40, n_v=20, center=(-5.0, -10.0, 30.0), radius=8.0, seed=3, wobble=0.15):
    """Closed lumpy sphere mesh with 2*n_u*(n_v-1) triangles (seeded), for mesh configs whose
    original model file is not shipped."""
    rng = np.random.default_rng(seed)
    th = np.linspace(0, np.pi, n_v + 1)
    ph = np.linspace(0, 2 * np.pi, n_u, endpoint=False)
    r = radius * (1 + wobble * (rng.random((n_v + 1, n_u)) - 0.5))
    r[0, :] = r[0, 0]
    r[-1, :] = r[-1, 0]
    P = np.zeros((n_v + 1, n_u, 3))
    P[..., 0] = r * np.sin(th)[:, None] * np.cos(ph)[None, :]
    P[..., 1] = r * np.cos(th)[:, None]
    P[..., 2] = r * np.sin(th)[:, None] * np.sin(ph)[None, :]
    P += np.asarray(center, np.float64)
    tris = []
    for i in range(n_v):
        for j in range(n_u):
            j2 = (j + 1) % n_u
            a, b, c, d = P[i, j], P[i, j2], P[i + 1, j], P[i + 1, j2]
            if i > 0:
                tris.append([a, b, c])
            if i < n_v - 1:
                tris.append([d, b, c])
    return np.asarray(tris, np.float64).reshape(-1, 9)


def scene_c4(n_u=320, n_v=158):
    """C4 stand-in: untextured planes + a ~100k-triangle diffuse procedural mesh placed where the
    dragon sits (main.cpp:292: scale 1.5, offset (-5,-20,30), colour (0.25,0.25,0.5))."""
    m = TriangleMesh.from_triangles(procedural_mesh(n_u, n_v, (-5.0, -10.0, 30.0), 9.0), (0.25, 0.25, 0.5), 0.0, 0.0, 1)
    return planes() + [m]


def vase_bezier(refl=0.5, transp=0.0):
    # main.cpp:371-376
    cp = [(0, -10, 4), (0, 2, 4), (0, -2, 0), (0, 10, 2)]
    return Bezier(cp, (15, -10.1, 35), (1.0, 1.0, 1.0), refl, transp)


def scene_c5(tex=None):
    """C5: planes with bump floor + Bezier vase."""
    return planes(tex) + [vase_bezier()]


def textured_walls():
    """Textures in all three orientations of Texture::color (texture.h:39-72): the chessboard on the floor (|d.y| branch),
    on the back wall (|d.z| branch, vertically flipped) and on the right-hand wall (|d.x| branch, tested first), sized so
    that part of every wall lies outside the texture rectangle (flat colour there, objects.h:533-539)."""
    chess = load_asset("chessboard_rgb.npz")["rgb"]
    floor = Texture(chess, (0, 1, 0), (-21, -20, 0), 42, 40, False)
    back = Texture(chess, (0, 0, -1), (-15, -18, 40), 30, 25, False)
    side = Texture(chess, (-1, 0, 0), (20, -16, 5), 30, 28, False)
    return [
        Plane((0.0, -20, 0), (0, 1, 0), (0.15, 0.15, 0.15), 0.0, 0.0, floor),
        Plane((20, 0.0, 0), (-1, 0, 0), (0.15, 0.50, 0.15), 0.0, 0.0, side),
        Plane((-20, 0.0, 0), (1, 0, 0), (0.50, 0.15, 0.15), 0.0, 0.0),
        Plane((0.0, 0.0, 40), (0, 0, -1), (0.15, 0.15, 0.15), 0.0, 0.0, back),
        Plane((0.0, 20, 0), (0, -1, 0), (0.15, 0.15, 0.15), 0.0, 0.0),
    ]


def scene_textured_walls():
    """textured_walls() + a mirror and a glass sphere, so reflected and refracted rays reach the walls at all angles."""
    return textured_walls() + [Sphere((9.0, -13.0, 30), 7, (1.0, 1.0, 1.0), 0.8, 0.0),
                               Sphere((-8.0, -13.0, 25), 7, (1.0, 1.0, 1.0), 0.8, 0.5)]


def scene_glass_bump_floor():
    """A TRANSPARENT bump-mapped floor: its displacement mesh goes through the tree (the improvement counter is observable
    for a refracting owner), not the height-field walk of opaque floors; a second textured floor below catches
    the refracted rays."""
    pl = planes(None)
    pl[0] = Plane((0.0, -20, 0), (0, 1, 0), (0.9, 0.9, 0.9), 0.8, 0.5, chessboard_texture(True))
    chess = load_asset("chessboard_rgb.npz")["rgb"]
    below = Plane((0.0, -24, 0), (0, 1, 0), (0.2, 0.2, 0.3), 0.0, 0.0, Texture(chess, (0, 1, 0), (-30, -24, 0), 60, 60, False))
    return pl + [below]


def cam_pinhole():
    return Camera()


def cam_dof():
    return Camera(lens_radius=1.5)  # main.cpp:178-181


def dragon_tris(a=1.5, b=(-5.0, -20.0, 30.0)):
    """model/dragon.txt (type-1 file) through the loader transform (x,y,-z)*a+b (objects.h:365,371)."""
    d = load_asset("dragon_mesh.npz")
    v = d["v1e4"].astype(np.float64) / 1e4
    v = v * np.array([1.0, 1.0, -1.0])
    v = v * a + np.asarray(b, np.float64)
    return v[d["faces"] - 1].reshape(-1, 9)


def scene_dragon():
    """The committed main() scene minus the bump floor: planes + diffuse dragon (main.cpp:292,348-353)."""
    m = TriangleMesh.from_triangles(dragon_tris(), (0.25, 0.25, 0.5), 0.0, 0.0, 1)
    return planes() + [m]


def many_spheres(n, seed, head=None, dup_pairs=()):
    """Scenes of many top-level objects: `head` (default: the five wall spheres) and then seeded spheres of all three
    materials (half diffuse, a quarter mirror, a quarter glass) up to exactly n objects, about one in twenty followed by an
    exact duplicate.  dup_pairs: (a, b) with a < b -- object b is an exact duplicate (magenta, diffuse) of sphere a, both placed
    in plain view near the front of the room, so that the earlier object visibly has to win the tie (main.cpp:57) whatever
    separates a from b (an LDS boundary)."""
    rng = np.random.default_rng(seed)
    objs = list(wall_spheres() if head is None else head)
    pairs = {a: b for a, b in dup_pairs if b < n}
    dups = {}
    while len(objs) < n:
        i = len(objs)
        if i in dups:
            objs.append(dups.pop(i))
            continue
        if i in pairs:
            k = sorted(pairs).index(i)
            c = (-12.0 + 6.0 * (k % 5), -8.0 + 8.0 * ((k // 5) % 3), 14.0)
            s = Sphere(c, 1.5, (0.2, 0.9, 0.4), *[(0, 0), (0.8, 0), (0.8, 0.5)][k % 3])
            objs.append(s)
            dups[pairs[i]] = Sphere(c, s.radius, (1.0, 0.0, 1.0), 0, 0)
            continue
        c = (rng.uniform(-17, 17), rng.uniform(-18, 17), rng.uniform(12, 38))
        refl, transp = [(0, 0), (0, 0), (0.8, 0), (0.8, 0.5)][rng.integers(0, 4)]
        s = Sphere(c, rng.uniform(0.3, 1.6), tuple(rng.uniform(0.2, 1, 3)), refl, transp)
        objs.append(s)
        if len(objs) < n and len(objs) not in dups and len(objs) not in pairs and rng.random() < 0.05:
            objs.append(Sphere(c, s.radius, (1.0, 0.0, 1.0), 0, 0))  # an exact duplicate later in the list
    return objs


def room_with_objects(n, seed, mesh=None, floor_tex=None, extra=(), dup_pairs=()):
    """A room of five planes (`planes(floor_tex)`: they lead the list, so the plane-run test stays in play), then `mesh` and
    `extra` objects if given, then spheres up to exactly n top-level objects (many_spheres, with its duplicates)."""
    head = planes(floor_tex) + ([mesh] if mesh is not None else []) + list(extra)
    objs = many_spheres(n, seed, head=head, dup_pairs=dup_pairs)
    assert len(objs) == n
    return objs


# ---- planes in general position (tests/test_planes_general_host.py, tests/test_gpu_planes_general.py) --------------------------
GP_POINT = (1.0, -2.0, 25.0)  # every near plane of general_planes() passes through it
GP_BOX = (np.array([-19.0, -20.0, 5.0]), np.array([21.0, 20.0, 45.0]))  # the 40-unit box of the random origins, around it
GP_FAR_POINT = (0.0, -3e9, 0.0)
K_INF = 1e10  # main.cpp: nearest = INF; a length that is not below it never wins
RAY_CLASSES = ("a", "b", "c", "d", "e", "f", "g")


def general_planes():
    """[(name, Plane)]: single planes for the function-level tests.  Only axis_unit, far_axis_unit and the two axis_negzero planes
    are classified axis-aligned (HostScene::add_plane: a component exactly +-1, the others == 0.0, which -0.0 is); all the others
    take the general form of Plane::intersect, len = ((p - o) . n) / (d . n) with the normal as given (objects.h:505-509)."""
    n123 = np.array([1.0, 2.0, 3.0])
    unit = n123 / np.sqrt(14.0)  # (n1, 2 n1, fl(3 / sqrt 14)): scaling by two is exact
    mk = lambda p, n: Plane(tuple(p), tuple(n), (0.4, 0.6, 0.8), 0.0, 0.0)
    return [
        ("oblique", mk(GP_POINT, unit)),
        ("oblique_nonunit", mk(GP_POINT, n123)),
        ("axis_nonunit", mk(GP_POINT, (0.0, 2.0, 0.0))),
        ("axis_half", mk(GP_POINT, (0.0, 0.5, 0.0))),
        ("axis_triple", mk(GP_POINT, (0.0, 3.0, 0.0))),  # fl(3 a) / fl(3 b) is not a / b: unlike 2 and 0.5 this scaling is visible
        ("axis_negzero_up", mk(GP_POINT, (-0.0, 1.0, 0.0))),
        ("axis_negzero_down", mk(GP_POINT, (0.0, -1.0, -0.0))),
        ("near_axis_x", mk(GP_POINT, (1e-17, 1.0, 0.0))),
        ("near_axis_z", mk(GP_POINT, (0.0, 1.0, 1e-300))),
        ("axis_unit", mk(GP_POINT, (0.0, 1.0, 0.0))),
        ("far_axis_unit", mk(GP_FAR_POINT, (0.0, 1.0, 0.0))),
        ("far_oblique", mk(GP_FAR_POINT, unit)),
    ]


def ref_dot(a, b):
    """Vec3::dot in the reference's order, (x x' + y y') + z z' (vec3.h:61-63), on [n,3] arrays: numpy's elementwise double
    operations are the IEEE ones, without contraction."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def plane_terms(plane, org, dirs):
    """(numerator, denominator, len) of Plane::intersect (objects.h:506-507) in numpy, operation for operation"""
    n = np.asarray(plane.normal, np.float64)
    num = ref_dot(np.asarray(plane.position, np.float64) - org, n)
    den = ref_dot(dirs, n)
    with np.errstate(all="ignore"):
        return num, den, num / den


def _unit_rows(v):
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _uniform_dirs(rng, n):
    return _unit_rows(rng.normal(size=(n, 3)))


def _zero_component_dirs(rng, n):
    """unit directions with one (first half) or two (second half) components exactly +0.0 or -0.0"""
    d = _uniform_dirs(rng, n)
    k = rng.integers(0, 3, n)
    d[np.arange(n), k] = 0.0
    two = np.arange(n) >= n // 2
    k2 = (k + 1 + rng.integers(0, 2, n)) % 3
    d[np.nonzero(two)[0], k2[two]] = 0.0
    d = _unit_rows(d)  # x / sqrt(x * x) is exactly +-1 for the rows with one component left
    neg = rng.random((n, 3)) < 0.5
    return np.where((d == 0.0) & neg, -0.0, d)


def _normal_axis(plane):
    """the axis a plane's normal lies on (one non-zero component, whatever its length), or -1"""
    nz = [k for k in range(3) if plane.normal[k] != 0.0]
    return nz[0] if len(nz) == 1 else -1


def _in_plane_offsets(plane, rng, n):
    """Vectors v with v . normal == 0 exactly in the reference's order (candidates; the caller keeps the exact ones): for a normal
    on an axis every vector with that component zero; otherwise dyadic multiples (steps of 2^-10) of small integer vectors
    perpendicular to (1, 2, 3), the near-axis normals' zero components doing the rest."""
    ax = _normal_axis(plane)
    nrm = np.asarray(plane.normal, np.float64)
    if ax >= 0:
        v = rng.integers(-20 * 1024, 20 * 1024, (n, 3)) / 1024.0
        v[:, ax] = 0.0
        return v
    if abs(nrm[1] - 1.0) < 1e-5:  # near_axis: (1e-17, 1, 0) and (0, 1, 1e-300): the offset lies along the normal's exact zero
        v = np.zeros((n, 3))
        free = 2 if nrm[2] == 0.0 else 0
        v[:, free] = rng.integers(-20 * 1024, 20 * 1024, n) / 1024.0
        return v
    perp = np.array([(2, -1, 0), (3, 0, -1), (1, 1, -1), (0, 3, -2), (1, -2, 1), (4, 1, -2), (5, -1, -1), (2, 2, -2), (-1, 2, -1),
                     (7, -2, -1), (1, 4, -3), (6, 0, -2)], np.float64)
    pick = perp[rng.integers(0, len(perp), n)] * rng.choice([-1.0, 1.0], n)[:, None]
    return pick * (rng.integers(1, 4 * 1024, n) / 1024.0)[:, None]


def _parallel_dirs(plane, rng, n):
    """Unit directions with d . normal == 0 exactly (candidates): the normal's component set to zero for a normal on an axis;
    for the near-axis normals d_y = -fl(d_x n_x) resp. -fl(d_z n_z), which cancels the one non-zero product exactly; for
    (1, 2, 3) and its unit form normalised small-integer vectors such as (3, 0, -1) / sqrt(10)."""
    ax = _normal_axis(plane)
    nrm = np.asarray(plane.normal, np.float64)
    if ax >= 0:
        d = _uniform_dirs(rng, n)
        d[:, ax] = 0.0
        d = _unit_rows(d)
        return np.where((d == 0.0) & (rng.random((n, 3)) < 0.5), -0.0, d)
    if abs(nrm[1] - 1.0) < 1e-5:
        d = _uniform_dirs(rng, n)
        d[:, 1] = 0.0
        d = _unit_rows(d)
        d[:, 1] = -(d[:, 0] * nrm[0] + d[:, 2] * nrm[2])  # one of the two products is an exact zero
        return d
    return _unit_rows(_in_plane_offsets(plane, rng, n))


def _box_origins(rng, n, box=None):
    lo, hi = GP_BOX if box is None else box
    return rng.uniform(lo, hi, (n, 3))


def _exact_zero(plane, org, dirs):
    num, den, _ = plane_terms(plane, org, dirs)
    return num == 0.0, den == 0.0


def _interleave(zero_rays, other_rays, rng, waves=63):
    """Class (f): `waves` waves of 64 rays.  Wave 0 holds zero lanes only (numerator or denominator exactly zero); wave 1 one zero
    lane, at lane 0; wave 2 one, at lane 63; wave 3 both of these; every later wave a random number (1..63) of zero lanes at
    random places -- every wave mixes both kinds but the first."""
    zo, zd = zero_rays
    oo, od = other_rays
    org, dirs = np.empty((waves * 64, 3)), np.empty((waves * 64, 3))
    zi = oi = 0
    for w in range(waves):
        if w == 0:
            lanes = np.ones(64, bool)
        else:
            lanes = np.zeros(64, bool)
            if w == 1:
                lanes[0] = True
            elif w == 2:
                lanes[63] = True
            elif w == 3:
                lanes[[0, 63]] = True
            else:
                lanes[rng.permutation(64)[: rng.integers(1, 64)]] = True
        for lane in range(64):
            if lanes[lane]:
                org[w * 64 + lane], dirs[w * 64 + lane] = zo[zi % len(zo)], zd[zi % len(zo)]
                zi += 1
            else:
                org[w * 64 + lane], dirs[w * 64 + lane] = oo[oi % len(oo)], od[oi % len(oo)]
                oi += 1
    return org, dirs


def plane_ray_classes(plane, seed, n=4000, box=None):
    """{class: (org [m,3], dirs [m,3])} for one plane of general_planes(), seeded, unit directions, about n rays per class:
      a  origins in the 40-unit box GP_BOX (or `box`), uniform directions
      b  the same origins, directions with one or two components exactly zero (of either sign)
      c  directions exactly parallel to the plane: d . n == 0 exactly in the reference's order (only those are kept)
      d  origins exactly in the plane: (p - o) . n == 0 exactly (only those are kept)
      e  both: 0 / 0
      f  a..e interleaved wave by wave (_interleave)
      g  origins 1e6 and 1e8 away from the box, uniform directions
      h  (planes through GP_FAR_POINT only) exact distances within 8 ulps of 1e10 -- and of 1e9, plane_run's `unsure` threshold -- on
         both sides and on the value itself."""
    rng = np.random.default_rng(seed)
    far = tuple(plane.position) == GP_FAR_POINT
    p = np.asarray(plane.position, np.float64)
    out = {}
    out["a"] = (_box_origins(rng, n, box), _uniform_dirs(rng, n))
    out["b"] = (_box_origins(rng, n, box), _zero_component_dirs(rng, n))
    # c: keep the exactly parallel ones
    d = _parallel_dirs(plane, rng, 3 * n)
    o = _box_origins(rng, 3 * n, box)
    keep = _exact_zero(plane, o, d)[1]
    out["c"] = (o[keep][:n], d[keep][:n])
    # d: keep the origins exactly in the plane
    o = p - _in_plane_offsets(plane, rng, 3 * n)
    d = _uniform_dirs(rng, 3 * n)
    zn, zd = _exact_zero(plane, o, d)
    keep = zn & ~zd
    out["d"] = (o[keep][:n], d[keep][:n])
    # e: both
    o = p - _in_plane_offsets(plane, rng, 3 * n)
    d = _parallel_dirs(plane, rng, 3 * n)
    zn, zd = _exact_zero(plane, o, d)
    keep = zn & zd
    out["e"] = (o[keep][:n], d[keep][:n])
    # f: zero lanes from c, d and e in turn, the others from a and b
    m = min(len(out[k][0]) for k in "cde")
    zero = tuple(np.stack([out[k][i][:m] for k in "cde"], axis=1).reshape(-1, 3) for i in (0, 1))
    ao, ad = out["a"]
    bo, bd = out["b"]
    zn, zd = _exact_zero(plane, bo, bd)
    nz = ~(zn | zd)
    other = (np.concatenate([ao, bo[nz]]), np.concatenate([ad, bd[nz]]))
    out["f"] = _interleave(zero, other, rng)
    # g: far origins
    dist = np.where(np.arange(n) % 2 == 0, 1e6, 1e8)[:, None]
    out["g"] = (_box_origins(rng, n, box) + _uniform_dirs(rng, n) * dist, _uniform_dirs(rng, n))
    if far:
        out["h"] = _near_limit_rays(plane, rng, n)
    return out


def _near_limit_rays(plane, rng, n):
    """Class (h): for a target length L in {1e10, 1e9} take an origin (for 1e9: 2.5e9 below the box, so that a unit direction can
    reach the plane in 1e9), a direction whose component along the normal is num / (L |n|^2) and a random tangent, step that
    component through a few hundred neighbouring doubles, and keep the rays whose length -- evaluated in the reference's order --
    lies within 8 ulps of L: below it, on it and above it."""
    nrm = np.asarray(plane.normal, np.float64)
    nn = float(nrm @ nrm)
    orgs, dirs = [], []
    for L in (K_INF, 1e9):
        m = 40 * n
        o = _box_origins(rng, m)
        if L == 1e9:
            o[:, 1] -= 2.5e9
        num = ref_dot(np.asarray(plane.position, np.float64) - o, nrm)
        c = num / (L * nn) * (1.0 + rng.integers(-300, 301, m) * 2.0 ** -53)  # d = c n + s t, t a unit tangent
        t = np.cross(_uniform_dirs(rng, m), nrm)
        t = _unit_rows(t)
        s = np.sqrt(np.maximum(0.0, 1.0 - c * c * nn))
        d = c[:, None] * nrm + s[:, None] * t
        ln = plane_terms(plane, o, d)[2]
        ulp = np.spacing(L)
        keep = np.abs(ln - L) <= 8 * ulp
        orgs.append(o[keep][: n // 2])
        dirs.append(d[keep][: n // 2])
    return np.concatenate(orgs), np.concatenate(dirs)


# ---- rooms around the run of axis-aligned planes (cgrt_scene_walk.hpp plane_run) ------------------------------------------------
ROOM_COLOURS = [(0.9, 0.2, 0.2), (0.2, 0.9, 0.2), (0.2, 0.2, 0.9), (0.9, 0.9, 0.2), (0.2, 0.9, 0.9)]
ROOM_BOX = (np.array([-11.0, -11.0, -9.0]), np.array([11.0, 11.0, 13.0]))
RATIO_KS = (0.0, 2.0 ** -10, 0.25, 0.5, 0.9, 0.99, 0.999, 1.0, 1.001, 1.01, 1.1, 2.0)  # r - 1 = 2^-14 k
TILT_AXIS, TILT_ANGLE, TILT_PIVOT = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), 0.6, np.array([0.0, 0.0, 4.0])


def room_walls(scale=(1, 1, 1, 1, 1), mirror=2):
    """The room of test_gpu_parity.test_plane_group_test_edges_corners_and_degenerate_rays: floor y = -12, walls x = 12 and
    x = -12 (`mirror`: the index of the wall that reflects, or None), back wall z = 14, ceiling y = 12; open towards the
    camera.  scale[i] multiplies wall i's normal."""
    pos = [(0.0, -12.0, 0.0), (12.0, 0.0, 0.0), (-12.0, 0.0, 0.0), (0.0, 0.0, 14.0), (0.0, 12.0, 0.0)]
    nrm = [(0, 1, 0), (-1, 0, 0), (1, 0, 0), (0, 0, -1), (0, -1, 0)]
    return [Plane(pos[i], tuple(float(scale[i]) * c for c in nrm[i]), ROOM_COLOURS[i], 0.8 if i == mirror else 0.0, 0.0)
            for i in range(5)]


def tilt_matrix():
    """Rodrigues' rotation by TILT_ANGLE about TILT_AXIS"""
    k = TILT_AXIS
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(TILT_ANGLE) * K + (1 - np.cos(TILT_ANGLE)) * (K @ K)


def tilt_points(p):
    return (np.asarray(p, np.float64) - TILT_PIVOT) @ tilt_matrix().T + TILT_PIVOT


def hidden_vase():
    """The vase of main.cpp:371-376 behind the back wall z = 14: its presence selects the Bezier kernels, and no ray that starts
    in front of the wall reaches it first -- the Newton draws never decide a result."""
    cp = [(0, -10, 4), (0, 2, 4), (0, -2, 0), (0, 10, 2)]
    return Bezier(cp, (0.0, -1.9, 24.0), (1.0, 1.0, 1.0), 0.5, 0.0)


def ratio_sweep_room(k, swapped=False):
    """[floor y = -12, x = 12, x = -12, z = 14, floor y = -12 r] with r = 1 + 2^-14 k: all five in the run; `swapped` exchanges the
    two floors' places in the list.  The second floor is magenta."""
    r = 1.0 + 2.0 ** -14 * k
    w = room_walls(mirror=None)
    a, b = w[0], Plane((0.0, -12.0 * r, 0.0), (0, 1, 0), (1.0, 0.0, 1.0), 0.0, 0.0)
    return ([b] + w[1:4] + [a]) if swapped else ([a] + w[1:4] + [b])


def run_rooms():
    """{name: object list}: the multi-object scenes of the plane tests.  What each is for, and the run [prun_begin, prun_end) that
    scene_traits finds in it (asserted by tests/test_planes_general_host.py through tests/native/plane_runs.cpp)."""
    sphere = lambda c=(3.0, -4.0, 6.0), refl=0.0, transp=0.0: Sphere(c, 2.0, (0.7, 0.7, 0.7), refl, transp)
    rooms = {}
    # every wall rotated about an oblique axis: general form only, no run
    R = tilt_matrix()
    rooms["tilted_room"] = [Plane(tuple(tilt_points(p.position)), tuple(R @ np.asarray(p.normal)), p.surfaceColor, p.reflection, 0.0)
                            for p in room_walls()] + [sphere(tuple(tilt_points((3.0, -4.0, 6.0))))]
    # normals on the axes, none of unit length: general form, no run; the mirror wall and the glass sphere take them into
    # reflect / refract unnormalised
    rooms["nonunit_room"] = room_walls((2, 0.5, 3, 0.25, 7)) + [sphere(refl=0.8, transp=0.5)]
    # a general-form twin of the floor in front of the run ties with it on every floor-bound ray and, first in the list, wins
    front = Plane((0.0, -12.0, 0.0), (0, 2, 0), (1.0, 0.0, 1.0), 0.0, 0.0)
    rooms["front_tie_room"] = [front] + room_walls() + [sphere(), hidden_vase()]
    rooms["front_tie_room_no_vase"] = [front] + room_walls() + [sphere()]
    # an oblique plane cutting the corner (12, 12, 14) in front of the run: no exact ties
    cut = Plane((9.0, 9.0, 11.0), tuple(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)), (1.0, 0.0, 1.0), 0.0, 0.0)
    rooms["front_oblique_room"] = [cut] + room_walls() + [sphere(), hidden_vase()]
    # the run leads; behind it the floor's general-form twin and a sphere that touches the floor from above
    rooms["behind_tie_room"] = room_walls() + [front, Sphere((0.0, -10.0, 6.0), 2.0, (0.7, 0.7, 0.7), 0.0, 0.0)]
    # the same floor twice inside the run
    w = room_walls()
    rooms["twin_in_run"] = [w[0], Plane(w[0].position, w[0].normal, (1.0, 0.0, 1.0), 0.0, 0.0)] + w[1:] + [sphere()]
    # a transparent wall inside the run (the any-hit kernel may not use the run when transparent objects are skipped), the floor's
    # general-form twin and a glass sphere behind it
    w = room_walls(mirror=None)
    w[1] = Plane(w[1].position, w[1].normal, w[1].surfaceColor, 0.8, 0.5)
    rooms["glass_wall_room"] = w + [front, sphere(refl=0.8, transp=0.5)]
    # an opaque bump floor, then a non-unit ceiling, then a run of three walls; every plane diffuse and a mirror sphere, so a
    # scheduled frame has light tiles, whose launch walks height fields only (HFONLY)
    w = room_walls(mirror=None)
    bump = Plane((0.0, -12.0, 0.0), (0, 1, 0), ROOM_COLOURS[0], 0.0, 0.0, chessboard_texture(True))
    rooms["bump_front_room"] = [bump, Plane(w[4].position, (0, -2, 0), w[4].surfaceColor, 0.0, 0.0)] + w[1:4] + [sphere(refl=0.8)]
    for k in RATIO_KS:
        rooms["ratio_sweep_%g" % k] = ratio_sweep_room(k)
        rooms["ratio_sweep_%g_swapped" % k] = ratio_sweep_room(k, True)
    return rooms


# what scene_traits must find: name -> (prun_begin, prun_end, axis of every plane in list order; -1 = general form)
ROOM_RUNS = {
    "tilted_room": (0, 0, [-1] * 5),
    "nonunit_room": (0, 0, [-1] * 5),
    "front_tie_room": (1, 6, [-1, 1, 0, 0, 2, 1]),
    "front_tie_room_no_vase": (1, 6, [-1, 1, 0, 0, 2, 1]),
    "front_oblique_room": (1, 6, [-1, 1, 0, 0, 2, 1]),
    "behind_tie_room": (0, 5, [1, 0, 0, 2, 1, -1]),
    "twin_in_run": (0, 6, [1, 1, 0, 0, 2, 1]),
    "glass_wall_room": (0, 5, [1, 0, 0, 2, 1, -1]),
    "bump_front_room": (2, 5, [1, -1, 0, 0, 2]),
}
ROOM_RUNS.update({"ratio_sweep_%g%s" % (k, s): (0, 5, [1, 0, 0, 2, 1]) for k in RATIO_KS for s in ("", "_swapped")})


def mesh_behind_planes(replaced):
    """scene_pyramid(False) -- five planes, then an opaque mesh: the primary-walk kernel's scene -- with plane `replaced` given a
    normal of length two: replaced = 0 leaves a run behind a general-form plane, 2 leaves no run, 4 a run of four."""
    objs = scene_pyramid(False)
    p = objs[replaced]
    objs[replaced] = Plane(p.position, tuple(2.0 * c for c in p.normal), p.surfaceColor, 0.0, 0.0)
    return objs


MESH_RUNS = {0: (1, 5), 2: (0, 0), 4: (0, 4)}


def room_rays(seed, degenerate_plane, tilt=False, floor_origins=False, in_front=False):
    """At most 20 000 rays for a room of run_rooms(), in groups (name -> slice, returned beside org and dirs):
      degenerate  plane_ray_classes(degenerate_plane)["f"]: rays parallel to that plane, starting in it, or both, interleaved with
                  ordinary ones wave by wave; first, so that the waves are the call's
      random      origins in the room's interior, uniform directions
      axis        axis-parallel directions
      on_wall     origins exactly on a wall
      edges       aimed at points of the room's eight edges: two exact distances coincide or lie within a few ulps
      corners     aimed at its four corners: three
      near_edges  aimed beside an edge, so that the two walls' exact distances have a ratio between 1 + 2^-26 and 1 + 2^-12
      far         origins 0.9e9 .. 1.1e9 away, aimed into the room: approximate distances on both sides of plane_run's 1e9
      level       (floor_origins) origins with y = 0 exactly
    tilt: every ray is rotated with tilted_room's walls (the degenerate group is then nearly, no longer exactly, degenerate with
    respect to the rotated plane).
    in_front: no ray may pass behind the back wall z = 14, where scenes with hidden_vase() keep it: a ray that starts behind the
    wall is mirrored in z = 0 (origin and direction; y and so the floor's exact zeros are untouched), one that starts on it
    points to -z."""
    rng = np.random.default_rng(seed)
    lo, hi = ROOM_BOX
    groups, org, dirs = {}, [], []

    def add(name, o, d):
        at = sum(len(x) for x in org)
        groups[name] = slice(at, at + len(o))
        org.append(o)
        dirs.append(d)

    add("degenerate", *plane_ray_classes(degenerate_plane, seed, n=4000, box=ROOM_BOX)["f"])
    add("random", rng.uniform(lo, hi, (6000, 3)), _uniform_dirs(rng, 6000))
    ax = np.zeros((1500, 3))
    ax[np.arange(1500), rng.integers(0, 3, 1500)] = rng.choice([-1.0, 1.0], 1500)
    add("axis", rng.uniform(lo, hi, (1500, 3)), ax)
    on = rng.uniform(lo, hi, (1500, 3))
    wall = rng.integers(0, 5, 1500)
    coord = np.array([1, 0, 0, 2, 1])[wall]
    on[np.arange(1500), coord] = np.array([-12.0, 12.0, -12.0, 14.0, 12.0])[wall]
    add("on_wall", on, _uniform_dirs(rng, 1500))
    # edges: (x, y) in {+-12}^2 along z; (x = +-12, z = 14) along y; (y = +-12, z = 14) along x
    n = 2000
    pt = rng.uniform([-12.0, -12.0, -8.0], [12.0, 12.0, 14.0], (n, 3))
    kind = rng.integers(0, 3, n)
    sx, sy = rng.choice([-12.0, 12.0], n), rng.choice([-12.0, 12.0], n)
    pt[:, 0] = np.where(kind != 2, sx, pt[:, 0])
    pt[:, 1] = np.where(kind != 1, sy, pt[:, 1])
    pt[:, 2] = np.where(kind != 0, 14.0, pt[:, 2])
    o = np.round(rng.uniform(lo, hi, (n, 3)) * 8.0) / 8.0  # dyadic origins: the numerators are exact
    add("edges", o, _unit_rows(pt - o))
    n = 500
    pt = np.stack([rng.choice([-12.0, 12.0], n), rng.choice([-12.0, 12.0], n), np.full(n, 14.0)], axis=1)
    o = np.round(rng.uniform(lo, hi, (n, 3)) * 8.0) / 8.0
    add("corners", o, _unit_rows(pt - o))
    # beside the edges: aimed at a point of wall A such that wall B, on another axis, is r times as far, r - 1 log-uniform over
    # [2^-26, 2^-12] -- from the fp32 estimates' own error to four times plane_run's bound.  (Two planes on ONE axis share the
    # reciprocal, and rounding is monotone: their estimates can tie but never swap, so only a pair on two axes can show a bound
    # that trusts the estimates too early.)
    n = 2000
    o = np.round(rng.uniform(lo, hi, (n, 3)) * 8.0) / 8.0
    pt = rng.uniform([-11.0, -11.0, -8.0], [11.0, 11.0, 13.0], (n, 3))
    wall_c = np.array([[-12.0, 12.0], [-12.0, 12.0], [14.0, 14.0]])
    a = rng.integers(0, 3, n)
    b = (a + 1 + rng.integers(0, 2, n)) % 3
    rows = np.arange(n)
    pt[rows, a] = wall_c[a, rng.integers(0, 2, n)]
    cb = wall_c[b, rng.integers(0, 2, n)]
    r = 1.0 + 2.0 ** rng.uniform(-26.0, -12.0, n)
    pt[rows, b] = o[rows, b] + (cb - o[rows, b]) / r
    add("near_edges", o, _unit_rows(pt - o))
    n = 600
    d = _uniform_dirs(rng, n)
    add("far", rng.uniform(lo, hi, (n, 3)) - d * rng.uniform(0.9e9, 1.1e9, n)[:, None], d)
    if floor_origins:
        o = rng.uniform(lo, hi, (1500, 3))
        o[:, 1] = 0.0
        add("level", o, _uniform_dirs(rng, 1500))
    org, dirs = np.concatenate(org), np.concatenate(dirs)
    if tilt:
        org, dirs = tilt_points(org), dirs @ tilt_matrix().T
    if in_front:
        behind = org[:, 2] > 14.0
        org[behind, 2] *= -1.0
        dirs[behind, 2] *= -1.0
        on = (org[:, 2] == 14.0) & (dirs[:, 2] > 0)
        dirs[on, 2] *= -1.0
    assert len(org) <= 20000
    return np.ascontiguousarray(org), np.ascontiguousarray(dirs), groups


def behind_tie_rays():
    """behind_tie_room's own rays, all straight down: from (x, 0, 6) with x stepping in single doubles through +-2 -- the rim of the
    sphere (centre (0, -10, 6), radius 2), where its two roots meet --, and from inside the sphere on its vertical axis (dyadic
    heights: the sphere's far root and the floor's distance are both y0 + 12, exactly) and beside the axis.
    Returns (org, dirs, slice of the on-axis group)."""
    xs = 2.0 + np.arange(-8, 9) * np.spacing(2.0)
    org = [(s * x, 0.0, 6.0) for x in xs for s in (1.0, -1.0)] + [(0.0, 0.0, 6.0 + s * x) for x in xs for s in (1.0, -1.0)]
    first = len(org)
    ys = np.arange(-11.75, -8.0, 0.125)
    org += [(0.0, y, 6.0) for y in ys]
    last = len(org)
    org += [(dx, y, 6.0) for dx in (0.5, 1.0, -1.5) for y in ys[::3]]
    org = np.array(org, np.float64)
    return org, np.tile([0.0, -1.0, 0.0], (len(org), 1)), slice(first, last)


def textured_oblique_cases(n=3000, seed=5):
    """[(name, plane, points on it)] for getSurfaceColor on a textured oblique plane (texture.h:39-72).
      own_normal  the texture's normal is the plane's, (1, -2, 3) / sqrt(14): Texture::color projects P - position into the plane
                  and then asks for a component within 1e-2 of zero, so it returns false for most points.  A third of the
                  points lie beside the line d.x = 0 (d.y = 1.5 d.z: both positive, inside the rectangle or past its end), a third
                  beside d.z = 0 (d.x = 2 d.y), a third anywhere.  (With (1, 2, 3) no in-plane vector has one component zero and
                  the other two positive: the texel outcome could not occur.  Hence the sign.)
      up_normal   the texture's normal is (0, 1, 0) on the plane (1, 2, 3) / sqrt(14): the |d.y| branch, d.x and d.z measured
                  along the axes; points inside and outside the 20 x 20 rectangle."""
    rng = np.random.default_rng(seed)
    chess = load_asset("chessboard_rgb.npz")["rgb"]
    p0 = np.array(GP_POINT)
    n_own = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    own = Plane(GP_POINT, tuple(n_own), (0.4, 0.6, 0.8), 0.0, 0.0, Texture(chess, tuple(n_own), GP_POINT, 10, 10, False))
    m = n // 3
    dz, dx = rng.uniform(-1.0, 8.0, m), rng.uniform(-0.02, 0.02, m)
    beside_x = np.stack([dx, (dx + 3.0 * dz) / 2.0, dz], axis=1)
    dy, dz = rng.uniform(-1.0, 7.0, m), rng.uniform(-0.02, 0.02, m)
    beside_z = np.stack([2.0 * dy - 3.0 * dz, dy, dz], axis=1)
    e1, e2 = _unit_rows(np.array([[2.0, 1.0, 0.0]]))[0], _unit_rows(np.cross(n_own, [[2.0, 1.0, 0.0]]))[0]
    anywhere = rng.uniform(-15, 15, (n - 2 * m, 1)) * e1 + rng.uniform(-15, 15, (n - 2 * m, 1)) * e2
    pts_own = p0 + np.concatenate([beside_x, beside_z, anywhere])
    n_up = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    up = Plane(GP_POINT, tuple(n_up), (0.4, 0.6, 0.8), 0.0, 0.0, Texture(chess, (0, 1, 0), (-9.0, 0.0, 15.0), 20, 20, False))
    e1, e2 = _unit_rows(np.array([[2.0, -1.0, 0.0]]))[0], _unit_rows(np.cross(n_up, [[2.0, -1.0, 0.0]]))[0]
    pts_up = p0 + rng.uniform(-15, 15, (n, 1)) * e1 + rng.uniform(-15, 15, (n, 1)) * e2
    return [("own_normal", own, np.ascontiguousarray(pts_own)), ("up_normal", up, np.ascontiguousarray(pts_up))]


def bump_floor_plane():
    """The floor y = -12 with the chessboard as an opaque bump map (heights 0 on the black squares, 0.48 on the white ones)"""
    return Plane((0.0, -12.0, 0.0), (0, 1, 0), ROOM_COLOURS[0], 0.0, 0.0, chessboard_texture(True))


def bump_parallel_rays(seed, n=4000):
    """{class: (org, dirs)} for bump_floor_plane(): the one place where the SIGN of a plane's infinite length decides a result.
    A ray exactly parallel to the floor has len = num / (+-0); Plane::intersect consults the bump tree when len > 0, which +inf
    is, and a bump hit is nearer than +inf (objects.h:508-518).  The zero is the three-term sum (d.x * 0 + d.y * 1) + d.z * 0: -0 only
    when all three terms are -0, so for d.y = -0.0 with d.x or d.z positive it is +0 while d.y itself is -0 -- the one-subtraction
    form num / d.y has the other sign there.
      c  origins inside the layer of the bumps (y in (-12, -11.55)) and below the floor, directions (cos a, +-0.0, sin a)
      f  these interleaved wave by wave (_interleave) with rays from above that point down at the floor"""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-20.0, 0.0, 1.0], [20.0, 0.0, 39.0], (n, 3))
    u = rng.uniform(0.01, 0.45, n)
    o[:, 1] = np.where(np.arange(n) % 4 == 3, -12.0 - u, -12.0 + u)
    a = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(a), np.where(rng.random(n) < 0.5, -0.0, 0.0), np.sin(a)], axis=1)
    oo = rng.uniform([-20.0, -11.0, 1.0], [20.0, 5.0, 39.0], (n, 3))
    od = _unit_rows(rng.uniform([-20.0, -12.0, 1.0], [20.0, -12.0, 39.0], (n, 3)) - oo)
    return {"c": (o, d), "f": _interleave((o, d), (oo, od), rng)}
