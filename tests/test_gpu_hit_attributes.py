"""Hit attributes of caller-supplied rays on the GPU (cgrt_ray_hit_attributes): triangle index, barycentrics, surface colour
and material behind a nearest-hit query.

The check is bit for bit.  numpy restates Triangle::intersect (objects.h:96-111) with the determinant association of
vec3.h:95-97, operation by operation in IEEE double: det2/det1 of the reported triangle must BE the query's hit_t,
(det3/det1, det4/det1) must BE uv, and normalize((pa-pb) x (pa-pc)) the query's normal up to sign.  Where the triangle count
allows, a brute force over every triangle of the object confirms that the reported one is a nearest one (a tie passes by
membership).  Rays per scene: a 64x48 pinhole frame plus 4 096 seeded random rays aimed at the objects under test."""
import numpy as np
import pytest

import scenes
from cgraytracing_amd.scene import TriangleMesh

pytestmark = pytest.mark.gpu

ROOM_LO, ROOM_HI = np.array([-19.0, -19.0, -9.0]), np.array([19.0, 19.0, 38.0])
ROOM_BOX = (np.array([-20.0, -20.0, 0.0]), np.array([20.0, 20.0, 40.0]))
FLOOR_BOX = (np.array([-20.0, -20.0, -9.0]), np.array([20.0, -20.0, 40.0]))  # z < 0: the flat part beyond the bump texture
INF = 1e10  # main.cpp:25


# ---- the reference's triangle arithmetic in numpy ------------------------------------------------------------------------
def _det(a, b, c):
    """vec3.h:95-97, the same products and the same left-to-right sum."""
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
    return ax * by * cz + bx * cy * az + cx * ay * bz - ax * cy * bz - bx * ay * cz - cx * by * az


def tri_eval(org, dirs, tri9):
    """Triangle::intersect for broadcastable (org, dirs, tri9): (t, u, v, accepted)."""
    pa, pb, pc = tri9[..., 0:3], tri9[..., 3:6], tri9[..., 6:9]
    e1, e2, s = pa - pb, pa - pc, pa - org
    det1, det2, det3, det4 = _det(dirs, e1, e2), _det(s, e1, e2), _det(dirs, s, e2), _det(dirs, e1, s)
    with np.errstate(all="ignore"):
        t, u, v, w = det2 / det1, det3 / det1, det4 / det1, (det3 + det4) / det1
        ok = (det1 != 0.0) & (t > 0.0) & (u >= 0.0) & (v >= 0.0) & (w <= 1.0) & (t < INF)  # the four acceptance tests
    return t, u, v, ok


def tri_normal(tri9):
    """((pa - pb).cross(pa - pc)).normalize(), objects.h:107, vec3.h:35-44,80-83."""
    pa, pb, pc = tri9[..., 0:3], tri9[..., 3:6], tri9[..., 6:9]
    a, b = pa - pb, pa - pc
    x = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    y = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    z = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    r = 1 / np.sqrt(x * x + y * y + z * z)
    return np.stack([x * r, y * r, z * r], axis=-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def brute_nearest(org, dirs, tri9, flat=False, chunk=256):
    """min over ALL triangles of the accepted det2/det1 per ray; INF where none is hit.

    Every (ray, triangle) pair is looked at by a first pass that only drops pairs which cannot be a hit; the pairs it keeps
    get tri_eval's exact arithmetic, which alone decides.
    General meshes: the first pass evaluates the four determinants as matrix products (det(a,b,c) = a . (b x c), split into
    per-ray and per-triangle factors) and keeps the pairs that pass the acceptance tests with 1e-4 to spare in u, v and
    u + v, and every pair whose ray is within 1e-5 of the triangle's plane, where that pass cannot be trusted; its error
    elsewhere is ~1e-12 / (1e-5 * edge length), far inside the margin for the meshes used here.
    flat=True (a bump floor: 20 k triangles within half a unit of height): a hit point lies inside its triangle, so it lies
    between the mesh's lowest and highest vertex and over the triangle's x-z box; the first pass keeps the pairs whose
    triangle's x-z box (grown by 1e-6) meets the x-z box of the part of the ray that runs between those heights (t <= 1e4)."""
    pa, pb, pc = tri9[:, 0:3], tri9[:, 3:6], tri9[:, 6:9]
    e1, e2 = pa - pb, pa - pc
    best = np.full(len(org), INF)
    if flat:
        v = tri9.reshape(-1, 3, 3)
        lo, hi = v.min(axis=1) - 1e-6, v.max(axis=1) + 1e-6
        ylo, yhi = lo[:, 1].min(), hi[:, 1].max()
    else:
        N, A, B = _cross(e1, e2), _cross(pa, e2), _cross(e1, pa)
        paN, normN = (pa * N).sum(axis=1), np.sqrt((N * N).sum(axis=1))
    for k in range(0, len(org), chunk):
        o, d = org[k:k + chunk], dirs[k:k + chunk]
        with np.errstate(all="ignore"):
            if flat:
                level = d[:, 1] == 0.0
                t1 = np.where(level, 0.0, (ylo - o[:, 1]) / d[:, 1])
                t2 = np.where(level, np.where((o[:, 1] >= ylo) & (o[:, 1] <= yhi), 1e4, -1.0), (yhi - o[:, 1]) / d[:, 1])
                ta, tb = np.clip(np.minimum(t1, t2), 0.0, 1e4), np.clip(np.maximum(t1, t2), -1.0, 1e4)
                xa, xb, za, zb = o[:, 0] + d[:, 0] * ta, o[:, 0] + d[:, 0] * tb, o[:, 2] + d[:, 2] * ta, o[:, 2] + d[:, 2] * tb
                cand = ((ta <= tb)[:, None] & (hi[None, :, 0] >= np.minimum(xa, xb)[:, None]) & (lo[None, :, 0] <= np.maximum(xa, xb)[:, None]) &
                        (hi[None, :, 2] >= np.minimum(za, zb)[:, None]) & (lo[None, :, 2] <= np.maximum(za, zb)[:, None]))
            else:
                q = _cross(d, o)
                det1 = d @ N.T
                det2 = paN[None, :] - o @ N.T
                det3 = d @ A.T - q @ e2.T
                det4 = d @ B.T + q @ e1.T
                t, u, w = det2 / det1, det3 / det1, det4 / det1
                cand = (np.abs(det1) <= 1e-5 * normN[None, :]) | ((t > -1e-4) & (u >= -1e-4) & (w >= -1e-4) & (u + w <= 1 + 1e-4))
        ri, ti = np.nonzero(cand)
        te, _, _, ok = tri_eval(o[ri], d[ri], tri9[ti])
        np.minimum.at(best, k + ri[ok], te[ok])
    return best


# ---- rays and runs -------------------------------------------------------------------------------------------------------
def aimed_rays(boxes, seed, n=4096):
    """n rays from the room's interior, each towards a uniform point of one of `boxes` picked per ray (so the rays of one wave
    go for different objects)."""
    rng = np.random.default_rng(seed)
    org = rng.uniform(ROOM_LO, ROOM_HI, (n, 3))
    which = rng.integers(0, len(boxes), n)
    lo, hi = np.array([b[0] for b in boxes])[which], np.array([b[1] for b in boxes])[which]
    v = rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo) + lo - org
    return org, v / np.sqrt((v * v).sum(axis=1))[:, None]


def miss_rays(walls, seed, n=64):
    """Rays built to miss everything, as tests/test_gpu_rays.py::random_rays builds them."""
    rng = np.random.default_rng(seed)
    if walls == "planes":
        return rng.uniform([-19.0, -15.0, -9.0], [19.0, 19.0, 5.0], (n, 3)), np.tile([0.0, 0.0, -1.0], (n, 1))
    th, ph = np.radians(rng.uniform(0, 2.0, n)), rng.uniform(0, 2 * np.pi, n)
    return (rng.uniform([-10.0, -10.0, -60.0], [10.0, 10.0, -20.0], (n, 3)),
            np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], axis=1))


def bbox(tri9):
    v = tri9.reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


def make_rays(sc, boxes, seed, misses=None):
    co, cd, _ = sc.camera_rays(64, 48, 1, scenes.cam_pinhole())
    parts = [(co.cpu().numpy(), cd.cpu().numpy()), aimed_rays(boxes, seed)]
    if misses:
        parts.append(miss_rays(misses, seed + 1))
    return (np.ascontiguousarray(np.concatenate([p[0] for p in parts])),
            np.ascontiguousarray(np.concatenate([p[1] for p in parts])))


def query(sc, org, dirs, **kw):
    """(hit, attr) as numpy dicts: trace_rays(want=("hit",)) and hit_attributes on its answers."""
    import torch

    dev = torch.device("cuda", sc.device)
    to, td = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
    hit = sc.trace_rays(to, td, want=("hit",))
    attr = sc.hit_attributes(to, td, hit["hit_obj"], hit["hit_t"], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in hit.items()}, {k: v.cpu().numpy() for k, v in attr.items()}


# ---- checks --------------------------------------------------------------------------------------------------------------
def check_triangle_hits(org, dirs, hit, attr, sel, tri9, brute):
    """Rays `sel` hit a triangle of tri9 (construction order): the reported one reproduces hit_t, uv and the normal."""
    o, d, p = org[sel], dirs[sel], attr["prim"][sel]
    assert len(p) > 0
    assert (p >= 0).all() and (p < len(tri9)).all(), (int(p.min()), int(p.max()), len(tri9))
    t, u, v, ok = tri_eval(o, d, tri9[p])
    assert ok.all(), "the reported triangle fails an acceptance test on %d rays" % int((~ok).sum())
    assert np.array_equal(t, hit["hit_t"][sel])
    assert np.array_equal(np.stack([u, v], axis=1), attr["uv"][sel])
    n, got = tri_normal(tri9[p]), hit["hit_normal"][sel]
    assert ((got == n).all(axis=1) | (got == -n).all(axis=1)).all()
    if brute:  # the reported triangle is one of the nearest: its t is the minimum over all of them
        assert np.array_equal(brute_nearest(o, d, tri9), hit["hit_t"][sel])


def check_no_triangle(attr, sel):
    assert (attr["prim"][sel] == -1).all() and (attr["uv"][sel] == 0.0).all()


def check_color_material(sc, objs, org, dirs, hit, attr):
    """color == Scene.surface_colors(obj, P) per object, P = org + dirs * hit_t in numpy; material == the constructor's values;
    zeros on a miss."""
    obj, P = hit["hit_obj"], org + dirs * hit["hit_t"][:, None]
    mats = np.array([[o.reflection, o.transparency] for o in objs], np.float64)
    for i in np.unique(obj[obj >= 0]):
        sel = obj == i
        assert np.array_equal(attr["color"][sel], sc.surface_colors(int(i), P[sel])), i
        assert np.array_equal(attr["material"][sel], np.tile(mats[i], (int(sel.sum()), 1))), i
    miss = obj < 0
    assert (attr["color"][miss] == 0.0).all() and (attr["material"][miss] == 0.0).all()
    assert (attr["prim"][miss] == -1).all() and (attr["uv"][miss] == 0.0).all()


def mesh(tri9, glass, color=(0.6, 0.7, 0.9)):
    return TriangleMesh.from_triangles(tri9, color, 0.8 if glass else 0.0, 0.5 if glass else 0.0)


# ---- test 1: small meshes ------------------------------------------------------------------------------------------------
SMALL = [("pyramid_opaque", scenes.pyramid_tris, False, None), ("pyramid_glass", scenes.pyramid_tris, True, None),
         ("bunny_glass", scenes.bunny_tris, True, None), ("bunny_opaque", scenes.bunny_tris, False, None),
         ("pyramid_opaque_device", scenes.pyramid_tris, False, "device"), ("bunny_opaque_device", scenes.bunny_tris, False, "device")]


@pytest.mark.parametrize("name,tris,glass,build", SMALL, ids=[c[0] for c in SMALL])
def test_small_meshes(gpu_ready, name, tris, glass, build):
    import cgraytracing_amd as cg

    tri9 = tris()
    objs = scenes.planes(scenes.chessboard_texture(False)) + [mesh(tri9, glass)]
    m = len(objs) - 1
    with cg.Scene(objs, build=build) as sc:
        org, dirs = make_rays(sc, [bbox(tri9)], 101)
        hit, attr = query(sc, org, dirs)
        check_color_material(sc, objs, org, dirs, hit, attr)
    on = hit["hit_obj"] == m
    print("%s: %d of %d rays hit the mesh" % (name, int(on.sum()), len(on)))
    assert on.sum() > 1000
    check_triangle_hits(org, dirs, hit, attr, on, tri9, brute=True)
    check_no_triangle(attr, ~on)


# ---- test 2: the dragon (opaque, 4-wide walk, 100 k triangles) --------------------------------------------------------------
def test_dragon(gpu_ready):
    import cgraytracing_amd as cg

    tri9 = scenes.dragon_tris()
    objs = scenes.scene_dragon()
    m = len(objs) - 1
    with cg.Scene(objs) as sc:
        org, dirs = make_rays(sc, [bbox(tri9)], 202)
        hit, attr = query(sc, org, dirs)
        check_color_material(sc, objs, org, dirs, hit, attr)
    on = hit["hit_obj"] == m
    print("dragon: %d of %d rays hit the mesh" % (int(on.sum()), len(on)))
    assert on.sum() > 1000
    check_triangle_hits(org, dirs, hit, attr, on, tri9, brute=False)  # hit_t is pinned against the oracle elsewhere
    check_no_triangle(attr, ~on)


# ---- test 3: bump floors ---------------------------------------------------------------------------------------------------
def check_cells(tex, org, dirs, hit, attr, sel):
    """prim // 2 is the cell (row i along z, column j along x, objects.h:486-497) whose footprint holds P's (x, z), to 1e-9
    cell pitches (the project's fp64 position bar)."""
    rows, cols = tex.data.shape[0], tex.data.shape[1]
    nxc, nzc = cols // 3 - 1, rows // 3 - 1
    P = org[sel] + dirs[sel] * hit["hit_t"][sel][:, None]
    cell = attr["prim"][sel] // 2
    assert (attr["prim"][sel] >= 0).all() and (cell < nxc * nzc).all()
    i, j = cell // nxc, cell % nxc
    fx = (P[:, 0] - tex.position[0]) / (tex.lenx * 3 / cols)
    fz = (P[:, 2] - tex.position[2]) / (tex.leny * 3 / rows)
    assert ((fx >= j - 1e-9) & (fx <= j + 1 + 1e-9)).all()
    assert ((fz >= i - 1e-9) & (fz <= i + 1 + 1e-9)).all()


def _chess_bump_scene():
    return scenes.planes(scenes.chessboard_texture(True))


BUMP = [("chess_opaque_hfield", _chess_bump_scene), ("chess_glass_tree", scenes.scene_glass_bump_floor)]


@pytest.mark.parametrize("name,mk", BUMP, ids=[c[0] for c in BUMP])
def test_bump_floors(gpu_ready, name, mk):
    import cgraytracing_amd as cg

    objs = mk()
    with cg.Scene(objs) as sc:
        tri9 = sc.tree_dump(0)[3]
        org, dirs = make_rays(sc, [FLOOR_BOX], 303)
        hit, attr = query(sc, org, dirs)
        check_color_material(sc, objs, org, dirs, hit, attr)
    tex = objs[0].texture
    assert len(tri9) == 2 * (tex.data.shape[1] // 3 - 1) * (tex.data.shape[0] // 3 - 1)
    floor = np.nonzero(hit["hit_obj"] == 0)[0]
    near = brute_nearest(org[floor], dirs[floor], tri9, flat=True)
    bump = np.zeros(len(org), bool)
    bump[floor] = near == hit["hit_t"][floor]
    print("%s: %d rays on the floor, %d of them on the displacement mesh" % (name, len(floor), int(bump.sum())))
    assert bump.sum() > 1000 and (~bump[floor]).sum() > 50
    assert np.array_equal(attr["prim"] >= 0, bump)  # exactly where the brute force has a hit with t == hit_t
    check_triangle_hits(org, dirs, hit, attr, bump, tri9, brute=False)  # (the brute force is `near` above)
    check_no_triangle(attr, ~bump)  # the flat part and the walls
    check_cells(tex, org, dirs, hit, attr, bump)


def test_bump_floor_device_built(gpu_ready):
    """No reference vertices here (the heights come from the device's own exp): range, barycentric range and the cell."""
    import cgraytracing_amd as cg

    objs = _chess_bump_scene()
    with cg.Scene(objs, build="device") as sc:
        assert sc.build_info()["n_device_trees"] == 1
        org, dirs = make_rays(sc, [FLOOR_BOX], 303)
        hit, attr = query(sc, org, dirs)
        check_color_material(sc, objs, org, dirs, hit, attr)
    bump = attr["prim"] >= 0
    print("device-built chess floor: %d rays on the displacement mesh" % int(bump.sum()))
    assert bump.sum() > 1000 and (hit["hit_obj"][bump] == 0).all()
    u, v = attr["uv"][bump, 0], attr["uv"][bump, 1]
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1).all()
    check_no_triangle(attr, ~bump)
    check_cells(objs[0].texture, org, dirs, hit, attr, bump)


# ---- test 4: colour and material -------------------------------------------------------------------------------------------
COLOR = [("textured_walls", scenes.scene_textured_walls, "planes"), ("c2", scenes.scene_c2, "spheres"),
         ("chess_floor", lambda: scenes.scene_c3(True), "planes")]


@pytest.mark.parametrize("name,mk,walls", COLOR, ids=[c[0] for c in COLOR])
def test_color_and_material(gpu_ready, name, mk, walls):
    import cgraytracing_amd as cg

    objs = mk()
    with cg.Scene(objs) as sc:
        org, dirs = make_rays(sc, [ROOM_BOX], 404, misses=walls)
        hit, attr = query(sc, org, dirs)
        check_color_material(sc, objs, org, dirs, hit, attr)
    seen = np.unique(hit["hit_obj"])
    print("%s: objects hit %s, misses %d" % (name, seen.tolist(), int((hit["hit_obj"] < 0).sum())))
    hidden = {5} if name == "c2" else set()  # C2's diffuse sphere (z = 50 .. 70) lies behind the back wall (z = 40)
    assert (hit["hit_obj"] < 0).sum() >= 64 and set(seen.tolist()) == set(range(-1, len(objs))) - hidden  # every object, and the misses
    if name != "chess_floor":
        check_no_triangle(attr, np.ones(len(org), bool))
    if name != "c2":  # Texture::color really was in play: colours that are not the flat one
        floor = hit["hit_obj"] == 0
        assert (attr["color"][floor] != np.asarray(objs[0].surfaceColor)).any()


# ---- test 5: more objects than the LDS list holds --------------------------------------------------------------------------
def test_beyond_the_lds_list(gpu_ready):
    import cgraytracing_amd as cg

    tri9 = scenes.pyramid_tris()
    objs = scenes.room_with_objects(906, 5, mesh=mesh(tri9, False))  # 5 planes, the pyramid, 900 spheres
    with cg.Scene(objs) as sc:
        org, dirs = make_rays(sc, [bbox(tri9), ROOM_BOX], 505)
        hit, attr = query(sc, org, dirs)
        check_color_material(sc, objs, org, dirs, hit, attr)
    on, late = hit["hit_obj"] == 5, hit["hit_obj"] > 768
    print("906 objects: %d mesh hits, %d hits on objects above 768 (%d distinct)" %
          (int(on.sum()), int(late.sum()), len(np.unique(hit["hit_obj"][late]))))
    assert on.sum() > 100 and late.sum() > 100
    check_triangle_hits(org, dirs, hit, attr, on, tri9, brute=True)
    check_no_triangle(attr, ~on)


# ---- tests 6 and 7 share one scene: two meshes and a bump floor ------------------------------------------------------------
def _three_trees():
    """(objs, [(object index, tri9 or None)], boxes): an opaque bump floor (height-field walk), an opaque pyramid (4-wide walk)
    and a glass bunny (leaf-queue walk); the rays of a wave go for all three."""
    pyr, bun = scenes.pyramid_tris(1.0, (-9.0, -5.0, 22.0)), scenes.bunny_tris()
    objs = _chess_bump_scene() + [mesh(pyr, False), mesh(bun, True, (1.0, 1.0, 1.0))]
    return objs, pyr, bun


_SHARED = {}


def _three_trees_run():
    """The scene's rays and the full call's answers, computed once."""
    import cgraytracing_amd as cg

    if "run" not in _SHARED:
        objs, pyr, bun = _three_trees()
        with cg.Scene(objs) as sc:
            floor9 = sc.tree_dump(0)[3]
            org, dirs = make_rays(sc, [FLOOR_BOX, bbox(pyr), bbox(bun)], 606, misses="planes")
            hit, attr = query(sc, org, dirs)
            check_color_material(sc, objs, org, dirs, hit, attr)
        for a in list(hit.values()) + list(attr.values()) + [org, dirs]:
            a.setflags(write=False)
        _SHARED["run"] = (objs, pyr, bun, floor9, org, dirs, hit, attr)
    return _SHARED["run"]


def test_two_meshes_and_a_bump_floor(gpu_ready):
    objs, pyr, bun, floor9, org, dirs, hit, attr = _three_trees_run()
    obj = hit["hit_obj"]
    on_pyr, on_bun, floor = obj == 5, obj == 6, np.nonzero(obj == 0)[0]
    bump = np.zeros(len(org), bool)
    bump[floor] = brute_nearest(org[floor], dirs[floor], floor9, flat=True) == hit["hit_t"][floor]
    # waves (64 consecutive rays) that hold hits on all three trees: the one-tree-at-a-time loop really runs three rounds
    n64 = len(org) // 64 * 64
    mixed = (on_pyr[:n64].reshape(-1, 64).any(axis=1) & on_bun[:n64].reshape(-1, 64).any(axis=1) & bump[:n64].reshape(-1, 64).any(axis=1))
    print("pyramid %d, bunny %d, bump floor %d hits; waves with all three: %d" %
          (int(on_pyr.sum()), int(on_bun.sum()), int(bump.sum()), int(mixed.sum())))
    assert on_pyr.sum() > 300 and on_bun.sum() > 300 and bump.sum() > 300 and mixed.sum() >= 16
    check_triangle_hits(org, dirs, hit, attr, on_pyr, pyr, brute=True)
    check_triangle_hits(org, dirs, hit, attr, on_bun, bun, brute=True)
    check_triangle_hits(org, dirs, hit, attr, bump, floor9, brute=False)
    check_cells(objs[0].texture, org, dirs, hit, attr, bump)
    check_no_triangle(attr, ~(on_pyr | on_bun | bump))


def test_schedule_independence_and_partial_output(gpu_ready):
    import cgraytracing_amd as cg
    import torch

    objs, pyr, bun, floor9, org, dirs, hit, attr = _three_trees_run()
    n = len(org)
    names = ("prim", "uv", "color", "material")
    with cg.Scene(objs) as sc:
        dev = torch.device("cuda", sc.device)
        to, td = torch.from_numpy(org.copy()).to(dev), torch.from_numpy(dirs.copy()).to(dev)
        tobj, tt = torch.from_numpy(hit["hit_obj"].copy()).to(dev), torch.from_numpy(hit["hit_t"].copy()).to(dev)

        def run(o=to, d=td, ho=tobj, ht=tt, **kw):
            res = sc.hit_attributes(o, d, ho, ht, **kw)
            torch.cuda.synchronize()
            return res

        # a fresh handle gives the first run's bits again
        full = run()
        assert sorted(full) == sorted(names)
        for k in names:
            assert np.array_equal(full[k].cpu().numpy(), attr[k]), k
        # one array alone: the bits of the full call, and nothing else is returned
        for w in ("prim", "uv", "color", "material"):
            res = run(want=(w,))
            assert list(res) == [w] and np.array_equal(res[w].cpu().numpy(), attr[w]), w
        # permuted rays give permuted results
        perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
        res = run(to[perm].contiguous(), td[perm].contiguous(), tobj[perm].contiguous(), tt[perm].contiguous())
        for k in names:
            assert np.array_equal(res[k].cpu().numpy(), attr[k][perm.cpu().numpy()]), k
        # out= tensors are written in place
        out = dict(prim=torch.full((n,), 77, dtype=torch.int32, device=dev), uv=torch.full((n, 2), 7.0, dtype=torch.float64, device=dev),
                   color=torch.full((n, 3), 7.0, dtype=torch.float64, device=dev),
                   material=torch.full((n, 2), 7.0, dtype=torch.float64, device=dev))
        res = run(out=out)
        for k in names:
            assert res[k] is out[k] and np.array_equal(out[k].cpu().numpy(), attr[k]), k
        with pytest.raises(ValueError):
            sc.hit_attributes(to, td, tobj, tt, out=dict(prim=out["prim"][:-1]))
        # a stream of the caller's
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            res = sc.hit_attributes(to, td, tobj, tt)
        side.synchronize()
        for k in names:
            assert np.array_equal(res[k].cpu().numpy(), attr[k]), k
        res = sc.hit_attributes(to, td, tobj, tt, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(res["prim"].cpu().numpy(), attr["prim"])
        # no rays; a last wave with one live ray
        res = run(to[:0], td[:0], tobj[:0], tt[:0])
        assert [tuple(res[k].shape) for k in names] == [(0,), (0, 2), (0, 3), (0, 2)]
        res = run(to[:4097], td[:4097], tobj[:4097], tt[:4097])
        for k in names:
            assert np.array_equal(res[k].cpu().numpy(), attr[k][:4097]), k
        # the host form on numpy arrays
        host = sc.hit_attributes_host(org[:700], dirs[:700], hit["hit_obj"][:700], hit["hit_t"][:700])
        for k in names:
            assert np.array_equal(host[k], attr[k][:700]), k
        # distances that are not the query's (one ulp off) and objects that do not exist: no triangle, on those rays only
        tri = np.nonzero(attr["prim"] >= 0)[0]
        pick = np.concatenate([tri[hit["hit_obj"][tri] == i][:8] for i in (0, 5, 6)])
        assert len(pick) == 24
        t2 = hit["hit_t"].copy()
        t2[pick[0::2]] = np.nextafter(t2[pick[0::2]], np.inf)
        t2[pick[1::2]] = np.nextafter(t2[pick[1::2]], 0.0)
        res = run(ht=torch.from_numpy(t2).to(dev), want=("prim", "uv"))
        want_prim, want_uv = attr["prim"].copy(), attr["uv"].copy()
        want_prim[pick], want_uv[pick] = -1, 0.0
        assert np.array_equal(res["prim"].cpu().numpy(), want_prim) and np.array_equal(res["uv"].cpu().numpy(), want_uv)
        o2 = hit["hit_obj"].copy()
        gone = np.concatenate([pick, np.nonzero(attr["prim"] < 0)[0][:8]])
        o2[gone[0::2]], o2[gone[1::2]] = len(objs), -7
        res = run(ho=torch.from_numpy(o2).to(dev))
        for k in names:
            got, want = res[k].cpu().numpy(), attr[k].copy()
            want[gone] = -1 if k == "prim" else 0.0
            assert np.array_equal(got, want), k
        # the table behind prim belongs to the handle and is counted once it exists
        assert sc.stats()["device_bytes"] > 0


def test_table_is_built_on_the_first_call_that_asks(gpu_ready):
    """A scene that never asks for prim keeps the device bytes of its commit; the first call that asks adds 4 bytes per triangle."""
    import cgraytracing_amd as cg

    objs, pyr, bun, floor9, org, dirs, hit, attr = _three_trees_run()
    o, d, ho, ht = org[:256], dirs[:256], hit["hit_obj"][:256], hit["hit_t"][:256]
    with cg.Scene(objs) as sc:
        before = sc.stats()["device_bytes"]
        res = sc.hit_attributes_host(o, d, ho, ht, want=("uv", "color", "material"))
        assert sc.stats()["device_bytes"] == before
        assert np.array_equal(res["uv"], attr["uv"][:256])
        res = sc.hit_attributes_host(o, d, ho, ht, want=("prim",))
        assert np.array_equal(res["prim"], attr["prim"][:256])
        after = sc.stats()["device_bytes"]
        assert after - before == 4 * (len(pyr) + len(bun) + len(floor9))
        sc.hit_attributes_host(o, d, ho, ht)
        assert sc.stats()["device_bytes"] == after
