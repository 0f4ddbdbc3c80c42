"""Designed inputs for the photon gather (cgrt_ppm_table.hpp, photon_pairs_kernel, photon_apply_kernel) and the numpy replay
they are checked against.  A helper, not a test module.

The replay: replay_expected() is main.cpp:103-125 and 252-258 over arbitrary Hitpoint records and photon events, with the
reference's table (hash.h:20-42), cell walk and update, operation for operation in IEEE doubles.

The design: two diffuse planes -- a floor y = -20 with normal (0, 1, 0) and a back wall z = 40 with normal (0, 0, -1) -- and
photons of depth 1 that fly along (0, -1, 0) from y = 10 or along (0, 0, 1) from z = 0, so that a photon lands exactly at its
origin's (x, z) resp. (x, y).  The events every class is built on are the ORACLE's (oracle_photon_events), asserted equal to
the intended landing spots before anything depends on that.  Hitpoint records and photons are placed class by class where
the gather makes a decision:

  A  a record on either side of the first radius: the last position inside and the first outside, adjacent doubles along a
     random in-plane direction, found by bisection on the reference's own expression; for r0 = 0.25 also exact equality
  B  a record at an earlier photon's landing spot and a later photon on either side of the SECOND radius fl(r0^2 g0), or
     between the two radii; the two photons in one batch of 64 or in two
  C  record normals at the threshold of n . n' > 1e-4
  D  a record two cells away from its photon and inside the radius (cells are shorter than r0): the reference does not count
     it; and the same distance one cell away, which it does count
  E  landing spots and records outside the 70^3 box of the hash grid: negative cell indices and indices above 1023
  F  197 photons and 48 records in one hash cell: a whole wave of 64 events with 48 pairs each, more than its 768-entry
     buffer holds
  G  is A-D again under hashsize 7 and 101 (design(classes="ABCD"))

Landing spots of different sites are at least 1.0 apart, so a record meets only the photons of its own site."""
import math

import numpy as np

EPS = 1e-4               # main.cpp:24
PI_REF = 3.14159265358979  # main.cpp:26
R0_DEFAULT = 200.0 / 768  # main.cpp:84 with the reference's compile-time height
HASHSIZE_DEFAULT = 1000001
ALPHA_DEFAULT = 0.7
ORIGIN = (-35.0, -35.0, -15.0)  # hash.h: XMIN, YMIN, ZMIN
SIZE_OF_SCENE = 70.0
FLOOR_Y, WALL_Z = -20.0, 40.0
N_FLOOR, N_WALL = (0.0, 1.0, 0.0), (0.0, 0.0, -1.0)
SEED = 5  # of design(); tests/test_photon_gather_host.py checks that it has every property the classes promise
WIDTH, ROWS = 16, 12  # the image the designed records gather into
BATCH_SMALL = 64


# ---- the replay: main.cpp:103-125 and 252-258 over arbitrary records -------------------------------------------------
def cell_length(r0):  # hash.h:25-26
    return SIZE_OF_SCENE / math.ceil(SIZE_OF_SCENE / r0)


def hash_np(ix, iy, iz, hashsize=HASHSIZE_DEFAULT):  # hash.h:35-37, wrapping 32-bit products
    m = 0xFFFFFFFF
    return ((((ix & m) * 73856093) & m) ^ (((iy & m) * 19349663) & m) ^ (((iz & m) * 83492791) & m)) % hashsize


def coord_np(P, cl):  # hash.h:38-42
    return [np.floor((P[:, k] - off) / cl).astype(np.int64) for k, off in enumerate(ORIGIN)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _bits(path):
    """the path's bits behind its leading 1 as text: Python compares strings lexicographically, a prefix first"""
    return bin(int(path))[3:]


_VECTOR_FROM = 8  # buckets of at least this many records are screened with numpy before the serial loop


def replay_expected(ray, path, hp9, texel, events, npix, spp, nphotons, alpha=ALPHA_DEFAULT, r0=R0_DEFAULT,
                    hashsize=HASHSIZE_DEFAULT, stats=None):
    """From the records and the photon events ([m,10] = photon, P, n, flux in photon order) alone: the table in the order
    contract (bucket of pos, texel, ray, path as a bit string, input position; path None: every record is its ray's root),
    each record's rank within its ray, the replay of main.cpp:103-125 over the events in photon order, and the gathered
    image of main.cpp:252-258.
    Returns (table [n,16] as hitpoints(), image [npix,3], candidates): candidates is the number of (Hitpoint, event, walked
    cell) triples with n . n' > EPS and dd . dd <= r0^2 -- a bucket met twice counting twice --, the candidate pairs of a run
    whose photons form a single batch.
    stats (a dict, optional) receives: duplicates = candidates beyond the first of their (Hitpoint, event); shrunk_out = the
    (Hitpoint, event) pairs accepted at their first copy and refused at a later one, the radius having shrunk meanwhile."""
    cl = cell_length(r0)
    n = len(ray)
    r2_0 = r0 * r0
    if path is None:
        path = np.ones(n, np.uint32)
    bucket = hash_np(*coord_np(hp9[:, 3:6], cl), hashsize) if n else np.zeros(0, np.int64)
    order = sorted(range(n), key=lambda i: (int(bucket[i]), int(texel[i]), int(ray[i]), _bits(path[i]), i))
    rank, seen = {}, {}
    for i in sorted(range(n), key=lambda i: (int(ray[i]), _bits(path[i]), i)):
        rank[i] = seen.get(int(ray[i]), 0)
        seen[int(ray[i])] = rank[i] + 1
    hps = [dict(f=[float(v) for v in hp9[i, 0:3]], pos=[float(v) for v in hp9[i, 3:6]], n=[float(v) for v in hp9[i, 6:9]],
                flux=[0.0, 0.0, 0.0], r2=r2_0, cnt=0, i=i) for i in order]
    buckets = {}
    for h in hps:
        buckets.setdefault(int(bucket[h["i"]]), []).append(h)
    # a large bucket's positions and normals as arrays: what can never pass (the radii only shrink while alpha <= 1) is
    # screened out with the same IEEE operations, elementwise, before the serial loop
    arrays = {b: (np.array([h["pos"] for h in lst]), np.array([h["n"] for h in lst])) for b, lst in buckets.items()
              if len(lst) >= _VECTOR_FROM}
    # the 27 buckets of every event; only events that meet an occupied bucket can change anything
    ix, iy, iz = coord_np(events[:, 1:4], cl)
    cells = np.stack([hash_np(ix - 1 + dx, iy - 1 + dy, iz - 1 + dz, hashsize) for dx in range(3) for dy in range(3)
                      for dz in range(3)], axis=1)
    live = np.isin(cells, np.fromiter(buckets.keys(), np.int64, len(buckets)))
    candidates = duplicates = shrunk_out = 0
    for e in np.nonzero(live.any(axis=1))[0]:
        ev = events[e]
        Pe, ne, fe = [float(v) for v in ev[1:4]], [float(v) for v in ev[4:7]], [float(v) for v in ev[7:10]]
        first = {}  # id of a Hitpoint that was a candidate of this event -> whether its first copy was accepted
        for c in np.nonzero(live[e])[0]:  # in the reference's dx, dy, dz order; a bucket met twice is walked twice
            b = int(cells[e, c])
            lst = buckets[b]
            if b in arrays:
                pos, nrm = arrays[b]
                dd = pos - ev[1:4]
                d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
                nn = (nrm[:, 0] * ev[4] + nrm[:, 1] * ev[5]) + nrm[:, 2] * ev[6]
                cand = (nn > EPS) & (d2 <= r2_0)
                if alpha <= 1.0:
                    lst = [lst[k] for k in np.nonzero(cand)[0]]
                counted = int(cand.sum())
            else:
                counted = None
            for h in lst:
                dd = [h["pos"][0] - Pe[0], h["pos"][1] - Pe[1], h["pos"][2] - Pe[2]]
                facing, d2 = _dot(h["n"], ne) > EPS, _dot(dd, dd)
                if counted is None and facing and d2 <= r2_0:
                    candidates += 1
                took = facing and d2 <= h["r2"]  # main.cpp:116
                if facing and d2 <= r2_0:
                    if id(h) in first:
                        duplicates += 1
                        if first[id(h)] is True and not took:
                            shrunk_out += 1
                            first[id(h)] = None  # counted once
                    else:
                        first[id(h)] = took
                if took:
                    g = (h["cnt"] * alpha + alpha) / (h["cnt"] * alpha + 1.0)  # main.cpp:119
                    h["r2"] *= g
                    h["cnt"] += 1
                    h["flux"] = [(h["flux"][k] + (h["f"][k] * fe[k]) * (1.0 / PI_REF)) * g for k in range(3)]  # main.cpp:122
            if counted is not None:
                candidates += counted
    table = np.zeros((n, 16))
    image = np.zeros((npix, 3))
    norm = float(nphotons) * spp
    for k, h in enumerate(hps):
        i = h["i"]
        table[k] = [int(ray[i]), rank[i]] + h["f"] + h["pos"] + h["n"] + h["flux"] + [h["r2"], h["cnt"]]
        s = 1.0 / (PI_REF * h["r2"] * norm)  # main.cpp:256
        for c in range(3):
            image[int(texel[i]), c] += h["flux"][c] * s
    if stats is not None:
        stats.update(duplicates=duplicates, shrunk_out=shrunk_out)
    return table, image, candidates


# ---- the designed input ----------------------------------------------------------------------------------------------
def scene():
    from cgraytracing_amd.scene import Plane
    return [Plane((0.0, FLOOR_Y, 0.0), N_FLOOR, (0.6, 0.5, 0.4), 0.0, 0.0),
            Plane((0.0, 0.0, WALL_Z), N_WALL, (0.3, 0.5, 0.7), 0.0, 0.0)]


def inside(pos, Pe, r2):
    """the reference's radius test (main.cpp:115-116) in Python floats: dd = pos - Pe; dd . dd <= r2"""
    dd = [float(pos[0]) - float(Pe[0]), float(pos[1]) - float(Pe[1]), float(pos[2]) - float(Pe[2])]
    return _dot(dd, dd) <= r2


def dist2(pos, Pe):
    dd = [float(pos[0]) - float(Pe[0]), float(pos[1]) - float(Pe[1]), float(pos[2]) - float(Pe[2])]
    return _dot(dd, dd)


def boundary(fixed, u, r2, moving_is_pos=True):
    """Bisection along direction u from `fixed` down to adjacent doubles of the distance t: the last point inside
    fl(dd . dd) <= r2 and the first outside, dd taken as the reference takes it (pos - P: `moving_is_pos` says which of the two
    moves).  Returns (point inside, point outside), which differ."""
    fixed, u = np.asarray(fixed, np.float64), np.asarray(u, np.float64)
    at = lambda t: fixed + t * u
    test = (lambda t: inside(at(t), fixed, r2)) if moving_is_pos else (lambda t: inside(fixed, at(t), r2))
    lo, hi = 0.0, 4.0 * math.sqrt(r2)
    assert test(lo) and not test(hi)
    while np.nextafter(lo, np.inf) < hi:
        mid = lo + (hi - lo) / 2
        if test(mid):
            lo = mid
        else:
            hi = mid
    p_in, p_out = at(lo), at(hi)
    assert test(lo) and not test(hi) and not np.array_equal(p_in, p_out)
    return p_in, p_out


def cell_edge(k, axis, cl):
    """(largest double in a cell below k, smallest double of cell k) along `axis`, by hash.h:39-41's own expression"""
    coord = lambda x: math.floor((x - ORIGIN[axis]) / cl)
    lo, hi = ORIGIN[axis] + (k - 0.5) * cl, ORIGIN[axis] + (k + 0.5) * cl
    assert coord(lo) == k - 1 and coord(hi) == k
    while np.nextafter(lo, np.inf) < hi:
        mid = lo + (hi - lo) / 2
        if coord(mid) < k:
            lo = mid
        else:
            hi = mid
    return float(lo), float(hi)


def event_sort_keys(P, cl):
    """event_keys_kernel's key: the event's cell, clamped to 10 bits a coordinate (for the ORDER of the search only)"""
    ix, iy, iz = coord_np(P, cl)
    return (np.clip(iz, 0, 1022) << 20) | (np.clip(iy, 0, 1023) << 10) | np.clip(ix, 0, 1023)


class _Builder:
    """Collects sites (landing spots at least 1.0 apart), their photons and their records."""

    def __init__(self, rng):
        self.rng = rng
        self.photons = []  # dict(plane, a, b, cls, tag): lands at (a, FLOOR_Y, b) on the floor, (a, b, WALL_Z) on the wall
        self.records = []  # dict(pos, n, cls, tag, expect)
        # lattices of sites, 2.5 apart and jittered by at most 0.2 in steps of 2^-10 (so that dyadic offsets stay exact); a
        # site's photons land within 0.4 of it: landing spots of two sites are at least 1.3 apart (design() asserts 1.0)
        self.free = {"floor": [(x, z) for x in np.arange(-30.0, 30.1, 2.5) for z in np.arange(-10.0, 35.1, 2.5)],
                     "wall": [(x, y) for x in np.arange(-30.0, 30.1, 2.5) for y in np.arange(-30.0, 30.1, 2.5)]}
        for v in self.free.values():
            rng.shuffle(v)
        self.n_sites = 0

    def new_site(self):
        self.n_sites += 1

    def site(self, plane):
        self.new_site()
        a, b = self.free[plane].pop()
        j = self.rng.integers(-204, 205, 2) / 1024.0
        return float(a + j[0]), float(b + j[1])

    @staticmethod
    def point(plane, a, b):
        return np.array([a, FLOOR_Y, b]) if plane == "floor" else np.array([a, b, WALL_Z])

    def photon(self, plane, a, b, cls, tag=None):
        self.photons.append(dict(plane=plane, a=float(a), b=float(b), cls=cls, tag=tag, site=self.n_sites))
        return len(self.photons) - 1

    def record(self, pos, plane, cls, tag, expect=None, normal=None):
        n = normal if normal is not None else (N_FLOOR if plane == "floor" else N_WALL)
        self.records.append(dict(pos=np.asarray(pos, np.float64), n=np.asarray(n, np.float64), cls=cls, tag=tag, expect=expect))

    def in_plane_dir(self, plane):
        t = self.rng.uniform(0, 2 * math.pi)
        return np.array([math.cos(t), 0.0, math.sin(t)]) if plane == "floor" else np.array([math.cos(t), math.sin(t), 0.0])


def screen_loses(pos, Pe, r2):
    """photon_pairs_kernel's fp32 screen with its margin removed, `sq_f32 > (float)r2`, in numpy: the differences rounded to
    fp32, their squares summed in fp32"""
    dd = (np.asarray(pos, np.float64) - np.asarray(Pe, np.float64)).astype(np.float32)
    return bool(np.float32(np.float32(dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]) > np.float32(r2))


def _class_a(B, r0, n_floor=160, n_wall=60, n_exact=24):
    """Every event's direction is random; for every second event up to 32 random directions are tried and the first is kept whose
    inside record the screen without its margin would lose (in fp32 the sum exceeds r2 for a few per cent of the directions
    where r2 is a power of two, for about two in five elsewhere)."""
    r2 = r0 * r0
    for k in range(n_floor + n_wall):
        plane = "floor" if k < n_floor else "wall"
        a, b = B.site(plane)
        Pe = B.point(plane, a, b)
        B.photon(plane, a, b, "A")
        for _ in range(32 if k % 2 else 1):
            p_in, p_out = boundary(Pe, B.in_plane_dir(plane), r2)
            if screen_loses(p_in, Pe, r2):
                break
        B.record(p_in, plane, "A", "inside", expect=1)
        B.record(p_out, plane, "A", "outside", expect=0)
        if r0 == 0.25 and plane == "floor" and k < n_exact:  # dd . dd == r2 exactly, and the next double outward
            for off in ((0.25, 0, 0), (-0.25, 0, 0), (0, 0, 0.25), (0, 0, -0.25)):
                p = Pe + np.array(off)
                assert dist2(p, Pe) == r2
                B.record(p, plane, "A", "equal", expect=1)
                q = p.copy()
                ax = 0 if off[0] else 2
                while inside(q, Pe, r2):
                    q[ax] = np.nextafter(q[ax], math.copysign(np.inf, off[ax]))
                B.record(q, plane, "A", "equal_next", expect=0)


def _class_b(B, r0, alpha, per_variant=34):
    """per_variant triples of each of inside / outside / between, for same-batch and for split placement each"""
    g0 = (0 * alpha + alpha) / (0 * alpha + 1.0)
    r2_0 = r0 * r0
    r2_1 = r2_0 * g0  # the radius after the first photon (main.cpp:119-120)
    for split in (False, True):
        for variant in ("inside", "outside", "between"):
            for _ in range(per_variant):
                plane = "floor" if B.rng.random() < 0.75 else "wall"
                a, b = B.site(plane)
                PA = B.point(plane, a, b)
                u = B.in_plane_dir(plane)
                if variant == "between":
                    PB = PA + B.rng.uniform(math.sqrt(g0) * 1.02, 0.98) * r0 * u
                    assert inside(PA, PB, r2_0) and not inside(PA, PB, r2_1)
                else:
                    p_in, p_out = boundary(PA, u, r2_1, moving_is_pos=False)
                    PB = p_in if variant == "inside" else p_out
                tag = (variant, "split" if split else "same")
                ia = B.photon(plane, a, b, "B", tag + ("first",))
                ib = B.photon(plane, *((PB[0], PB[2]) if plane == "floor" else (PB[0], PB[1])), "B", tag + ("second",))
                B.photons[ia]["partner"] = ib
                B.record(PA, plane, "B", tag, expect=2 if variant == "inside" else 1)


def _class_c(B, sites=10):
    th = math.radians(89.99)
    for _ in range(sites):
        a, b = B.site("floor")
        Pe = B.point("floor", a, b)
        B.photon("floor", a, b, "C")
        for tag, nrm, expect in (("at_eps", (0.0, EPS, 0.0), 0), ("above_eps", (0.0, float(np.nextafter(EPS, 1.0)), 0.0), 1),
                                 ("opposite", (0.0, -1.0, 0.0), 0), ("grazing", (math.sin(th), math.cos(th), 0.0), 1)):
            off = B.rng.uniform(-0.1, 0.1, 3) * np.array([1.0, 0.0, 1.0])
            B.record(Pe + off, "floor", "C", tag, expect=expect, normal=nrm)


def _class_d(B, r0, per_axis=10):
    cl = cell_length(r0)
    assert cl < r0
    for plane, axis in (("floor", 0), ("floor", 2), ("wall", 1)):
        for j in range(per_axis):
            for kind in ("two_cells", "one_cell"):
                a, b = B.site(plane)
                P = B.point(plane, a, b)
                k = int(math.floor((P[axis] - ORIGIN[axis]) / cl))
                below, _ = cell_edge(k, axis, cl)       # the event: in cell k - 1, at its upper edge
                _, at = cell_edge(k + 1, axis, cl)      # the record: in cell k + 1, at its lower edge
                if j % 2:
                    below = float(np.nextafter(below, -np.inf))  # (an ulp further from the edge)
                shift = 0.0 if kind == "two_cells" else 0.1  # the same two points moved into cells k and k + 1
                Pe, Ph = P.copy(), P.copy()
                Pe[axis], Ph[axis] = below + shift, at + shift
                ce = math.floor((Pe[axis] - ORIGIN[axis]) / cl)
                ch = math.floor((Ph[axis] - ORIGIN[axis]) / cl)
                assert ch - ce == (2 if kind == "two_cells" else 1), (ce, ch)
                assert inside(Ph, Pe, r0 * r0) and math.sqrt(dist2(Ph, Pe)) > 0.2602, "inside the radius: the slack is 1.9e-4"
                B.photon(plane, *((Pe[0], Pe[2]) if plane == "floor" else (Pe[0], Pe[1])), "D")
                B.record(Ph, plane, "D", kind, expect=0 if kind == "two_cells" else 1)


def _class_e(B, r0):
    """Sites outside the lattices: x of the floor's and the wall's in OUT_X, y of the wall's in OUT_Y; a record 0.8 r0 away on
    either side along the axis that leaves the box (so that one of them lies in another cell, across -35 where the site is
    next to it) and one 1.2 r0 away."""
    below = float(np.nextafter(-35.0, -np.inf))
    out_x = (-50.3, below, 231.2, 300.0)
    out_y = (-40.0, below)
    sites = [("floor", x, z, 0) for x in out_x for z in (-3.7, 11.3)]
    sites += [("wall", x, y, 1) for x in (-12.4, 7.9) for y in out_y]
    sites += [("wall", x, y, 0) for x in out_x for y in out_y]
    for plane, a, b, axis in sites:
        B.new_site()
        Pe = B.point(plane, a, b)
        B.photon(plane, a, b, "E")
        for s, expect in ((0.8, 1), (-0.8, 1), (1.2, 0), (-1.2, 0)):
            p = Pe.copy()
            p[axis] += s * r0
            assert inside(p, Pe, r0 * r0) == bool(expect)
            B.record(p, plane, "E", "in" if expect else "out", expect=expect)


F_RECORDS, F_PHOTONS, F_SPREAD = 48, 197, 0.04
F_NEAR = (33.0, 15.0)  # F's cell is the one that holds this (x, z): beyond the floor's lattice, whose last column is at 30.2


def f_cell(r0):
    """(ix, iz) of class F's cell"""
    cl = cell_length(r0)
    return int(math.floor((F_NEAR[0] - ORIGIN[0]) / cl)), int(math.floor((F_NEAR[1] - ORIGIN[2]) / cl))


def _class_f(B, r0):
    cl = cell_length(r0)
    B.new_site()
    ix, iz = f_cell(r0)
    cx, cz = ORIGIN[0] + (ix + 0.5) * cl, ORIGIN[2] + (iz + 0.5) * cl  # the cell's centre; F_SPREAD < cl / 2 keeps all inside

    def spot():
        t, r = B.rng.uniform(0, 2 * math.pi), F_SPREAD * math.sqrt(B.rng.random())
        return cx + r * math.cos(t), cz + r * math.sin(t)

    for _ in range(F_PHOTONS):
        B.photon("floor", *spot(), "F")
    for _ in range(F_RECORDS):
        x, z = spot()
        B.record((x, FLOOR_Y, z), "floor", "F", "wave")


_CACHE = {}


def design(orc, r0=R0_DEFAULT, classes="ABCDEF", alpha=ALPHA_DEFAULT, seed=SEED):
    """The designed records and photons for initial radius r0 (classes A-C and, where the cell is shorter than r0, D; E and F
    on request), computed once per argument set.  Returns a dict:
      hp9 [n,9], ray [n] (distinct ids, not the index), pixel [n], rec_cls / rec_tag / rec_expect (per record; expect = the
      photons a record must end with under the default hashsize, or None),
      org, dirs, flux [m,3] (the photons in feeding order), ph_cls / ph_tag (per photon), events [m,10] = photon, P, n, flux:
      the oracle's, objs (the scene), width, rows."""
    key = (r0, classes, alpha, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    B = _Builder(rng)
    if "A" in classes:
        _class_a(B, r0)
    if "B" in classes:
        _class_b(B, r0, alpha)
    if "C" in classes:
        _class_c(B)
    if "D" in classes and cell_length(r0) < r0:
        _class_d(B, r0)
    if "E" in classes:
        _class_e(B, r0)
    if "F" in classes:
        _class_f(B, r0)
    # ---- feeding order: the first photons of B's split triples, then B's same-batch triples as adjacent pairs (from an even
    # position: one batch of 64 holds both), then every other photon -- F's in one run, so that batches of 64 are full waves of
    # its cell too --, then the split triples' second photons
    ph = B.photons
    is_b = lambda i, place, which: ph[i]["cls"] == "B" and ph[i]["tag"][1] == place and ph[i]["tag"][2] == which
    first_split = [i for i in range(len(ph)) if is_b(i, "split", "first")]
    pairs = [j for i in range(len(ph)) if is_b(i, "same", "first") for j in (i, ph[i]["partner"])]
    rest = [i for i in range(len(ph)) if ph[i]["cls"] not in ("B", "F")]
    rng.shuffle(rest)
    run_f = [i for i in range(len(ph)) if ph[i]["cls"] == "F"]
    if len(first_split) % 2:
        first_split.append(rest.pop())
    feed = first_split + pairs + rest[: len(rest) // 2] + run_f + rest[len(rest) // 2:]
    feed += [ph[i]["partner"] for i in first_split if ph[i]["cls"] == "B"]
    assert sorted(feed) == list(range(len(ph)))
    at = {p: k for k, p in enumerate(feed)}
    for i in range(len(ph)):
        if ph[i]["cls"] == "B" and ph[i]["tag"][2] == "first":
            same = at[i] // BATCH_SMALL == at[ph[i]["partner"]] // BATCH_SMALL
            assert at[i] < at[ph[i]["partner"]] and same == (ph[i]["tag"][1] == "same")
    m = len(feed)
    org, dirs = np.zeros((m, 3)), np.zeros((m, 3))
    land = np.zeros((m, 3))
    for k, i in enumerate(feed):
        p = ph[i]
        if p["plane"] == "floor":
            org[k], dirs[k], land[k] = (p["a"], 10.0, p["b"]), (0.0, -1.0, 0.0), (p["a"], FLOOR_Y, p["b"])
        else:
            org[k], dirs[k], land[k] = (p["a"], p["b"], 0.0), (0.0, 0.0, 1.0), (p["a"], p["b"], WALL_Z)
    site = np.array([ph[i]["site"] for i in feed])
    gap = np.sqrt(((land[:, None, :] - land[None, :, :]) ** 2).sum(axis=2))
    assert gap[site[:, None] != site[None, :]].min() >= 1.0, "landing spots of different sites are at least 1.0 apart"
    flux = np.ascontiguousarray(rng.uniform(0.5, 1.5, (m, 3)) * np.array([9000.0, 6000.0, 2500.0]))
    # ---- the events are the oracle's; the classes above rest on their being the intended landing spots
    from test_gpu_photon_rays import oracle_photon_events
    objs = scene()
    valid, ev9 = oracle_photon_events(orc, objs, org, dirs, flux)
    assert valid.all(), "every designed photon lands on a diffuse plane"
    assert np.array_equal(ev9[:, 0:3], land), "the oracle's events are not the intended landing spots"
    floor = np.array([ph[i]["plane"] == "floor" for i in feed])
    assert np.array_equal(ev9[:, 3:6], np.where(floor[:, None], N_FLOOR, N_WALL)) and np.array_equal(ev9[:, 6:9], flux)
    events = np.concatenate([np.arange(m, dtype=np.float64)[:, None], ev9], axis=1)
    # ---- the records: a value per record and channel, distinct ray ids, a texel of the record's own (several records share one)
    n = len(B.records)
    hp9 = np.zeros((n, 9))
    hp9[:, 0:3] = rng.uniform(0.05, 0.95, (n, 3))
    hp9[:, 3:6] = [r["pos"] for r in B.records]
    hp9[:, 6:9] = [r["n"] for r in B.records]
    ray = rng.permutation(4 * n)[:n].astype(np.int64)
    pixel = rng.integers(0, WIDTH * ROWS, n).astype(np.int64)
    assert np.abs(hp9[:, 3:6]).max() < 1e4 and np.abs(org).max() < 1e4
    d = dict(hp9=np.ascontiguousarray(hp9), ray=ray, pixel=pixel, rec_cls=np.array([r["cls"] for r in B.records]),
             rec_tag=[r["tag"] for r in B.records], rec_expect=[r["expect"] for r in B.records],
             org=np.ascontiguousarray(org), dirs=np.ascontiguousarray(dirs), flux=flux,
             ph_cls=np.array([ph[i]["cls"] for i in feed]), ph_tag=[ph[i]["tag"] for i in feed], events=events, objs=objs,
             width=WIDTH, rows=ROWS, r0=r0, alpha=alpha)
    if "F" in classes:  # the run of F's cell in the order of the search holds a whole wave of 64 lanes
        cl = cell_length(r0)
        keys = event_sort_keys(events[:, 1:4], cl)
        fkeys = keys[d["ph_cls"] == "F"]
        ixyz = np.stack(coord_np(events[d["ph_cls"] == "F", 1:4], cl), axis=1)
        assert (ixyz == ixyz[0]).all() and (ixyz[0, 0], ixyz[0, 2]) == f_cell(r0), "F's photons land in one cell, the chosen one"
        rc = np.stack(coord_np(hp9[d["rec_cls"] == "F", 3:6], cl), axis=1)
        assert (rc == ixyz[0]).all(), "and its records lie in it"
        d["f_run"] = int((keys == fkeys[0]).sum())
        assert d["f_run"] >= 127 and d["f_run"] == len(fkeys)
        d["f_wave_pairs"] = 64 * F_RECORDS
    _CACHE[key] = d
    return d


def expected(d, hashsize=HASHSIZE_DEFAULT, stats=None):
    """replay_expected over a design: (table, image [npix,3], candidates); computed once per (design, hashsize)"""
    memo = d.setdefault("_expected", {})
    if hashsize not in memo:
        st = {}
        memo[hashsize] = replay_expected(d["ray"], None, d["hp9"], d["pixel"], d["events"], d["width"] * d["rows"], 1, len(d["org"]),
                                         alpha=d["alpha"], r0=d["r0"], hashsize=hashsize, stats=st) + (st,)
    if stats is not None:
        stats.update(memo[hashsize][3])
    return memo[hashsize][:3]


def counts_by_record(d, table):
    """the table's photon counts (column 15) per input record, through the records' distinct ray ids"""
    by_ray = {int(r): float(c) for r, c in zip(table[:, 0], table[:, 15])}
    return np.array([by_ray[int(r)] for r in d["ray"]])


def screen_without_margin(d):
    """screen_loses on class A's `inside` records against their own event: True where the screen without its margin would drop a
    pair that the exact test accepts."""
    sel = np.nonzero((d["rec_cls"] == "A") & np.array([t == "inside" for t in d["rec_tag"]]))[0]
    a_events = d["events"][d["ph_cls"] == "A", 1:4]
    r2 = d["r0"] * d["r0"]
    lost = np.zeros(len(sel), bool)
    for k, i in enumerate(sel):
        pos = d["hp9"][i, 3:6]
        lost[k] = screen_loses(pos, a_events[np.argmin(((a_events - pos) ** 2).sum(axis=1))], r2)
    return lost
