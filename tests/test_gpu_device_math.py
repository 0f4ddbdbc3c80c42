"""The unwrapped square root and reciprocal of cgrt_device_math.hpp (sqrt_cr, normalized) and Sphere::intersect's distance
(sphere_len) against exact rounding, function by function (cgrt_math_probe calls the very inlines the render kernels call), and
the same edges through Scene.trace_rays / Scene.intersect_rays on a sphere-only scene at four scales.  Every comparison is on
bits; no tolerance appears in this file.

References.  Square root: the correctly rounded root from Python integers (sqrt_int).  normalized: numpy fp64 in vec3.h:31-43's
operation order.  sphere_len: objects.h:45-68 in numpy fp64.  The tests without the gpu mark check the inputs themselves on the
CPU: np.sqrt equals the integer reference on every square-root input, the hard-case count, the constructions' exactness, and
the oracle's hit / miss shares at every scale.

Input classes for the root (all at floor(log2 x) in [-766, 999], the short form's range, unless said otherwise):
  recipe    20 000 random 53-bit M: the two doubles that bracket (2M+1)^2, for an even and an odd exponent (80 000 values).
            Their roots lie within an ulp of a rounding midpoint, NOT within 2^-53 ulp: the doubles next to (2M+1)^2 are up to
            2^55 apart from it, which moves the root by up to an ulp.
  hard      the doubles whose root really lies within 2^-50 ulp of a midpoint.  There are only about two dozen such mantissas
            (the root m + 1/2 + e needs m^2 + m = r (mod 2^52 or 2^53) with |r + 1/4| < 2^-50 (2m + 1), which is 8 to 16;
            each r has two solutions, found by Hensel lifting; all |r| <= 16 are taken), so the count the suite wants -- at
            least 10 000 inputs within 2^-50 ulp, checked with integers -- is reached by placing each at every exponent of its
            parity.  Mantissas with |r| <= 2048 (within 2^-42 ulp) are added at 8 exponents each.
  squares   m^2 for random 26-bit m and the doubles on either side, at scattered even and odd exponents.
  range     2^-767 and 2^1000 with their neighbours, DBL_MIN, subnormals, +-0, DBL_MAX, inf, NaN, negatives, and 50 000 values
            log-uniform over [2^-1074, 2^1024).
Every in-range class runs twice: as it is (no lane out of range: the short form) and with lane 0 of every wave replaced by 0
(the whole wave takes the library form), so both forms see every hard case.

Measured on an MI355X: 0 mismatches in every class and arrangement.  Mutations tried once by hand: sqrt_cr without its last
correction fails on 1 766 values of hard50 and 48 of hard43 (and on no other class); normalized without its third refinement
fails on 2 338 vectors of rcp_edge and 461 of s2_sqrtish; the ballots replaced by per-lane tests change nothing."""
import math

import numpy as np
import pytest

import scenes
from backends import BackendScene
from cgraytracing_amd.scene import Sphere

LO, HI = 2.0 ** -767, 2.0 ** 1000  # sqrt_cr's short form: every active lane of the wave has LO <= x <= HI
E_MIN, E_MAX = -766, 999           # floor(log2 x) of the in-range classes
KINF = 1e10                        # cgrt_types.h kInf, objects.h:15 doubleINF


# ---- exact references ------------------------------------------------------------------------------------------------
def _split(x):
    """x = M * 2^q with 2^52 <= M < 2^53, for a positive finite double (subnormals included)."""
    m, e = math.frexp(x)
    return int(m * 9007199254740992.0), e - 53


def sqrt_int(x):
    """The correctly rounded square root of a positive finite double, from integers: isqrt of the mantissa shifted to 110
    or 111 bits (exponent made even), rounded to nearest at 53 bits.  A root is never an exact midpoint (asserted)."""
    M, q = _split(x)
    sh = 58 if q % 2 == 0 else 57
    N = M << sh
    r = math.isqrt(N)
    k = r.bit_length() - 53
    hi, lo, half = r >> k, r & ((1 << k) - 1), 1 << (k - 1)
    assert not (lo == half and r * r == N), "a root on a midpoint"
    if lo >= half:  # lo == half: N is no square there, so the root lies above r, past the midpoint
        hi += 1
    return math.ldexp(float(hi), k + (q - sh) // 2)


def near_midpoint(x):
    """True when sqrt(x) lies within 2^-50 ulp of a rounding midpoint (integers only).  With the root scaled to
    [2^52, 2^53) -- one ulp = 1 -- the nearest midpoint is floor(root) + 1/2."""
    M, q = _split(x)
    N = M << (52 + (q & 1))
    c = (math.isqrt(N) << 51) + (1 << 50)  # the midpoint times 2^51; 2^-50 ulp is 2 in that scale
    NN = N << 102
    return (c - 2) * (c - 2) < NN < (c + 2) * (c + 2)


def sqrt_ref(x):
    """np.sqrt: equal to sqrt_int on every input of this file (test_np_sqrt_is_the_integer_reference_on_every_input)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(x)


def normalized_ref(a):
    """vec3.h:31-43 in numpy fp64 (numpy does not contract): len = sqrt(x*x + y*y + z*z); if (len > 0) each *= 1 / len."""
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    with np.errstate(all="ignore"):
        s2 = x * x + y * y + z * z
        ln = np.sqrt(s2)
        r = 1.0 / ln
        out = a * r[:, None]
    return np.where((ln > 0)[:, None], out, a), s2


def sphere_len_ref(q):
    """objects.h:45-68 on rows {centre, radius2, rayorig, raydir}; kInf where intersect() returns false."""
    c, r2, o, d = q[:, 0:3], q[:, 3], q[:, 4:7], q[:, 7:10]
    with np.errstate(all="ignore"):
        l = c - o
        tca = l[:, 0] * d[:, 0] + l[:, 1] * d[:, 1] + l[:, 2] * d[:, 2]
        l2 = l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1] + l[:, 2] * l[:, 2]
        miss = (tca < 0) & (l2 > r2)
        d2 = l2 - tca * tca
        miss |= d2 > r2
        arg = r2 - d2
        thc = np.sqrt(arg)
        t0, t1 = tca - thc, tca + thc
        ln = np.where(t0 < 0, t1, t0)
    return np.where(miss, KINF, ln), np.where(miss, np.nan, arg)


def same_bits(a, b):
    """Equal bit patterns, except that any NaN equals any NaN (the sign of a zero is compared)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def in_range(x):
    with np.errstate(invalid="ignore"):
        return (x >= LO) & (x <= HI)


def wrapped_waves(x):
    """How many of the waves (elements 64k .. 64k+63) of one probe call have a lane outside [LO, HI]."""
    bad = ~in_range(np.asarray(x, np.float64))
    pad = (-len(bad)) % 64
    return int(np.concatenate([bad, np.zeros(pad, bool)]).reshape(-1, 64).any(axis=1).sum())


# ---- inputs ----------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(fn):
    def wrapper():
        if fn.__name__ not in _CACHE:
            v = fn()
            for a in (v.values() if isinstance(v, dict) else v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _CACHE[fn.__name__] = v
        return _CACHE[fn.__name__]
    return wrapper


def _hard_mantissas(rmax):
    """(X, s, r): 2^52 <= X < 2^53 with X * 2^s = m^2 + m - r for an integer m, r even, |r| <= rmax; then
    sqrt(X * 2^s) = m + 1/2 - (r + 1/4) / (2m + 1) + ..., within (|r| + 1) * 2^-53 ulp of the midpoint m + 1/2.
    s = 52 / 53 is the parity of the exponent.  m^2 + m = r (mod 2^s) has one even and one odd solution; bit k of each is
    fixed by the residue modulo 2^(k+1) because the derivative 2m + 1 is odd."""
    out = []
    for s in (52, 53):
        for r in range(-rmax, rmax + 1, 2):
            for m0 in (0, 1):
                m = m0
                for k in range(1, s):
                    if (m * m + m - r) >> k & 1:
                        m += 1 << k
                for mm in (m, m + (1 << s)):
                    X, rem = divmod(mm * mm + mm - r, 1 << s)
                    assert rem == 0
                    if (1 << 52) <= X < (1 << 53):
                        out.append((X, s, r))
    return out


@_cached
def root_sets():
    """dict name -> float64 array; the four classes of the module docstring.  `hard50` is the subset placed at every
    exponent (the |r| <= 16 mantissas)."""
    rng = np.random.default_rng(20261018)
    recipe = []
    for M in rng.integers(1 << 52, 1 << 53, 20000):
        S = (2 * int(M) + 1) ** 2
        for odd in (0, 1):
            t = S.bit_length() - 53
            lo = S >> t
            E = int(rng.integers(E_MIN, E_MAX))  # E or E + 1 below, whichever has the parity
            sh = (E - 52 - t - odd) // 2 * 2 + odd
            recipe += [math.ldexp(float(lo), t + sh), math.ldexp(float(lo + 1), t + sh)]
    recipe = np.array(recipe)
    hard50, hard43 = [], []
    for X, s, r in _hard_mantissas(2048):
        first = E_MIN + ((s - E_MIN) % 2)  # the exponents floor(log2 x) = 52 + q of the parity of s
        if abs(r) <= 16:
            hard50 += [math.ldexp(float(X), E - 52) for E in range(first, E_MAX + 1, 2)]
        else:
            hard43 += [math.ldexp(float(X), int(E) - 52) for E in first + 2 * rng.integers(0, (E_MAX - first) // 2 + 1, 8)]
    squares = []
    for m in rng.integers(1 << 25, 1 << 26, 10000):
        E = int(rng.integers(E_MIN, E_MAX - 52))
        x = math.ldexp(float(int(m) ** 2), E - (int(m) ** 2).bit_length() + 1)
        squares += [np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)]
    squares = np.array(squares)
    sub = [5e-324, 1e-323, 2.0 ** -1060, 2.0 ** -1050 * 1.7, 2.0 ** -1030 * 1.3, np.nextafter(2.2250738585072014e-308, 0.0)]
    special = []
    for edge in (LO, HI):
        special += [np.nextafter(edge, 0.0), edge, np.nextafter(edge, np.inf)]
    special += [2.2250738585072014e-308] + sub + [0.0, -0.0, 1.7976931348623157e308, np.inf, np.nan, -1.0, -5e-324]
    mant = rng.integers(1 << 52, 1 << 53, 50000).astype(np.float64)
    wide = np.ldexp(mant, rng.integers(-1074, 1024, 50000) - 52)  # log-uniform over [2^-1074, 2^1024); subnormals round
    out = dict(recipe=recipe, hard50=np.array(hard50), hard43=np.array(hard43), squares=squares,
               range=np.concatenate([np.array(special), wide]))
    for k in ("recipe", "hard50", "hard43", "squares"):
        assert in_range(out[k]).all(), k
    return out


@_cached
def wave_values():
    """64 fixed in-range values for the wave compositions: the hardest mantissas of both parities and recipe values."""
    s = root_sets()
    step = len(s["hard50"]) // 40
    v = np.concatenate([s["hard50"][::step][:40], s["recipe"][:24]])
    assert len(v) == 64 and in_range(v).all()
    return v


OUT_OF_RANGE = [0.0, 2.0 ** -800, 2.0 ** 1010, np.nan, -1.0]


def wave_arrangements(v, bad, filler):
    """The arrangements of the 64 values v (rows of v for vectors) that a probe call must not tell apart.  bad: out-of-range
    replacements; filler: in-range elements for the full waves in front of a partial one.
    Returns a list of (name, call input, index of v's elements in the input, index into v of each)."""
    n = len(v)
    idx = np.arange(n)
    out = [("alone", v.copy(), idx, idx)]
    waves, where, which = [], [], []
    for b in bad:  # exactly one lane out of range
        for lane in (0, 31, 32, 63):
            w = v.copy()
            w[lane] = b
            keep = idx[idx != lane]
            where.append(len(waves) * 64 + keep)
            which.append(keep)
            waves.append(w)
    out.append(("one lane out of range", np.concatenate(waves), np.concatenate(where), np.concatenate(which)))
    head = filler[:3 * 64]
    part = np.concatenate([head, v[:37]])  # n % 64 == 37, nothing out of range: the short form, 27 lanes dead
    out.append(("partial wave, all in range", part, 192 + idx[:37], idx[:37]))
    part = part.copy()
    part[-1] = bad[0]  # ... and with the last live element out of range
    out.append(("partial wave, last element out of range", part, 192 + idx[:36], idx[:36]))
    waves = []
    for i in range(n):  # the other 63 lanes all out of range
        w = np.stack([bad[(i + j) % len(bad)] for j in range(64)])
        w[i] = v[i]
        waves.append(w)
    out.append(("63 lanes out of range", np.concatenate(waves), idx * 64 + idx, idx))
    return out


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


@_cached
def normalized_sets():
    """dict name -> [n,3] vectors.  `s2_targets` is built so that x*x + y*y + z*z, evaluated in numpy, IS a chosen
    square-root input (returned as normalized_targets()); the other classes are what their names say."""
    rng = np.random.default_rng(7)
    s = root_sets()
    T = np.concatenate([s["recipe"][::4], s["hard50"][::2], s["hard43"][::2], s["squares"][::3], s["range"]])
    ok = np.isfinite(T) & (T >= 2.0 ** -960)  # below that a square of a component is subnormal and its rounding is no longer relative
    Tk = T[ok]
    with np.errstate(all="ignore"):
        # three comparable components: x^2 ~ 0.6 T, z^2 ~ 0.3 T, y^2 = what is left
        x, z = np.sqrt(0.6 * Tk), np.sqrt(0.3 * Tk)
        y = np.sqrt(np.maximum(Tk - x * x - z * z, 0.0))
        three = np.stack([x, y, z], axis=1)
        hit3 = (x * x + y * y + z * z) == Tk
        # two components: x^2 ~ 0.9 T and the rest; |y*y - rest| < 0.3 * 2^-53 T < ulp(T) / 2, so the sum rounds to T
        x2 = np.sqrt(0.9 * Tk)
        two = np.stack([x2, np.sqrt(Tk - x2 * x2), np.zeros_like(x2)], axis=1)
        # one component (sqrt-ish, 0, 0): s2 = fl(x^2), whatever that is -- for every target, the unreachable ones included
        one = np.stack([np.sqrt(np.abs(T)), np.zeros_like(T), np.zeros_like(T)], axis=1)
    vec = np.where(hit3[:, None], three, two)
    targets = Tk
    tiny, huge = 2.0 ** -540, 2.0 ** 600
    edge = [[0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [np.nan, 1.0, 2.0], [1.0, np.nan, 0.0], [3.0, 4.0, np.nan], [np.inf, 1.0, 1.0],
            [tiny, tiny, tiny], [1.5 * tiny, -0.75 * tiny, 0.0], [2.0 ** -530, 0.0, 0.0], [-2.0 ** -537, 2.0 ** -537, 2.0 ** -538],
            [2.0 ** -511, 0.0, 0.0], [3 * 2.0 ** -520, -2.0 ** -519, 5 * 2.0 ** -522],
            [huge, huge, huge], [-huge, 0.0, 1.0], [2.0 ** 512, 2.0 ** 511, -2.0 ** 512], [2.0 ** 511 * 1.4, 0.0, 0.0]]
    u = _unit(rng, 4000)
    edge = np.concatenate([np.array(edge), u * tiny * rng.uniform(0.25, 64.0, 4000)[:, None], u * 2.0 ** -511 * rng.uniform(0.25, 4.0, 4000)[:, None],
                           u * huge * rng.uniform(0.25, 4.0, 4000)[:, None], u * 2.0 ** 512 * rng.uniform(0.7, 1.4, 4000)[:, None],
                           u * 2.0 ** -383.5 * rng.uniform(0.7, 1.4, 4000)[:, None], u * 2.0 ** 500 * rng.uniform(0.7, 1.4, 4000)[:, None]])
    # the reciprocal step: len = |v| exactly for (v, 0, 0) (sqrt(fl(v*v)) == |v| in binary fp).  Mantissas within 64 ulp above 1
    # and within 64 ulp below 2 (1 / len next to a representable number, resp. next to a midpoint), exponents over [-383, 499]
    k = rng.integers(0, 65, 50000)
    mant = np.where(rng.integers(0, 2, 50000) == 0, 1.0 + k * 2.0 ** -52, 2.0 - k * 2.0 ** -52)
    mant = np.where(mant >= 2.0, np.nextafter(2.0, 0.0), mant)
    ln = np.ldexp(mant, rng.integers(-383, 500, 50000)) * rng.choice([-1.0, 1.0], 50000)
    rcp_edge = np.zeros((50000, 3))
    rcp_edge[np.arange(50000), rng.integers(0, 3, 50000)] = ln
    rcp_random = _unit(rng, 50000) * np.ldexp(rng.uniform(1.0, 2.0, 50000), rng.integers(-380, 497, 50000))[:, None]
    # in-range targets first, so that their waves take the short form; the rest (whole exponent range, specials) behind them
    order = np.argsort(~in_range(targets), kind="stable")
    vec, targets, hit3 = vec[order], targets[order], hit3[order]
    with np.errstate(all="ignore"):
        one = one[np.argsort(~in_range(one[:, 0] * one[:, 0]), kind="stable")]
    return dict(s2_targets=vec, s2_sqrtish=one, edge=edge, rcp_edge=rcp_edge, rcp_random=rcp_random), targets, hit3, np.abs(ln)


def _rays_at(rng, centre, radius, n, spread, dist):
    """n rays towards points within spread * radius of the centre, from dist (array or scalar) * radius away."""
    o = centre + _unit(rng, n) * (radius * dist)
    v = centre + _unit(rng, n) * (radius * spread * rng.uniform(0, 1, n) ** (1 / 3))[:, None] - o
    d = v / np.sqrt((v * v).sum(axis=1))[:, None]
    return o, d


def _rows(c, r2, o, d):
    n = len(o)
    return np.concatenate([np.broadcast_to(c, (n, 3)), np.broadcast_to(r2, (n,))[:, None], o, d], axis=1).astype(np.float64)


@_cached
def sphere_sets():
    """list of (name, rows [n,10], wave-aligned?) for cgrt_math_probe(sphere_len); each class starts a new wave."""
    rng = np.random.default_rng(11)
    sets = []
    # tangent rays, r2 - d2 == 0 exactly: small-integer coordinates, axis directions (a permutation of the issue's example)
    tang = []
    for _ in range(256):
        c = rng.integers(-9, 10, 3).astype(np.float64)
        R, back = float(rng.integers(1, 8)), float(rng.integers(1, 12))
        a, b = rng.permutation(3)[:2]
        o = c.copy()
        o[a] += R * rng.choice([-1.0, 1.0])
        sgn = rng.choice([-1.0, 1.0])
        o[b] -= sgn * back
        d = np.zeros(3)
        d[b] = sgn
        tang.append(np.concatenate([c, [R * R], o, d]))
    tang = np.array(tang)
    tang[0] = [0, 0, 0, 1, 1, -5, 0, 0, 1, 0]
    ordinary = _rows(np.array([1.0, -2.0, 30.0]), 49.0, *_rays_at(rng, np.array([1.0, -2.0, 30.0]), 7.0, 1024, 1.3, rng.uniform(1.5, 6, 1024)[:, None]))
    mixed = ordinary.copy()
    mixed[rng.permutation(1024)[:192]] = tang[:192]
    sets += [("tangent, a whole wave", tang[192:256]), ("tangent among ordinary rays", mixed), ("ordinary rays", ordinary)]
    # origin on the sphere: t0 == +0 (towards the centre), t1 == 0 (away from it), and t0 == -0 (a point sphere at the origin of
    # a ray whose direction is negative in every component: tca = -0, thc = +0)
    on = []
    for c, R in (((0.0, 0.0, 0.0), 1.0), ((10.0, -13.0, 30.0), 7.0), ((-8.0, -13.0, 25.0), 7.0), ((3.0, 4.0, 5.0), 0.5)):
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                o = np.array(c)
                o[ax] -= sgn * R
                d = np.zeros(3)
                d[ax] = sgn
                on += [np.concatenate([c, [R * R], o, d]), np.concatenate([c, [R * R], o, -d])]
    for d in ((-1.0, -2.0, -3.0), (-0.25, -0.5, -0.125), (-1.0, -1.0, -1.0)):
        on.append(np.concatenate([[2.0, 3.0, 4.0], [0.0], [2.0, 3.0, 4.0], d]))
    sets.append(("origin on the sphere", np.array(on)))
    c = np.array([2.0, -1.0, 20.0])
    o = c + _unit(rng, 512) * (5.0 * rng.uniform(0, 1, 512))[:, None]
    sets.append(("origin inside", _rows(c, 25.0, o, _unit(rng, 512))))
    # centre behind the origin (tca < 0) with l2 == r2 and r2 one ulp either side; d2 == r2 and one ulp either side (tca == 0:
    # d2 = l2 = a^2 exactly)
    edge = []
    for a in (3.0, 7.0, 1.25, 1e4, 123456.0, 2.0 ** -20 * 3):
        for r2 in (np.nextafter(a * a, 0.0), a * a, np.nextafter(a * a, np.inf)):
            edge.append([0, 0, -a, r2, 0, 0, 0, 0, 0, 1])        # centre straight behind
            edge.append([0, 0, -a, r2, 0, 0, 0, 0.6, 0, 0.8])    # behind, oblique
            edge.append([a, 0, 0, r2, 0, 0, 0, 0, 1, 0])         # tca == 0, d2 == a^2
            edge.append([a, 0, 5, r2, 0, 0, 5, 0, 0, -1])
    sets.append(("l2 and d2 within an ulp of r2", np.array(edge, np.float64)))
    # the room's wall spheres (radius 1e4) from 1e8 away
    for w in scenes.wall_spheres()[:2]:
        o, d = _rays_at(rng, w.center, w.radius, 1024, 1.2, 1e4)
        sets.append(("wall sphere from 1e8", _rows(w.center, w.radius * w.radius, o, d)))
    # radius 2^-400: every intermediate is below 2^-767
    r = 2.0 ** -400
    c = np.array([3.0, -2.0, 7.0]) * r
    o, d = _rays_at(rng, c, r, 2048, 1.2, rng.uniform(1.5, 5, 2048)[:, None])
    sets.append(("radius 2^-400", _rows(c, r * r, o, d)))
    # radius 2^-383 and 1.5 * 2^-384: r2 = 2^-766 and 1.125 * 2^-767, so r2 - d2 straddles 2^-767 within a wave
    for r in (2.0 ** -383, 1.5 * 2.0 ** -384):
        c = np.array([1.0, 2.0, -3.0]) * r
        o, d = _rays_at(rng, c, r, 2048, 1.1, rng.uniform(1.5, 5, 2048)[:, None])
        sets.append(("radius %s" % float(r).hex(), _rows(c, r * r, o, d)))
    return [(name, np.ascontiguousarray(q)) for name, q in sets]


# ---- the same edges through the public calls ---------------------------------------------------------------------------
SCALES = [("2^-400", 2.0 ** -400), ("2^-383", 2.0 ** -383), ("1", 1.0), ("2^29", 2.0 ** 29)]


def scaled_c2(s):
    return [Sphere(o.center * s, o.radius * s, o.surfaceColor, o.reflection, o.transparency) for o in scenes.scene_c2()]


def edge_rays_c2():
    """Tangent and on-surface rays against scene_c2's mirror (10, -13, 30) and glass (-8, -13, 25) spheres, radius 7, and its
    diffuse sphere (-15, -20, 60), radius 10: integer coordinates, axis directions -- every term of Sphere::intersect exact."""
    org, dirs = [], []
    for c, R in (((10.0, -13.0, 30.0), 7.0), ((-8.0, -13.0, 25.0), 7.0), ((-15.0, -20.0, 60.0), 10.0)):
        for a in range(3):
            for b in range(3):
                if a == b:
                    continue
                for sa in (-1.0, 1.0):
                    for sb in (-1.0, 1.0):  # tangent: offset R along a, 5 back along b
                        o = np.array(c)
                        o[a] += sa * R
                        o[b] -= sb * 5.0
                        d = np.zeros(3)
                        d[b] = sb
                        org.append(o)
                        dirs.append(d)
            for sa in (-1.0, 1.0):  # on the surface, looking in and looking out
                o = np.array(c)
                o[a] -= sa * R
                d = np.zeros(3)
                d[a] = sa
                org += [o, o]
                dirs += [d, -d]
    return np.array(org), np.array(dirs)


@_cached
def scaled_cases():
    """per scale: (objs, org, dirs); about 8 000 of test_gpu_rays.random_rays' rays (every 7th, so all four groups are there),
    origins scaled; at scale 1 the exact constructions are appended."""
    from test_gpu_rays import random_rays
    org, dirs, _ = random_rays("spheres", 2024)
    org, dirs = org[::7], dirs[::7]
    out = {}
    for name, s in SCALES:
        o, d = org * s, dirs.copy()
        if s == 1.0:
            eo, ed = edge_rays_c2()
            o, d = np.concatenate([o, eo]), np.concatenate([d, ed])
        out[name] = (scaled_c2(s), np.ascontiguousarray(o), np.ascontiguousarray(d))
    return out


_ORACLE = {}


def oracle_case(orc, name):
    """The oracle's per-object intersect() and their composition (test_gpu_rays.oracle_nearest), computed once per scale."""
    from test_gpu_rays import oracle_nearest
    if name not in _ORACLE:
        objs, org, dirs = scaled_cases()[name]
        o, obj, t, nrm = oracle_nearest(orc, objs, org, dirs)
        per = [o.intersect_batch(i, org, dirs) for i in range(len(objs))]
        o.close()
        _ORACLE[name] = (obj, t, nrm, per)
    return _ORACLE[name]


# ---- CPU: the inputs are what they claim to be -------------------------------------------------------------------------
def test_np_sqrt_is_the_integer_reference_on_every_input():
    """np.sqrt == the integer reference on every square-root input of this file (bit for bit; zeros, inf, NaN and negatives by
    their IEEE values), after which the GPU tests may use np.sqrt.  And the hard-case count: at least 10 000 inputs whose root
    lies within 2^-50 ulp of a midpoint, counted with integers."""
    total = near = 0
    for name, x in root_sets().items():
        got = sqrt_ref(x)
        pos = np.isfinite(x) & (x > 0)
        want = np.array([sqrt_int(float(v)) for v in x[pos]])
        assert np.array_equal(got[pos].view(np.uint64), want.view(np.uint64)), name
        rest = x[~pos]
        for v, g in zip(rest, got[~pos]):
            if v == 0 or v == np.inf:
                assert g == v and np.signbit(g) == np.signbit(v)
            else:
                assert np.isnan(g)
        k = sum(near_midpoint(float(v)) for v in x[pos & in_range(x)])
        print("%-8s %6d values, %6d within 2^-50 ulp of a midpoint" % (name, len(x), k))
        total, near = total + len(x), near + k
        if name == "hard50":  # |r + 1/4| / (2m + 1) < 2^-50 holds for every |r| <= 6 and, by the size of m, for part of the rest
            assert k >= 10000, "the mantissas built to be hard are not"
    print("square-root inputs: %d, within 2^-50 ulp of a midpoint: %d" % (total, near))
    assert near >= 10000
    # both sides of the midpoint are there, and both parities of the exponent
    h = root_sets()["hard50"]
    up = np.array([sqrt_int(float(v)) ** 2 > v for v in h[::50]])  # rounded up: the root lay above the midpoint
    assert up.any() and (~up).any()
    assert len(set(_split(float(v))[1] % 2 for v in h[::50])) == 2


def test_wave_arrangements_cover_what_they_claim():
    v = wave_values()
    arr = wave_arrangements(v, OUT_OF_RANGE, root_sets()["recipe"][1000:])
    assert [wrapped_waves(a[1]) for a in arr] == [0, 20, 0, 1, 64]
    assert len(arr[2][1]) % 64 == 37 and len(arr[3][1]) % 64 == 37
    for name, x, where, which in arr:
        assert same_bits(x[where], v[which]).all(), name


def test_normalized_inputs_are_what_they_claim():
    """s2, evaluated in numpy, IS the chosen square-root input for every target of s2_targets; the underflow / overflow / NaN
    vectors have the s2 they were built for; (v, 0, 0) has len == |v| exactly."""
    sets, targets, hit3, lens = normalized_sets()
    _, s2 = normalized_ref(sets["s2_targets"])
    print("s2 targets: %d, hit with three comparable components: %d, with two: %d" % (len(targets), hit3.sum(), (~hit3).sum()))
    assert np.array_equal(s2, targets)
    assert hit3.mean() > 0.25
    assert sum(near_midpoint(float(v)) for v in targets[in_range(targets)]) >= 5000
    e = sets["edge"]
    _, s2 = normalized_ref(e)
    assert s2[0] == 0 and s2[1] == 0 and np.isnan(s2[2:5]).all() and s2[5] == np.inf
    assert (s2[6:10] < 2.0 ** -1022).all() and (s2[6:10] >= 0).all() and (np.abs(e[6:10]).max(axis=1) >= 2.0 ** -540).all()
    assert s2[6] == 0 and 0 < s2[8]  # underflow to zero, and to a subnormal
    assert (s2[12:15] == np.inf).all()
    blocks = [s2[16 + 4000 * i:16 + 4000 * (i + 1)] for i in range(6)]
    assert (blocks[0] < 2.0 ** -1022).all() and (blocks[0] == 0).any() and (blocks[0] > 0).any()
    assert (blocks[1] < LO).all() and (blocks[1] > 2.0 ** -1022).any() and (blocks[1] < 2.0 ** -1022).any()
    assert (blocks[2] == np.inf).all()
    assert (blocks[3] == np.inf).any() and (blocks[3] < np.inf).any()
    for b, edge in ((blocks[4], LO), (blocks[5], HI)):  # either side of the short form's range, within a wave
        assert 0.2 < (b < edge).mean() < 0.8
    _, s2 = normalized_ref(sets["rcp_edge"])
    assert np.array_equal(np.sqrt(s2), lens) and in_range(s2).all()
    _, s2 = normalized_ref(sets["rcp_random"])
    assert in_range(s2).all()


def test_sphere_constructions_are_exact():
    """r2 - d2 is exactly 0 on the tangent rays; t0 is +0 / -0 on the surface rays; the small spheres' sqrt arguments lie where
    they were meant to."""
    sets = dict((n, q) for n, q in sphere_sets() if not n.startswith("wall"))
    ln, arg = sphere_len_ref(sets["tangent, a whole wave"])
    assert (arg == 0).all() and (ln < KINF).all()
    ln, arg = sphere_len_ref(sets["tangent among ordinary rays"])
    assert (arg == 0).sum() == 192
    ln, arg = sphere_len_ref(sets["origin on the sphere"])
    assert (ln[:-3] == 0).all() and not np.signbit(ln[:-3]).any()
    assert (ln[-3:] == 0).all() and np.signbit(ln[-3:]).all()
    ln, arg = sphere_len_ref(sets["origin inside"])
    assert (ln > 0).all() and (ln < KINF).all()
    ln, arg = sphere_len_ref(sets["l2 and d2 within an ulp of r2"])
    assert (ln == KINF).any() and (ln < KINF).any() and (arg == 0).any()
    ln, arg = sphere_len_ref(sets["radius 2^-400"])
    assert (np.nan_to_num(arg, nan=0.0) < LO).all() and 0.2 < (ln < KINF).mean() < 0.95
    for r in (2.0 ** -383, 1.5 * 2.0 ** -384):
        ln, arg = sphere_len_ref(sets["radius %s" % float(r).hex()])
        hit = ln < KINF
        waves = (in_range(arg[hit.nonzero()[0]]).sum(), (~in_range(arg))[hit].sum())
        assert min(waves) > 100, waves
        a = in_range(np.where(hit, arg, LO)).reshape(-1, 64)
        assert (a.all(axis=1) | ~a.any(axis=1)).sum() < len(a) // 2  # most waves hold both sides of 2^-767
    for w, (name, q) in zip(scenes.wall_spheres()[:2], [s for s in sphere_sets() if s[0].startswith("wall")]):
        ln, arg = sphere_len_ref(q)
        assert 0.2 < (ln < KINF).mean() < 0.95 and (ln[ln < KINF] > 9e7).all()


def test_edge_rays_against_c2_are_exact():
    org, dirs = edge_rays_c2()
    n_t = 0
    for c, R in (((10.0, -13.0, 30.0), 7.0), ((-8.0, -13.0, 25.0), 7.0), ((-15.0, -20.0, 60.0), 10.0)):
        ln, arg = sphere_len_ref(_rows(np.array(c), R * R, org, dirs))
        n_t += int((arg == 0).sum())
    assert n_t >= 3 * 24


@pytest.mark.parametrize("name,s", SCALES, ids=[c[0] for c in SCALES])
def test_oracle_hit_and_miss_shares_per_scale(orc, name, s):
    """At every scale the oracle alone gives at least 1 % hits and 1 % misses, so both outcomes are tested.  The
    scales are the four first chosen; none had to be moved.  Shares (oracle, 8 000 rays): 2^-400 and 2^-383: 95.70 % hits, 4.30 %
    misses (a scaling by a power of two is exact while nothing underflows, so they agree with scale 1); 1, with its 108 exact
    rays: 95.76 % / 4.24 %; 2^29: 47.90 % / 52.10 % -- the wall spheres (radius 1e4 * 2^29) lie beyond kInf = 1e10."""
    obj, t, nrm, per = oracle_case(orc, name)
    hits = float((obj >= 0).mean())
    print("scale %s: %d rays, hits %.4f, misses %.4f" % (name, len(obj), hits, 1 - hits))
    assert hits >= 0.01 and 1 - hits >= 0.01


# ---- GPU -------------------------------------------------------------------------------------------------------------------
_BASE = {}


def _probe(op, x):
    import cgraytracing_amd as cg
    return cg.math_probe(op, x)


@pytest.mark.gpu
def test_sqrt_cr_is_the_exact_root(gpu_ready):
    """sqrt_cr on every class of the module docstring: the correctly rounded root, bit for bit, in the short form and in the
    library form.  Prints elements per class, how many lie within 2^-50 ulp of a midpoint (counted by the CPU test), the
    waves that took the library form by construction, and the mismatches."""
    bad_total = 0
    for name, x in root_sets().items():
        runs = [("as generated", x)]
        if name != "range":
            w = x.copy()
            w[::64] = 0.0
            runs.append(("lane 0 of every wave out of range", w))
        for how, inp in runs:
            got, want = _probe("sqrt", inp), sqrt_ref(inp)
            bad = np.nonzero(~same_bits(got, want))[0]
            n_waves = (len(inp) + 63) // 64
            print("sqrt %-8s %-34s %6d elements, %5d of %5d waves in the library form, mismatches %d %s" %
                  (name, how, len(inp), wrapped_waves(inp), n_waves, len(bad),
                   [(float(inp[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:4]]))
            if name != "range":
                assert wrapped_waves(inp) == (0 if how == "as generated" else n_waves)
            bad_total += len(bad)
    assert bad_total == 0


@pytest.mark.gpu
def test_sqrt_cr_wave_compositions(gpu_ready):
    """The 64 fixed values give the same bits -- the exact root -- alone in a wave, with one lane out of range (0, 2^-800,
    2^1010, NaN, -1 at lane 0, 31, 32, 63), as the first 37 lanes of a last partial wave with and without an out-of-range
    element, and with the other 63 lanes out of range; the out-of-range lanes give their IEEE results."""
    v = wave_values()
    want = np.array([sqrt_int(float(x)) for x in v])
    mism = 0
    for name, x, where, which in wave_arrangements(v, OUT_OF_RANGE, root_sets()["recipe"][1000:]):
        got = _probe("sqrt", x)
        b1 = int((~same_bits(got[where], want[which])).sum())
        b2 = int((~same_bits(got, sqrt_ref(x))).sum())
        print("sqrt waves: %-40s %5d elements, %3d waves in the library form, mismatches of the fixed values %d, of all %d" %
              (name, len(x), wrapped_waves(x), b1, b2))
        mism += b1 + b2
    assert mism == 0


@pytest.mark.gpu
def test_normalized_is_the_reference_expression(gpu_ready):
    """normalized() against vec3.h's expression in numpy, whatever that yields: s2 on the square-root inputs, zero vectors,
    underflowing and overflowing s2, NaN, the reciprocal's edge mantissas, random vectors -- each class as generated and with
    lane 0 of every wave replaced by the zero vector (the whole wave in the library form)."""
    sets = normalized_sets()[0]
    bad_total = 0
    for name, a in sets.items():
        for how in ("as generated", "lane 0 of every wave zero"):
            inp = a.copy()
            if how != "as generated":
                inp[::64] = 0.0
            want, s2 = normalized_ref(inp)
            got = _probe("normalized", inp)
            bad = np.nonzero(~same_bits(got, want).all(axis=1))[0]
            print("normalized %-11s %-26s %6d vectors, %5d of %5d waves in the library form, mismatches %d %s" %
                  (name, how, len(inp), wrapped_waves(s2), (len(inp) + 63) // 64, len(bad),
                   [([float(c).hex() for c in inp[i]], [float(c).hex() for c in got[i]], [float(c).hex() for c in want[i]]) for i in bad[:2]]))
            bad_total += len(bad)
    assert bad_total == 0


@pytest.mark.gpu
def test_normalized_wave_compositions(gpu_ready):
    """64 fixed vectors whose s2 are the fixed hard values: the same bits in every arrangement of test_sqrt_cr_wave_compositions,
    the odd lanes being vectors whose s2 is 0, 2^-800, 2^1010, NaN and inf."""
    sets, targets, hit3, _ = normalized_sets()
    pick = np.nonzero(in_range(targets))[0][:: max(1, int(in_range(targets).sum()) // 64)][:64]
    v = sets["s2_targets"][pick]
    bad = np.array([[0.0, 0.0, 0.0], [2.0 ** -400, 0.0, 0.0], [0.0, 2.0 ** 505, 0.0], [1.0, np.nan, 1.0], [2.0 ** 600, 1.0, 2.0 ** 600]])
    assert len(v) == 64 and not in_range(normalized_ref(bad)[1]).any()
    want = normalized_ref(v)[0]
    mism = 0
    for name, x, where, which in wave_arrangements(v, bad, sets["rcp_random"]):
        got = _probe("normalized", x)
        b1 = int((~same_bits(got[where], want[which]).all(axis=1)).sum())
        b2 = int((~same_bits(got, normalized_ref(x)[0]).all(axis=1)).sum())
        print("normalized waves: %-40s %5d vectors, %3d waves in the library form, mismatches of the fixed vectors %d, of all %d" %
              (name, len(x), wrapped_waves(normalized_ref(x)[1]), b1, b2))
        mism += b1 + b2
    assert mism == 0


@pytest.mark.gpu
def test_sphere_len_is_the_reference_expression(gpu_ready):
    """sphere_len against objects.h:45-68 in numpy, misses (kInf) included: exact tangents alone and among ordinary rays,
    origins on and inside the sphere, l2 and d2 within an ulp of r2, the wall spheres from 1e8, spheres of radius 2^-400 and
    about 2^-383.5."""
    bad_total = 0
    for name, q in sphere_sets():
        want, arg = sphere_len_ref(q)
        got = _probe("sphere_len", q)
        bad = np.nonzero(~same_bits(got, want))[0]
        lib = wrapped_waves(np.where(np.isnan(arg) & (want == KINF), 1.0, arg))  # a lane that misses does not reach the root
        print("sphere_len %-30s %5d rays, hits %5d, r2 - d2 == 0: %4d, waves with a lane in the library form (at least) %3d of %3d, mismatches %d %s"
              % (name, len(q), int((want < KINF).sum()), int((arg == 0).sum()), lib, (len(q) + 63) // 64, len(bad),
                 [(int(i), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:4]]))
        bad_total += len(bad)
    assert bad_total == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,s", SCALES, ids=[c[0] for c in SCALES])
def test_scaled_sphere_scene_through_the_public_calls(gpu_ready, orc, name, s):
    """scene_c2 with every centre and radius multiplied by a power of two (the SPH instantiation), ray origins multiplied
    alike, directions unit: Scene.trace_rays(want=("hit",)) gives the oracle's composition of intersect() (main.cpp:52-62) --
    hit_obj, hit_t, hit_normal bit for bit -- and Scene.intersect_rays gives each object's intersect().  At 2^-400 every sum of
    squares is below 2^-767 (library form), at 2^-383 they straddle it, at 2^29 the walls lie beyond kInf and lose `len <
    nearest`.  Scale 1 carries the exact tangent and on-surface rays of edge_rays_c2."""
    import cgraytracing_amd as cg
    import torch

    objs, org, dirs = scaled_cases()[name]
    obj, t, nrm, per = oracle_case(orc, name)
    with cg.Scene(objs) as sc:
        variant = sc.rays_variant(5, want=("hit",))
        dev = torch.device("cuda", sc.device)
        res = sc.trace_rays(torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev), want=("hit",))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        single = [sc.intersect_rays(i, org, dirs) for i in range(len(objs))]
    assert "SPH=1" in variant and "FIRST=1" in variant, variant
    bad = np.nonzero((got["hit_obj"] != obj) | ~same_bits(got["hit_t"], t) | ~same_bits(got["hit_normal"], nrm).all(axis=1))[0]
    print("scale %s: %s, %d rays, hits %d, misses %d, rays that differ %d %s" %
          (name, variant, len(org), int((obj >= 0).sum()), int((obj < 0).sum()), len(bad),
           [(int(i), int(got["hit_obj"][i]), int(obj[i]), float(got["hit_t"][i]).hex(), float(t[i]).hex()) for i in bad[:4]]))
    assert len(bad) == 0
    for i, ((hg, lg, ng), (hw, lw, nw)) in enumerate(zip(single, per)):
        with np.errstate(invalid="ignore"):
            m = (hw != 0) & (lw < KINF)  # the probe reports a hit as main.cpp:56 takes it: len < nearest = INF
        assert np.array_equal(hg != 0, m), (name, i)
        assert same_bits(lg[m], lw[m]).all() and same_bits(ng[m], nw[m]).all(), (name, i)
