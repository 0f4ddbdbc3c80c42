"""GPU, function level: sphere_len_pair -- the pair loop's routine -- against sphere_len, bit for bit.

cgrt_math_probe(CGRT_PROBE_SPHERE_LEN_PAIR) calls the very inline the pair variants of the eye pass call: two spheres A and B and
one ray per element, elements 64k .. 64k+63 the lanes of one wave.  Every len must be what sphere_len gives for that sphere and
that ray alone (the probe's CGRT_PROBE_SPHERE_LEN, itself compared with objects.h:45-68 in tests/test_gpu_device_math.py, whose
sphere inputs -- exact tangents, r2 - d2 = +-1 ulp, t0 = +-0, radii 2^-400 and 2^-383.5 -- are reused here), whatever the other
sphere of the pair is and whatever the wave's other lanes need: the routine decides per WAVE whether any root is taken and
which form of the square root each sphere gets."""
import numpy as np
import pytest

from test_gpu_device_math import KINF, in_range, same_bits, sphere_len_ref, sphere_sets


def _probe(op, x):
    import cgraytracing_amd as cg
    return cg.math_probe(op, x)


def _pairs(a, b):
    """rows {centre A, r2 A, centre B, r2 B, origin, direction} from sphere_len rows a (whose ray is kept) and the spheres of b"""
    return np.ascontiguousarray(np.concatenate([a[:, 0:4], b[:, 0:4], a[:, 4:10]], axis=1))


def _singles(p):
    return (np.ascontiguousarray(np.concatenate([p[:, 0:4], p[:, 8:14]], axis=1)),
            np.ascontiguousarray(np.concatenate([p[:, 4:8], p[:, 8:14]], axis=1)))


def _check(name, p):
    """The pair probe against the single probe (and numpy's expression) for both spheres; returns per lane (A needs a root, B
    needs a root, A's argument is outside sqrt_cr's short range, B's is)."""
    qa, qb = _singles(p)
    got = _probe("sphere_len_pair", p)
    need, lib = [], []
    for k, q in enumerate((qa, qb)):
        want_gpu = _probe("sphere_len", q)
        want_np, arg = sphere_len_ref(q)
        bad = np.nonzero(~same_bits(got[:, k], want_gpu) | ~same_bits(got[:, k], want_np))[0]
        assert len(bad) == 0, "%s, sphere %s: %d of %d differ, first %s" % (
            name, "AB"[k], len(bad), len(p), [(int(i), float(got[i, k]).hex(), float(want_gpu[i]).hex(), float(want_np[i]).hex()) for i in bad[:4]])
        need.append(~np.isnan(arg))
        lib.append(~np.isnan(arg) & ~in_range(arg))
    return need[0], need[1], lib[0], lib[1]


def _waves(x):
    pad = (-len(x)) % 64
    return np.concatenate([x, np.zeros(pad, bool)]).reshape(-1, 64)


def _far(q):
    """q's rays with a sphere none of them can hit: radius 1/8 of q's, 1000 radii off to the side of the ray and behind it"""
    r = np.where(q[:, 3] > 0, np.sqrt(q[:, 3]), 1.0)  # (a point sphere at the ray's origin: any distance will do)
    d = q[:, 7:10]
    side = np.cross(d, np.where(np.abs(d[:, :1]) < 0.5, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]))
    side /= np.sqrt((side * side).sum(axis=1))[:, None]
    f = q.copy()
    f[:, 0:3] = q[:, 4:7] + (side - d) * (1000.0 * r)[:, None]
    f[:, 3] = r * r / 64.0
    return f


@pytest.mark.gpu
def test_pair_is_sphere_len_twice(gpu_ready):
    """Every input class of tests/test_gpu_device_math.py::sphere_sets as A with three kinds of B on the same ray -- the same
    sphere, the concentric sphere of half the radius (hit by fewer rays) and a sphere no ray can hit -- and with A and B swapped.
    Prints per class the lanes that need a root of A only, of B only, of both, of none, and the waves in which a root's
    argument lies outside [2^-767, 2^1000]."""
    for name, q in sphere_sets():
        half = q.copy()
        half[:, 3] = q[:, 3] * 0.25
        for other, b in (("itself", q), ("half the radius", half), ("out of reach", _far(q))):
            for swapped in (False, True):
                p = _pairs(q, b)
                if swapped:
                    p[:, 0:8] = np.concatenate([p[:, 4:8], p[:, 0:4]], axis=1)
                na, nb, la, lb = _check("%s + %s%s" % (name, other, " (swapped)" if swapped else ""), p)
                print("pair %-30s B = %-16s %-9s %5d rays: A only %5d, B only %5d, both %5d, none %5d; waves with an argument out of range: A %3d, B %3d"
                      % (name, other, "swapped" if swapped else "", len(p), int((na & ~nb).sum()), int((nb & ~na).sum()), int((na & nb).sum()),
                         int((~na & ~nb).sum()), int(_waves(la).any(axis=1).sum()), int(_waves(lb).any(axis=1).sum())))
                if other == "out of reach":
                    assert not (na if swapped else nb).any(), "the far sphere was hit"


def _swap(p):
    p = p.copy()
    p[:, 0:8] = np.concatenate([p[:, 4:8], p[:, 0:4]], axis=1)
    return p


@pytest.mark.gpu
def test_wave_compositions(gpu_ready):
    """The compositions the routine decides by, each asserted to be what it claims:
    all four lane kinds (A needs a root, B needs one, both, neither) in every wave; waves in which no lane needs B's root and
    waves in which none needs A's; waves in which exactly one lane -- lane 0, 31, 32 or 63 -- has A's argument out of range
    (an exact tangent: r2 - d2 == 0) while every argument of B is in range, and the same with A and B swapped: the library form
    for that sphere only; and a partial last wave, the first 37 lanes of the first of these waves, behind a whole one."""
    sets = dict(sphere_sets())
    ordinary, tangent = sets["ordinary rays"], sets["tangent, a whole wave"]
    shifted = ordinary.copy()
    shifted[:, 0] += 6.0  # B: the same radius 6 to the side, so some rays hit A only, some B only, some both, some neither
    four = _pairs(ordinary, shifted)
    na, nb, la, lb = _check("four lane kinds", four)
    kinds = np.stack([_waves(na & ~nb).any(axis=1), _waves(nb & ~na).any(axis=1), _waves(na & nb).any(axis=1), _waves(~na & ~nb).any(axis=1)])
    assert kinds.all(), "waves without one of the four lane kinds: %r" % (np.nonzero(~kinds.all(axis=0))[0],)
    assert not la.any() and not lb.any()

    lone = _pairs(ordinary, _far(ordinary))
    na, nb, _, _ = _check("no lane needs B", lone)
    assert not nb.any() and _waves(na).any(axis=1).all()
    na, nb, _, _ = _check("no lane needs A", _swap(lone))
    assert not na.any() and _waves(nb).any(axis=1).all()

    # one lane's A: an exact tangent (argument 0, below 2^-767); its B: a sphere of radius 2 centred 20 along that lane's ray
    p = four[:256].copy()
    for w, lane in enumerate((0, 31, 32, 63)):
        t = tangent[w]
        i = 64 * w + lane
        p[i, 0:4] = t[0:4]
        p[i, 8:14] = t[4:10]
        p[i, 4:7] = t[4:7] + 20.0 * t[7:10]
        p[i, 7] = 4.0
    for swapped in (False, True):
        q = _swap(p) if swapped else p
        na, nb, la, lb = _check("one lane out of range%s" % (" (swapped)" if swapped else ""), q)
        one, none = (lb, la) if swapped else (la, lb)
        assert (_waves(one).sum(axis=1) == 1).all() and not none.any(), "not exactly one lane of one sphere out of range per wave"
        assert (_waves(na & nb).sum(axis=1) > 1).all(), "no other lane takes both roots beside it"
        na, nb, la, lb = _check("partial last wave%s" % (" (swapped)" if swapped else ""), np.concatenate([q[64:128], q[:37]]))
        assert int((la | lb)[64:].sum()) == 1 and len(la) == 101


def test_far_sphere_is_missed_and_tangents_are_exact():
    """CPU: the constructions above are what they claim -- no ray reaches the far sphere, and the tangent rows' argument is
    exactly zero."""
    for name, q in sphere_sets():
        want, arg = sphere_len_ref(_far(q))
        assert (want == KINF).all() and np.isnan(arg).all(), name
    t = dict(sphere_sets())["tangent, a whole wave"]
    assert (sphere_len_ref(t)[1] == 0).all()
