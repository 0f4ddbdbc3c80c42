"""CPU: the yardstick of tests/test_gpu_photon_gather.py and the designed input, checked without a GPU.

1. ppm_design.replay_expected is pinned to the compiled reference: on the smallest golden photon case it turns the fixture's
   Hitpoint geometry and the oracle's photon events into the fixture's flux, r2, n and image bit for bit.
2. The design (ppm_design.design) has the properties its classes promise, from the replay and the oracle alone -- conditions
   of the tests, not measurements."""
import os
import sys

import numpy as np
import pytest

import ppm_design as D
from backends import BackendScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_golden  # noqa: E402


# ---- 1. the replay against the compiled reference ------------------------------------------------------------------------
def test_replay_reproduces_the_compiled_reference(orc):
    """The fixture keeps the Hitpoints in canonical order (pixel, sample, pos), as test_gpu_ppm_session._canon makes it; a record's
    ray is sample * npix + pixel (test_gpu_ppm_rays._ray_to_ps read backwards) and its texel the pixel."""
    cases = {c[0]: c for c in make_golden.photon_cases()}
    gold = {name: np.load(os.path.join(GOLD, "ppm_%s.npz" % name)) for name in cases}
    name = min(cases, key=lambda k: len(gold[k]["hp"]) * cases[k][6])  # Hitpoints x photons: the least work
    _, mk, cam, W, H, spp, nph = cases[name]
    g = gold[name]["hp"]
    npix = W * H
    pix, smp = g[:, 0].astype(np.int64), g[:, 1].astype(np.int64)
    o = BackendScene(orc, mk())
    events = o.photon_events(0, nph, depth=5)
    o.close()
    table, image, cand = D.replay_expected(smp * npix + pix, None, g[:, 2:11], pix, events, npix, spp, nph)
    # back to the canonical order: the table's rays name the fixture's (pixel, sample); within one, by pos as _canon sorts
    ray = table[:, 0].astype(np.int64)
    canon = np.concatenate([(ray % npix)[:, None].astype(np.float64), (ray // npix)[:, None].astype(np.float64), table[:, 2:]], axis=1)
    canon = canon[np.lexsort([canon[:, 7], canon[:, 6], canon[:, 5], canon[:, 1], canon[:, 0]])]
    print(name, len(g), "Hitpoints,", len(events), "events,", cand, "candidates,", int((g[:, 15] > 0).sum()), "with photons")
    assert (g[:, 15] > 0).sum() >= 0.5 * len(g) and cand > 0
    assert np.array_equal(canon[:, :11], g[:, :11])
    assert np.array_equal(canon[:, 11:14], g[:, 11:14]), "flux"
    assert np.array_equal(canon[:, 14], g[:, 14]), "r2"
    assert np.array_equal(canon[:, 15], g[:, 15]), "n"
    assert np.array_equal(image.reshape(H, W, 3), gold[name]["image"]), "image"


# ---- 2. the design ---------------------------------------------------------------------------------------------------------
R0S = [D.R0_DEFAULT, 0.25]


def _sel(d, cls, tag=None):
    return np.array([c == cls and (tag is None or t == tag) for c, t in zip(d["rec_cls"], d["rec_tag"])])


@pytest.mark.parametrize("r0", R0S, ids=["r0_default", "r0_quarter"])
def test_design_classes_hold(orc, r0):
    d = D.design(orc, r0)
    table, _, cand = D.expected(d)
    n = D.counts_by_record(d, table)
    count = lambda cls, tag=None: int(_sel(d, cls, tag).sum())
    photons = lambda cls: int((d["ph_cls"] == cls).sum())
    print("r0 %.6g:" % r0, {c: (count(c), photons(c)) for c in "ABCDEF"}, "records / photons;", cand, "candidates")
    # every class at its stated minimum
    assert photons("A") >= 200 and count("A", "inside") == count("A", "outside") == photons("A")
    for v in ("inside", "outside", "between"):
        for place in ("same", "split"):
            assert count("B", (v, place)) >= 30
    assert count("B") >= 200 and photons("B") == 2 * count("B")
    assert all(count("C", t) >= 10 for t in ("at_eps", "above_eps", "opposite", "grazing"))
    assert count("E", "in") >= 30 and count("E", "out") >= 30 and photons("E") >= 16
    assert count("F") == D.F_RECORDS and photons("F") == D.F_PHOTONS >= 192
    # every record whose fate the design states ends with that many photons -- A's inside 1 and outside 0, B's inside 2, outside and
    # between 1 (the first photon's alone), C, D and E as their tags say
    want = np.array([-1 if e is None else e for e in d["rec_expect"]])
    stated = want >= 0
    assert stated.sum() == len(want) - D.F_RECORDS
    bad = np.nonzero(stated & (n != want))[0]
    assert len(bad) == 0, [(d["rec_cls"][i], d["rec_tag"][i], n[i], want[i]) for i in bad[:10]]
    assert (n[_sel(d, "A", "inside")] == 1).all() and (n[_sel(d, "A", "outside")] == 0).all()
    for place in ("same", "split"):
        assert (n[_sel(d, "B", ("between", place))] == 1).all()
    # bisection down to adjacent doubles often ends ON the radius: records that `<` in place of `<=` would lose
    a_events = d["events"][d["ph_cls"] == "A", 1:4]
    on_radius = sum(D.dist2(p, a_events[np.argmin(((a_events - p) ** 2).sum(axis=1))]) == r0 * r0
                    for p in d["hp9"][_sel(d, "A", "inside"), 3:6])
    print(on_radius, "inside records of A with dd . dd == r2 exactly")
    assert on_radius > 0
    # A is sensitive to the fp32 screen's margin: without it, inside records would be lost
    lost = D.screen_without_margin(d)
    print(int(lost.sum()), "of", len(lost), "inside records of A exceed (float)r2 in the fp32 sum")
    assert lost.sum() >= 10
    # B's between variant is a candidate of the search (inside r0^2) that the replay refuses (outside r0^2 g0)
    g0 = d["alpha"]
    firsts = d["events"][[t is not None and t[0] == "between" and t[2] == "first" for t in d["ph_tag"]], 1:4]
    seconds = d["events"][[t is not None and t[0] == "between" and t[2] == "second" for t in d["ph_tag"]], 1:4]
    assert len(firsts) == len(seconds) >= 60
    rec = d["hp9"][_sel(d, "B", ("between", "same")) | _sel(d, "B", ("between", "split")), 3:6]
    for p in rec:
        a = firsts[np.argmin(((firsts - p) ** 2).sum(axis=1))]
        b = seconds[np.argmin(((seconds - p) ** 2).sum(axis=1))]
        assert np.array_equal(a, p) and r0 * r0 * g0 < D.dist2(p, b) <= r0 * r0
    # F: a whole wave of one cell in the order of the search, and long chains
    assert d["f_run"] >= 127 and d["f_wave_pairs"] > 512
    assert n[_sel(d, "F")].min() >= 100, "every record of F replays a long chain"
    assert cand >= D.F_PHOTONS * D.F_RECORDS


def test_design_exact_equality_at_quarter_radius(orc):
    d = D.design(orc, 0.25)
    assert D.cell_length(0.25) == 0.25
    table, _, _ = D.expected(d)
    n = D.counts_by_record(d, table)
    eq, nxt = _sel(d, "A", "equal"), _sel(d, "A", "equal_next")
    a_events = d["events"][d["ph_cls"] == "A", 1:4]
    exact = 0
    for p in d["hp9"][eq, 3:6]:
        e = a_events[np.argmin(((a_events - p) ** 2).sum(axis=1))]
        exact += D.dist2(p, e) == 0.0625
    assert exact == eq.sum() >= 80 and nxt.sum() == eq.sum()
    assert (n[eq] == 1).all() and (n[nxt] == 0).all()


def test_design_two_cells_away(orc):
    d = D.design(orc)
    r0 = D.R0_DEFAULT
    cl = D.cell_length(r0)
    assert 1.9e-4 < r0 - cl < 2.0e-4
    table, _, _ = D.expected(d)
    n = D.counts_by_record(d, table)
    two, one = _sel(d, "D", "two_cells"), _sel(d, "D", "one_cell")
    assert two.sum() >= 30 and one.sum() >= 30
    assert (n[two] == 0).all() and (n[one] == 1).all()
    d_events = d["events"][d["ph_cls"] == "D", 1:4]
    axes = set()
    for p in d["hp9"][two, 3:6]:
        e = d_events[np.argmin(((d_events - p) ** 2).sum(axis=1))]
        assert D.dist2(p, e) <= r0 * r0, "inside the radius, and yet not counted"
        ce, cp = [int(c[0]) for c in D.coord_np(e[None, :], cl)], [int(c[0]) for c in D.coord_np(p[None, :], cl)]
        diff = [b - a for a, b in zip(ce, cp)]
        assert sorted(abs(x) for x in diff) == [0, 0, 2]
        axes.add(diff.index(2))
    assert axes == {0, 1, 2}


def test_design_outside_the_box(orc):
    d = D.design(orc)
    cl = D.cell_length(D.R0_DEFAULT)
    ix, iy, iz = D.coord_np(d["events"][d["ph_cls"] == "E", 1:4], cl)
    assert ix.min() < -1 and (ix == -1).any() and ix.max() > 1023 and (iy == -1).any() and iy.min() < -1
    rx = D.coord_np(d["hp9"][_sel(d, "E"), 3:6], cl)[0]
    assert rx.min() < 0 and rx.max() > 1023 and {-1, 0} <= set(rx.tolist())


@pytest.mark.parametrize("hashsize", [7, 101])
def test_design_colliding_cells(orc, hashsize):
    d = D.design(orc, classes="ABCD")
    assert len(d["org"]) <= 1000
    st = {}
    table, _, cand = D.expected(d, hashsize, stats=st)
    base = D.expected(d)
    print("hashsize", hashsize, len(d["org"]), "photons,", len(d["hp9"]), "records:", cand, "candidates,", st["duplicates"],
          "duplicates,", st["shrunk_out"], "accepted on the first copy and refused on a later one")
    assert st["duplicates"] > 0 and cand > base[2]
    assert st["shrunk_out"] >= 1
    assert table[:, 15].sum() > base[0][:, 15].sum(), "a photon counted twice"
