"""GPU: the photon gather -- the Hitpoint table (cgrt_ppm_table.hpp), the pair search (photon_pairs_kernel) and the ordered replay
(photon_apply_kernel) -- on designed Hitpoint records and photons (tests/ppm_design.py): records at the first and the second
radius to the last double, normals at the threshold, a record two cells away and inside the radius, cells outside the box, a
whole wave in one cell, colliding cells.  Every test checks the photons' events against the oracle's, feeds them to a
hitpoint session and compares the table (all 16 columns, in table order), the image and the counters with the numpy replay of
main.cpp:103-125,252-258, which tests/test_photon_gather_host.py pins to the compiled reference.  Every comparison is exact."""
import numpy as np
import pytest

import ppm_design as D

pytestmark = pytest.mark.gpu

R0S = [D.R0_DEFAULT, 0.25]
R0_IDS = ["r0_default", "r0_quarter"]
ONE_BATCH = 0  # stands for a batch that holds every photon of the design
BATCHES = [D.BATCH_SMALL, ONE_BATCH]
BATCH_IDS = ["batch_64", "one_batch"]
UNEVEN_CALLS = [1, 63, 129, 7, 300, 2]  # then the rest; with batches of 64 the calls end inside, at and beside batch boundaries
PAIR_CAP = 2048  # below the 64 * 48 = 3072 pairs that one wave of class F stages


def _t(sc, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", sc.device))


def _run(d, hashsize=D.HASHSIZE_DEFAULT, batch=ONE_BATCH, calls=(), pair_cap=0, perm=None):
    """The design's scene; its photons' events against the oracle's; a hitpoint session on its records (in the order `perm`)
    fed the photons in calls of the given sizes and then the rest.  Returns dict(hp, image, info)."""
    import cgraytracing_amd as cg
    m = len(d["org"])
    perm = np.arange(len(d["hp9"])) if perm is None else perm
    with cg.Scene(d["objs"]) as sc:
        ev = sc.photon_ray_events(d["org"], d["dirs"], d["flux"], max_depth=1)
        assert ev.shape == d["events"].shape and np.array_equal(ev, d["events"]), "the photons' events are the oracle's"
        r0 = d["r0"]
        with sc.ppm_session_hitpoints(_t(sc, d["hp9"][perm]), _t(sc, d["ray"][perm]), None, _t(sc, d["pixel"][perm]), width=d["width"],
                                      rows=d["rows"], spp=1, max_depth=1, hashsize=hashsize, alpha=d["alpha"],
                                      batch=batch if batch != ONE_BATCH else m, pair_cap=pair_cap,
                                      initial_radius=0.0 if r0 == D.R0_DEFAULT else r0) as ses:
            org, dirs, flux = _t(sc, d["org"]), _t(sc, d["dirs"]), _t(sc, d["flux"])
            off = 0
            for c in list(calls) + [m]:
                c = min(c, m - off)
                if c > 0:
                    ses.add_photon_rays(org[off:off + c], dirs[off:off + c], flux[off:off + c])
                    off += c
            assert off == m
            return dict(hp=ses.hitpoints(), image=ses.image(), info=ses.info(), photons_done=ses.photons_done)


def _check(got, d, hashsize=D.HASHSIZE_DEFAULT, pairs=False):
    table, image, cand = D.expected(d, hashsize)
    hp, inf = got["hp"], got["info"]
    m = len(d["org"])
    assert hp.shape == table.shape and inf["hp_count"] == len(table)
    assert np.array_equal(hp[:, :2], table[:, :2]), "ray / rank in table order"
    assert np.array_equal(hp[:, 2:11], table[:, 2:11]), "value, pos, normal"
    assert np.array_equal(hp[:, 15], table[:, 15]), "n: %s" % _first_diff(d, hp, table, 15)
    assert np.array_equal(hp[:, 14], table[:, 14]), "r2: %s" % _first_diff(d, hp, table, 14)
    assert np.array_equal(hp[:, 11:14], table[:, 11:14]), "flux"
    assert np.array_equal(got["image"].reshape(-1, 3), image), "image"
    assert inf["n_events"] == m and got["photons_done"] == m == inf["photons_done"]
    if pairs:
        assert inf["n_pairs"] == cand, "the candidate pairs of a single batch"


def _first_diff(d, hp, table, col):
    """class and tag of the records that differ in a column, for the assertion's message"""
    by_ray = {int(r): k for k, r in enumerate(d["ray"])}
    rows = np.nonzero(hp[:, col] != table[:, col])[0]
    return [(str(d["rec_cls"][by_ray[int(table[k, 0])]]), d["rec_tag"][by_ray[int(table[k, 0])]], hp[k, col], table[k, col])
            for k in rows[:8]] + [len(rows)]


@pytest.mark.parametrize("batch", BATCHES, ids=BATCH_IDS)
@pytest.mark.parametrize("r0", R0S, ids=R0_IDS)
def test_designed_records_and_photons(gpu_ready, orc, r0, batch):
    """Classes A-F at both radii; in batches of 64 (a record's photons in one batch or in several: the search's radius is the
    batch's first, the replay's the current one) and in one batch, whose candidate pairs are the replay's count."""
    d = D.design(orc, r0)
    _check(_run(d, batch=batch), d, pairs=batch == ONE_BATCH)


@pytest.mark.parametrize("batch", BATCHES, ids=BATCH_IDS)
@pytest.mark.parametrize("hashsize", [7, 101])
def test_colliding_cells(gpu_ready, orc, hashsize, batch):
    """Class G: a bucket is walked once per cell that hashes to it, so a photon counts twice -- unless the radius, shrunk by the
    first copy, no longer reaches."""
    d = D.design(orc, classes="ABCD")
    _check(_run(d, hashsize=hashsize, batch=batch), d, hashsize, pairs=batch == ONE_BATCH)


def test_uneven_calls(gpu_ready, orc):
    d = D.design(orc)
    assert sum(UNEVEN_CALLS) < len(d["org"])
    _check(_run(d, batch=D.BATCH_SMALL, calls=UNEVEN_CALLS), d)


def test_pair_buffer_smaller_than_one_wave_of_pairs(gpu_ready, orc):
    d = D.design(orc)
    assert PAIR_CAP < d["f_wave_pairs"]
    got = _run(d, pair_cap=PAIR_CAP)
    assert got["info"]["n_batch_halvings"] > 0
    _check(got, d)


def test_shuffled_records(gpu_ready, orc):
    """The table does not depend on the order of the input (the records' ray ids are distinct)."""
    d = D.design(orc)
    _check(_run(d, perm=np.random.default_rng(41).permutation(len(d["hp9"]))), d, pairs=True)
