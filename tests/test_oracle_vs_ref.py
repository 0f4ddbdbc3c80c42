"""CPU: the oracle against the compiled reference's answers on random and procedural cases, stored in
tests/golden/oracle_vs_ref.npz (tests/golden/make_golden.py oracle_vs_ref, which builds the cases below).  Complements
the other golden vectors with fresh random cases; every comparison is exact.  Frame sums and hitpoint streams are compared
through make_golden.array_digest (equal digests <=> np.array_equal), which keeps the stored file small."""
import os
import sys

import numpy as np
import pytest

import scenes
from backends import BackendScene, lens_samples

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD_DIR)
import make_golden  # noqa: E402

GOLD = np.load(os.path.join(GOLD_DIR, "oracle_vs_ref.npz"))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sphere_scenes(orc, seed):
    a = BackendScene(orc, make_golden.random_sphere_scene(seed)).trace_grid(scenes.cam_dof(), 80, 60, 3, 5, seed=seed,
                                                                             capture=True)
    assert a["nrays"] == int(GOLD["spheres%d_nrays" % seed]) and len(a["hp"]) == int(GOLD["spheres%d_nhp" % seed])
    assert make_golden.array_digest(a["acc_sum"]) == str(GOLD["spheres%d_acc_sum_sha256" % seed])
    assert make_golden.array_digest(a["hp"]) == str(GOLD["spheres%d_hp_sha256" % seed])


def test_procedural_glass_mesh(orc):
    a = BackendScene(orc, make_golden.procedural_glass_mesh_scene()).trace_grid(scenes.cam_dof(), 64, 64, 2, 5, capture=True)
    assert a["nrays"] == int(GOLD["mesh_nrays"]) and len(a["hp"]) == int(GOLD["mesh_nhp"])
    assert make_golden.array_digest(a["hp"]) == str(GOLD["mesh_hp_sha256"])


def test_lens_sampler(orc):
    assert np.array_equal(lens_samples(orc, *make_golden.lens_probe()), GOLD["lens_out"])


def test_bezier_function_level(orc):
    h1, l1, n1 = BackendScene(orc, [scenes.vase_bezier()]).intersect_batch(0, *make_golden.bezier_probe())
    h2, l2, n2 = GOLD["bez_hit"], GOLD["bez_len"], GOLD["bez_n"]
    assert np.array_equal(h1, h2) and np.array_equal(l1, l2) and np.array_equal(n1[h1 == 1], n2[h2 == 1])
