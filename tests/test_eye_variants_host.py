"""CPU: the lists of compiled eye kernels (CGRT_EYE_VARIANTS, CGRT_EYE_POSED_VARIANTS of cgrt_variants.h) against the chooser.

tests/native/eye_choice_walk.cpp walks eye_choice over every scene class, camera and flag combination and prints each distinct
choice.  A row's SCHED column is 1 exactly when some launch takes the scheduled form with the row's flags; every flag tuple a
launch can choose is compiled (but CGRT_GRID_STATS under a pose, which the library refuses); and the rows no launch chooses as
its main kernel are the ones the launch sequence derives from it -- the light tiles' HFONLY form, the diffuse launch and the START
and LTAB twins.  This pins what test_gpu_eye_variants.py expects to see launched to the chooser without a GPU."""
import os
import subprocess

import pytest

import variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = "TREES BEZ DOF GLASS SPH STATS HPS NT SPILL HFONLY DIFF PAIR START LTAB".split()
STATS, HFONLY, DIFF, START, LTAB = (COLUMNS.index(c) for c in ("STATS", "HFONLY", "DIFF", "START", "LTAB"))


def table_rows():
    """{(the 14 columns..., POSE)} of both lists, and the subset with SCHED=1"""
    rows = [v[:14] + (0,) for v in variants.eye_variants()] + [v[:14] + (1,) for v in variants.posed_eye_variants()]
    sched = [v[:14] + (pose,) for pose, lst in ((0, variants.eye_variants()), (1, variants.posed_eye_variants())) for v in lst if v[14]]
    assert len(set(rows)) == len(rows), "a row stands twice in a list"
    return set(rows), set(sched)


def test_lists_have_fifteen_columns():
    plain, posed = variants.eye_variants(), variants.posed_eye_variants()
    assert len(plain) >= 34 - 4 and len(posed) >= 20  # (the lists may lose a dead row; they do not vanish)
    for v in plain + posed:
        assert len(v) == 15 and v[7] in (64, 256) and all(x in (0, 1) for x in v[:7] + v[8:]), v
    # POSE forms have no STATS, HFONLY, DIFF, PAIR, START or LTAB column set (cgrt_frame.h: no tile order, no light split)
    assert all(not any(v[c] for c in (STATS, HFONLY, DIFF, COLUMNS.index("PAIR"), START, LTAB)) for v in posed)


@pytest.fixture(scope="module")
def choices(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eye_choice") / "eye_choice_walk")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", csrc, os.path.join(ROOT, "tests", "native", "eye_choice_walk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    sched, grid = set(), set()
    assert "launch record ok" in out.stdout, out.stdout[-300:]
    for ln in out.stdout.split("\n"):
        if ln and not ln.startswith("launch record"):
            form, *cols = ln.split()
            assert form in ("sched", "grid") and len(cols) == 15, ln
            (sched if form == "sched" else grid).add(tuple(int(c) for c in cols))
    assert len(sched) >= 20 and len(grid) >= 40, out.stderr
    return sched, grid


def test_sched_column_is_what_the_chooser_schedules(choices):
    sched, _ = choices
    _, want = table_rows()
    sched = {v for v in sched if not (v[STATS] and v[14])}  # (CGRT_GRID_STATS under a pose is refused: no such kernel, in either form)
    assert sched == want, dict(sched_column_nothing_selects=sorted(want - sched), scheduled_without_sched_column=sorted(sched - want))


def test_every_choice_is_compiled_and_the_rest_is_derived(choices):
    sched, grid = choices
    rows, _ = table_rows()
    chosen = sched | grid
    refused = {v for v in chosen if v[STATS] and v[14]}  # CGRT_GRID_STATS under a pose: CGRT_ERR_UNSUPPORTED
    assert chosen - rows == refused, sorted(chosen - rows - refused)
    derived = {v for v in rows if v[HFONLY] or v[DIFF] or v[START] or v[LTAB]}
    assert rows - chosen == derived, dict(never_chosen=sorted(rows - chosen - derived), chosen_though_derived=sorted(derived - (rows - chosen)))
