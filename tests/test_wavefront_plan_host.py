"""CPU: the wavefront trace's plan (cgrt_wavefront_plan.h) and the launch plan of its levels (cgrt_rays_plan.h:
RaysKind::Wavefront), under ASan + UBSan (tests/native/wavefront_plan.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wavefront_plan(tmp_path):
    """The sort key orders the leaf sets of 4 000 random binary trees down to level 31 exactly as a recursive depth-first walk
    (reflected subtree first) and as emission_order's left-aligned bit strings, also at path 1, 2^30 and 2^31 - 1 and at local
    root 0 and the largest a slice can hold; its inverse round-trips; the radix sort's end_bit covers every key of a slice and
    no bit more, its begin_bit leaves out only bits that are zero in every key of a tree of that many levels; capacities from
    work_bytes never exceed it and a refusal's byte count is enough; the default work memory respects both bounds; the slice schedule covers every root once and in order under scripted overflows and ends with a failure
    exactly when a one-root slice overflows; a Wavefront plan equals the First plan field for field over the trait sweep of
    tests/native/rays_plan.cpp; the kernel names of a sphere, a mesh, a Bezier and the two SPILL scenes are the literal
    strings."""
    exe = str(tmp_path / "wavefront_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    native = os.path.join(ROOT, "tests", "native")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-I", native, os.path.join(native, "wavefront_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
    m = re.search(r"trees checked: (\d+) \((\d+) leaves, deepest level (\d+)\)", out.stdout)
    assert m and int(m.group(1)) >= 3000 and int(m.group(2)) >= 10000 and int(m.group(3)) == 31, out.stdout
    m = re.search(r"plans checked: (\d+)", out.stdout)
    assert m and int(m.group(1)) >= 5 * 2 * 16 * 5, out.stdout
