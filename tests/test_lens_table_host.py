"""CPU: the lens table of classes 0-2 (cgrt_lens_stage.h) -- the table's layout and capacity rule, simulated waves of 64 lanes
through lens_table_kernel's per-thread routine against the per-sample rejection loop, and the frame plan's conditions with and
without CGRT_GRID_NO_LENS_TABLE (tests/native/lens_table.cpp), built without FMA contraction, under ASan + UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lens_table_under_sanitizers(tmp_path):
    """lens_table_at is injective and in bounds at budgets of nothing, one entry, an exact fit and too little; every table draw of
    50 waves at 1, 31, 32, 33 and 64 samples, sample offsets 0 and 3, rebuilds the bits of the per-sample loop, dead lanes write 0;
    C2's plan and parameters differ between flag and no flag in the table's fields alone."""
    exe = str(tmp_path / "lens_table")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "native", "lens_table.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
    m = re.search(r"draws compared: (\d+)", out.stdout)
    assert m and int(m.group(1)) >= 50000, out.stdout
