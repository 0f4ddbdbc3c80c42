"""CPU: the host side of cgrt_trace_grid -- sample chunks, tile counts, heavy-tile capacity, scheduling and the layout of the
handle's launch scratch (cgrt_frame.h: frame_plan) -- on hand-checked frames, under ASan + UBSan (tests/native/frame_plan.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_plan_under_sanitizers(tmp_path):
    """Chunking and its 4 GiB cap, row-major / XCD / one-wave tile counts, kmax from the device, the budget and the wave tiles,
    the scratch regions at several capacities (inside the total, disjoint, aligned, the total of the rule), the scheduled
    launch's queue sizes and switches, the fitting rule against a refused size, and the eye pass's switches."""
    exe = str(tmp_path / "frame_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "frame_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
