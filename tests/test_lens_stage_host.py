"""CPU: lens points staged ahead of the sample loop (cgrt_lens_stage.h) -- simulated waves of 64 lanes through the header's
stager against the per-sample rejection loop, the rounds a wave needs per sample, the LDS slots' layout and the frame plan's
conditions (tests/native/lens_stage.cpp), built without FMA contraction, under ASan + UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lens_stage_under_sanitizers(tmp_path):
    """At least 10^5 (pixel, first sample, count) draws at counts 0, 1, 15, 16, 17, 32 and 64, with dead lanes, sample offsets and
    streams of six attempts and more: every staged draw rebuilds the bits of the per-sample loop.  Rounds per sample over 1000
    waves: at most 1.8 at batches of 16 and 1.65 at 32 (the per-sample loop: above 3)."""
    exe = str(tmp_path / "lens_stage")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "native", "lens_stage.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
    m = re.search(r"draws compared: (\d+), of them with >= 6 attempts: (\d+)", out.stdout)
    assert m and int(m.group(1)) >= 100000 and int(m.group(2)) >= 64, out.stdout
