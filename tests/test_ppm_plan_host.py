"""CPU: the host side of the photon pass -- batch size, pair buffer, sort key width, overlap, the hash cell (cgrt_ppm_plan.h:
ppm_setup, ppm_grid) and the batch schedule that cgrt_ppm_session::photons follows (PpmSchedule) -- driven by a fake pair counter
in place of the GPU, under ASan + UBSan (tests/native/ppm_plan.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ppm_plan_under_sanitizers(tmp_path):
    """Setup values on hand-checked inputs; the applied batches tile the photons once and in order through every chunking and
    overflow; no batch beyond batch_max (a batch halved from a non-power-of-two size and grown back included); the one-photon
    overflow; reuse of the batch traced ahead only when first and count match, and never of one whose produce failed; three
    decision traces written out by hand; and step-for-step agreement with the loop as it stood before the schedule left it."""
    exe = str(tmp_path / "ppm_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    # no ROCm include path: the header is plain C++
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "ppm_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
