"""CPU: the order of caller-supplied Hitpoint records (cgrt_hp_order.h: the total path key, which records are kept, the radix
passes' widths) against bit-string comparisons written out in the test program, under ASan + UBSan (tests/native/hp_order.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hp_order_under_sanitizers(tmp_path):
    """For every path with up to 10 bits behind its leading 1 and a few hundred random ones up to 30 bits: comparing keys is
    comparing the bit strings lexicographically with a prefix first; distinct paths have distinct keys; the key's upper 30 bits
    are wavefront_sort_key(0, path); every key is below 2^35."""
    exe = str(tmp_path / "hp_order")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    # no ROCm include path: the header is plain C++
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "hp_order.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
