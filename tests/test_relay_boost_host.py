"""CPU: four chunks for the relay's heaviest tiles (cgrt_relay.h), the rule the host, the relay_boost kernels and the GPU test
share, and the frame plan's choice of it (cgrt_frame.h), under ASan + UBSan (tests/native/relay_boost.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name):
    exe = str(tmp_path / name)
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout


def test_relay_boost_table_and_frame_plan(tmp_path):
    """Lists of 1, 28, 105 and 600 tiles; 64, 70 (short last chunk), 48 (three chunks) and 40 samples (nothing to promote to: the
    table is relay_start_table's word for word); thresholds 0/1 (all that fit), a mid value with both kinds present and one above
    every weight (none: relay_start_table's table again); a boost area for 0 tiles, for 1 and ending inside the promoted set --
    the heaviest entries win, ties in entry order; both extents; plan[2] = 0, plan[3] = plan[2]; equal costs, costs with zeros.
    The items are a permutation of exactly the (entry, chunk) set the rule defines, every sample of every tile lies in exactly
    one item, weights do not increase along the table with ties in order, nothing is written beyond the item count, and the
    kernels' batched counts over virtual items give the same slots and the same table.  The frame plan: spheres(1920, 1080) at 64
    samples plans promotion with k_boost 4 while relay_k, relay_start_words, relay_cap and relay_order keep their values; at 32 and
    40 samples there is none; flags and knob switch it either way, flags before the knob; a list start never promotes; the order
    buffer's new parts lie behind the old ones."""
    _run(tmp_path, "relay_boost")
