"""CPU: the relay's start order by cost (cgrt_relay.h), which the host, relay_start_kernel and the GPU test share, and the frame
plan's choice of it (cgrt_frame.h), under ASan + UBSan (tests/native/relay_start.cpp, tests/native/frame_plan_start.cpp)."""
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


def test_relay_start_table(tmp_path):
    """Lists of 1, 28, 105 and 600 tiles; K = 2, 3, 4 at 32, 40 and 64 samples and with a short last chunk (33, 50, 70); an area
    for 0 and 1 tiles, ending below, inside and beyond each class; plan[2] = 0, plan[3] = plan[2], plan[3] = 0 and a list wholly of
    classes 0-2; both extents; varied costs, equal costs, costs with zeros and all zero.  The table is a permutation of exactly
    the (entry, chunk) relay_block_ordered gives to b < t (the same set in all three orders), weights do not increase along it,
    ties stand in (entry, chunk) order, an item's weight is its tile's largest wave cost times the samples it runs, nothing is
    written beyond t, and the ranking kernel's batched count gives the same table; the table's parts of the order buffer lie
    behind the parts of a launch without one."""
    _run(tmp_path, "relay_start")


def test_frame_plan_relay_start(tmp_path):
    """spheres(1920, 1080) plans the cost start with the interleaved order behind it; an order named by flag or by knob, a relay
    asked for by flag, no relay, the second launch and fewer than 32 samples give the list; the flags and the knob
    CGRT_RELAY_START switch it either way, flags before the knob; the probe never has more samples than the launch; the table's
    words are the launch's workgroups.  The four form decisions (extent, order, start, promotion) equal the header's rules,
    restated by the test, for every combination of the relay's flags and knobs (31 104 of them)."""
    _run(tmp_path, "frame_plan_start")
