"""CPU: the sample relay's launch map with an extent and an order (relay_block_ordered, cgrt_relay.h) and the frame plan's choice
of both (cgrt_frame.h), which the host and trace_grid_kernel share, under ASan + UBSan (tests/native/relay_order.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relay_order_map_and_plan(tmp_path):
    """Launches of 1, 15, 105 and 8100 tiles; plan[3] at 0, 1, the middle and the end of the list and plan[2] likewise within it;
    an area for 0 and 1 tiles, ending inside classes 0-1, at plan[2], inside class 2, at plan[3] and holding the whole list;
    K = 2, 3, 4; both extents, all three orders.  Every workgroup of relay_grid renders exactly one (entry, chunk) or leaves,
    and those that leave are the launch's last; every (entry, chunk) that should exist -- K per split entry, one per other --
    is rendered once; the split entries are the prefix the extent names; the glass extent with chunks first is relay_block
    for every workgroup; mirror first puts every class-2 workgroup before any of classes 0-1; interleaved keeps the class-2
    count of every prefix within one of its share; both sequences keep their order in every form; class 3 follows in entry
    order.  The plan: both are 0 unless the relay is engaged, CGRT_GRID_SAMPLE_RELAY alone keeps classes 0-1 and chunks
    first, flags go before knobs."""
    exe = str(tmp_path / "relay_order")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "relay_order.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
