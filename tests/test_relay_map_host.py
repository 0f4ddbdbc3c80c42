"""CPU: the sample relay's index arithmetic (cgrt_relay.h) and its part of the frame plan (cgrt_frame.h), which the host and
trace_grid_kernel share, under ASan + UBSan (tests/native/relay_map.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relay_map_chunks_bytes_and_capacity(tmp_path):
    """Launches of 1, 15, 105 and 8100 tiles with 0, 1, half and all of them of class 0 or 1, an area for 0, 1, 3 and all tiles,
    K = 2, 3, 4: every workgroup of the grid renders exactly one (entry, chunk) or leaves, every (entry, chunk) that should
    exist is rendered once, the entries at or behind plan[3] are the diffuse body's; the chunks of 32, 33, 48, 64, 70 and 1024
    samples partition [0, spp); bytes per tile equal the written-out sum; the capacity respects the budget and the bound; the
    frame plan engages the relay only from 32 samples and 4 tiles per compute unit on, or by its flag."""
    exe = str(tmp_path / "relay_map")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "relay_map.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
