"""CPU: the host side of cgrt_scene_commit -- where every record goes in the device arrays (scene_layout) and the DeviceScene
fields that select kernel variants (scene_traits) -- on hand-checked scenes, under ASan + UBSan (tests/native/commit_layout.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_commit_layout_and_traits_under_sanitizers(tmp_path):
    """Diffuse spheres, plane runs (with a bump floor in front), one opaque mesh with and without a bump floor, glass and
    Bezier objects, more objects than the LDS list holds and the LDS cap, the reference tree order, device-built trees
    behind host-built records, and the commit's switches read afresh at every commit."""
    exe = str(tmp_path / "commit_layout")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "commit_layout.cpp"),
                           os.path.join(csrc, "cgrt_build.cpp"), "-pthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
