"""CPU: the candidate test behind the terminal-diffuse body's sphere masks (cgrt_sphere_mask.h: sphere_surely_missed) against
every ray of a set of frames, under ASan + UBSan and without FMA contraction (tests/native/sphere_mask.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sphere_masks_are_conservative_and_not_vacuous(tmp_path):
    """No sphere the test drops from a wave tile gets a distance from sphere_len for any pixel of the tile at 33 lens points (C2
    at 1920x1080 and with partial tiles, pinhole, a tiny and a huge lens, cameras off centre, in the room and inside a wall
    sphere, spheres at the lens plane and behind the camera, a sphere tangent to a tile's outermost ray, two stripe mappings);
    and on the C2 frame a class-3 wave tile keeps at most 3.5 of the 8 spheres on average."""
    exe = str(tmp_path / "sphere_mask")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "native", "sphere_mask.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
