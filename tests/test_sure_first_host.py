"""CPU: the proven first hit behind the sure tiles (cgrt_sure_first.h: sphere_sure_first) against every ray of a set of frames,
under ASan + UBSan and without FMA contraction (tests/native/sure_first.cpp)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_sure_first_is_sound_refuses_and_is_not_vacuous(tmp_path):
    """Every pixel of every wave tile with a winner, at 33 lens points, hits that winner first in a replica of the device's
    sphere loop (C2 thin lens and pinhole at 1920x1080, 192x108, 200x52 with ragged edges, a striped frame, row bands, C1,
    many_spheres(32)); no winner where rays can miss, with the camera inside a sphere, with a lens camera at z >= 0, over a
    sphere poking 0.01 out of a wall, beside a sphere tangent to the beam, on either copy of a duplicated wall, among 33 spheres;
    and at least 80 % of the wave tiles of C2's class-3 tiles at 1920x1080 have a winner (the program prints the share)."""
    import scenes

    exe = str(tmp_path / "sure_first")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "native", "sure_first.cpp"), "-o", exe])
    spheres = tmp_path / "many_spheres_32.txt"
    with open(spheres, "w") as f:
        for s in scenes.many_spheres(32, 11):
            f.write("%r %r %r %r %d\n" % (float(s.center[0]), float(s.center[1]), float(s.center[2]), float(s.radius),
                                           1 if (s.reflection > 0 or s.transparency > 0) else 0))
    out = subprocess.run([exe, str(spheres)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "scene file, lens" in out.stdout
    assert "ok: 0 failed checks" in out.stdout, out.stdout
