"""CPU: the inside trips' rule (cgrt_inside_sphere.h: inside_mask, starts_inside, inside_trait) against a replica of the device's
sphere loop, under ASan + UBSan and without FMA contraction (tests/native/inside_sphere.cpp)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_inside_mask_is_sound_refuses_and_is_not_vacuous(tmp_path):
    """For every refracting sphere of C2, of C2 with the glass sphere touching and overlapping the floor, 1e-3 and 0.1 from a wall,
    overlapping the mirror, around a small diffuse sphere, inside a larger glass sphere, beside a second glass sphere, with
    kInsideMax + 1 glass spheres and of many_spheres(32): rays from the shell r - kEps, the shell at r_in, the centre and random
    points inside, in random, aimed, grazing, tangential and centre-line directions, end on the same (len, id) in the loop over all
    spheres and in the loop over the mask.  Spheres that are not finite or too small give the full mask, too many candidates or
    spheres no trait.  C2's glass sphere keeps only itself, and the simulated body over its centre has every active lane inside in
    at least a third of its trips (the program prints the share)."""
    import scenes

    exe = str(tmp_path / "inside_sphere")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "native", "inside_sphere.cpp"), "-o", exe])
    spheres = tmp_path / "many_spheres_32.txt"
    with open(spheres, "w") as f:
        for s in scenes.many_spheres(32, 11):
            f.write("%r %r %r %r %r %r\n" % (float(s.center[0]), float(s.center[1]), float(s.center[2]), float(s.radius),
                                             float(s.reflection), float(s.transparency)))
    out = subprocess.run([exe, str(spheres)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "scene file" in out.stdout
    assert "ok: 0 failed checks" in out.stdout, out.stdout
