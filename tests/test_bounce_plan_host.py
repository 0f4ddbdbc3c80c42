"""CPU: the launch plan of the bounce query (cgrt_rays_plan.h: RaysKind::Bounce), which cgrt_bounce_rays launches and
cgrt_bounce_rays_variant names, under ASan + UBSan (tests/native/bounce_plan.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bounce_plan_equals_the_nearest_hit_plan(tmp_path):
    """Over the trait sweep of tests/native/rays_plan.cpp (every combination scene_traits can produce; 1, 768, 769, 1000 and 2^20
    objects with 768 or 7 of them at most in LDS), max_depth 1 and 5, STATS on and off, 1, 64, 65, 100 000 and 2^36 rays: a
    Bounce plan equals the First plan field for field (flags, resident objects, LDS bytes, workgroups, refusal name), its variant
    is an entry of CGRT_RAY_VARIANTS with has_bounce and without GLASS, max_depth changes nothing; has_bounce holds for the
    nearest-hit rows only; the names of a sphere, a Bezier, a mesh and two SPILL scenes are the literal strings."""
    exe = str(tmp_path / "bounce_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    native = os.path.join(ROOT, "tests", "native")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-I", native, os.path.join(native, "bounce_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
    m = re.search(r"plans checked: (\d+)", out.stdout)
    assert m and int(m.group(1)) >= 5 * 2 * 16 * 5, out.stdout  # the sweep ran: counts x LDS lists x traits x (depth, stats, n)
