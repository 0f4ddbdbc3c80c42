"""CPU: the launch plan of the ray-list queries (cgrt_rays_plan.h: rays_plan), which cgrt_trace_rays, the Hitpoint capture over a
ray buffer and cgrt_occlusion_rays launch and the three *_variant entry points name, under ASan + UBSan
(tests/native/rays_plan.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rays_plan_over_every_trait_combination(tmp_path):
    """Every trait combination scene_traits can produce (spheres only: no tree, no Bezier object; cached and wide trees only with
    a tree), 1, 768, 769, 1000 and 2^20 objects with 768 or 7 of them at most in LDS, max_depth 1 and 5, STATS on and off, the
    four kinds of query: the chosen flags are an entry of CGRT_RAY_VARIANTS that has a capture kernel for a capture and an
    occlusion kernel for an occlusion query; the LDS is the variant's layout for the resident count and fits 160 KiB beside the
    static bytes; the general variant keeps 723 / 659 objects resident beside a full list (wg_lds.cpp's 727 / 663 at 336 B
    static, less its four staging records); the workgroup count is the written-out formula at 1, 64, 65 and 2^36 rays and at one
    and two chips' worth of rays plus and minus a block; the names of five fixed scenes are the literal strings."""
    exe = str(tmp_path / "rays_plan")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "rays_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
    m = re.search(r"plans checked: (\d+)", out.stdout)
    assert m and int(m.group(1)) >= 5 * 2 * 16 * 4, out.stdout  # the sweep ran: counts x LDS lists x (depth, stats, kind) x traits
