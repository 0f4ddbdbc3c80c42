"""CPU: a workgroup's dynamic LDS layout (cgrt_wg_lds.h: wg_lds), which the launch plans and the kernels' carve-up both use,
for every compiled kernel variant against byte counts written out from the record sizes, under ASan + UBSan
(tests/native/wg_lds.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wg_lds_layout_matches_the_written_out_byte_counts(tmp_path):
    """Every flag tuple of CGRT_EYE_VARIANTS and CGRT_RAY_VARIANTS (cgrt_variants.h, walked by the program; the four START / LTAB
    twins' LDS equal to their PAIR parents'), the photon forms and the primary walk at 0, 1, 255,
    257, 600, 727 and 768 objects, with and without a 255-node cached tree and a wide tree: regions in the documented order,
    16-byte aligned and disjoint, the total the end of the last one and equal to the literal formula (ObjRec 128 B, pending
    levels 38 912 B at 256 threads and a quarter at 64, BezLds 7 872 B per wave, node 32 B, wide stack 32 768 B); the general
    variant's resident limits 727 / 663 beside 336 B static; an HFONLY variant has no node and no wide-stack region."""
    exe = str(tmp_path / "wg_lds")
    csrc = os.path.join(ROOT, "cgraytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "wg_lds.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr
    assert "ok: 0 failed checks" in out.stdout, out.stdout
