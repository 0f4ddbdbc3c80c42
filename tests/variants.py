"""The kernel variants that are compiled, read from cgraytracing_amd/csrc/cgrt_variants.h itself: the X(...) entries of
CGRT_EYE_VARIANTS, CGRT_EYE_POSED_VARIANTS and CGRT_RAY_VARIANTS as tuples of ints, and the two families derived from the ray list by the header's rules
(has_capture, has_occlusion)."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cgraytracing_amd", "csrc", "cgrt_variants.h")


def _entries(macro, columns):
    lines = open(HEADER).read().split("\n")
    at = next(i for i, line in enumerate(lines) if line.startswith("#define %s(X)" % macro))
    end = next(i for i in range(at, len(lines)) if not lines[i].rstrip().endswith("\\"))  # the macro's last line
    out = [tuple(int(x) for x in m.split(",")) for m in re.findall(r"\bX\(([\d,\s]+)\)", "\n".join(lines[at + 1:end + 1]))]
    assert out and all(len(v) == columns for v in out), (macro, out)
    return out


def eye_variants():
    """(TREES, BEZ, DOF, GLASS, SPH, STATS, HPS, NT, SPILL, HFONLY, DIFF, PAIR, START, LTAB, SCHED) of every trace_grid_kernel."""
    return _entries("CGRT_EYE_VARIANTS", 15)


def posed_eye_variants():
    """The same columns of every trace_grid_kernel with POSE (CGRT_EYE_POSED_VARIANTS)."""
    return _entries("CGRT_EYE_POSED_VARIANTS", 15)


def ray_variants():
    """(TREES, BEZ, GLASS, SPH, STATS, SPILL, FIRST, NT) of every trace_rays_kernel."""
    return _entries("CGRT_RAY_VARIANTS", 8)


def capture_variants():
    """(TREES, BEZ, GLASS, SPH, SPILL, NT) of every capture_rays_kernel: has_capture(f) is !f.stats && !f.first."""
    return [(t, b, g, p, sp, nt) for t, b, g, p, s, sp, f, nt in ray_variants() if not s and not f]


def occlusion_variants():
    """(TREES, BEZ, SPH, STATS, SPILL, NT) of every occlusion_rays_kernel: has_occlusion(f) is f.first; no such entry has GLASS."""
    first = [v for v in ray_variants() if v[6]]
    assert all(v[2] == 0 for v in first), first
    return [(t, b, p, s, sp, nt) for t, b, g, p, s, sp, f, nt in first]
