// eye_choice (cgrt_variants.h) walked over every scene class, camera and flag combination it reads, on the CPU: one line per
// distinct (form, template flags) it can return -- "sched" or "grid", then TREES BEZ DOF GLASS SPH STATS HPS NT SPILL HFONLY DIFF
// PAIR START LTAB POSE.  tests/test_eye_variants_host.py compares the lines with the lists of compiled instantiations: a row has
// SCHED=1 exactly when some launch takes the scheduled form with its flags, and no launch chooses flags that are not compiled
// (but CGRT_GRID_STATS under a pose, which the library refuses).  Then the launch record's own arithmetic (EyeLaunchLog).  Plain C++,
// no HIP.
#include <cstdio>
#include <set>
#include <vector>

#include "cgrt_variants.h"

static void line(std::set<std::vector<int>> &seen, bool sched, const EyeFlags &k) {
    const std::vector<int> v{sched, k.trees, k.bez, k.dof, k.glass, k.sph, k.stats, k.hps, k.nt, k.spill, k.hfonly, k.diff, k.pair, k.start, k.ltab, k.pose};
    if (!seen.insert(v).second) return;
    std::printf("%s", sched ? "sched" : "grid");
    for (size_t i = 1; i < v.size(); i++) std::printf(" %d", v[i]);
    std::printf("\n");
}

int main() {
    std::set<std::vector<int>> seen;
    long walked = 0;
    const int flag_bits[] = {CGRT_GRID_POSED, CGRT_GRID_STATS, CGRT_GRID_NO_REORDER, CGRT_GRID_FORCE_REORDER, CGRT_GRID_NO_SPHERE_PAIRS};
    // the scene classes scene_traits (cgrt_build.cpp) can commit: a sphere-only scene has no tree and no Bezier object; a
    // single-ray scene neither, and nothing of glass; the tile order serves spheres and planes only
    for (int bits = 0; bits < 64; bits++) {
        EyeSceneTraits d{};
        d.all_spheres = bits & 1, d.has_mesh = bits & 2, d.has_bezier = bits & 4, d.has_glass = bits & 8, d.single_ray = bits & 16, d.order_ok = bits & 32;
        if (d.all_spheres && (d.has_mesh || d.has_bezier)) continue;
        if (d.single_ray && (d.has_mesh || d.has_bezier || d.has_glass)) continue;
        if (d.order_ok && (d.has_mesh || d.has_bezier)) continue;
        for (int n_objs : {9, 900}) {
            d.n_objs = n_objs, d.n_lds = n_objs < 768 ? n_objs : 768;
            for (double lens : {0.0, 1.5})
                for (int spp : {1, 2, 4, 64})
                    for (int depth : {1, 5})
                        for (int wh : {0, 1})  // one wave tile, which is never scheduled, and a frame of several
                            for (int fb = 0; fb < 32; fb++)
                                for (int knob = 0; knob < 2; knob++)
                                    for (int capture = 0; capture < 2; capture++) {
                                        cgrt_camera cam{};
                                        cam.cam[2] = -10, cam.half_width = 10, cam.focus_plane = 20, cam.lens_radius = lens;
                                        cgrt_grid g{};
                                        g.width = wh ? 40 : 16, g.height = g.rows = wh ? 18 : 4;
                                        g.stripe_nranks = 1, g.spp = g.spp_total = spp, g.max_depth = depth;
                                        for (int b = 0; b < 5; b++)
                                            if (fb >> b & 1) g.flags |= flag_bits[b];
                                        const EyeChoice c = eye_choice(d, cam, g, knob != 0, capture != 0);
                                        walked++;
                                        line(seen, c.form == EyeForm::Sched, c.k);
                                        // eye_launch clears SPILL of the general forms where every object stays resident
                                        if (c.form == EyeForm::Capture && c.k.spill) {
                                            EyeFlags k = c.k;
                                            k.spill = false;
                                            line(seen, false, k);
                                        }
                                    }
        }
    }
    // the launch record (EyeLaunchLog): rows in launch order with the lists' columns, 16 entries and a flag beyond, cleared whole
    EyeLaunchLog log;
    const EyeFlags pair_ltab{false, false, true, true, true, false, false, false, false, kThreads, false, true, false, true, false};
    EyeFlags walk{};
    walk.dof = true;
    log.add(kEyeGrid, posed_flags(general_flags(true, true, true)));
    log.add(kEyeSched, pair_ltab);
    log.add(kEyePrimaryWalk, walk);
    int32_t r[3][kEyeLogCols];
    for (int i = 0; i < 3; i++) log.row(i, r[i]);
    const int32_t want[3][kEyeLogCols] = {{0, 1, 1, 1, 1, 0, 0, 1, 256, 1, 0, 0, 0, 0, 0, 1},
                                          {1, 0, 0, 1, 1, 1, 0, 0, 256, 0, 0, 0, 1, 0, 1, 0},
                                          {2, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
    bool ok = log.n == 3 && !log.overflow;
    for (int i = 0; i < 3; i++)
        for (int c = 0; c < kEyeLogCols; c++) ok = ok && r[i][c] == want[i][c];
    for (int i = 3; i < EyeLaunchLog::kCap; i++) log.add(kEyeGrid, pair_ltab);
    ok = ok && log.n == EyeLaunchLog::kCap && !log.overflow;
    log.add(kEyeGrid, pair_ltab);
    ok = ok && log.n == EyeLaunchLog::kCap && log.overflow;
    log.clear();
    ok = ok && log.n == 0 && !log.overflow;
    std::printf("launch record %s\n", ok ? "ok" : "FAILED");
    std::fprintf(stderr, "walked %ld launches, %zu distinct choices\n", walked, seen.size());
    return ok ? 0 : 1;
}
