// What the commit makes of a list of planes: ObjRec.axis of every plane (HostScene::add_plane: >= 0 only for a normal that is
// exactly +-e_k) and the run [prun_begin, prun_end) that scene_traits finds (cgrt_build.cpp).  Reads one object per line from
// stdin -- the scenes of tests/scenes.py run_rooms(), written out by tests/test_planes_general_host.py --
//     plane px py pz nx ny nz refl transp bump      (bump = 1: an opaque bump map over a 12 x 15 texture)
//     sphere refl transp | mesh transp | bezier
// with the doubles as C99 hex floats, and prints "prun_begin prun_end" and then kind:axis of every object.  Plain CPU build.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cgrt_build.h"

using namespace cgrt;

int main() {
    HostScene H;
    const double grey[3] = {0.5, 0.5, 0.5};
    char line[512];
    while (std::fgets(line, sizeof line, stdin)) {
        char kind[16];
        int used = 0;
        if (std::sscanf(line, "%15s%n", kind, &used) != 1) continue;
        std::vector<double> v;
        char *p = line + used, *end = p;
        for (double x = std::strtod(p, &end); end != p; x = std::strtod(p, &end)) {
            v.push_back(x);
            p = end;
        }
        int id = -1;
        if (!std::strcmp(kind, "plane") && v.size() == 9) {
            int tex = -1;
            if (v[8] != 0) {
                std::vector<uint8_t> rgb(12 * 15 * 3);
                for (size_t k = 0; k < rgb.size(); k++) rgb[k] = (uint8_t)(k * 37u & 255u);
                const double n[3] = {0, 1, 0}, at[3] = {-21, 0, 0};
                tex = H.add_texture(rgb.data(), 12, 15, n, at, 42, 40, 1);
            }
            id = H.add_plane(&v[0], &v[3], grey, v[6], v[7], tex);
        } else if (!std::strcmp(kind, "sphere") && v.size() == 2) {
            const double c[3] = {0, 0, 20};
            id = H.add_sphere(c, 1.0, grey, v[0], v[1]);
        } else if (!std::strcmp(kind, "mesh") && v.size() == 1) {
            const double t9[18] = {0, 0, 30, 1, 0, 30, 0, 1, 30, 1, 1, 30, 1, 0, 30, 0, 1, 30};
            id = H.add_mesh_triangles(t9, 2, grey, 0.0, v[0], 0);
        } else if (!std::strcmp(kind, "bezier")) {
            const double cp[4 * 3] = {0, 0, 0.5, 0, 0.5, 1.0, 0, 1.0, 0.8, 0, 1.5, 0.2}, pos[3] = {3, -4, 25};
            id = H.add_bezier(cp, 4, pos, grey, 0, 0);
        }
        if (id < 0) {
            std::fprintf(stderr, "bad line: %s", line);
            return 2;
        }
    }
    const CommitKnobs knobs;
    const SceneLayout L = scene_layout(H, knobs);
    DeviceScene d{};
    scene_traits(H, L.trees, knobs, d);
    std::printf("%d %d", d.prun_begin, d.prun_end);
    for (const ObjRec &o : H.objs) std::printf(" %d:%d", (int)o.kind, o.kind == KIND_PLANE ? (int)o.axis : -1);
    std::printf("\n");
    return 0;
}
