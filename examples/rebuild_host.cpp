// A mesh that moves between frames and is refitted or REBUILT by its tree cost, from a plain C++ program over
// include/cgrt_host.hpp: a triangle soup beside a mirror sphere is committed once with its structures built on the device
// (DeformingScene, CGRT_BUILD_DEVICE).  Every frame the soup is stirred -- each triangle drifts towards the place of another
// one -- and refitted; when the hierarchy's surface-area cost (DeformingScene::cost) has grown past RATIO times its value after
// the last build, the mesh is rebuilt in place instead (DeformingScene::rebuild), which brings the cost back down.  Every frame
// is compared with the frame of a scene freshly committed on the same vertices: a random soup has no exact ties, so the two
// are the same floats (cgrt.h, "rebuild", parity class).
//   cgrt_rebuild_host [--tris N] [--width W] [--height H] [--frames F] [--ratio RATIO]
// Exit status 0 and "ok: F frames equal (... R rebuilds)" when every frame matched.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cgrt_host.hpp"

using namespace cgrt_host;

static double unit(uint64_t &state) {  // splitmix64 -> [0, 1)
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0;
}

static std::vector<double> soup(int n, uint64_t seed) {
    std::vector<double> t((size_t)n * 9);
    for (int i = 0; i < n; i++) {
        const double c[3] = {-6 + 12 * unit(seed), -8 - 6 + 12 * unit(seed), 30 - 6 + 12 * unit(seed)};
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) t[(size_t)i * 9 + 3 * v + k] = c[k] + (-1.5 + 3 * unit(seed));
    }
    return t;
}

// frame f of `frames`: triangle i has drifted the fraction f / frames of the way to the place of triangle (i * 7919 + 13) % n --
// neighbours in the first pose end far apart, which is what a kept topology pays for
static std::vector<double> pose(const std::vector<double> &t0, int f, int frames) {
    const size_t n = t0.size() / 9;
    std::vector<double> t(t0.size());
    const double w = (double)f / frames;
    for (size_t i = 0; i < n; i++) {
        const size_t j = (i * 7919 + 13) % n;
        for (int k = 0; k < 3; k++) {
            const double shift = w * (t0[j * 9 + k] - t0[i * 9 + k]);
            for (int v = 0; v < 3; v++) t[i * 9 + 3 * v + k] = t0[i * 9 + 3 * v + k] + shift;
        }
    }
    return t;
}

int main(int argc, char **argv) {
    int ntri = 500, frames = 4;
    double ratio = 1.5;
    RenderParams rp;
    rp.width = 96;
    rp.height = 72;
    rp.num_of_samples = 2;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!std::strcmp(argv[i], "--tris")) ntri = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--width")) rp.width = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--height")) rp.height = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--frames")) frames = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--ratio")) ratio = std::atof(argv[i + 1]);
        else {
            std::fprintf(stderr, "unknown option %s\n", argv[i]);
            return 2;
        }
    }
    try {
        const std::vector<double> t0 = soup(ntri, 42);
        Plane floor(Vec3(0, -15, 0), Vec3(0, 1, 0), Vec3(0.75, 0.75, 0.75));
        Plane back(Vec3(0, 0, 50), Vec3(0, 0, -1), Vec3(0.25, 0.25, 0.75));
        Sphere ball(Vec3(8, -11, 26), 4, Vec3(1, 1, 1), 0.8, 0.0);
        TriangleSoup mesh(t0, Vec3(0.6, 0.7, 0.9));
        const int mesh_at = 3;
        DeformingScene scene({&floor, &back, &ball, &mesh}, 0, CGRT_BUILD_DEVICE);
        cgrt_tree_cost c = scene.cost(mesh_at);
        double built = c.node_cost + c.tri_cost;  // the cost after the last build
        std::vector<float> got, want;
        int refits = 0, rebuilds = 0;
        for (int f = 1; f <= frames; f++) {
            const std::vector<double> t = pose(t0, f, frames);
            scene.refit_mesh(mesh_at, t);
            refits++;
            c = scene.cost(mesh_at);
            const double refitted = c.node_cost + c.tri_cost;
            bool rebuilt = false;
            if (refitted > ratio * built) {
                scene.rebuild(mesh_at, t);
                c = scene.cost(mesh_at);
                built = c.node_cost + c.tri_cost;
                rebuilds++;
                rebuilt = true;
            }
            std::printf("frame %d: cost %.2f after the refit%s\n", f, refitted, rebuilt ? (", rebuilt: " + std::to_string(built)).c_str() : "");
            scene.render(rp, got);
            TriangleSoup moved(t, Vec3(0.6, 0.7, 0.9));
            render({&floor, &back, &ball, &moved}, rp, want);
            if (got != want) {
                std::fprintf(stderr, "frame %d: the %s scene's frame differs from the fresh scene's\n", f, rebuilt ? "rebuilt" : "refitted");
                return 1;
            }
        }
        const cgrt_refit_info ri = scene.refit_info(mesh_at);
        const cgrt_rebuild_info bi = scene.rebuild_info(mesh_at);
        if (ri.refits != refits || bi.rebuilds != rebuilds || ri.geometry_gen != (uint64_t)(refits + rebuilds)) {
            std::fprintf(stderr, "info: %lld refits, %lld rebuilds, generation %llu\n", (long long)ri.refits, (long long)bi.rebuilds,
                         (unsigned long long)ri.geometry_gen);
            return 1;
        }
        std::printf("ok: %d frames equal (%d triangles, %d wide nodes, %d refits, %d rebuilds)\n", frames, ri.ntris, bi.nwide, refits, rebuilds);
    } catch (const Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
