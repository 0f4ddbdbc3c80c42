// A mesh that moves between frames, from a plain C++ program over include/cgrt_host.hpp: a triangle soup beside a mirror sphere
// is committed once (DeformingScene), then given new vertices per frame with refit_mesh -- rotated about y, squashed and
// jittered -- and rendered.  Every refitted frame is compared with the frame of a scene freshly committed on the same
// vertices: a random soup has no exact ties, so the two are the same floats (cgrt.h, "refit", parity class).
//   cgrt_refit_host [--tris N] [--width W] [--height H] [--frames F] [--png PREFIX]
// Exit status 0 and "ok: F frames equal" when every frame matched.
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

// frame f of the animation: a turn about the vertical axis through (0, -8, 30), a squash, a little noise per vertex
static std::vector<double> pose(const std::vector<double> &t0, int f) {
    std::vector<double> t(t0.size());
    const double a = 0.35 * f, ca = std::cos(a), sa = std::sin(a), sy = 1.0 / (1.0 + 0.25 * f);
    uint64_t seed = 1000 + (uint64_t)f;
    for (size_t v = 0; v < t0.size(); v += 3) {
        const double x = t0[v], y = t0[v + 1] + 8, z = t0[v + 2] - 30;
        t[v] = ca * x + sa * z + 0.05 * unit(seed);
        t[v + 1] = sy * y - 8 + 0.05 * unit(seed);
        t[v + 2] = -sa * x + ca * z + 30 + 0.05 * unit(seed);
    }
    return t;
}

int main(int argc, char **argv) {
    int ntri = 500, frames = 3;
    RenderParams rp;
    rp.width = 96;
    rp.height = 72;
    rp.num_of_samples = 2;
    std::string png;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!std::strcmp(argv[i], "--tris")) ntri = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--width")) rp.width = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--height")) rp.height = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--frames")) frames = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--png")) png = argv[i + 1];
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
        DeformingScene scene({&floor, &back, &ball, &mesh});
        std::vector<float> got, want;
        for (int f = 1; f <= frames; f++) {
            const std::vector<double> t = pose(t0, f);
            scene.refit_mesh(mesh_at, t);
            scene.render(rp, got);
            TriangleSoup moved(t, Vec3(0.6, 0.7, 0.9));
            render({&floor, &back, &ball, &moved}, rp, want);
            if (got != want) {
                std::fprintf(stderr, "frame %d: the refitted scene's frame differs from the fresh scene's\n", f);
                return 1;
            }
            if (!png.empty()) {
                std::vector<unsigned char> rgb8(got.size());
                for (size_t i = 0; i < got.size(); i++) {
                    const float c = got[i] < 0 ? 0.f : (got[i] > 1 ? 1.f : got[i]);
                    rgb8[i] = (unsigned char)(std::pow(c, 1 / 2.2f) * 255 + 0.5f);
                }
                // (row 0 of the frame is the bottom row: flip)
                std::vector<unsigned char> flip(rgb8.size());
                const size_t row = (size_t)rp.width * 3;
                for (int y = 0; y < rp.height; y++) std::memcpy(&flip[(size_t)y * row], &rgb8[(size_t)(rp.height - 1 - y) * row], row);
                write_png((png + std::to_string(f) + ".png").c_str(), rp.width, rp.height, flip);
            }
        }
        const cgrt_refit_info inf = scene.refit_info(mesh_at);
        if (inf.refits != frames || inf.geometry_gen != (uint64_t)frames || !inf.plan_built) {
            std::fprintf(stderr, "refit_info: %lld refits, generation %llu\n", (long long)inf.refits, (unsigned long long)inf.geometry_gen);
            return 1;
        }
        std::printf("ok: %d frames equal (%d triangles, %d wide nodes, plan %.2f ms)\n", frames, inf.ntris, inf.nwide, inf.ms_plan);
    } catch (const Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
