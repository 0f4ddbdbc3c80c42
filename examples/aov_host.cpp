// A frame's feature buffers from a plain C++ program over include/cgrt_host.hpp: render_aov gives, per pixel, the first hit's
// albedo, normal, depth, coverage and object -- here of two planes, a diffuse and a glass sphere under the pinhole camera --,
// which the program checks against what it knows of the scene (an untextured object's albedo is its colour, a sphere's normal
// points from its centre to the hit, the hit lies at `depth` along the pixel's ray) and against the same call on a scene
// committed once (DeformingScene::render_aov).
//   cgrt_aov_host [--width W] [--height H] [--png PREFIX]
// Exit status 0 and "ok: ..." when everything matched; with --png, PREFIXalbedo.png, PREFIXnormal.png and PREFIXdepth.png.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cgrt_host.hpp"

using namespace cgrt_host;

// a [height][width][3] float frame in [0, 1], row 0 = bottom, as an 8-bit PNG
static void png3(const std::string &path, int width, int height, const std::vector<float> &v) {
    std::vector<unsigned char> rgb8(v.size());
    const size_t row = (size_t)width * 3;
    for (int y = 0; y < height; y++)
        for (size_t c = 0; c < row; c++) {
            const float x = v[(size_t)(height - 1 - y) * row + c];
            rgb8[(size_t)y * row + c] = (unsigned char)((x < 0 ? 0.f : (x > 1 ? 1.f : x)) * 255 + 0.5f);
        }
    write_png(path.c_str(), width, height, rgb8);
}

int main(int argc, char **argv) {
    RenderParams rp;
    rp.width = 96;
    rp.height = 72;
    rp.num_of_samples = 1;
    std::string png;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!std::strcmp(argv[i], "--width")) rp.width = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--height")) rp.height = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--png")) png = argv[i + 1];
        else {
            std::fprintf(stderr, "unknown option %s\n", argv[i]);
            return 2;
        }
    }
    try {
        const double col[4][3] = {{0.75, 0.75, 0.75}, {0.25, 0.25, 0.75}, {0.9, 0.3, 0.2}, {1, 1, 1}};
        const double centre[2][3] = {{-5, -9, 28}, {6, -10, 24}}, radius[2] = {6, 5};
        Plane floor(Vec3(0, -15, 0), Vec3(0, 1, 0), Vec3(col[0][0], col[0][1], col[0][2]));
        Plane back(Vec3(0, 0, 50), Vec3(0, 0, -1), Vec3(col[1][0], col[1][1], col[1][2]));
        Sphere matte(Vec3(centre[0][0], centre[0][1], centre[0][2]), radius[0], Vec3(col[2][0], col[2][1], col[2][2]), 0.0, 0.0);
        Sphere glass(Vec3(centre[1][0], centre[1][1], centre[1][2]), radius[1], Vec3(col[3][0], col[3][1], col[3][2]), 0.0, 0.9);
        const std::vector<Object *> objs = {&floor, &back, &matte, &glass};
        GridAov a, b;
        RenderStats st;
        render_aov(objs, rp, a, &st);
        DeformingScene(objs).render_aov(rp, b);
        if (a.albedo != b.albedo || a.normal != b.normal || a.depth != b.depth || a.hits != b.hits || a.obj_id != b.obj_id) {
            std::fprintf(stderr, "render_aov and DeformingScene::render_aov differ\n");
            return 1;
        }
        const size_t npx = (size_t)rp.width * rp.height;
        if (st.rays != npx) {
            std::fprintf(stderr, "%llu rays for %zu pixels\n", (unsigned long long)st.rays, npx);
            return 1;
        }
        size_t seen[5] = {0, 0, 0, 0, 0};
        double cam[3];
        rp.camorg.get(cam);
        for (int h = 0; h < rp.height; h++)
            for (int w = 0; w < rp.width; w++) {
                const size_t px = (size_t)h * rp.width + w;
                const int id = a.obj_id[px];
                if (id < -1 || id > 3 || a.hits[px] != (id >= 0 ? 1u : 0u)) {
                    std::fprintf(stderr, "pixel (%d, %d): object %d, %u hits\n", w, h, id, a.hits[px]);
                    return 1;
                }
                seen[id + 1]++;
                if (id < 0) continue;
                for (int k = 0; k < 3; k++)
                    if (a.albedo[3 * px + k] != (float)col[id][k]) {
                        std::fprintf(stderr, "pixel (%d, %d): albedo is not object %d's colour\n", w, h, id);
                        return 1;
                    }
                // the pixel's ray (main.cpp:188-189,209) and the point at `depth` along it
                double d[3] = {(2.0 * ((double)w / rp.width) - 1) * rp.half_width - cam[0],
                               (2.0 * ((double)h / rp.height) - 1) * rp.half_width * rp.height / rp.width - cam[1], 0 - cam[2]};
                const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                double P[3], nd = 0;
                for (int k = 0; k < 3; k++) {
                    d[k] /= len;
                    P[k] = cam[k] + d[k] * (double)a.depth[px];
                    nd += (double)a.normal[3 * px + k] * d[k];
                }
                bool ok = nd < 0;  // turned against the ray
                if (id >= 2)       // a sphere: on its surface, the normal along centre -> P
                    for (int k = 0; k < 3; k++) ok = ok && std::fabs((P[k] - centre[id - 2][k]) / radius[id - 2] - (double)a.normal[3 * px + k]) < 1e-4;
                else
                    ok = ok && std::fabs(id == 0 ? P[1] + 15 : P[2] - 50) < 1e-3;
                if (!ok) {
                    std::fprintf(stderr, "pixel (%d, %d): depth %g and normal do not fit object %d\n", w, h, (double)a.depth[px], id);
                    return 1;
                }
            }
        if (!seen[1] || !seen[2] || !seen[3] || !seen[4]) {
            std::fprintf(stderr, "an object is not in the frame\n");
            return 1;
        }
        if (!png.empty()) {
            std::vector<float> nrm(a.normal.size()), dep(a.albedo.size());
            for (size_t i = 0; i < nrm.size(); i++) nrm[i] = 0.5f * a.normal[i] + 0.5f;
            for (size_t i = 0; i < npx; i++) dep[3 * i] = dep[3 * i + 1] = dep[3 * i + 2] = a.hits[i] ? 10.f / a.depth[i] : 0.f;
            png3(png + "albedo.png", rp.width, rp.height, a.albedo);
            png3(png + "normal.png", rp.width, rp.height, nrm);
            png3(png + "depth.png", rp.width, rp.height, dep);
        }
        std::printf("ok: %zu pixels -- floor %zu, wall %zu, matte sphere %zu, glass sphere %zu, sky %zu\n", npx, seen[1], seen[2], seen[3], seen[4],
                    seen[0]);
    } catch (const Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
