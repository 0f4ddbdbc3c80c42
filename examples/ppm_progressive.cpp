// Progressive photon mapping as an interactive host would drive it, over include/cgrt_host.hpp: the eye pass and the
// hitpoint table are built once (PpmSession), then photons arrive in K passes and the image is written after each one.
// Pass k holds the first N*k/K photons, and its PNG is the one a one-shot render of that many photons writes.
//
//   cgrt_ppm_progressive [--scene c2|planes] [--width W] [--height H] [--spp S] [--photons N] [--passes K]
//                        [--png-prefix P]          writes P1.png .. PK.png (default prefix "pass")
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cgrt_host.hpp"

using namespace cgrt_host;

int main(int argc, char *argv[]) {
    RenderParams rp;
    rp.width = 256;
    rp.height = 192;
    std::string scene = "c2", prefix = "pass";
    long long photons = 200000;
    int passes = 4;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "--scene") scene = next();
        else if (a == "--width") rp.width = std::atoi(next());
        else if (a == "--height") rp.height = std::atoi(next());
        else if (a == "--spp") rp.num_of_samples = std::atoi(next());
        else if (a == "--photons") photons = std::atoll(next());
        else if (a == "--passes") passes = std::atoi(next());
        else if (a == "--png-prefix") prefix = next();
        else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    if (passes < 1 || photons < passes) {
        std::fprintf(stderr, "need --passes >= 1 and --photons >= --passes\n");
        return 2;
    }

    // the scenes of main_dropin.cpp: C2 (the walls as large spheres, a mirror and a glass sphere) or the plane room
    std::vector<Sphere> sphs;
    std::vector<Plane> plns;
    if (scene == "c2") {
        const Vec3 grey(0.25, 0.25, 0.25);
        sphs.push_back(Sphere(Vec3(0.0, -10020, 0), 10000, grey));
        sphs.push_back(Sphere(Vec3(10020, 0.0, 0), 10000, Vec3(0.25, 0.75, 0.25)));
        sphs.push_back(Sphere(Vec3(-10020, 0.0, 0), 10000, Vec3(0.75, 0.25, 0.25)));
        sphs.push_back(Sphere(Vec3(0.0, 0.0, 10040), 10000, grey));
        sphs.push_back(Sphere(Vec3(0.0, 10020, 0), 10000, grey));
        sphs.push_back(Sphere(Vec3(-15.0, -20.0, 60), 10, Vec3(0.3, 0.3, 0.3)));
        sphs.push_back(Sphere(Vec3(10.0, -13.0, 30), 7, Vec3(1.0, 1.0, 1.0), 0.8, 0.0));
        sphs.push_back(Sphere(Vec3(-8.0, -13.0, 25), 7, Vec3(1.0, 1.0, 1.0), 0.8, 0.5));
    } else if (scene == "planes") {
        const Vec3 grey(0.15, 0.15, 0.15);
        plns.push_back(Plane(Vec3(0.0, -20, 0), Vec3(0, 1, 0), grey));
        plns.push_back(Plane(Vec3(20, 0.0, 0), Vec3(-1, 0, 0), Vec3(0.15, 0.50, 0.15)));
        plns.push_back(Plane(Vec3(-20, 0.0, 0), Vec3(1, 0, 0), Vec3(0.50, 0.15, 0.15)));
        plns.push_back(Plane(Vec3(0.0, 0.0, 40), Vec3(0, 0, -1), grey));
        plns.push_back(Plane(Vec3(0.0, 20, 0), Vec3(0, -1, 0), grey));
        sphs.push_back(Sphere(Vec3(5, -12, 30), 5, Vec3(1, 1, 1), 0.8, 0.5));
    } else {
        std::fprintf(stderr, "unknown scene %s\n", scene.c_str());
        return 2;
    }
    std::vector<Object *> objs;
    for (Sphere &s : sphs) objs.push_back(&s);
    for (Plane &p : plns) objs.push_back(&p);

    try {
        PpmSession session(objs, rp, PhotonParams());
        const cgrt_ppm_session_info start = session.info();
        std::printf("hitpoints: %llu; eye %.2f ms, table %.2f ms\n", (unsigned long long)start.hp_count, start.ms_eye,
                    start.ms_table);
        std::vector<double> image;
        std::vector<unsigned char> image_data;
        for (int k = 1; k <= passes; k++) {
            const long long target = photons * k / passes;
            session.add_photons(target - session.photons_done());
            session.image(image, image_data);
            const std::string path = prefix + std::to_string(k) + ".png";
            write_png(path.c_str(), rp.width, rp.height, image_data);
            const cgrt_ppm_session_info inf = session.info();
            std::printf("pass %d: %lld photons, %llu events; add %.2f ms, image %.3f ms -> %s\n", k, (long long)inf.photons_done,
                        (unsigned long long)inf.n_events, inf.ms_last_add, inf.ms_last_image, path.c_str());
        }
    } catch (const Error &e) {
        std::fprintf(stderr, "render failed (%d): %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
