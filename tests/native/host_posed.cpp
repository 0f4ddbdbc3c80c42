// The posed camera in the C++ host layer (include/cgrt_host.hpp: RenderParams::look_at / set_pose / camera): a plain C++14 program
// linked against libcgrt.so, no GPU -- the default RenderParams is the built-in camera without the flag, look_at and set_pose fill a
// cgrt_posed_camera whose base goes where a cgrt_camera goes.  Driven by tests/test_posed_camera_host.py.
#include <cmath>
#include <cstdio>

#include "cgrt_host.hpp"

using namespace cgrt_host;

static int g_failed = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_failed++;                                                \
        }                                                              \
    } while (0)

int main() {
    {   // the default: the built-in camera, no flag
        RenderParams rp;
        cgrt_posed_camera pc;
        cgrt_grid g{};
        const cgrt_camera *cam = rp.camera(pc, g);
        CHECK(cam == &pc.base && g.flags == 0 && !rp.posed);
        CHECK(cam->cam[0] == 0 && cam->cam[1] == 0 && cam->cam[2] == -10 && cam->half_width == 10.0 && cam->focus_plane == 20.0 && cam->lens_radius == 0.0);
        rp.depth_of_field = true;
        CHECK(rp.camera(pc, g)->lens_radius == 1.5 && g.flags == 0);
    }
    {   // look_at: the library's frame, and rays from it
        RenderParams rp;
        rp.radius = 0.5;
        rp.depth_of_field = true;
        rp.look_at(Vec3(17, 8, 2), Vec3(-2, -13, 30), Vec3(0, 1, 0), 70.0, 30.0);
        cgrt_posed_camera pc, want;
        cgrt_grid g{};
        g.width = 9; g.height = g.rows = 5; g.stripe_nranks = 1; g.spp = g.spp_total = 1; g.max_depth = 5; g.seed = 1;
        const cgrt_camera *cam = rp.camera(pc, g);
        CHECK(rp.posed && (g.flags & CGRT_GRID_POSED) && cam == &pc.base);
        const double eye[3] = {17, 8, 2}, target[3] = {-2, -13, 30}, up[3] = {0, 1, 0};
        CHECK(cgrt_look_at(eye, target, up, 70.0, 30.0, 0.5, &want) == CGRT_OK);
        for (int k = 0; k < 3; k++)
            CHECK(pc.origin[k] == want.origin[k] && pc.right[k] == want.right[k] && pc.up[k] == want.up[k] && pc.forward[k] == want.forward[k] &&
                  pc.base.cam[k] == want.base.cam[k]);
        CHECK(pc.base.half_width == want.base.half_width && pc.base.focus_plane == want.base.focus_plane && pc.base.lens_radius == 0.5);
        double org[45 * 3], dir[45 * 3];
        CHECK(cgrt_camera_rays_host(cam, &g, org, dir, nullptr) == CGRT_OK);
        CHECK(std::fabs(org[0] - 17) < 1.0 && std::fabs(org[1] - 8) < 1.0 && std::fabs(org[2] - 2) < 1.0);  // on the lens about the eye
        bool threw = false;
        try {
            rp.look_at(Vec3(1, 1, 1), Vec3(1, 1, 1), Vec3(0, 1, 0), 70.0, 30.0);
        } catch (...) {
            threw = true;
        }
        CHECK(threw);
    }
    {   // set_pose: a quarter turn about y
        RenderParams rp;
        rp.set_pose(Vec3(-8, 0, 20), Vec3(0, 0, -1), Vec3(0, 1, 0), Vec3(1, 0, 0));
        cgrt_posed_camera pc;
        cgrt_grid g{};
        g.width = g.height = g.rows = 1; g.stripe_nranks = 1; g.spp = g.spp_total = 1; g.max_depth = 5;
        const cgrt_camera *cam = rp.camera(pc, g);
        CHECK(g.flags == CGRT_GRID_POSED && pc.forward[0] == 1 && pc.right[2] == -1 && pc.origin[0] == -8);
        double org[3], dir[3];
        CHECK(cgrt_camera_rays_host(cam, &g, org, dir, nullptr) == CGRT_OK);
        CHECK(org[0] == -18 && org[1] == 0 && org[2] == 20 && dir[0] > 0.5);
    }
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
