/* The posed camera's ABI as compile-time asserts of a strict C99 translation unit (gcc -std=c99 -pedantic -Wall -Wextra -Werror,
 * tests/test_posed_camera_host.py), linked against libcgrt.so: cgrt_posed_camera begins with the cgrt_camera it extends, neither
 * of the pinned structs has grown, and CGRT_GRID_POSED is the bit the header documents. */
#include <stddef.h>

#include "cgrt.h"

#define STATIC_ASSERT(c, name) typedef char static_assert_##name[(c) ? 1 : -1]
STATIC_ASSERT(sizeof(cgrt_camera) == 48, camera_size);
STATIC_ASSERT(sizeof(cgrt_grid) == 56, grid_size);
STATIC_ASSERT(sizeof(cgrt_posed_camera) == 144, posed_size);
STATIC_ASSERT(offsetof(cgrt_posed_camera, base) == 0, base_first);
STATIC_ASSERT(offsetof(cgrt_posed_camera, origin) == 48, origin_at);
STATIC_ASSERT(offsetof(cgrt_posed_camera, right) == 72, right_at);
STATIC_ASSERT(offsetof(cgrt_posed_camera, up) == 96, up_at);
STATIC_ASSERT(offsetof(cgrt_posed_camera, forward) == 120, forward_at);
STATIC_ASSERT(CGRT_GRID_POSED == (1 << 26), posed_bit);

int cgrt_abi_posed_smoke(void) {
    const double eye[3] = {0.0, 0.0, -10.0}, target[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 1.0, 0.0};
    cgrt_posed_camera pc;
    cgrt_grid g;
    double org[3], dir[3];
    g.width = 1; g.height = 1; g.rows = 1; g.row_offset = 0; g.stripe_rows = 0; g.stripe_rank = 0; g.stripe_nranks = 1;
    g.spp = 1; g.sample_offset = 0; g.spp_total = 1; g.max_depth = 5; g.flags = CGRT_GRID_POSED; g.seed = 1;
    if (cgrt_look_at(eye, target, up, 90.0, 30.0, 0.0, &pc) != CGRT_OK) return 1;
    /* the built-in camera's frame and eye */
    if (pc.origin[0] != 0.0 || pc.origin[1] != 0.0 || pc.origin[2] != 0.0) return 2;
    if (pc.right[0] != 1.0 || pc.up[1] != 1.0 || pc.forward[2] != 1.0) return 3;
    if (pc.base.cam[2] != -10.0 || pc.base.focus_plane != 20.0) return 4;
    /* the sockaddr idiom: the base goes where a cgrt_camera goes */
    if (cgrt_camera_rays_host(&pc.base, &g, org, dir, 0) != CGRT_OK) return 5;
    if (org[2] != -10.0 || !(dir[2] > 0.0)) return 6;
    pc.up[1] = 1.0 + 1e-6;
    if (cgrt_camera_rays_host(&pc.base, &g, org, dir, 0) != CGRT_ERR_INVALID) return 7;
    g.flags = 0; /* without the flag the pose is not looked at */
    if (cgrt_camera_rays_host(&pc.base, &g, org, dir, 0) != CGRT_OK) return 8;
    if (cgrt_look_at(eye, eye, up, 90.0, 30.0, 0.0, &pc) != CGRT_ERR_INVALID) return 9;
    return 0;
}
