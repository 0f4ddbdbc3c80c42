/* cgrt_hitpoints and cgrt_ppm_session_create_hitpoints, seen from strict C99: the struct's layout (pinned in
 * cgraytracing_amd/_capi.py too) and the declaration's types. */
#include <stddef.h>

#include "cgrt.h"

#define STATIC_ASSERT(c, name) typedef char static_assert_##name[(c) ? 1 : -1]

STATIC_ASSERT(sizeof(cgrt_hitpoints) == 72, hitpoints_size);
STATIC_ASSERT(offsetof(cgrt_hitpoints, n) == 0, hitpoints_n);
STATIC_ASSERT(offsetof(cgrt_hitpoints, hp9) == 8, hitpoints_hp9);
STATIC_ASSERT(offsetof(cgrt_hitpoints, ray) == 16, hitpoints_ray);
STATIC_ASSERT(offsetof(cgrt_hitpoints, path) == 24, hitpoints_path);
STATIC_ASSERT(offsetof(cgrt_hitpoints, pixel) == 32, hitpoints_pixel);
STATIC_ASSERT(offsetof(cgrt_hitpoints, width) == 40, hitpoints_width);
STATIC_ASSERT(offsetof(cgrt_hitpoints, rows) == 44, hitpoints_rows);
STATIC_ASSERT(offsetof(cgrt_hitpoints, spp) == 48, hitpoints_spp);
STATIC_ASSERT(offsetof(cgrt_hitpoints, max_depth) == 52, hitpoints_max_depth);
STATIC_ASSERT(offsetof(cgrt_hitpoints, reserved) == 56, hitpoints_reserved);
STATIC_ASSERT(CGRT_VERSION == 112, version);

/* null arguments are refused before any device call: returns 0 when the call says CGRT_ERR_INVALID and leaves no session */
int cgrt_abi_hitpoints_smoke(void) {
    int (*create)(const cgrt_scene *, const cgrt_hitpoints *, const cgrt_photons *, int, cgrt_ppm_session **) =
        cgrt_ppm_session_create_hitpoints;
    cgrt_ppm_session *ses = NULL;
    if (create(NULL, NULL, NULL, 0, &ses) != CGRT_ERR_INVALID || ses != NULL) return 1;
    if (create(NULL, NULL, NULL, 0, NULL) != CGRT_ERR_INVALID) return 2;
    return 0;
}
