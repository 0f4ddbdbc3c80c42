/* cgrt_ray_pixels and the two ray-buffer photon entry points, seen from strict C99: the struct's layout (pinned in
 * cgraytracing_amd/_capi.py too) and the declarations' types. */
#include <stddef.h>

#include "cgrt.h"

#define STATIC_ASSERT(c, name) typedef char static_assert_##name[(c) ? 1 : -1]

STATIC_ASSERT(sizeof(cgrt_ray_pixels) == 24, ray_pixels_size);
STATIC_ASSERT(offsetof(cgrt_ray_pixels, width) == 0, ray_pixels_width);
STATIC_ASSERT(offsetof(cgrt_ray_pixels, rows) == 4, ray_pixels_rows);
STATIC_ASSERT(offsetof(cgrt_ray_pixels, spp) == 8, ray_pixels_spp);
STATIC_ASSERT(offsetof(cgrt_ray_pixels, pad_) == 12, ray_pixels_pad);
STATIC_ASSERT(offsetof(cgrt_ray_pixels, pixel) == 16, ray_pixels_pixel);
STATIC_ASSERT(CGRT_RAYS_HITPOINTS == 4, rays_hitpoints_flag);

/* null arguments are refused before any device call: returns 0 when both calls say CGRT_ERR_INVALID */
int cgrt_abi_ray_pixels_smoke(void) {
    int (*create)(const cgrt_scene *, const cgrt_rays *, const cgrt_ray_pixels *, const cgrt_photons *, int, cgrt_ppm_session **) =
        cgrt_ppm_session_create_rays;
    int (*capture)(const cgrt_scene *, const cgrt_rays *, double *, uint64_t, uint64_t *) = cgrt_trace_rays_hitpoints;
    cgrt_ppm_session *ses = NULL;
    uint64_t count = 0;
    if (create(NULL, NULL, NULL, NULL, 0, &ses) != CGRT_ERR_INVALID || ses != NULL) return 1;
    if (capture(NULL, NULL, NULL, 0, &count) != CGRT_ERR_INVALID) return 2;
    return 0;
}
