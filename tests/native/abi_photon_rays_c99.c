/* cgrt_photon_rays and the caller-supplied-photon entry points, seen from strict C99: the struct's layout (pinned in
 * cgraytracing_amd/_capi.py too) and the declarations' types. */
#include <stddef.h>

#include "cgrt.h"

#define STATIC_ASSERT(c, name) typedef char static_assert_##name[(c) ? 1 : -1]

STATIC_ASSERT(sizeof(cgrt_photon_rays) == 48, photon_rays_size);
STATIC_ASSERT(offsetof(cgrt_photon_rays, n) == 0, photon_rays_n);
STATIC_ASSERT(offsetof(cgrt_photon_rays, org3) == 8, photon_rays_org3);
STATIC_ASSERT(offsetof(cgrt_photon_rays, dir3) == 16, photon_rays_dir3);
STATIC_ASSERT(offsetof(cgrt_photon_rays, flux3) == 24, photon_rays_flux3);
STATIC_ASSERT(offsetof(cgrt_photon_rays, keys) == 32, photon_rays_keys);
STATIC_ASSERT(offsetof(cgrt_photon_rays, draws) == 40, photon_rays_draws);

/* One photon of the built-in emitter through the host form, and the refusals that need no device: 0 when all is as documented. */
int cgrt_abi_photon_rays_smoke(void) {
    int (*add)(cgrt_ppm_session *, const cgrt_photon_rays *) = cgrt_ppm_session_add_photon_rays;
    int (*emit)(const cgrt_photons *, int64_t, int64_t, double *, double *, double *, uint64_t *, uint32_t *, void *) = cgrt_photon_emit;
    int (*emit_host)(const cgrt_photons *, int64_t, int64_t, double *, double *, double *, uint64_t *, uint32_t *) =
        cgrt_photon_emit_host;
    int (*probe)(const cgrt_scene *, const cgrt_photon_rays *, uint64_t, int64_t, int, double *, uint8_t *) = cgrt_photon_ray_events;
    cgrt_photons ph;
    cgrt_photon_rays pr;
    double o[3], d[3], f[3];
    uint64_t key = 0;
    uint32_t draws = 0;
    ph.light[0] = 0.0; ph.light[1] = 19.999; ph.light[2] = 20.0;
    ph.jitter = 2.0; ph.power = 700.0; ph.alpha = 0.7;
    ph.nphotons = 0; ph.hashsize = 1000001; ph.batch = 0; ph.seed = 777; ph.initial_radius = 0.0; ph.pair_cap = 0;
    if (emit_host(&ph, 0, 1, o, d, f, &key, &draws) != CGRT_OK) return 1;
    if (draws < 5 || o[1] != 19.999 || f[0] != f[2]) return 2;
    pr.n = 1; pr.org3 = o; pr.dir3 = d; pr.flux3 = f; pr.keys = &key; pr.draws = &draws;
    if (add(NULL, &pr) != CGRT_ERR_INVALID) return 3;
    if (add(NULL, NULL) != CGRT_ERR_INVALID) return 4;
    if (emit(NULL, 0, 1, NULL, NULL, NULL, NULL, NULL, NULL) != CGRT_ERR_INVALID) return 5;
    if (probe(NULL, &pr, 777, 0, 5, NULL, NULL) != CGRT_ERR_INVALID) return 6;
    return 0;
}
