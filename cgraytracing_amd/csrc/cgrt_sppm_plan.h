// Stochastic progressive photon mapping in plain C++ (no HIP): the per-texel update a pass ends with -- one inline function,
// which sppm_pixel_update_kernel (cgrt_sppm.hpp) calls and cgrt_sppm_update_host exports -- and the argument checks of
// cgrt_sppm_session_create and of a pass's grid, which need neither a scene nor a device.  tests/test_sppm_host.py checks both
// on the CPU.
#ifndef CGRT_SPPM_PLAN_H
#define CGRT_SPPM_PLAN_H
#include <cstdint>

#include "../../include/cgrt.h"
#include "cgrt_rng.hpp"  // CGRT_HD

static constexpr int kSppmPixelDoubles = 8;  // a texel's record: {N, R2, tau[3], M_p and Hitpoints of the last pass, 0}

// The end of a pass for one texel that M photon hits reached with the summed flux phi (Hachisuka & Jensen 2009, eq. 9-12 with
// the statistics kept per texel): in fp64, in this order, and only where M > 0 -- a texel nothing reached keeps its bits.
// alpha in (0, 1] makes g <= 1: radii only shrink, which is what keeps the session's hash grid valid.
CGRT_HD void sppm_update(double &N, double &R2, double tau[3], double M, const double phi[3], double alpha) {
    if (!(M > 0)) return;
    const double Nn = N + alpha * M;
    const double g = Nn / (N + M);
    R2 = R2 * g;
    for (int k = 0; k < 3; k++) tau[k] = (tau[k] + phi[k]) * g;
    N = Nn;
}

// What is wrong with the arguments of cgrt_sppm_session_create (ph->nphotons is not looked at), or nullptr; *code is set with it
inline const char *sppm_create_args(int width, int rows, int spp, int photon_depth, const cgrt_photons *ph, int flags, int *code) {
    *code = CGRT_ERR_INVALID;
    if (!ph) return "null argument";
    if (width <= 0 || rows <= 0 || spp <= 0) return "sppm session: width, rows and spp must be positive";
    if (photon_depth < 1 || photon_depth > 5) return "sppm session: photon_depth must be 1..5";
    if (ph->hashsize < 1 || ph->hashsize > (1 << 20) || ph->batch < 0 || !(ph->initial_radius >= 0) || ph->pair_cap < 0)
        return "bad photon parameters";
    if (!(ph->alpha > 0 && ph->alpha <= 1)) return "sppm session: alpha must lie in (0, 1] (radii must not grow)";
    if (flags != 0) return "unknown session flags";
    *code = CGRT_ERR_LIMIT;
    if ((long long)width * rows >= (1ll << 31)) return "sppm session: 2^31 texels or more";
    *code = CGRT_OK;
    return nullptr;
}

// The stripes of a grid as the triple a session keeps: a contiguous grid is (0, 0, 1) whatever its unused fields hold
struct SppmStripe {
    int rows = 0, rank = 0, nranks = 1;
    bool operator==(const SppmStripe &o) const { return rows == o.rows && rank == o.rank && nranks == o.nranks; }
};
inline SppmStripe sppm_stripe(const cgrt_grid *g) {
    SppmStripe t;
    if (g->stripe_nranks > 1) {
        t.rows = g->stripe_rows; t.rank = g->stripe_rank; t.nranks = g->stripe_nranks;
    }
    return t;
}
// What is wrong with a pass's grid for a session of width x rows texels and spp samples, or nullptr.  fixed: the stripes of the
// session's first pass (null before it)
inline const char *sppm_pass_grid_args(int width, int rows, int spp, const cgrt_grid *g, const SppmStripe *fixed) {
    if (!g) return "null argument";
    if (g->width != width || g->rows != rows || g->spp != spp) return "sppm pass: the grid's width, rows and spp must be the session's";
    if (fixed && !(sppm_stripe(g) == *fixed)) return "sppm pass: the grid's stripes differ from the first pass's";
    return nullptr;
}

#endif
