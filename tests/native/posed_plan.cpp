// The posed camera on the host (cgrt_frame.h: pose_point, pose_error, look_at_camera, grid_params, frame_plan; cgrt_variants.h:
// eye_choice, CGRT_EYE_POSED_VARIANTS): the identity frame maps every point to itself, the validation's bounds, the look-at frame,
// and the launch plan of a posed launch over a sphere scene, a mesh scene and a Bezier scene -- no tile order, relay, lens table,
// light split or primary walk, a POSE kernel that is compiled, every compiled POSE kernel reachable, the launch without the flag
// untouched.  CPU build under ASan + UBSan, driven by tests/test_posed_camera_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "cgrt_variants.h"

static int g_failed = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

struct Eye { int T, B, D, G, P, S, H, NT, SP, HF, DF, PR, ST, LT, SCHED; };
#define X(...) {__VA_ARGS__},
static const Eye kPosed[] = {CGRT_EYE_POSED_VARIANTS(X)};
static const Eye kPlain[] = {CGRT_EYE_VARIANTS(X)};
#undef X
static EyeFlags flags_of(const Eye &e, bool pose) {
    return {e.T != 0, e.B != 0, e.D != 0, e.G != 0, e.P != 0, e.S != 0, e.H != 0, e.SP != 0, e.HF != 0, e.NT, e.DF != 0, e.PR != 0, e.ST != 0, e.LT != 0, pose};
}

static cgrt_grid grid(int W, int H, int spp, int depth, int flags) {
    cgrt_grid g{};
    g.width = W;
    g.height = g.rows = H;
    g.stripe_nranks = 1;
    g.spp = g.spp_total = spp;
    g.max_depth = depth;
    g.flags = flags;
    g.seed = 12345;
    return g;
}
static cgrt_posed_camera camera(double lens) {
    cgrt_posed_camera pc{};
    pc.base.cam[2] = -10;
    pc.base.half_width = 10;
    pc.base.focus_plane = 20;
    pc.base.lens_radius = lens;
    pc.right[0] = pc.up[1] = pc.forward[2] = 1;
    return pc;
}
// C2: nine spheres, one of glass; a glass mesh among planes; a Bezier vase among planes
static const EyeSceneTraits kSpheres{true, false, false, true, false, true, 9, 9};
static const EyeSceneTraits kMesh{false, true, false, true, false, false, 7, 7};
static const EyeSceneTraits kBezier{false, false, true, true, false, false, 7, 7};

// frame_inputs of cgrt_hip.hip, for a scene of these traits on a 256-CU device
static FrameInputs inputs(const EyeSceneTraits &d, const EyeChoice &c, const cgrt_posed_camera &pc, const cgrt_grid &g) {
    FrameInputs in{};
    in.grid = g;
    in.cam = pc.base;
    in.sched = c.form == EyeForm::Sched;
    in.spill = c.k.spill;
    in.stats = c.k.stats;
    in.glass = c.k.glass;
    in.nt = c.k.nt;
    in.has_mesh = d.has_mesh;
    in.has_bezier = d.has_bezier;
    in.prim_finish = d.has_mesh;
    in.light_ok = d.has_mesh || d.has_bezier;
    in.prim_obj = d.has_mesh ? 5 : -1;
    in.mem_total = 288000000000ull;
    in.n_cu = 256;
    in.waves_per_simd = c.k.nt == 64 ? kBezWaves : (c.k.trees ? kSchedTreeWaves : 4);
    in.image = c.form == EyeForm::Image;
    in.sph = c.k.sph;
    in.pair = c.k.pair;
    in.order_ok = d.order_ok;
    in.aux_stream = true;
    in.all_spheres = d.all_spheres;
    in.n_objs = d.n_objs;
    in.n_lds = d.n_lds;
    in.posed = c.k.pose;
    if (in.posed) in.posed_cam = pc;
    return in;
}

static void identity_and_validation() {
    const cgrt_posed_camera pc = camera(1.5);
    cgrt_grid g = grid(67, 45, 3, 5, CGRT_GRID_POSED);
    CHECK(pose_error(&pc.base, &g) == nullptr);
    const GridParams gp = grid_params(&pc.base, &g);
    CHECK(gp.posed == 1);
    const double pts[][3] = {{0, 0, -10}, {3.25, -7.5, 0}, {1e-300, 5e8, -0.1}, {-9.999999999999998, 1.0 / 3, 20}};
    for (const auto &p : pts) {
        double x, y, z;
        pose_point(gp, p[0], p[1], p[2], x, y, z);
        CHECK(x == p[0] && y == p[1] && z == p[2]);
    }
    // without the flag: the identity frame, nothing behind the 48 bytes read (ASan would see a read past this cgrt_camera)
    cgrt_grid g0 = grid(67, 45, 3, 5, 0);
    const cgrt_camera *lone = new cgrt_camera(pc.base);
    CHECK(pose_error(lone, &g0) == nullptr);
    const GridParams g1 = grid_params(lone, &g0);
    delete lone;
    CHECK(g1.posed == 0 && g1.pose_right[0] == 1 && g1.pose_up[1] == 1 && g1.pose_forward[2] == 1 && g1.pose_origin[0] == 0);
    // the bounds: 1e-9 passes on both counts, 1e-6 does not; a mirrored basis passes
    cgrt_posed_camera b = pc;
    b.right[0] = 1 + 5e-10;
    CHECK(pose_error(&b.base, &g) == nullptr);
    b.right[0] = 1 + 1e-6;
    CHECK(pose_error(&b.base, &g) != nullptr);
    b = pc;
    b.up[0] = 5e-10;
    CHECK(pose_error(&b.base, &g) == nullptr);
    b.up[0] = 1e-6;
    CHECK(pose_error(&b.base, &g) != nullptr);
    b = pc;
    b.forward[2] = -1;
    CHECK(pose_error(&b.base, &g) == nullptr);
    b = pc;
    b.origin[1] = std::nan("");
    CHECK(pose_error(&b.base, &g) != nullptr);
    b = pc;
    b.forward[0] = INFINITY;
    CHECK(pose_error(&b.base, &g) != nullptr);
}

static void look_at() {
    cgrt_posed_camera pc{};
    const double eye[3] = {17, 8, 2}, target[3] = {-2, -13, 30}, up[3] = {0, 1, 0};
    CHECK(look_at_camera(eye, target, up, 70, 25, 0.5, &pc) == nullptr);
    cgrt_grid g = grid(9, 5, 1, 5, CGRT_GRID_POSED);
    CHECK(pose_error(&pc.base, &g) == nullptr);
    const double D = std::sqrt(19.0 * 19 + 21.0 * 21 + 28.0 * 28);
    CHECK(std::fabs(-pc.base.cam[2] - D) <= 1e-12 * D && pc.base.cam[0] == 0 && pc.base.cam[1] == 0);
    CHECK(std::fabs(pc.base.half_width - D * std::tan(35 * M_PI / 180)) <= 1e-12 * D);
    CHECK(std::fabs((pc.base.focus_plane - pc.base.cam[2]) - 25) <= 1e-12);
    CHECK(pc.base.lens_radius == 0.5);
    // right is horizontal (no y), up points up, forward points at the target; right-handed: right x up = forward
    CHECK(std::fabs(pc.right[1]) <= 1e-15 && pc.up[1] > 0);
    for (int k = 0; k < 3; k++) CHECK(std::fabs(pc.forward[k] - (target[k] - eye[k]) / D) <= 1e-15);
    const double cx = pc.right[1] * pc.up[2] - pc.right[2] * pc.up[1];
    CHECK(std::fabs(cx - pc.forward[0]) <= 1e-15);
    // the eye maps to eye
    const GridParams gp = grid_params(&pc.base, &g);
    double x, y, z;
    pose_point(gp, pc.base.cam[0], pc.base.cam[1], pc.base.cam[2], x, y, z);
    CHECK(std::fabs(x - 17) <= 1e-13 && std::fabs(y - 8) <= 1e-13 && std::fabs(z - 2) <= 1e-13);
    // the refusals
    const double par[3] = {-19, -21, 28}, zero[3] = {0, 0, 0};
    CHECK(look_at_camera(eye, eye, up, 70, 25, 0, &pc) != nullptr);
    CHECK(look_at_camera(eye, target, par, 70, 25, 0, &pc) != nullptr);
    CHECK(look_at_camera(eye, target, zero, 70, 25, 0, &pc) != nullptr);
    CHECK(look_at_camera(eye, target, up, 0, 25, 0, &pc) != nullptr);
    CHECK(look_at_camera(eye, target, up, 180, 25, 0, &pc) != nullptr);
    CHECK(look_at_camera(eye, target, up, std::nan(""), 25, 0, &pc) != nullptr);
    CHECK(look_at_camera(eye, target, up, 70, 0, 0, &pc) != nullptr);
    CHECK(look_at_camera(eye, target, up, 70, 25, -1, &pc) != nullptr);
}

static bool in_list(const Eye *list, size_t n, const EyeFlags &f, bool pose, bool *sched = nullptr) {
    for (size_t i = 0; i < n; i++)
        if (flags_of(list[i], pose).id() == f.id()) {
            if (sched) *sched = list[i].SCHED != 0;
            return true;
        }
    return false;
}

static void plans() {
    const cgrt_posed_camera pc = camera(1.5);
    const int asks = CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_LENS_TABLE | CGRT_GRID_DIFFUSE_TILES;
    // ---- the sphere scene: C2 at 1920 x 1080, 64 samples, thin lens ----
    for (int extra : {0, asks}) {
        const cgrt_grid g0 = grid(1920, 1080, 64, 5, extra == asks ? (CGRT_GRID_SAMPLE_RELAY | CGRT_GRID_LENS_TABLE) : 0), g1 = grid(1920, 1080, 64, 5, extra | CGRT_GRID_POSED);
        const EyeChoice c0 = eye_choice(kSpheres, pc.base, g0, false, false), c1 = eye_choice(kSpheres, pc.base, g1, false, false);
        // without the flag: the pair kernel in tile order with its relay and lens table, as ever
        CHECK(c0.form == EyeForm::Image && c0.k.pair && !c0.k.pose && c0.k.sph && c0.k.glass && c0.k.dof);
        const FramePlan p0 = frame_plan(inputs(kSpheres, c0, pc, g0), 0);
        CHECK(p0.order.on && p0.order.class3 == TileOrderPlan::InKernel && p0.order.masks && p0.order.sure);
        CHECK(p0.order.lens_stage == kLensStageLds && p0.relay.relays() && p0.order.lens_table_cap > 0);
        // (what it does not read: the posed camera of the inputs)
        FrameInputs in0 = inputs(kSpheres, c0, pc, g0), in0b = in0;
        in0b.posed_cam.origin[0] = 99;
        const FramePlan p0b = frame_plan(in0b, 0);
        CHECK(p0b.order.on == p0.order.on && p0b.relay.bytes() == p0.relay.bytes() && p0b.order.lens_table_bytes == p0.order.lens_table_bytes &&
              p0b.grid_dim == p0.grid_dim && p0b.scratch.total == p0.scratch.total);
        const GridParams q0 = frame_params(in0, p0), q0b = frame_params(in0b, p0b);
        CHECK(std::memcmp(&q0, &q0b, sizeof(GridParams)) == 0 && q0.posed == 0);
        // with it: image order, row-major, the plain sphere kernel with POSE, nothing of the tile order
        CHECK(c1.form == EyeForm::Image && !c1.k.pair && c1.k.pose && c1.k.sph && c1.k.glass && c1.k.dof && !c1.k.start && !c1.k.ltab);
        CHECK(in_list(kPosed, sizeof(kPosed) / sizeof(kPosed[0]), c1.k, true));
        const FrameInputs in1 = inputs(kSpheres, c1, pc, g1);
        const FramePlan p1 = frame_plan(in1, 0);
        CHECK(!p1.order.on && p1.order.class3 == TileOrderPlan::None && !p1.order.masks && !p1.order.sure);
        CHECK(p1.order.lens_stage == kLensStageOff && !p1.relay.relays() && p1.order.lens_table_cap == 0 && p1.order.lens_table_bytes == 0);
        CHECK(p1.chunks == 1 && !p1.xcd_tiles && p1.grid_dim == (size_t)60 * 135 && p1.kmax == 0 && p1.scratch.total == 0);
        const GridParams q1 = frame_params(in1, p1);
        CHECK(q1.posed == 1 && q1.tile_order == 0 && q1.lens_batch == 0 && q1.lens_table_cap == 0 && q1.relay_k == 0);
        // the unposed launch under CGRT_GRID_NO_TILE_ORDER has the same plan: that is the form a posed launch runs
        cgrt_grid gn = g0;
        gn.flags |= CGRT_GRID_NO_TILE_ORDER;
        const FramePlan pn = frame_plan(inputs(kSpheres, eye_choice(kSpheres, pc.base, gn, false, false), pc, gn), 0);
        CHECK(!pn.order.on && pn.grid_dim == p1.grid_dim && !pn.relay.relays() && pn.order.lens_table_cap == 0);
    }
    {   // split samples keep working under a pose: the same chunks as without
        const cgrt_grid g0 = grid(1920, 1080, 64, 5, CGRT_GRID_SPLIT_SAMPLES | CGRT_GRID_NO_TILE_ORDER), g1 = grid(1920, 1080, 64, 5, CGRT_GRID_SPLIT_SAMPLES | CGRT_GRID_POSED);
        const FramePlan p0 = frame_plan(inputs(kSpheres, eye_choice(kSpheres, pc.base, g0, false, false), pc, g0), 0);
        const FramePlan p1 = frame_plan(inputs(kSpheres, eye_choice(kSpheres, pc.base, g1, false, false), pc, g1), 0);
        CHECK(p0.chunks == 4 && p1.chunks == 4 && p1.chunk_spp == p0.chunk_spp && p1.grid_dim == p0.grid_dim && p1.scratch.total == p0.scratch.total);
    }
    {   // force_reorder, by flag or knob, is not followed under a pose
        const cgrt_grid g1 = grid(1920, 1080, 64, 5, CGRT_GRID_FORCE_REORDER | CGRT_GRID_POSED), g0 = grid(1920, 1080, 64, 5, CGRT_GRID_FORCE_REORDER);
        CHECK(eye_choice(kSpheres, pc.base, g0, false, false).form == EyeForm::Sched);
        CHECK(eye_choice(kSpheres, pc.base, g1, true, false).form == EyeForm::Image);
    }
    // ---- the mesh scene and the Bezier scene: the cost scheduler stays, the light split and the primary walk go ----
    for (const EyeSceneTraits *d : {&kMesh, &kBezier}) {
        const cgrt_grid g0 = grid(1024, 1024, 8, 5, 0), g1 = grid(1024, 1024, 8, 5, CGRT_GRID_POSED);
        const cgrt_posed_camera pin = camera(0);
        const EyeChoice c0 = eye_choice(*d, pin.base, g0, false, false), c1 = eye_choice(*d, pin.base, g1, false, false);
        CHECK(c0.form == EyeForm::Sched && c1.form == EyeForm::Sched && !c0.k.pose && c1.k.pose);
        CHECK(c1.k.trees && c1.k.bez == d->has_bezier && c1.k.nt == (d->has_bezier ? 64 : 256) && c1.k.glass && !c1.k.dof);
        bool sched = false;
        CHECK(in_list(kPosed, sizeof(kPosed) / sizeof(kPosed[0]), c1.k, true, &sched) && sched);
        const FrameInputs in0 = inputs(*d, c0, pin, g0), in1 = inputs(*d, c1, pin, g1);
        const FramePlan p0 = frame_plan(in0, max_heavy_tiles(in0)), p1 = frame_plan(in1, max_heavy_tiles(in1));
        CHECK(p0.kmax > 0 && p1.kmax > 0 && p0.heavy_blocks > 0 && p1.heavy_blocks > 0);
        CHECK(p0.split_light && !p1.split_light && p1.scratch.light.bytes == 0);
        CHECK(p0.use_prim == d->has_mesh && !p1.use_prim && !p1.prim_done && p1.scratch.prim_len.bytes == 0);
        CHECK(p1.tile_queue == p0.tile_queue && p1.xcd_tiles == p0.xcd_tiles && p1.items_per_tile == p0.items_per_tile && p1.wave_slots == p0.wave_slots);
        const GridParams q1 = frame_params(in1, p1);
        CHECK(q1.posed == 1 && q1.prim_obj == -1 && q1.prim_done == 0);
        // image order below 4 samples or on request
        cgrt_grid gi = g1;
        gi.flags |= CGRT_GRID_NO_REORDER;
        CHECK(eye_choice(*d, pin.base, gi, false, false).form == EyeForm::Image);
        // no STATS kernel has POSE: the choice names one that is not compiled, which the library refuses
        cgrt_grid gs = g1;
        gs.flags |= CGRT_GRID_STATS;
        const EyeChoice cs = eye_choice(*d, pin.base, gs, false, false);
        if (d->has_mesh && !d->has_bezier) CHECK(cs.k.stats && cs.k.pose && !in_list(kPosed, sizeof(kPosed) / sizeof(kPosed[0]), cs.k, true));
    }
}

// every POSE kernel that is compiled is chosen by some launch, and every launch without STATS chooses one that is compiled
static void reachability() {
    const EyeSceneTraits plain{false, false, false, true, false, false, 5, 5}, plain_dull{false, false, false, false, false, false, 5, 5};
    const EyeSceneTraits dull_spheres{true, false, false, false, false, false, 9, 9}, many_spheres{true, false, false, true, false, false, 900, 768};
    const EyeSceneTraits many_general{false, true, false, true, false, false, 900, 768}, dull_mesh{false, true, false, false, false, false, 7, 7};
    const EyeSceneTraits dull_bezier{false, false, true, false, false, false, 7, 7};
    const EyeSceneTraits *scenes[] = {&kSpheres, &kMesh, &kBezier, &plain, &plain_dull, &dull_spheres, &many_spheres, &many_general, &dull_mesh, &dull_bezier};
    std::set<int> grid_ids, sched_ids;
    for (const EyeSceneTraits *d : scenes)
        for (double lens : {0.0, 1.5})
            for (int spp : {1, 8})
                for (int capture = 0; capture < 2; capture++)
                    for (int flags : {0, (int)CGRT_GRID_NO_REORDER}) {
                        const cgrt_posed_camera pc = camera(lens);
                        const cgrt_grid g = grid(256, 256, spp, 5, flags | CGRT_GRID_POSED);
                        EyeChoice c = eye_choice(*d, pc.base, g, false, capture != 0);
                        CHECK(c.k.pose && !c.k.pair && !c.k.diff && !c.k.start && !c.k.ltab && !c.k.hfonly && !c.k.stats);
                        // (eye_launch clears spill where everything stays resident: a capture's case only, the SPILL form has
                        // more objects than the list holds)
                        for (int resident = 0; resident < 2; resident++) {
                            if (resident && c.form != EyeForm::Capture) continue;
                            if (resident) c.k.spill = false;
                            bool sched = false;
                            CHECK(in_list(kPosed, sizeof(kPosed) / sizeof(kPosed[0]), c.k, true, &sched));
                            grid_ids.insert(c.k.id());
                            if (c.form == EyeForm::Sched) {
                                CHECK(sched);
                                sched_ids.insert(c.k.id());
                            }
                        }
                        // the same launch without the flag chooses a kernel of the other list
                        cgrt_grid gu = g;
                        gu.flags &= ~CGRT_GRID_POSED;
                        const EyeChoice u = eye_choice(*d, pc.base, gu, false, capture != 0);
                        CHECK(!u.k.pose && in_list(kPlain, sizeof(kPlain) / sizeof(kPlain[0]), u.k, false));
                    }
    for (const Eye &e : kPosed) {
        const EyeFlags f = flags_of(e, true);
        CHECK(grid_ids.count(f.id()) == 1);
        CHECK((sched_ids.count(f.id()) == 1) == (e.SCHED != 0));
        CHECK(f.id() != flags_of(e, false).id());  // POSE is part of a variant's identity
    }
    CHECK(grid_ids.size() == sizeof(kPosed) / sizeof(kPosed[0]));
}

int main() {
    identity_and_validation();
    look_at();
    plans();
    reachability();
    std::printf("ok: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
