// cgrt_host.hpp -- header-only C++ host layer over the C ABI (cgrt.h).
//
// Keeps the reference's host-side API surface -- Vec3 (headers/vec3.h), Texture (headers/texture.h), Object /
// Sphere / Plane / TriangleMesh (headers/objects.h), Bezier (headers/bezier.h) with the SAME constructor
// signatures, and a render(objs) entry shaped like main.cpp:169 -- so that the scene-building part of a
// main() written against the reference compiles against this header unchanged.  Nothing is traced on the host
// (Object::intersect, too, runs on the device):
// render() flattens `objs` through cgrt_scene_add_* and launches the eye pass on the GPU with
// cgrt_trace_grid_host().  This file is original code; it mirrors interfaces, not implementations.
#ifndef CGRT_HOST_HPP
#define CGRT_HOST_HPP

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "cgrt.h"

namespace cgrt_host {

// ---- vec3.h:11-119 ------------------------------------------------------------------------------
class Vec3 {
  public:
    double x, y, z;
    Vec3(double x_ = 0, double y_ = 0, double z_ = 0) : x(x_), y(y_), z(z_) {}
    double norm() const { return std::sqrt(x * x + y * y + z * z); }
    Vec3 normalize() {  // mutates and returns a copy, like the reference (vec3.h:36-44)
        double len = norm();
        if (len > 0) { x *= 1 / len; y *= 1 / len; z *= 1 / len; }
        return *this;
    }
    Vec3 copy() const { return Vec3(x, y, z); }
    Vec3 operator*(const double &f) const { return Vec3(x * f, y * f, z * f); }
    Vec3 operator*(const Vec3 &v) const { return Vec3(x * v.x, y * v.y, z * v.z); }
    Vec3 mul(const Vec3 &v) const { return Vec3(x * v.x, y * v.y, z * v.z); }
    double dot(const Vec3 &v) const { return x * v.x + y * v.y + z * v.z; }
    Vec3 operator+(const Vec3 &v) const { return Vec3(x + v.x, y + v.y, z + v.z); }
    Vec3 operator+(double b) const { return Vec3(x + b, y + b, z + b); }
    Vec3 operator-(const Vec3 &v) const { return Vec3(x - v.x, y - v.y, z - v.z); }
    Vec3 operator-(double b) const { return Vec3(x - b, y - b, z - b); }
    Vec3 operator-() const { return Vec3(-x, -y, -z); }
    Vec3 cross(const Vec3 &b) const { return Vec3(y * b.z - z * b.y, z * b.x - x * b.z, x * b.y - y * b.x); }
    void print() const { std::printf("x: %.6lf, y: %.6lf, z: %.6lf\n", x, y, z); }
    void get(double out[3]) const { out[0] = x; out[1] = y; out[2] = z; }
};
inline double det(const Vec3 &a, const Vec3 &b, const Vec3 &c) {
    return (a.x * b.y * c.z + b.x * c.y * a.z + c.x * a.y * b.z - a.x * c.y * b.z - b.x * a.y * c.z - c.x * b.y * a.z);
}
inline Vec3 matrixVectorProduct(const Vec3 &a, const Vec3 &b, const Vec3 &c, const Vec3 &d) {
    return a * d.x + b * d.y + c * d.z;
}
// adjugate / determinant, "singular" when |det| < 1e-4 (vec3.h:103-119)
inline bool inv(const Vec3 &a, const Vec3 &b, const Vec3 &c, Vec3 &resa, Vec3 &resb, Vec3 &resc) {
    const double d = det(a, b, c);
    if (d < 1e-4 && d > -1e-4) return false;
    resa = Vec3((b.y * c.z - b.z * c.y) / d, (c.y * a.z - c.z * a.y) / d, (a.y * b.z - a.z * b.y) / d);
    resb = Vec3((c.x * b.z - c.z * b.x) / d, (a.x * c.z - a.z * c.x) / d, (b.x * a.z - b.z * a.x) / d);
    resc = Vec3((b.x * c.y - c.x * b.y) / d, (c.x * a.y - c.y * a.x) / d, (a.x * b.y - a.y * b.x) / d);
    return true;
}

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
inline int check(int rc) {
    if (rc < 0) throw Error(rc, std::string("libcgrt: ") + cgrt_last_error());
    return rc;
}

// ---- texture.h:14-83 ------------------------------------------------------------------------------
// The reference builds `data` from 8-bit image bytes as byte/256 (main.cpp:303-316); the device stores the
// bytes, so every texel must be k/256 for an integer k in 0..255 (anything else is rejected).
class Texture {
  public:
    Texture() : rows(0), cols(0), lenx(0), leny(0), isbump(false), htexture(false) {}
    Texture(const std::vector<std::vector<Vec3> > &d, const Vec3 &n, const Vec3 &p, double lx, double ly,
            bool flag = false)
        : rows((int)d.size()), cols(d.empty() ? 0 : (int)d[0].size()), normal(n), position(p), lenx(lx), leny(ly),
          isbump(flag), htexture(true) {
        rgb.resize((size_t)rows * cols * 3);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++) {
                const double c[3] = {d[i][j].x, d[i][j].y, d[i][j].z};
                for (int k = 0; k < 3; k++) {
                    const double b = c[k] * 256.0;
                    if (!(b >= 0 && b <= 255 && b == std::floor(b)))
                        throw Error(CGRT_ERR_INVALID, "Texture: texel is not byte/256");
                    rgb[3 * ((size_t)i * cols + j) + k] = (uint8_t)b;
                }
            }
    }
    // same object straight from decoder output (rows*cols*3 bytes)
    Texture(const uint8_t *bytes, int rows_, int cols_, const Vec3 &n, const Vec3 &p, double lx, double ly,
            bool flag = false)
        : rows(rows_), cols(cols_), rgb(bytes, bytes + (size_t)rows_ * cols_ * 3), normal(n), position(p), lenx(lx),
          leny(ly), isbump(flag), htexture(true) {}
    int rows, cols;
    std::vector<uint8_t> rgb;
    Vec3 normal, position;
    double lenx, leny;
    bool isbump, htexture;
};

// ---- objects.h:17-24 ------------------------------------------------------------------------------
class SceneBuilder;
class Object {
  public:
    Object() : probe_(nullptr) {}
    Object(const Object &) : probe_(nullptr) {}  // a copy builds its own probe scene when first asked
    Object &operator=(const Object &);           // the assigned-to object's cached probe scene is dropped
    virtual ~Object();
    // objects.h:20: nearest intersection of one ray with this object.  Runs ON THE DEVICE (this object alone, committed
    // once on `intersect_device` and cached; the function-level probe cgrt_intersect_rays) -- there is no host tracer.
    // len and normalvec are written only on a hit.  For many rays use intersect_batch.
    bool intersect(const Vec3 &rayorig, const Vec3 &raydir, double &len, Vec3 &normalvec) const;
    // n rays at once: org3 / dir3 are n x 3 doubles; hit, len, normal3 receive n, n and n x 3 values
    void intersect_batch(const double *org3, const double *dir3, int n, int32_t *hit, double *len, double *normal3) const;
    virtual double getTransparency() const = 0;
    virtual double getReflection() const = 0;
    virtual Vec3 getSurfaceColor(const Vec3 &) const = 0;  // flat colour; textured lookups happen on the device
    virtual int add_to(SceneBuilder &sb) const = 0;         // appends this object to a cgrt_scene
    int intersect_device = 0;

  private:
    mutable SceneBuilder *probe_;
};

class SceneBuilder {
  public:
    cgrt_scene *scene;
    std::map<const Texture *, int> tex_ids;
    SceneBuilder() : scene(nullptr) { check(cgrt_scene_create(&scene)); }
    ~SceneBuilder() { cgrt_scene_destroy(scene); }
    SceneBuilder(const SceneBuilder &) = delete;
    SceneBuilder &operator=(const SceneBuilder &) = delete;
    int texture(const Texture &t) {
        if (!t.htexture) return -1;
        auto it = tex_ids.find(&t);
        if (it != tex_ids.end()) return it->second;
        double n[3], p[3];
        t.normal.get(n);
        t.position.get(p);
        int id = check(cgrt_scene_add_texture(scene, t.rgb.data(), t.rows, t.cols, n, p, t.lenx, t.leny, t.isbump));
        tex_ids[&t] = id;
        return id;
    }
};

inline Object::~Object() { delete probe_; }
inline Object &Object::operator=(const Object &) {
    delete probe_;
    probe_ = nullptr;
    return *this;
}
inline void Object::intersect_batch(const double *org3, const double *dir3, int n, int32_t *hit, double *len,
                                    double *normal3) const {
    if (!probe_) {
        SceneBuilder *sb = new SceneBuilder();
        try {
            add_to(*sb);
            check(cgrt_scene_commit(sb->scene, intersect_device));
        } catch (...) {
            delete sb;
            throw;
        }
        probe_ = sb;
    }
    check(cgrt_intersect_rays(probe_->scene, 0, org3, dir3, nullptr, n, hit, len, normal3));
}
inline bool Object::intersect(const Vec3 &rayorig, const Vec3 &raydir, double &len, Vec3 &normalvec) const {
    double o[3], d[3], l = 0, nv[3] = {0, 0, 0};
    int32_t h = 0;
    rayorig.get(o);
    raydir.get(d);
    intersect_batch(o, d, 1, &h, &l, nv);
    if (h) {
        len = l;
        normalvec = Vec3(nv[0], nv[1], nv[2]);
    }
    return h != 0;
}

// Sphere(c, r, sc, refl, transp, ec)   objects.h:28-38
class Sphere : public Object {
  public:
    Sphere(const Vec3 &c, const double &r, const Vec3 &sc, const double &refl = 0, const double &transp = 0,
           const Vec3 & /*ec*/ = 0)
        : center(c), radius(r), surfaceColor(sc), transparency(transp), reflection(refl) {}
    double getTransparency() const override { return transparency; }
    double getReflection() const override { return reflection; }
    Vec3 getSurfaceColor(const Vec3 &) const override { return surfaceColor.copy(); }
    int add_to(SceneBuilder &sb) const override {
        double c[3], s[3];
        center.get(c);
        surfaceColor.get(s);
        return check(cgrt_scene_add_sphere(sb.scene, c, radius, s, reflection, transparency));
    }
  private:
    Vec3 center;
    double radius;
    Vec3 surfaceColor;
    double transparency, reflection;
};

// Plane(p, n, sc, refl, transp, tx, ec)   objects.h:480
class Plane : public Object {
  public:
    Plane(const Vec3 &p, const Vec3 &n, const Vec3 &sc, const double &refl = 0, const double &transp = 0,
          const Texture &tx = Texture(), const Vec3 & /*ec*/ = 0)
        : position(p), normal(n), surfaceColor(sc), transparency(transp), reflection(refl), texture(tx) {}
    double getTransparency() const override { return transparency; }
    double getReflection() const override { return reflection; }
    Vec3 getSurfaceColor(const Vec3 &) const override { return surfaceColor.copy(); }
    int add_to(SceneBuilder &sb) const override {
        double p[3], n[3], s[3];
        position.get(p);
        normal.get(n);
        surfaceColor.get(s);
        return check(cgrt_scene_add_plane(sb.scene, p, n, s, reflection, transparency, sb.texture(texture)));
    }
  private:
    Vec3 position, normal, surfaceColor;
    double transparency, reflection;
    Texture texture;
};

// TriangleMesh(filename, a, b, sc, refl, transp, typeofdata, ec)   objects.h:338-340
class TriangleMesh : public Object {
  public:
    TriangleMesh(const char *filename, double a_, const Vec3 &b_, const Vec3 &sc, const double &refl = 0,
                 const double &transp = 0, int typeofdata = 0, const Vec3 & /*ec*/ = 0)
        : file(filename ? filename : ""), a(a_), b(b_), surfaceColor(sc), transparency(transp), reflection(refl),
          objtype(typeofdata) {}
    double getTransparency() const override { return transparency; }
    double getReflection() const override { return reflection; }
    Vec3 getSurfaceColor(const Vec3 &) const override { return surfaceColor.copy(); }
    int add_to(SceneBuilder &sb) const override {
        double bb[3], s[3];
        b.get(bb);
        surfaceColor.get(s);
        return check(cgrt_scene_add_mesh_file(sb.scene, file.c_str(), a, bb, s, reflection, transparency, objtype));
    }
  private:
    std::string file;
    double a;
    Vec3 b, surfaceColor;
    double transparency, reflection;
    int objtype;
};

// The same object from triangles in memory (cgrt_scene_add_mesh_triangles): 9 doubles per triangle -- pa, pb, pc, already
// transformed.  What a program that animates a mesh starts from (DeformingScene below).
class TriangleSoup : public Object {
  public:
    TriangleSoup(std::vector<double> tri9_, const Vec3 &sc, const double &refl = 0, const double &transp = 0, int typeofdata = 0)
        : tri9(std::move(tri9_)), surfaceColor(sc), transparency(transp), reflection(refl), objtype(typeofdata) {
        if (tri9.size() % 9) throw Error(CGRT_ERR_INVALID, "TriangleSoup: 9 doubles per triangle");
    }
    double getTransparency() const override { return transparency; }
    double getReflection() const override { return reflection; }
    Vec3 getSurfaceColor(const Vec3 &) const override { return surfaceColor.copy(); }
    int add_to(SceneBuilder &sb) const override {
        double s[3];
        surfaceColor.get(s);
        return check(cgrt_scene_add_mesh_triangles(sb.scene, tri9.data(), (int)(tri9.size() / 9), s, reflection, transparency, objtype));
    }
    std::vector<double> tri9;
  private:
    Vec3 surfaceColor;
    double transparency, reflection;
    int objtype;
};

// Bezier(points, pos, sc, refl, transp, typeofdata, ec)   bezier.h:44-45
class Bezier : public Object {
  public:
    Bezier(std::vector<Vec3> points, const Vec3 &pos, const Vec3 &sc, const double &refl = 0,
           const double &transp = 0, int /*typeofdata*/ = 0, const Vec3 & /*ec*/ = 0)
        : cpoints(points), position(pos), surfaceColor(sc), transparency(transp), reflection(refl) {}
    double getTransparency() const override { return transparency; }
    double getReflection() const override { return reflection; }
    Vec3 getSurfaceColor(const Vec3 &) const override { return surfaceColor.copy(); }
    int add_to(SceneBuilder &sb) const override {
        std::vector<double> cp;
        for (const Vec3 &v : cpoints) { cp.push_back(v.x); cp.push_back(v.y); cp.push_back(v.z); }
        double p[3], s[3];
        position.get(p);
        surfaceColor.get(s);
        return check(cgrt_scene_add_bezier(sb.scene, cp.data(), (int)cpoints.size(), p, s, reflection, transparency));
    }
  private:
    std::vector<Vec3> cpoints;
    Vec3 position, surfaceColor;
    double transparency, reflection;
};

// ---- render(), main.cpp:169-219 -------------------------------------------------------------------
// The reference's compile-time constants and render() locals, as runtime fields with the same defaults.
struct RenderParams {
    int width = 1024, height = 768;       // main.cpp:28-29
    int num_of_samples = 1;               // main.cpp:177
    double focus_plane = 20.0;            // main.cpp:178
    double radius = 1.5;                  // main.cpp:179 (lens radius)
    Vec3 camorg = Vec3(0, 0, -10);        // main.cpp:181
    int max_depth = 5;                    // MAX_DEPTH, main.cpp:35
    bool depth_of_field = false;          // false: the committed pinhole call (main.cpp:209); true: main.cpp:207
    uint64_t seed = 12345;
    int device = 0;
    double half_width = 10.0;             // the literal 10.0 of main.cpp:188-189
    // The posed camera (cgrt_posed_camera): camorg, half_width, focus_plane and radius describe the camera in its own frame;
    // set_pose / look_at place that frame in the world.  Unset, the frame is the built-in one and nothing changes.
    bool posed = false;
    double pose_origin[3] = {0, 0, 0}, pose_right[3] = {1, 0, 0}, pose_up[3] = {0, 1, 0}, pose_forward[3] = {0, 0, 1};
    void set_pose(const Vec3 &origin, const Vec3 &right, const Vec3 &up, const Vec3 &forward) {
        origin.get(pose_origin);
        right.get(pose_right);
        up.get(pose_up);
        forward.get(pose_forward);
        posed = true;
    }
    // cgrt_look_at: the eye at `eye`, the image centre on `target`, horizontal field of view fov_x_deg, sharp at
    // focus_distance from the eye (the lens stays `radius`, used when depth_of_field is set)
    void look_at(const Vec3 &eye, const Vec3 &target, const Vec3 &up_hint, double fov_x_deg, double focus_distance) {
        double e[3], t[3], u[3];
        eye.get(e);
        target.get(t);
        up_hint.get(u);
        cgrt_posed_camera pc;
        check(cgrt_look_at(e, t, u, fov_x_deg, focus_distance, radius, &pc));
        camorg = Vec3(pc.base.cam[0], pc.base.cam[1], pc.base.cam[2]);
        half_width = pc.base.half_width;
        focus_plane = pc.base.focus_plane;
        for (int k = 0; k < 3; k++) {
            pose_origin[k] = pc.origin[k];
            pose_right[k] = pc.right[k];
            pose_up[k] = pc.up[k];
            pose_forward[k] = pc.forward[k];
        }
        posed = true;
    }
    // The camera of a call over grid g: pc filled from these fields, CGRT_GRID_POSED set in g where a pose is; what to pass
    const cgrt_camera *camera(cgrt_posed_camera &pc, cgrt_grid &g) const {
        camorg.get(pc.base.cam);
        pc.base.half_width = half_width;
        pc.base.focus_plane = focus_plane;
        pc.base.lens_radius = depth_of_field ? radius : 0.0;
        for (int k = 0; k < 3; k++) {
            pc.origin[k] = pose_origin[k];
            pc.right[k] = pose_right[k];
            pc.up[k] = pose_up[k];
            pc.forward[k] = pose_forward[k];
        }
        if (posed) g.flags |= CGRT_GRID_POSED;
        return &pc.base;
    }
};
struct RenderStats {
    uint64_t rays = 0, hitpoints = 0;
};

// Eye pass of render(objs): image[h][w] (row 0 = bottom, main.cpp:185-189) receives, per channel, the sum of
// hp.f over the pixel's hitpoints divided by num_of_samples, as float RGB.  (For the photon pass and tone mapping
// that follow in the reference, main.cpp:223-258, see render_ppm below.)
inline void render(const std::vector<Object *> &objs, const RenderParams &rp, std::vector<float> &image,
                   RenderStats *stats = nullptr) {
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    check(cgrt_scene_commit(sb.scene, rp.device));
    cgrt_grid g{};
    cgrt_posed_camera pc;
    const cgrt_camera *cam = rp.camera(pc, g);
    g.width = rp.width;
    g.height = rp.height;
    g.rows = rp.height;
    g.stripe_nranks = 1;
    g.spp = rp.num_of_samples;
    g.spp_total = rp.num_of_samples;
    g.max_depth = rp.max_depth;
    g.seed = rp.seed;
    image.assign((size_t)rp.width * rp.height * 3, 0.f);
    uint64_t cnt[CGRT_NCOUNTERS] = {0};
    check(cgrt_trace_grid_host(sb.scene, cam, &g, image.data(), nullptr, cnt));
    if (stats) {
        stats->rays = cnt[CGRT_CNT_RAYS];
        stats->hitpoints = cnt[CGRT_CNT_HITPOINTS];
    }
}

// The frame's feature buffers (cgrt_trace_grid_aov_host): per pixel of render()'s frame, row 0 = bottom, the first hit's albedo
// and normal (turned against the ray) averaged over the samples, the summed hit distance / num_of_samples, the samples that hit
// and the object -- its position in objs -- the first sample hits, or -1.  What a denoiser, a compositor or a picker asks for.
struct GridAov {
    std::vector<float> albedo, normal;  // 3 per pixel
    std::vector<float> depth;           // mean depth over the hits: depth * num_of_samples / hits
    std::vector<uint32_t> hits;
    std::vector<int32_t> obj_id;
};
inline void render_aov(cgrt_scene *scene, const RenderParams &rp, GridAov &aov, RenderStats *stats) {
    cgrt_grid g{};
    cgrt_posed_camera pc;
    const cgrt_camera *cam = rp.camera(pc, g);
    g.width = rp.width;
    g.height = rp.height;
    g.rows = rp.height;
    g.stripe_nranks = 1;
    g.spp = rp.num_of_samples;
    g.spp_total = rp.num_of_samples;
    g.seed = rp.seed;
    const size_t npx = (size_t)rp.width * rp.height;
    aov.albedo.assign(npx * 3, 0.f);
    aov.normal.assign(npx * 3, 0.f);
    aov.depth.assign(npx, 0.f);
    aov.hits.assign(npx, 0u);
    aov.obj_id.assign(npx, -1);
    const cgrt_grid_aov out = {aov.albedo.data(), aov.normal.data(), aov.depth.data(), aov.hits.data(), aov.obj_id.data()};
    uint64_t cnt[CGRT_NCOUNTERS] = {0};
    check(cgrt_trace_grid_aov_host(scene, cam, &g, &out, cnt));
    if (stats) stats->rays = cnt[CGRT_CNT_RAYS];
}
inline void render_aov(const std::vector<Object *> &objs, const RenderParams &rp, GridAov &aov, RenderStats *stats = nullptr) {
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    check(cgrt_scene_commit(sb.scene, rp.device));
    render_aov(sb.scene, rp, aov, stats);
}

// trace() for rays of the caller's own (cgrt_trace_rays_host): acc[i] = the sum of hp.f over ray i's Hitpoints (three doubles, not
// divided by anything), nhit[i] their number; dir is used as given (unit length is the caller's contract).  A look-at camera,
// a fisheye or a light probe is a ray list away.
struct RayHit {
    std::vector<int32_t> obj;   // position in objs of the nearest object hit by the ray itself, -1 for none
    std::vector<double> t, normal;  // its distance (0 on a miss); the normal intersect() returned (3 per ray)
};
inline void trace_rays(const std::vector<Object *> &objs, const std::vector<double> &org3, const std::vector<double> &dir3,
                       std::vector<double> &acc3, std::vector<uint32_t> *nhit = nullptr, RayHit *hit = nullptr, int max_depth = 5,
                       uint64_t seed = 12345, int device = 0, RenderStats *stats = nullptr) {
    if (org3.size() != dir3.size() || org3.size() % 3) throw Error(CGRT_ERR_INVALID, "trace_rays: org3 / dir3 are n x 3 doubles");
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    check(cgrt_scene_commit(sb.scene, device));
    const size_t n = org3.size() / 3;
    cgrt_rays r{};
    r.n = (int64_t)n;
    r.org3 = org3.data();
    r.dir3 = dir3.data();
    r.seed = seed;
    r.max_depth = max_depth;
    acc3.assign(3 * n, 0.0);
    cgrt_ray_results out{};
    out.acc3 = acc3.data();
    if (nhit) {
        nhit->assign(n, 0u);
        out.nhit = nhit->data();
    }
    if (hit) {
        hit->obj.assign(n, -1);
        hit->t.assign(n, 0.0);
        hit->normal.assign(3 * n, 0.0);
        out.hit_obj = hit->obj.data();
        out.hit_t = hit->t.data();
        out.hit_normal3 = hit->normal.data();
    }
    uint64_t cnt[CGRT_NCOUNTERS] = {0};
    check(cgrt_trace_rays_host(sb.scene, &r, &out, cnt));
    if (stats) {
        stats->rays = cnt[CGRT_CNT_RAYS];
        stats->hitpoints = cnt[CGRT_CNT_HITPOINTS];
    }
}

// What a host program needs to shade the hits trace_rays reported (cgrt_ray_hit_attributes_host): per ray the triangle of a
// mesh or bump floor in construction order (-1 where the hit is no triangle) with the point on it -- (1-u-v)*pa + u*pb + v*pc
// --, getSurfaceColor at the hit and the object's (reflection, transparency).  `hits` is the RayHit trace_rays filled for the
// same org3 / dir3.
struct HitAttributes {
    std::vector<int32_t> prim;               // 1 per ray
    std::vector<double> uv, color, material; // 2, 3 and 2 per ray
};
inline void hit_attributes(const std::vector<Object *> &objs, const std::vector<double> &org3, const std::vector<double> &dir3,
                           const RayHit &hits, HitAttributes &attr, int device = 0) {
    if (org3.size() != dir3.size() || org3.size() % 3) throw Error(CGRT_ERR_INVALID, "hit_attributes: org3 / dir3 are n x 3 doubles");
    const size_t n = org3.size() / 3;
    if (hits.obj.size() != n || hits.t.size() != n) throw Error(CGRT_ERR_INVALID, "hit_attributes: hits holds one entry per ray");
    attr.prim.assign(n, -1);
    attr.uv.assign(2 * n, 0.0);
    attr.color.assign(3 * n, 0.0);
    attr.material.assign(2 * n, 0.0);
    if (n == 0) return;
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    check(cgrt_scene_commit(sb.scene, device));
    cgrt_rays r{};
    r.n = (int64_t)n;
    r.org3 = org3.data();
    r.dir3 = dir3.data();
    cgrt_hit_attributes out{};
    out.prim = attr.prim.data();
    out.uv2 = attr.uv.data();
    out.color3 = attr.color.data();
    out.material2 = attr.material.data();
    check(cgrt_ray_hit_attributes_host(sb.scene, &r, hits.obj.data(), hits.t.data(), &out));
}

// "Is anything between these two points?" (cgrt_occlusion_rays_host): occ[i] = 1 exactly when some object's intersect() gives
// a length < tmax[i] for ray i -- the nearest hit trace_rays would report lies before tmax[i] --, else 0.  An empty tmax means
// no limit.  skip_transparent: objects with transparency >= 1e-4 block nothing (shadow rays through glass).  `seed` keys the
// Bezier draws as trace_rays' does.
inline void occluded(const std::vector<Object *> &objs, const std::vector<double> &org3, const std::vector<double> &dir3,
                     const std::vector<double> &tmax, std::vector<uint8_t> &occ, bool skip_transparent = false, uint64_t seed = 12345,
                     int device = 0) {
    if (org3.size() != dir3.size() || org3.size() % 3) throw Error(CGRT_ERR_INVALID, "occluded: org3 / dir3 are n x 3 doubles");
    const size_t n = org3.size() / 3;
    if (!tmax.empty() && tmax.size() != n) throw Error(CGRT_ERR_INVALID, "occluded: tmax holds one entry per ray, or none");
    occ.assign(n, 0);
    if (n == 0) return;
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    check(cgrt_scene_commit(sb.scene, device));
    cgrt_rays r{};
    r.n = (int64_t)n;
    r.org3 = org3.data();
    r.dir3 = dir3.data();
    r.seed = seed;
    r.max_depth = 1;
    r.flags = skip_transparent ? CGRT_RAYS_SKIP_TRANSPARENT : 0;
    cgrt_occlusion out{};
    out.tmax = tmax.empty() ? nullptr : tmax.data();
    out.occluded = occ.data();
    check(cgrt_occlusion_rays_host(sb.scene, &r, &out, nullptr));
}

// One step of trace() per ray (cgrt_bounce_rays_host): the nearest hit, then what trace() does there -- a Hitpoint's value
// f * adj, or the child rays with their throughput.  Feed child_org / child_dir / child_adj / child_path / child_keys back as
// the next level's org3 / dir3 / adj3 / path / keys (rows with dir = 0 are absent children and are not traced), as deep as the
// caller likes; the Hitpoint values of a root's tree, summed depth first with the reflected subtree before the refracted one,
// are trace_rays' sum for that root.
struct BounceLevel {
    std::vector<uint8_t> step;                                      // [n] CGRT_STEP_*
    std::vector<int32_t> obj;                                       // [n] nearest object, -1 for none
    std::vector<double> t, pos, normal, value;                      // [n], [n][3] x 3
    std::vector<double> child_org, child_dir, child_adj;            // [2n][3]: row i reflected, row n + i refracted child
    std::vector<uint32_t> child_path;                               // [2n]
    std::vector<uint64_t> child_keys;                               // [2n]
};
// adj3 / path / keys: empty for the roots' defaults -- (1,1,1), 1, the keys derived from `seed`
inline void bounce(const std::vector<Object *> &objs, const std::vector<double> &org3, const std::vector<double> &dir3,
                   const std::vector<double> &adj3, const std::vector<uint32_t> &path, const std::vector<uint64_t> &keys,
                   BounceLevel &out, uint64_t seed = 12345, int device = 0) {
    if (org3.size() != dir3.size() || org3.size() % 3) throw Error(CGRT_ERR_INVALID, "bounce: org3 / dir3 are n x 3 doubles");
    const size_t n = org3.size() / 3;
    if ((!adj3.empty() && adj3.size() != 3 * n) || (!path.empty() && path.size() != n) || (!keys.empty() && keys.size() != n))
        throw Error(CGRT_ERR_INVALID, "bounce: adj3, path and keys hold one entry per ray, or none");
    out.step.assign(n, 0);
    out.obj.assign(n, -1);
    out.t.assign(n, 0.0);
    out.pos.assign(3 * n, 0.0);
    out.normal.assign(3 * n, 0.0);
    out.value.assign(3 * n, 0.0);
    out.child_org.assign(6 * n, 0.0);
    out.child_dir.assign(6 * n, 0.0);
    out.child_adj.assign(6 * n, 0.0);
    out.child_path.assign(2 * n, 0u);
    out.child_keys.assign(2 * n, 0u);
    if (n == 0) return;
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    check(cgrt_scene_commit(sb.scene, device));
    cgrt_rays r{};
    r.n = (int64_t)n;
    r.org3 = org3.data();
    r.dir3 = dir3.data();
    r.keys = keys.empty() ? nullptr : keys.data();
    r.seed = seed;
    r.max_depth = 1;
    cgrt_bounce b{};
    b.adj3 = adj3.empty() ? nullptr : adj3.data();
    b.path = path.empty() ? nullptr : path.data();
    b.step = out.step.data();
    b.hit_obj = out.obj.data();
    b.hit_t = out.t.data();
    b.pos3 = out.pos.data();
    b.normal3 = out.normal.data();
    b.value3 = out.value.data();
    b.child_org3 = out.child_org.data();
    b.child_dir3 = out.child_dir.data();
    b.child_adj3 = out.child_adj.data();
    b.child_path = out.child_path.data();
    b.child_keys = out.child_keys.data();
    check(cgrt_bounce_rays_host(sb.scene, &r, &b, nullptr));
}

// The depth loop over bounce() inside the library (cgrt_wavefront_rays_host): every ray traced to max_depth levels (1..31), its
// Hitpoint values summed in emission order -- trace_rays' sum for max_depth <= 5, and beyond.  min_adj: a child whose throughput
// has max(x, y, z) < min_adj is not spawned.  hp_cap > 0: the Hitpoint records too, by ray, then emission order.
struct WavefrontResult {
    std::vector<double> acc;        // [n][3]
    std::vector<uint32_t> nhit;     // [n]
    std::vector<double> hp9;        // [min(hp_count, hp_cap)][9] value, pos, normal
    std::vector<int64_t> hp_ray;    // the record's ray
    std::vector<uint32_t> hp_path;  // its place in the ray's tree
    uint64_t hp_count = 0, rays = 0;
    int64_t slices = 0, halvings = 0;
    int32_t levels = 0;
};
inline void wavefront(const std::vector<Object *> &objs, const std::vector<double> &org3, const std::vector<double> &dir3,
                      const std::vector<uint64_t> &keys, int max_depth, WavefrontResult &out, double min_adj = 0.0, uint64_t hp_cap = 0,
                      uint64_t seed = 12345, int64_t work_bytes = 0, int device = 0) {
    if (org3.size() != dir3.size() || org3.size() % 3) throw Error(CGRT_ERR_INVALID, "wavefront: org3 / dir3 are n x 3 doubles");
    const size_t n = org3.size() / 3;
    if (!keys.empty() && keys.size() != n) throw Error(CGRT_ERR_INVALID, "wavefront: keys hold one entry per ray, or none");
    out = WavefrontResult();
    out.acc.assign(3 * n, 0.0);
    out.nhit.assign(n, 0u);
    out.hp9.assign(9 * (size_t)hp_cap, 0.0);
    out.hp_ray.assign((size_t)hp_cap, 0);
    out.hp_path.assign((size_t)hp_cap, 0u);
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    if (n > 0) check(cgrt_scene_commit(sb.scene, device));
    cgrt_rays r{};
    r.n = (int64_t)n;
    r.org3 = org3.data();
    r.dir3 = dir3.data();
    r.keys = keys.empty() ? nullptr : keys.data();
    r.seed = seed;
    r.max_depth = 1;
    cgrt_wavefront w{};
    w.max_depth = max_depth;
    w.min_adj = min_adj;
    w.work_bytes = work_bytes;
    w.acc3 = out.acc.data();
    w.nhit = out.nhit.data();
    w.hp9 = hp_cap ? out.hp9.data() : nullptr;
    w.hp_ray = hp_cap ? out.hp_ray.data() : nullptr;
    w.hp_path = hp_cap ? out.hp_path.data() : nullptr;
    w.hp_cap = hp_cap;
    uint64_t counters[CGRT_NCOUNTERS] = {};
    check(cgrt_wavefront_rays_host(sb.scene, &r, &w, counters, &out.hp_count));
    out.rays = counters[CGRT_CNT_RAYS];
    const size_t m = (size_t)(out.hp_count < hp_cap ? out.hp_count : hp_cap);
    out.hp9.resize(9 * m);
    out.hp_ray.resize(m);
    out.hp_path.resize(m);
    if (n > 0) check(cgrt_scene_last_wavefront(sb.scene, &out.slices, &out.halvings, &out.levels));
}

// ---- the whole of render() + main()'s PNG loop: main.cpp:169-258, 403-412 ---------------------------------------
// Photon-pass constants of the reference as runtime fields with the same defaults.
struct PhotonParams {
    Vec3 lightorg = Vec3(0, 19.999, 20);   // main.cpp:180
    double jitter = 2.0;                   // main.cpp:240-241 (u*4-2)
    double power = 700.0;                  // main.cpp:246
    double alpha = 0.7;                    // main.cpp:36
    long long num_photon = 2560000;        // main.cpp:223
    int num_threads = 8;                   // main.cpp:224: total photons = num_photon * num_threads
    int hashsize = 1000001;                // main.cpp:184
    uint64_t seed = 777;
    double initial_radius = 0.0;           // main.cpp:84,183: 200.0 / height with the reference's compile-time height;
                                           // 0 = the committed 200.0 / 768
};
struct PpmStats {
    uint64_t hitpoints = 0, photon_events = 0;
    double ms_eye = 0, ms_table = 0, ms_photons = 0, ms_gather = 0;
};

// render(objs) as the reference runs it: eye pass, photon pass (serial semantics: photon i on the keyed stream
// (seed, i); the reference's racing OpenMP threads over time-seeded rand() have no reproducible meaning), final
// gather into image[h][w] (doubles, row 0 = bottom, main.cpp:252-258) and the tone-mapped, flipped bytes that
// main.cpp:403-411 hands to stbi_write_png.
inline void render_ppm(const std::vector<Object *> &objs, const RenderParams &rp, const PhotonParams &pp,
                       std::vector<double> &image, std::vector<unsigned char> &image_data, PpmStats *stats = nullptr) {
    SceneBuilder sb;
    for (const Object *o : objs) o->add_to(sb);
    check(cgrt_scene_commit(sb.scene, rp.device));
    cgrt_grid g{};
    cgrt_posed_camera pc;
    const cgrt_camera *cam = rp.camera(pc, g);
    g.width = rp.width;
    g.height = rp.height;
    g.rows = rp.height;
    g.stripe_nranks = 1;
    g.spp = rp.num_of_samples;
    g.spp_total = rp.num_of_samples;
    g.max_depth = rp.max_depth;
    g.seed = rp.seed;
    cgrt_photons ph{};
    pp.lightorg.get(ph.light);
    ph.jitter = pp.jitter;
    ph.power = pp.power;
    ph.alpha = pp.alpha;
    ph.nphotons = pp.num_photon * pp.num_threads;
    ph.hashsize = pp.hashsize;
    ph.seed = pp.seed;
    ph.initial_radius = pp.initial_radius;  // 0: the reference's committed 200.0 / 768 (main.cpp:84,183)
    image.assign((size_t)rp.width * rp.height * 3, 0.0);
    image_data.assign((size_t)rp.width * rp.height * 3, 0);
    cgrt_ppm_result out{};
    out.image = image.data();
    out.rgb8 = image_data.data();
    check(cgrt_ppm_render(sb.scene, cam, &g, &ph, &out));
    if (stats) {
        stats->hitpoints = out.hp_count;
        stats->photon_events = out.n_events;
        stats->ms_eye = out.ms_eye; stats->ms_table = out.ms_table;
        stats->ms_photons = out.ms_photons; stats->ms_gather = out.ms_gather;
    }
}

// render() as a live, resumable render: the eye pass and hash table once, then photons added in as many steps as wanted
// (cgrt_ppm_session).  After add_photons calls totalling k, image() equals render_ppm with k photons bit for bit.
// pp.num_photon / pp.num_threads are not used here: no photon is traced until add_photons.
class PpmSession {
  public:
    PpmSession(const std::vector<Object *> &objs, const RenderParams &rp, const PhotonParams &pp, bool lookahead = true)
        : width_(rp.width), height_(rp.height), session_(nullptr) {
        for (const Object *o : objs) o->add_to(sb_);
        check(cgrt_scene_commit(sb_.scene, rp.device));
        cgrt_grid g{};
        cgrt_posed_camera pc;
        const cgrt_camera *cam = rp.camera(pc, g);
        g.width = rp.width;
        g.height = rp.height;
        g.rows = rp.height;
        g.stripe_nranks = 1;
        g.spp = rp.num_of_samples;
        g.spp_total = rp.num_of_samples;
        g.max_depth = rp.max_depth;
        g.seed = rp.seed;
        const cgrt_photons ph = photons(pp);
        check(cgrt_ppm_session_create(sb_.scene, cam, &g, &ph, lookahead ? 0 : CGRT_PPM_SESSION_NO_LOOKAHEAD, &session_));
    }
    // The same live render over caller-supplied rays (cgrt_ppm_session_create_rays): any camera, or probe rays.  rays' arrays
    // and px.pixel are DEVICE pointers on device `device`, read before the constructor returns; px names the image that
    // image() fills (px.width x px.rows, row 0 = bottom).  For cgrt_camera_rays' rays of a grid and px.pixel == nullptr the
    // session is the grid constructor's, bit for bit.
    PpmSession(const std::vector<Object *> &objs, const cgrt_rays &rays, const cgrt_ray_pixels &px, const PhotonParams &pp,
               int device = 0, bool lookahead = true)
        : width_(px.width), height_(px.rows), session_(nullptr) {
        for (const Object *o : objs) o->add_to(sb_);
        check(cgrt_scene_commit(sb_.scene, device));
        const cgrt_photons ph = photons(pp);
        check(cgrt_ppm_session_create_rays(sb_.scene, &rays, &px, &ph, lookahead ? 0 : CGRT_PPM_SESSION_NO_LOOKAHEAD, &session_));
    }
    // The same live render over caller-supplied Hitpoint records (cgrt_ppm_session_create_hitpoints): the records of a wavefront
    // trace of any depth, records shaded or culled by the caller, or probes at given points and normals.  hps' arrays are DEVICE
    // pointers on device `device`, read before the constructor returns; hps names the image that image() fills (hps.width x
    // hps.rows, row 0 = bottom) and the photons' depth limit.  For all records of cgrt_wavefront_rays at max_depth <= 5 the
    // session is the ray constructor's on the same rays, bit for bit.
    PpmSession(const std::vector<Object *> &objs, const cgrt_hitpoints &hps, const PhotonParams &pp, int device = 0,
               bool lookahead = true)
        : width_(hps.width), height_(hps.rows), session_(nullptr) {
        for (const Object *o : objs) o->add_to(sb_);
        check(cgrt_scene_commit(sb_.scene, device));
        const cgrt_photons ph = photons(pp);
        check(cgrt_ppm_session_create_hitpoints(sb_.scene, &hps, &ph, lookahead ? 0 : CGRT_PPM_SESSION_NO_LOOKAHEAD, &session_));
    }
    ~PpmSession() { cgrt_ppm_session_destroy(session_); }  // before sb_ destroys the scene
    PpmSession(const PpmSession &) = delete;
    PpmSession &operator=(const PpmSession &) = delete;

    // traces photons [photons_done(), photons_done() + n) and applies them
    void add_photons(long long n) { check(cgrt_ppm_session_add_photons(session_, n)); }
    // caller-supplied photons (cgrt_ppm_session_add_photon_rays): pr's arrays are DEVICE pointers on the scene's device, read before
    // the call returns; the photons take the indices [photons_done(), photons_done() + pr.n), photons with dir = 0 included
    void add_photon_rays(const cgrt_photon_rays &pr) { check(cgrt_ppm_session_add_photon_rays(session_, &pr)); }
    long long photons_done() const { return (long long)info().photons_done; }
    // the gathered image (doubles, row 0 = bottom) and the bytes main.cpp:403-411 hands to stbi_write_png
    void image(std::vector<double> &image, std::vector<unsigned char> &image_data) const {
        image.assign((size_t)width_ * height_ * 3, 0.0);
        image_data.assign((size_t)width_ * height_ * 3, 0);
        check(cgrt_ppm_session_image(session_, image.data(), image_data.data()));
    }
    cgrt_ppm_session_info info() const {
        cgrt_ppm_session_info inf{};
        check(cgrt_ppm_session_get_info(session_, &inf));
        return inf;
    }

  private:
    static cgrt_photons photons(const PhotonParams &pp) {  // a session starts without photons
        cgrt_photons ph{};
        pp.lightorg.get(ph.light);
        ph.jitter = pp.jitter;
        ph.power = pp.power;
        ph.alpha = pp.alpha;
        ph.nphotons = 0;
        ph.hashsize = pp.hashsize;
        ph.seed = pp.seed;
        ph.initial_radius = pp.initial_radius;
        return ph;
    }
    int width_, height_;
    SceneBuilder sb_;
    cgrt_ppm_session *session_;
};

// Stochastic progressive photon mapping (cgrt_sppm_session): the statistics belong to the pixel, every pass traces
// rp.num_of_samples fresh eye samples per pixel and a fresh photon batch, and memory does not grow with the passes.  Pass k
// traces the samples k * num_of_samples .. of rp's camera; pp.num_photon / pp.num_threads are not used: add_passes says how many
// photons a pass traces.  pp.alpha must lie in (0, 1].
class SppmSession {
  public:
    SppmSession(const std::vector<Object *> &objs, const RenderParams &rp, const PhotonParams &pp, int photon_depth = 5)
        : width_(rp.width), height_(rp.height), session_(nullptr), grid_() {
        for (const Object *o : objs) o->add_to(sb_);
        check(cgrt_scene_commit(sb_.scene, rp.device));
        rp.camera(cam_, grid_);
        grid_.width = rp.width;
        grid_.height = rp.height;
        grid_.rows = rp.height;
        grid_.stripe_nranks = 1;
        grid_.spp = rp.num_of_samples;
        grid_.spp_total = rp.num_of_samples;
        grid_.max_depth = rp.max_depth;
        grid_.seed = rp.seed;
        cgrt_photons ph{};
        pp.lightorg.get(ph.light);
        ph.jitter = pp.jitter;
        ph.power = pp.power;
        ph.alpha = pp.alpha;
        ph.hashsize = pp.hashsize;
        ph.seed = pp.seed;
        ph.initial_radius = pp.initial_radius;
        check(cgrt_sppm_session_create(sb_.scene, rp.width, rp.height, rp.num_of_samples, photon_depth, &ph, 0, &session_));
    }
    ~SppmSession() { cgrt_sppm_session_destroy(session_); }  // before sb_ destroys the scene
    SppmSession(const SppmSession &) = delete;
    SppmSession &operator=(const SppmSession &) = delete;

    // n passes of the camera, each with photons_per_pass fresh photons
    void add_passes(int n, long long photons_per_pass) {
        for (int k = 0; k < n; k++) {
            grid_.sample_offset = (int32_t)(info().passes * grid_.spp);
            check(cgrt_sppm_session_pass_grid(session_, &cam_.base, &grid_, photons_per_pass));
        }
    }
    // one pass over caller-supplied rays (cgrt_sppm_session_pass_rays): DEVICE arrays on the scene's device; pixel may be null
    void add_pass_rays(const cgrt_rays &rays, const int64_t *pixel, long long nphotons) {
        check(cgrt_sppm_session_pass_rays(session_, &rays, pixel, nphotons));
    }
    long long passes() const { return (long long)info().passes; }
    long long photons_done() const { return (long long)info().photons_done; }
    // the image (doubles, row 0 = bottom) and the bytes main.cpp:403-411 hands to stbi_write_png
    void image(std::vector<double> &image, std::vector<unsigned char> &image_data) const {
        image.assign((size_t)width_ * height_ * 3, 0.0);
        image_data.assign((size_t)width_ * height_ * 3, 0);
        check(cgrt_sppm_session_image(session_, image.data(), image_data.data()));
    }
    // per pixel {N, R2, tau[3], M_p and Hitpoints of the last pass, 0}
    void pixels(std::vector<double> &px8) const {
        px8.assign((size_t)width_ * height_ * 8, 0.0);
        check(cgrt_sppm_session_pixels(session_, px8.data()));
    }
    cgrt_sppm_session_info info() const {
        cgrt_sppm_session_info inf{};
        check(cgrt_sppm_session_get_info(session_, &inf));
        return inf;
    }

  private:
    int width_, height_;
    SceneBuilder sb_;
    cgrt_sppm_session *session_;
    cgrt_posed_camera cam_;  // the camera with its pose (RenderParams::camera)
    cgrt_grid grid_;
};

// A scene committed ONCE whose opaque meshes move between frames (cgrt_scene_refit_mesh_host): refit_mesh gives object `obj` --
// its position in objs -- new vertices, 9 doubles per triangle in the order the mesh was made from; the hierarchy keeps its
// topology and the next render sees the moved mesh.  What may be refitted, the refusals and the parity class: cgrt.h.
// rebuild gives a device-built mesh a new topology too; cost tells when that pays.
class DeformingScene {
  public:
    // build: CGRT_BUILD_HOST / CGRT_BUILD_DEVICE for this scene's structures, or -1 for the default (rebuild() needs the latter)
    explicit DeformingScene(const std::vector<Object *> &objs, int device = 0, int build = -1) {
        if (build >= 0) check(cgrt_scene_set_build(sb_.scene, build));
        for (const Object *o : objs) o->add_to(sb_);
        check(cgrt_scene_commit(sb_.scene, device));
    }
    void refit_mesh(int obj, const std::vector<double> &tri9) {
        if (tri9.size() % 9) throw Error(CGRT_ERR_INVALID, "refit_mesh: 9 doubles per triangle");
        check(cgrt_scene_refit_mesh_host(sb_.scene, obj, tri9.data(), (int)(tri9.size() / 9)));
    }
    cgrt_refit_info refit_info(int obj) const {
        cgrt_refit_info inf;
        check(cgrt_scene_refit_info(sb_.scene, obj, &inf));
        return inf;
    }
    // A new hierarchy for these vertices, in place (cgrt_scene_rebuild_mesh_host): what a refit's kept topology costs in frame
    // time, a rebuild cures.  The mesh must have been built on the device (the constructor's build = CGRT_BUILD_DEVICE).
    void rebuild(int obj, const std::vector<double> &tri9) {
        if (tri9.size() % 9) throw Error(CGRT_ERR_INVALID, "rebuild: 9 doubles per triangle");
        check(cgrt_scene_rebuild_mesh_host(sb_.scene, obj, tri9.data(), (int)(tri9.size() / 9)));
    }
    cgrt_rebuild_info rebuild_info(int obj) const {
        cgrt_rebuild_info inf;
        check(cgrt_scene_rebuild_info(sb_.scene, obj, &inf));
        return inf;
    }
    // The surface-area cost of the hierarchy the device walks for mesh `obj` now (cgrt_scene_mesh_cost_host).  Rule of thumb:
    // rebuild when node_cost + tri_cost exceeds some multiple of its value after the last build.
    cgrt_tree_cost cost(int obj) const {
        cgrt_tree_cost c;
        check(cgrt_scene_mesh_cost_host(sb_.scene, obj, &c));
        return c;
    }
    // render()'s eye pass on the scene as it stands (rp.device is the constructor's)
    void render(const RenderParams &rp, std::vector<float> &image, RenderStats *stats = nullptr) const {
        cgrt_grid g{};
        cgrt_posed_camera pc;
        const cgrt_camera *cam = rp.camera(pc, g);
        g.width = rp.width;
        g.height = rp.height;
        g.rows = rp.height;
        g.stripe_nranks = 1;
        g.spp = rp.num_of_samples;
        g.spp_total = rp.num_of_samples;
        g.max_depth = rp.max_depth;
        g.seed = rp.seed;
        image.assign((size_t)rp.width * rp.height * 3, 0.f);
        uint64_t cnt[CGRT_NCOUNTERS] = {0};
        check(cgrt_trace_grid_host(sb_.scene, cam, &g, image.data(), nullptr, cnt));
        if (stats) {
            stats->rays = cnt[CGRT_CNT_RAYS];
            stats->hitpoints = cnt[CGRT_CNT_HITPOINTS];
        }
    }
    // render_aov()'s feature buffers of the scene as it stands
    void render_aov(const RenderParams &rp, GridAov &aov, RenderStats *stats = nullptr) const { cgrt_host::render_aov(sb_.scene, rp, aov, stats); }

  private:
    SceneBuilder sb_;
};

// stbi_write_png("test.png", width, height, 3, image_data, width * 3), main.cpp:412
inline void write_png(const char *path, int width, int height, const std::vector<unsigned char> &image_data) {
    check(cgrt_write_png(path, width, height, image_data.data()));
}

}  // namespace cgrt_host
#endif
