// C++ host mirror of the reference's public crate surface (src/lib.rs:1-10) for the render
// path: World / Camera / materials / textures / hittables with the reference's constructor
// names and argument order, so that its scene scripts (src/main.rs) transliterate line by
// line. Everything here is a thin description graph (shared_ptr ~ Arc) that is replayed onto
// the C ABI of include/pt_amd.h when World::build_bvh() runs; the integrator itself
// (Camera::render, camera.rs:79) executes in the HIP kernels behind pt_render().
//
// The reference is Rust; no Rust toolchain exists in this environment, hence C++ here. A Rust
// crate would bind the same C ABI. Rust `T::new(..)` is spelled `T::new_(..)`.
// Error behaviour follows the reference: asset/handle errors are fatal (Rust: unwrap()/panic;
// here: std::runtime_error), a failed image save is only reported (camera.rs:118-123).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"

namespace path_tracer {

struct Vec3 {
    double x = 0, y = 0, z = 0;
    static Vec3 new_(double x, double y, double z) { return Vec3{x, y, z}; }
    static Vec3 splat(double s) { return Vec3{s, s, s}; }
    static const Vec3 ZERO, ONE, X, Y, Z;
    Vec3 operator+(Vec3 o) const { return {x + o.x, y + o.y, z + o.z}; }
    Vec3 operator-(Vec3 o) const { return {x - o.x, y - o.y, z - o.z}; }
    Vec3 operator*(double s) const { return {x * s, y * s, z * s}; }
};
inline const Vec3 Vec3::ZERO{0, 0, 0}, Vec3::ONE{1, 1, 1}, Vec3::X{1, 0, 0}, Vec3::Y{0, 1, 0}, Vec3::Z{0, 0, 1};

[[noreturn]] inline void panic(const std::string& what) { throw std::runtime_error(what + ": " + pt_last_error()); }

// One replay of the description graph onto a pt_scene; memoises shared nodes (Arc sharing).
struct Volume;
struct Emitter {
    pt_scene* scene;
    std::string asset_dir;
    std::map<const void*, int> done;
    int override_mat = -1;   // >= 0: the primitives emitted now carry this material instead of their own (HomogeneousVolume's boundary)
    const Volume* glass_interior = nullptr;   // the interior of every GlassBSDF without one of its own (World::glass_interior)
    double glass_dispersion = 0.0;            // the Abbe number of every GlassBSDF without one of its own (World::glass_dispersion), 0 = none
    bool instance_motion = false;             // every Instance without keys of its own moves by motion[0..2] and turns by motion[3] radians (World::instance_motion)
    double motion[4] = {0.0, 0.0, 0.0, 0.0};
};

// ---- textures (src/texture.rs) ---------------------------------------------------------
template <class T>
struct Texture {
    virtual ~Texture() = default;
    virtual int emit(Emitter& e) const = 0;
};
template <class T>
using TexPtr = std::shared_ptr<Texture<T>>;

template <class T>
struct SolidTexture;
template <>
struct SolidTexture<Vec3> : Texture<Vec3> {
    Vec3 value;
    static std::shared_ptr<SolidTexture> new_(Vec3 v) { auto t = std::make_shared<SolidTexture>(); t->value = v; return t; }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_tex_solid_rgb(e.scene, value.x, value.y, value.z);
        if (h < 0) panic("SolidTexture");
        return e.done[this] = h;
    }
};
template <>
struct SolidTexture<double> : Texture<double> {
    double value;
    static std::shared_ptr<SolidTexture> new_(double v) { auto t = std::make_shared<SolidTexture>(); t->value = v; return t; }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_tex_solid_f(e.scene, value);
        if (h < 0) panic("SolidTexture");
        return e.done[this] = h;
    }
};
template <class T>
struct CheckerTexture : Texture<T> {
    double scale;
    TexPtr<T> tex1, tex2;
    static std::shared_ptr<CheckerTexture> new_(double scale, TexPtr<T> a, TexPtr<T> b) {
        auto t = std::make_shared<CheckerTexture>();
        t->scale = scale; t->tex1 = a; t->tex2 = b;
        return t;
    }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_tex_checker(e.scene, scale, tex1->emit(e), tex2->emit(e));
        if (h < 0) panic("CheckerTexture");
        return e.done[this] = h;
    }
};
// ImageTexture::new(filename) texture.rs:62-69. Decoding: .hdr, .png and .jpg natively (pt_load_hdr_rgb8, pt_load_png_rgb8, pt_load_jpeg_rgb8);
// anything else must have been handed over decoded (pt_register_image, keyed by the path
// relative to the asset directory; a registered image always wins) or sit next to the file as a "<file>.rgb8" sidecar
// ("PTRGB8 <w> <h>\n" + w*h*3 bytes; tools/prepare_assets.py writes them with Pillow).
struct ImageTexture : Texture<Vec3> {
    std::string filename;
    static std::shared_ptr<ImageTexture> new_(const std::string& f) { auto t = std::make_shared<ImageTexture>(); t->filename = f; return t; }
    int emit(Emitter& e) const override;
};
// not in the reference: the physical sky (pt_tex_sky; include/pt_amd.h has the rule) as an image texture that is baked on the GPU when the
// world is emitted instead of read from a file: Camera::environment = EnvironmentType::Map(Sky::new_(opts)).
struct Sky : ImageTexture {
    pt_sky_opts opts;
    uint32_t width = 2048, height = 1024;
    static pt_sky_opts defaults() { pt_sky_opts o; pt_sky_opts_default(&o); return o; }
    static std::shared_ptr<Sky> new_(const pt_sky_opts& o, uint32_t w = 2048, uint32_t h = 1024) {
        auto t = std::make_shared<Sky>();
        t->opts = o; t->width = w; t->height = h;
        t->filename = "<sky>";
        return t;
    }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_tex_sky(e.scene, &opts, width, height);
        if (h < 0) panic("Sky");
        return e.done[this] = h;
    }
};

// ---- materials (src/bsdf/*.rs, src/material.rs:150-191) ---------------------------------
struct BxDFMaterial {
    virtual ~BxDFMaterial() = default;
    virtual int emit(Emitter& e) const = 0;
};
using MatPtr = std::shared_ptr<BxDFMaterial>;

struct DiffuseBRDF : BxDFMaterial {   // diffuse.rs:21-47
    TexPtr<Vec3> base_color;
    std::shared_ptr<ImageTexture> normal_map;
    static std::shared_ptr<DiffuseBRDF> new_(TexPtr<Vec3> c) { auto m = std::make_shared<DiffuseBRDF>(); m->base_color = c; return m; }
    static std::shared_ptr<DiffuseBRDF> from_rgb(Vec3 c) { return new_(SolidTexture<Vec3>::new_(c)); }
    static std::shared_ptr<DiffuseBRDF> with_normal(Vec3 c, std::shared_ptr<ImageTexture> n) { auto m = from_rgb(c); m->normal_map = n; return m; }
    static std::shared_ptr<DiffuseBRDF> from_textures(TexPtr<Vec3> c, std::shared_ptr<ImageTexture> n) { auto m = new_(c); m->normal_map = n; return m; }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_mat_diffuse(e.scene, base_color->emit(e), normal_map ? normal_map->emit(e) : -1);
        if (h < 0) panic("DiffuseBRDF");
        return e.done[this] = h;
    }
};
struct MetalBRDF : BxDFMaterial {   // metal.rs:23-35
    TexPtr<Vec3> base_color;
    TexPtr<double> roughness;
    static std::shared_ptr<MetalBRDF> new_(TexPtr<Vec3> c, TexPtr<double> r) { auto m = std::make_shared<MetalBRDF>(); m->base_color = c; m->roughness = r; return m; }
    static std::shared_ptr<MetalBRDF> from_rgb(Vec3 c, double r) { return new_(SolidTexture<Vec3>::new_(c), SolidTexture<double>::new_(r)); }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_mat_metal(e.scene, base_color->emit(e), roughness->emit(e));
        if (h < 0) panic("MetalBRDF");
        return e.done[this] = h;
    }
};
struct GlassBSDF : BxDFMaterial {   // glass.rs:28-49
    TexPtr<Vec3> base_color;
    TexPtr<double> roughness;
    double anisotropic = 0, ior = 1.5;
    static std::shared_ptr<GlassBSDF> new_(TexPtr<Vec3> c, TexPtr<double> r, double aniso, double ior) {
        auto m = std::make_shared<GlassBSDF>();
        m->base_color = c; m->roughness = r; m->anisotropic = aniso; m->ior = ior;
        return m;
    }
    static std::shared_ptr<GlassBSDF> basic(double ior) { return new_(SolidTexture<Vec3>::new_(Vec3::ONE), SolidTexture<double>::new_(0.001), 0.0, ior); }
    // this build's addition: the medium that fills objects of this glass (pt_mat_glass_set_interior); the volume's
    // boundary, if it has one, is not used
    std::shared_ptr<Volume> interior;
    std::shared_ptr<GlassBSDF> with_interior(std::shared_ptr<Volume> v) const {
        auto m = std::make_shared<GlassBSDF>(*this);
        m->interior = v;
        return m;
    }
    // this build's addition: spectral dispersion — `ior` is then n_d and `abbe` the Abbe number V_d (pt_mat_glass_set_dispersion); 0 = none
    double abbe = 0.0;
    std::shared_ptr<GlassBSDF> with_dispersion(double v_d) const {
        auto m = std::make_shared<GlassBSDF>(*this);
        m->abbe = v_d;
        return m;
    }
    int emit(Emitter& e) const override;   // (below Volume)
};
struct PrincipledBSDF : BxDFMaterial {   // principled.rs:45-73, same argument order
    TexPtr<Vec3> base_color;
    double p[11];
    static std::shared_ptr<PrincipledBSDF> new_(TexPtr<Vec3> base_color, double metallic, double roughness, double subsurface,
                                                double specular, double specular_tint, double ior, double spec_trans,
                                                double sheen, double sheen_tint, double clearcoat, double clearcoat_gloss) {
        auto m = std::make_shared<PrincipledBSDF>();
        m->base_color = base_color;
        const double v[11] = {metallic, roughness, subsurface, specular, specular_tint, ior, spec_trans, sheen, sheen_tint, clearcoat, clearcoat_gloss};
        std::memcpy(m->p, v, sizeof v);
        return m;
    }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_mat_principled(e.scene, base_color->emit(e), p);
        if (h < 0) panic("PrincipledBSDF");
        return e.done[this] = h;
    }
};
struct DiffuseLight : BxDFMaterial {   // material.rs:155-164
    TexPtr<Vec3> emission;
    static std::shared_ptr<DiffuseLight> new_(TexPtr<Vec3> t) { auto m = std::make_shared<DiffuseLight>(); m->emission = t; return m; }
    static std::shared_ptr<DiffuseLight> from_rgb(Vec3 c) { return new_(SolidTexture<Vec3>::new_(c)); }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_mat_light(e.scene, emission->emit(e));
        if (h < 0) panic("DiffuseLight");
        return e.done[this] = h;
    }
};

struct MixBxDf : BxDFMaterial {   // mix.rs:14-20
    double t;
    MatPtr bxdf1, bxdf2;
    static std::shared_ptr<MixBxDf> new_(double t, MatPtr a, MatPtr b) { auto m = std::make_shared<MixBxDf>(); m->t = t; m->bxdf1 = a; m->bxdf2 = b; return m; }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_mat_mix(e.scene, t, bxdf1->emit(e), bxdf2->emit(e));
        if (h < 0) panic("MixBxDf");
        return e.done[this] = h;
    }
};
struct SheenBRDF : BxDFMaterial {   // sheen.rs:17-22
    Vec3 base_color;
    double sheen_tint;
    static std::shared_ptr<SheenBRDF> new_(Vec3 c, double tint) { auto m = std::make_shared<SheenBRDF>(); m->base_color = c; m->sheen_tint = tint; return m; }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_mat_sheen(e.scene, base_color.x, base_color.y, base_color.z, sheen_tint);
        if (h < 0) panic("SheenBRDF");
        return e.done[this] = h;
    }
};
struct ClearcoatBRDF : BxDFMaterial {   // clearcoat.rs:14-18
    double clearcoat_gloss;
    static std::shared_ptr<ClearcoatBRDF> new_(double gloss) { auto m = std::make_shared<ClearcoatBRDF>(); m->clearcoat_gloss = gloss; return m; }
    int emit(Emitter& e) const override {
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = pt_mat_clearcoat(e.scene, clearcoat_gloss);
        if (h < 0) panic("ClearcoatBRDF");
        return e.done[this] = h;
    }
};

// ---- hittables (src/hittable/*.rs) -------------------------------------------------------
struct Hittable {
    virtual ~Hittable() = default;
    virtual int emit(Emitter& e) const = 0;
    // grows [lo, hi] by the object's world-space bounds (the role of Hittable::bounding_box; pt_render --fog wraps the world in them)
    virtual void bounds(Vec3& lo, Vec3& hi) const = 0;
};
inline void grow_bounds(Vec3& lo, Vec3& hi, Vec3 p) {
    lo = Vec3{std::min(lo.x, p.x), std::min(lo.y, p.y), std::min(lo.z, p.z)};
    hi = Vec3{std::max(hi.x, p.x), std::max(hi.y, p.y), std::max(hi.z, p.z)};
}
using HitPtr = std::shared_ptr<Hittable>;

struct Sphere : Hittable {   // sphere.rs:22-46
    double radius;
    Vec3 position1, position2;
    MatPtr material;
    static std::shared_ptr<Sphere> new_still(double r, Vec3 p, MatPtr m) { return new_moving(r, p, p, m); }
    static std::shared_ptr<Sphere> new_moving(double r, Vec3 p1, Vec3 p2, MatPtr m) {
        auto s = std::make_shared<Sphere>();
        s->radius = r; s->position1 = p1; s->position2 = p2; s->material = m;
        return s;
    }
    int emit(Emitter& e) const override {
        const double a[3] = {position1.x, position1.y, position1.z}, b[3] = {position2.x, position2.y, position2.z};
        int h = pt_sphere(e.scene, radius, a, b, e.override_mat >= 0 ? e.override_mat : material->emit(e));
        if (h < 0) panic("Sphere");
        return h;
    }
    void bounds(Vec3& lo, Vec3& hi) const override {
        for (Vec3 c : {position1, position2}) {
            grow_bounds(lo, hi, Vec3{c.x - radius, c.y - radius, c.z - radius});
            grow_bounds(lo, hi, Vec3{c.x + radius, c.y + radius, c.z + radius});
        }
    }
};
struct Quad : Hittable {   // quad.rs:17-36
    Vec3 q, u, v;
    MatPtr material;
    static std::shared_ptr<Quad> new_(Vec3 q, Vec3 u, Vec3 v, MatPtr m) {
        auto s = std::make_shared<Quad>();
        s->q = q; s->u = u; s->v = v; s->material = m;
        return s;
    }
    int emit(Emitter& e) const override {
        const double a[3] = {q.x, q.y, q.z}, b[3] = {u.x, u.y, u.z}, c[3] = {v.x, v.y, v.z};
        int h = pt_quad(e.scene, a, b, c, e.override_mat >= 0 ? e.override_mat : material->emit(e));
        if (h < 0) panic("Quad");
        return h;
    }
    void bounds(Vec3& lo, Vec3& hi) const override {
        for (int i = 0; i < 4; ++i)
            grow_bounds(lo, hi, Vec3{q.x + (i & 1) * u.x + (i >> 1) * v.x, q.y + (i & 1) * u.y + (i >> 1) * v.y, q.z + (i & 1) * u.z + (i >> 1) * v.z});
    }
};
struct Cuboid : Hittable {   // cuboid.rs:11-58
    Vec3 a, b;
    MatPtr material;
    static std::shared_ptr<Cuboid> new_(Vec3 a, Vec3 b, MatPtr m) {
        auto s = std::make_shared<Cuboid>();
        s->a = a; s->b = b; s->material = m;
        return s;
    }
    int emit(Emitter& e) const override {
        const double p[3] = {a.x, a.y, a.z}, q[3] = {b.x, b.y, b.z};
        int h = pt_cuboid(e.scene, p, q, e.override_mat >= 0 ? e.override_mat : material->emit(e));
        if (h < 0) panic("Cuboid");
        return h;
    }
    void bounds(Vec3& lo, Vec3& hi) const override { grow_bounds(lo, hi, a); grow_bounds(lo, hi, b); }
};
// tobj::Mesh as the reference consumes it (mesh.rs:149-170): f32 attributes, u32 position indices
struct Mesh {
    std::vector<float> positions, normals, texcoords;
    std::vector<uint32_t> indices;
    // not in the reference: mesh tessellation and displacement (include/pt_amd.h has the rule).
    // grid: the (nu x nv)-cell mesh that stands in for Quad::new_(q, u, v, ..) (pt_mesh_grid); tessellated: `opts.levels` subdivisions and
    // the displacement by opts.height on the GPU (pt_mesh_tessellate). Hand either to TriangleMesh::from_obj.
    static Mesh grid(Vec3 q, Vec3 u, Vec3 v, uint32_t nu, uint32_t nv) {
        const double a[3] = {q.x, q.y, q.z}, b[3] = {u.x, u.y, u.z}, c[3] = {v.x, v.y, v.z};
        float *pos, *nrm, *uv;
        uint32_t *idx, np, ni;
        if (pt_mesh_grid(a, b, c, nu, nv, &pos, &np, &idx, &ni, &nrm, &uv) != 0) panic("Mesh::grid");
        return take(pos, np, idx, ni, nrm, uv);
    }
    Mesh tessellated(pt_ctx* ctx, const pt_tess_opts& opts) const {
        float *pos, *nrm, *uv;
        uint32_t *idx, np, ni;
        if (pt_mesh_tessellate(ctx, &opts, (uint32_t)(positions.size() / 3), positions.data(), (uint32_t)indices.size(), indices.data(), (uint32_t)(normals.size() / 3),
                               normals.data(), (uint32_t)(texcoords.size() / 2), texcoords.data(), &pos, &np, &idx, &ni, &nrm, &uv) != 0)
            panic("Mesh::tessellated");
        return take(pos, np, idx, ni, nrm, uv);
    }
    // not in the reference: Loop subdivision on the GPU (pt_mesh_subdivide; include/pt_amd.h has the rule): the cage's
    // positions and texcoords in (its normals are not read), a rounder mesh with smooth normals out. crease: one flag per index, or NULL;
    // out_crease: the flags of the result, for a further call. Hand the result to TriangleMesh::from_obj, or to tessellated() to displace it.
    Mesh subdivided(pt_ctx* ctx, const pt_subdiv_opts& opts, const std::vector<uint8_t>* crease = nullptr, std::vector<uint8_t>* out_crease = nullptr) const {
        float *pos, *nrm, *uv;
        uint32_t *idx, np, ni;
        uint8_t* flags = nullptr;
        if (crease && crease->size() != indices.size()) panic("Mesh::subdivided: one crease flag per index");
        if (pt_mesh_subdivide(ctx, &opts, (uint32_t)(positions.size() / 3), positions.data(), (uint32_t)indices.size(), indices.data(), (uint32_t)(texcoords.size() / 2),
                              texcoords.data(), crease ? crease->data() : nullptr, &pos, &np, &idx, &ni, &nrm, &uv, out_crease ? &flags : nullptr) != 0)
            panic("Mesh::subdivided");
        if (out_crease) out_crease->assign(flags, flags + ni);
        pt_free(flags);
        return take(pos, np, idx, ni, nrm, uv);
    }
    // not in the reference: the level set of a grid of samples as a mesh, on the GPU (pt_mesh_isosurface; include/pt_amd.h has the rule;
    // DESIGN.md section 29). values: nx * ny * nz samples at the cell centres of the box (HeterogeneousVolume::from_grid's layout). Hand the
    // result to TriangleMesh::from_obj, or to subdivided() / tessellated() first.
    static Mesh isosurface(pt_ctx* ctx, const pt_iso_opts& opts, uint32_t nx, uint32_t ny, uint32_t nz, const std::vector<float>& values, Vec3 lo, Vec3 hi) {
        const double a[3] = {lo.x, lo.y, lo.z}, b[3] = {hi.x, hi.y, hi.z};
        float *pos, *nrm;
        uint32_t *idx, np, ni;
        if (values.size() != (size_t)nx * ny * nz) panic("Mesh::isosurface: one value per cell");
        if (pt_mesh_isosurface(ctx, &opts, nx, ny, nz, values.data(), a, b, &pos, &np, &idx, &ni, &nrm) != 0) panic("Mesh::isosurface");
        return take(pos, np, idx, ni, nrm, nullptr);
    }
    // not in the reference: welding and simplification by quadric vertex clustering on the GPU (pt_mesh_simplify; include/pt_amd.h has
    // the rule): positions and texcoords in (normals are not read), a smaller mesh out. out_map: for every input
    // vertex its vertex in the result, or 0xFFFFFFFF. welded(): vertices of equal position become one, nothing else changes.
    Mesh simplified(pt_ctx* ctx, const pt_simplify_opts& opts, std::vector<uint32_t>* out_map = nullptr) const {
        float *pos, *nrm, *uv;
        uint32_t *idx, np, ni, *map = nullptr;
        if (pt_mesh_simplify(ctx, &opts, (uint32_t)(positions.size() / 3), positions.data(), (uint32_t)indices.size(), indices.data(), (uint32_t)(texcoords.size() / 2),
                             texcoords.data(), &pos, &np, &idx, &ni, &nrm, &uv, out_map ? &map : nullptr) != 0)
            panic("Mesh::simplified");
        if (out_map) out_map->assign(map, map + positions.size() / 3);
        pt_free(map);
        return take(pos, np, idx, ni, nrm, uv);
    }
    Mesh welded(pt_ctx* ctx) const {
        pt_simplify_opts o;
        pt_simplify_opts_default(&o);
        o.mode = 0;
        o.normals = normals.empty() ? 1 : 0;
        return simplified(ctx, o);
    }

private:
    static Mesh take(float* pos, uint32_t np, uint32_t* idx, uint32_t ni, float* nrm, float* uv) {
        Mesh m;
        m.positions.assign(pos, pos + 3 * (size_t)np);
        m.indices.assign(idx, idx + ni);
        if (nrm) m.normals.assign(nrm, nrm + 3 * (size_t)np);
        if (uv) m.texcoords.assign(uv, uv + 2 * (size_t)np);
        pt_free(pos); pt_free(idx); pt_free(nrm); pt_free(uv);
        return m;
    }
};
// not in the reference: a mesh sampled into a 3-D grid on the GPU (pt_mesh_sdf; include/pt_amd.h has the rule): the
// signed distance (positive inside), the distance, the occupancy or a density ramp at the cell centres of a box, in the layout
// HeterogeneousVolume::from_grid and Mesh::isosurface read. fit: cubic cells around the mesh (pt_mesh_fit_grid).
struct Grid {
    uint32_t nx = 0, ny = 0, nz = 0;
    Vec3 lo, hi;
    std::vector<float> values;
    double cell() const { return (hi.x - lo.x) / (double)nx; }   // (of a fitted grid: its cells are cubes)
    static Grid fit(const Mesh& mesh, uint32_t n_longest, double margin_cells) {
        Grid g;
        uint32_t n[3];
        double a[3], b[3];
        if (pt_mesh_fit_grid((uint32_t)(mesh.positions.size() / 3), mesh.positions.data(), n_longest, margin_cells, n, a, b) != 0) panic("Grid::fit");
        g.nx = n[0]; g.ny = n[1]; g.nz = n[2];
        g.lo = Vec3{a[0], a[1], a[2]}; g.hi = Vec3{b[0], b[1], b[2]};
        return g;
    }
    // the samples of `mesh` at the cells of `shape` (its dimensions and box; its values are not read)
    static Grid from_mesh(pt_ctx* ctx, const pt_sdf_opts& opts, const Mesh& mesh, const Grid& shape) {
        Grid g = shape;
        const double a[3] = {g.lo.x, g.lo.y, g.lo.z}, b[3] = {g.hi.x, g.hi.y, g.hi.z};
        g.values.assign((size_t)g.nx * g.ny * g.nz, 0.0f);
        if (pt_mesh_sdf(ctx, &opts, (uint32_t)(mesh.positions.size() / 3), mesh.positions.data(), (uint32_t)mesh.indices.size(), mesh.indices.data(), g.nx, g.ny, g.nz, a, b,
                        g.values.data()) != 0)
            panic("Grid::from_mesh");
        return g;
    }
};
namespace tobj {
struct Model { Mesh mesh; };
// tobj::load_obj(path, &OFFLINE_RENDERING_LOAD_OPTIONS).unwrap() — main.rs:408
inline std::vector<Model> load_obj(const std::string& path) {
    float *pos, *uv;
    uint32_t *idx, np, ni, nuv;
    if (pt_load_obj(path.c_str(), &pos, &np, &idx, &ni, &uv, &nuv) != 0) panic("tobj::load_obj");
    std::vector<Model> models(1);
    models[0].mesh.positions.assign(pos, pos + 3 * (size_t)np);
    models[0].mesh.indices.assign(idx, idx + ni);
    models[0].mesh.texcoords.assign(uv, uv + 2 * (size_t)nuv);
    pt_free(pos); pt_free(idx); pt_free(uv);
    return models;
}
}  // namespace tobj
struct TriangleMesh : Hittable {   // mesh.rs:149-197
    double scale;
    Mesh mesh;
    MatPtr material;
    static std::shared_ptr<TriangleMesh> from_obj(double scale, const Mesh& mesh, MatPtr m) {
        auto s = std::make_shared<TriangleMesh>();
        s->scale = scale; s->mesh = mesh; s->material = m;
        return s;
    }
    int emit(Emitter& e) const override {
        int h = pt_mesh(e.scene, scale, (uint32_t)(mesh.positions.size() / 3), mesh.positions.data(), (uint32_t)mesh.indices.size(),
                        mesh.indices.data(), (uint32_t)(mesh.normals.size() / 3), mesh.normals.data(),
                        (uint32_t)(mesh.texcoords.size() / 2), mesh.texcoords.data(), e.override_mat >= 0 ? e.override_mat : material->emit(e));
        if (h < 0) panic("TriangleMesh");
        return h;
    }
    void bounds(Vec3& lo, Vec3& hi) const override {
        for (size_t i = 0; i + 2 < mesh.positions.size(); i += 3)
            grow_bounds(lo, hi, Vec3{mesh.positions[i] * scale, mesh.positions[i + 1] * scale, mesh.positions[i + 2] * scale});
    }
};
struct Instance : Hittable {   // instance.rs:20-30 — rotate, then translate
    HitPtr object;
    Vec3 axis, translation;
    double angle;
    // this build's addition (pt_instance_moving): a second key — the pose goes from (angle, translation) at time 0 to (angle1, translation1) at time 1
    bool moving = false;
    Vec3 translation1;
    double angle1 = 0.0;
    static std::shared_ptr<Instance> new_(HitPtr obj, Vec3 axis, double angle, Vec3 translation) {
        auto s = std::make_shared<Instance>();
        s->object = obj; s->axis = axis; s->angle = angle; s->translation = translation;
        return s;
    }
    static std::shared_ptr<Instance> new_moving(HitPtr obj, Vec3 axis, double angle0, double angle1, Vec3 tr0, Vec3 tr1) {
        auto s = new_(obj, axis, angle0, tr0);
        s->moving = true; s->angle1 = angle1; s->translation1 = tr1;
        return s;
    }
    int emit(Emitter& e) const override {
        const double a[3] = {axis.x, axis.y, axis.z}, t[3] = {translation.x, translation.y, translation.z};
        int h;
        if (moving) {
            const double t1[3] = {translation1.x, translation1.y, translation1.z};
            h = pt_instance_moving(e.scene, object->emit(e), a, angle, angle1, t, t1);
        } else if (e.instance_motion) {   // World::instance_motion: tr1 = tr0 + D, angle1 = angle0 + the turn
            const double t1[3] = {translation.x + e.motion[0], translation.y + e.motion[1], translation.z + e.motion[2]};
            h = pt_instance_moving(e.scene, object->emit(e), a, angle, angle + e.motion[3], t, t1);
        } else {
            h = pt_instance(e.scene, object->emit(e), a, angle, t);
        }
        if (h < 0) panic("Instance");
        return h;
    }
    void bounds(Vec3& lo, Vec3& hi) const override {   // the box of the wrapped object's box, rotated (Rodrigues) and translated
        const double inf = std::numeric_limits<double>::infinity();
        Vec3 l{inf, inf, inf}, h{-inf, -inf, -inf};
        object->bounds(l, h);
        const double c = std::cos(angle), s = std::sin(angle);
        for (int i = 0; i < 8; ++i) {
            const Vec3 p{(i & 1) ? h.x : l.x, (i & 2) ? h.y : l.y, (i & 4) ? h.z : l.z};
            const double d = axis.x * p.x + axis.y * p.y + axis.z * p.z;
            const Vec3 x{axis.y * p.z - axis.z * p.y, axis.z * p.x - axis.x * p.z, axis.x * p.y - axis.y * p.x};
            grow_bounds(lo, hi, Vec3{p.x * c + x.x * s + axis.x * d * (1.0 - c) + translation.x, p.y * c + x.y * s + axis.y * d * (1.0 - c) + translation.y,
                                     p.z * c + x.z * s + axis.z * d * (1.0 - c) + translation.z});
        }
    }
};
// A participating medium and the closed object that bounds it. The boundary's own material is replaced by the medium: it is invisible.
// A volume without a boundary serves as World::camera_medium alone — an unbounded medium.
struct Volume : Hittable {
    HitPtr boundary;
    virtual int create(Emitter& e) const = 0;   // the medium's material (pt_mat_medium / pt_mat_medium_grid), or -1
    virtual const char* name() const = 0;
    int medium(Emitter& e) const {   // the medium's material handle
        auto it = e.done.find(this);
        if (it != e.done.end()) return it->second;
        int h = create(e);
        if (h < 0) panic(name());
        return e.done[this] = h;
    }
    int emit(Emitter& e) const override {
        if (!boundary) panic(std::string(name()) + " without a boundary in the world");
        const int saved = e.override_mat;
        e.override_mat = medium(e);
        const int h = boundary->emit(e);
        e.override_mat = saved;
        return h;
    }
    void bounds(Vec3& lo, Vec3& hi) const override { if (boundary) boundary->bounds(lo, hi); }
};
inline int GlassBSDF::emit(Emitter& e) const {
    auto it = e.done.find(this);
    if (it != e.done.end()) return it->second;
    int h = pt_mat_glass(e.scene, base_color->emit(e), roughness->emit(e), anisotropic, ior);
    if (h < 0) panic("GlassBSDF");
    const Volume* v = interior ? interior.get() : e.glass_interior;
    if (v && pt_mat_glass_set_interior(e.scene, h, v->medium(e)) != 0) panic("GlassBSDF::interior");
    const double v_d = abbe != 0.0 ? abbe : e.glass_dispersion;
    if (v_d != 0.0 && pt_mat_glass_set_dispersion(e.scene, h, v_d) != 0) panic("GlassBSDF::dispersion");
    return e.done[this] = h;
}
// HomogeneousVolume of the reference's commented-out volume.rs:15-41: a boundary filled with a medium of constant density and
// albedo. `g` (Henyey-Greenstein) is this build's addition; 0 is the isotropic phase function the stub names (pt_mat_medium).
struct HomogeneousVolume : Volume {
    double density = 1.0, g = 0.0;
    Vec3 albedo;
    static std::shared_ptr<HomogeneousVolume> from_albedo(HitPtr boundary, double density, Vec3 albedo, double g = 0.0) {
        auto v = std::make_shared<HomogeneousVolume>();
        v->boundary = boundary; v->density = density; v->albedo = albedo; v->g = g;
        return v;
    }
    // this build's addition: an absorption coefficient per channel on top of the scattering; density may then be 0 (pt_mat_medium_tinted)
    bool is_tinted = false;
    Vec3 absorption;
    static std::shared_ptr<HomogeneousVolume> tinted(HitPtr boundary, double density, Vec3 albedo, double g, Vec3 absorption) {
        auto v = from_albedo(boundary, density, albedo, g);
        v->is_tinted = true; v->absorption = absorption;
        return v;
    }
    int create(Emitter& e) const override {
        const double a[3] = {absorption.x, absorption.y, absorption.z};
        return is_tinted ? pt_mat_medium_tinted(e.scene, density, albedo.x, albedo.y, albedo.z, g, a) : pt_mat_medium(e.scene, density, albedo.x, albedo.y, albedo.z, g);
    }
    const char* name() const override { return "HomogeneousVolume"; }
};
// No counterpart in the reference: a medium whose density is scale * V(x), V trilinear in an nx x ny x nz grid of samples at the cell
// centres of the world-space box [box_lo, box_hi] (values[(k * ny + j) * nx + i]; pt_mat_medium_grid). The grid is fixed
// in world space whatever carries the medium.
struct HeterogeneousVolume : Volume {
    double scale = 1.0, g = 0.0;
    Vec3 albedo, box_lo, box_hi;
    uint32_t nx = 0, ny = 0, nz = 0;
    std::vector<float> values;
    static std::shared_ptr<HeterogeneousVolume> from_grid(HitPtr boundary, double scale, Vec3 albedo, double g, uint32_t nx, uint32_t ny, uint32_t nz,
                                                          std::vector<float> values, Vec3 box_lo, Vec3 box_hi) {
        auto v = std::make_shared<HeterogeneousVolume>();
        v->boundary = boundary; v->scale = scale; v->albedo = albedo; v->g = g;
        v->nx = nx; v->ny = ny; v->nz = nz; v->values = std::move(values); v->box_lo = box_lo; v->box_hi = box_hi;
        return v;
    }
    int create(Emitter& e) const override {
        if (values.size() != (size_t)nx * ny * nz) return pt_set_error_message("HeterogeneousVolume: values must hold nx * ny * nz samples");
        const double lo[3] = {box_lo.x, box_lo.y, box_lo.z}, hi[3] = {box_hi.x, box_hi.y, box_hi.z};
        return pt_mat_medium_grid(e.scene, scale, albedo.x, albedo.y, albedo.z, g, nx, ny, nz, values.data(), lo, hi);
    }
    const char* name() const override { return "HeterogeneousVolume"; }
};

// ---- punctual lights (the reference's unfinished hittable/light.rs PointLight, finished, and two siblings; pt_light_point / pt_light_spot /
// pt_light_directional). They have no geometry: World::add_punctual keeps them in a list of their own.
struct PunctualLight {
    virtual ~PunctualLight() = default;
    virtual int emit(pt_scene* s) const = 0;   // the light's index, or -1
};
struct PointLight : PunctualLight {   // light.rs: PointLight { position, power }
    Vec3 position, power;
    static std::shared_ptr<PointLight> new_(Vec3 position, Vec3 power) {
        auto l = std::make_shared<PointLight>();
        l->position = position; l->power = power;
        return l;
    }
    int emit(pt_scene* s) const override {
        const double p[3] = {position.x, position.y, position.z}, w[3] = {power.x, power.y, power.z};
        return pt_light_point(s, p, w);
    }
};
struct SpotLight : PunctualLight {
    Vec3 position, target, intensity;
    double inner_deg = 0.0, outer_deg = 0.0;
    static std::shared_ptr<SpotLight> new_(Vec3 position, Vec3 target, double inner_deg, double outer_deg, Vec3 intensity) {
        auto l = std::make_shared<SpotLight>();
        l->position = position; l->target = target; l->inner_deg = inner_deg; l->outer_deg = outer_deg; l->intensity = intensity;
        return l;
    }
    int emit(pt_scene* s) const override {
        const double p[3] = {position.x, position.y, position.z}, t[3] = {target.x, target.y, target.z}, i[3] = {intensity.x, intensity.y, intensity.z};
        return pt_light_spot(s, p, t, inner_deg, outer_deg, i);
    }
};
struct DirectionalLight : PunctualLight {
    Vec3 direction, irradiance;
    static std::shared_ptr<DirectionalLight> new_(Vec3 direction, Vec3 irradiance) {
        auto l = std::make_shared<DirectionalLight>();
        l->direction = direction; l->irradiance = irradiance;
        return l;
    }
    int emit(pt_scene* s) const override {
        const double d[3] = {direction.x, direction.y, direction.z}, e[3] = {irradiance.x, irradiance.y, irradiance.z};
        return pt_light_directional(s, d, e);
    }
};

// ---- World (src/hittable/world.rs:10-29) -------------------------------------------------
struct World {
    std::vector<HitPtr> objects, lights;
    std::vector<std::shared_ptr<PunctualLight>> punctual;   // this build's addition: the punctual lights (add_punctual)
    double punctual_fraction = 0.5;                         // ... and the selector's share of their branch (pt_scene_set_punctual_fraction)
    bool punctual_media = false;                            // ... and whether they light participating media (pt_scene_set_punctual_media: light shafts)
    int punctual_selection = 0;                             // ... how their branch picks its light: 0 uniformly, 1 the light grid (pt_scene_set_punctual_selection)
    uint32_t punctual_grid[3] = {0u, 0u, 0u};               // ... and the grid's dims, 0 0 0 = automatic, over the world's bounds (pt_scene_set_punctual_grid)
    template <class T> void add_punctual(std::shared_ptr<T> l) { punctual.push_back(l); }
    pt_scene* scene = nullptr;   // set by build_bvh / emit_into
    bool owns_scene = false;
    std::map<const void*, int> handles;   // description -> C-ABI handle (for Camera's env map)
    std::string asset_dir = "assets";
    static World new_() { return World(); }
    template <class T> void add_object(std::shared_ptr<T> o) { objects.push_back(o); }
    template <class T> void add_light(std::shared_ptr<T> o) { lights.push_back(o); }
    // flatten + BVH + upload into an existing scene
    void emit_into(pt_scene* s, std::shared_ptr<ImageTexture> env = nullptr) {
        Emitter e{s, asset_dir, {}};
        e.glass_interior = glass_interior.get();
        e.glass_dispersion = glass_dispersion;
        e.instance_motion = instance_motion;
        for (int i = 0; i < 4; ++i) e.motion[i] = motion[i];
        for (auto& o : objects) if (pt_world_add_object(s, o->emit(e)) != 0) panic("World::add_object");
        for (auto& l : lights) if (pt_world_add_light(s, l->emit(e)) != 0) panic("World::add_light");
        if (env) env->emit(e);
        for (auto& l : punctual) if (l->emit(s) < 0) panic("World::add_punctual");
        if (punctual_fraction != 0.5 && pt_scene_set_punctual_fraction(s, punctual_fraction) != 0) panic("set_punctual_fraction");
        if (punctual_media && pt_scene_set_punctual_media(s, 1) != 0) panic("set_punctual_media");
        if (punctual_selection != 0 && pt_scene_set_punctual_selection(s, punctual_selection) != 0) panic("set_punctual_selection");
        if (punctual_grid[0] != 0u && pt_scene_set_punctual_grid(s, punctual_grid[0], punctual_grid[1], punctual_grid[2], nullptr) != 0) panic("set_punctual_grid");
        if (camera_medium && pt_scene_set_camera_medium(s, camera_medium->medium(e)) != 0) panic("World::camera_medium");
        if (pt_world_build(s) != 0) panic("World::build_bvh");
        scene = s;
        handles = e.done;
    }
    std::shared_ptr<Volume> camera_medium;   // the medium camera rays start in (pt_scene_set_camera_medium); null = none
    std::shared_ptr<Volume> glass_interior;   // this build's option: the interior of every GlassBSDF that has none of its own (pt_render --interior)
    double glass_dispersion = 0.0;            // this build's option: the Abbe number of every GlassBSDF that has none of its own (pt_render --dispersion), 0 = none
    void bounds(Vec3& lo, Vec3& hi) const {             // of objects and lights
        for (auto& o : objects) o->bounds(lo, hi);
        for (auto& l : lights) l->bounds(lo, hi);
    }
    bool float_hdr = false;   // this build's option: Radiance .hdr images keep their f32 samples (no .to_rgb8(), texture.rs:67)
    int sampler = 0;             // this build's option: 0 independent draws (the reference's), 1 Owen-scrambled Sobol (pt_scene_set_sampler)
    double env_sampling = 0.0;   // this build's option: environment importance sampling weight (pt_scene_set_env_sampling; 0 = off)
    int light_sampling = 0;      // this build's option: 0 the reference's lights.sample / lights.pdf, 1 exact (pt_scene_set_light_sampling)
    int projection = 0;          // this build's option: 0 perspective (the reference's camera), 1 orthographic, 2 fisheye, 3 panorama (pt_scene_set_projection)
    // this build's options (motion blur of instances): the camera shutter (pt_scene_set_shutter), and a second key applied to every Instance a
    // scene script makes: tr1 = tr0 + motion[0..2], angle1 = angle0 + motion[3] radians (pt_render --motion)
    double shutter[2] = {0.0, 1.0};
    // this build's option: meshes of at least this many triangles get the GPU's LBVH builder (pt_world_set_device_bvh_threshold; 0 = always the
    // host's binned-SAH builder, -1 = the library's default)
    long long device_bvh_threshold = -1;
    bool instance_motion = false;
    double motion[4] = {0.0, 0.0, 0.0, 0.0};
    void build_bvh(pt_ctx* ctx, std::shared_ptr<ImageTexture> env = nullptr) {
        pt_scene* s = pt_scene_create(ctx);
        if (!s) panic("pt_scene_create");
        owns_scene = true;
        if (float_hdr) pt_scene_set_float_hdr(s, 1);
        if (env_sampling != 0.0 && pt_scene_set_env_sampling(s, env_sampling) != 0) panic("set_env_sampling");
        if (sampler != 0 && pt_scene_set_sampler(s, sampler) != 0) panic("set_sampler");
        if (light_sampling != 0 && pt_scene_set_light_sampling(s, light_sampling) != 0) panic("set_light_sampling");
        if (projection != 0 && pt_scene_set_projection(s, projection) != 0) panic("set_projection");
        if ((shutter[0] != 0.0 || shutter[1] != 1.0) && pt_scene_set_shutter(s, shutter[0], shutter[1]) != 0) panic("set_shutter");
        if (device_bvh_threshold >= 0 && pt_world_set_device_bvh_threshold(s, (uint32_t)device_bvh_threshold) != 0) panic("set_device_bvh_threshold");
        emit_into(s, env);
    }
    void release() {
        if (owns_scene && scene) pt_scene_destroy(scene);
        scene = nullptr;
        owns_scene = false;
    }
};

// ---- Camera (src/camera.rs:15-77) --------------------------------------------------------
struct EnvironmentType {
    bool is_map = false;
    Vec3 color;
    std::shared_ptr<ImageTexture> map;
    static EnvironmentType Color(Vec3 c) { EnvironmentType e; e.color = c; return e; }
    static EnvironmentType Map(std::shared_ptr<ImageTexture> t) { EnvironmentType e; e.is_map = true; e.map = t; return e; }
};
// not in the reference: the film stage between the accumulator and the files (pt_film_develop; include/pt_amd.h has the rule). The default
// is the reference's mean / sqrt gamma / quantise (camera.rs:109-130), so a default Film writes the PNG bytes written before it existed.
struct Film {
    double exposure_ev = 0.0;
    uint32_t tonemap = 0;   // 0 reference (sqrt), 1 srgb, 2 reinhard, 3 aces
    double white = 4.0, bloom_strength = 0.0, bloom_threshold = 1.0, bloom_sigma = 2.0;
    uint32_t bloom_levels = 5;
    std::string hdr_filename;   // if set: the scene-linear image (after exposure and glare), narrowed to f32, as .pfm or (any other extension) Radiance .hdr
    pt_film_opts to_c() const {
        pt_film_opts o;
        std::memset(&o, 0, sizeof o);
        o.exposure_ev = exposure_ev; o.tonemap = tonemap; o.white = white;
        o.bloom_strength = bloom_strength; o.bloom_threshold = bloom_threshold; o.bloom_sigma = bloom_sigma; o.bloom_levels = bloom_levels;
        return o;
    }
};
struct Camera {
    double aspect_ratio = 0;
    size_t image_width = 0, samples_per_pixel = 0, max_depth = 0;
    double vfov = 0;
    Vec3 look_from, look_at, vup;
    double blur_strength = 0, focal_length = 0, defocus_angle = 0;
    EnvironmentType environment = EnvironmentType::Color(Vec3::ZERO);
    size_t image_height = 0;
    double derived[18] = {0};   // forward,right,up,pixel00,pixel_du,pixel_dv
    Film film;                  // not in the reference (after its fields, so that aggregate initialisation in its order still holds)
    static Camera new_() { return Camera(); }

    pt_camera to_c(const World* world) const {
        pt_camera c;
        std::memset(&c, 0, sizeof c);
        c.aspect_ratio = aspect_ratio;
        c.image_width = (uint32_t)image_width;
        c.samples_per_pixel = (uint32_t)samples_per_pixel;
        c.max_depth = (uint32_t)max_depth;
        c.vfov = vfov;
        const Vec3 v[3] = {look_from, look_at, vup};
        double* d[3] = {c.look_from, c.look_at, c.vup};
        for (int i = 0; i < 3; ++i) { d[i][0] = v[i].x; d[i][1] = v[i].y; d[i][2] = v[i].z; }
        c.blur_strength = blur_strength;
        c.focal_length = focal_length;
        c.defocus_angle = defocus_angle;
        c.env_color[0] = environment.color.x; c.env_color[1] = environment.color.y; c.env_color[2] = environment.color.z;
        c.env_tex = -1;
        if (environment.is_map) {
            c.env_is_map = 1;
            if (world) {
                auto it = world->handles.find(environment.map.get());
                if (it == world->handles.end()) throw std::runtime_error("Camera: environment map was not emitted with the world");
                c.env_tex = it->second;
            }
        }
        return c;
    }
    void init() {   // camera.rs:51-77
        pt_camera c = to_c(nullptr);
        uint32_t h = 0;
        if (pt_camera_init(&c, derived, &h) != 0) panic("Camera::init");
        image_height = h;
    }
    // camera.rs:109-130 generalised: sums (of total_spp samples, or of counts[p] each) through the film stage into the PNG and, if asked
    // for, the float file
    void develop(World& world, const std::string& filename, const std::vector<double>& sums, uint32_t total_spp, const uint32_t* counts, const char* who) const {
        const size_t n = image_width * image_height;
        const pt_film_opts fo = film.to_c();
        std::vector<uint8_t> rgb(n * 3);
        std::vector<double> hdr(film.hdr_filename.empty() ? 0 : n * 3);
        if (pt_film_develop(pt_scene_ctx(world.scene), (uint32_t)image_width, (uint32_t)image_height, sums.data(), total_spp, counts, &fo,
                            hdr.empty() ? nullptr : hdr.data(), rgb.data()) != 0)
            panic(std::string(who) + ": " + pt_last_error());
        if (pt_save_png(filename.c_str(), (uint32_t)image_width, (uint32_t)image_height, rgb.data()) != 0)
            std::fprintf(stderr, "Failed to save image %s\n", pt_last_error());
        if (!hdr.empty()) {
            const std::vector<float> f(hdr.begin(), hdr.end());
            const std::string& name = film.hdr_filename;
            const bool pfm = name.size() >= 4 && name.compare(name.size() - 4, 4, ".pfm") == 0;
            if ((pfm ? pt_save_pfm : pt_save_hdr)(name.c_str(), (uint32_t)image_width, (uint32_t)image_height, f.data()) != 0)
                std::fprintf(stderr, "Failed to save image %s\n", pt_last_error());
        }
    }
    // camera.rs:79-126: render, gamma, quantise, save PNG, print the wall-clock seconds
    bool print_stats = false;   // this build's option (pt_render --stats): render() times every launch and prints the render's statistics as one JSON line
    void render(World& world, const std::string& filename, uint64_t seed = 1, pt_render_stats* stats_out = nullptr) const {
        auto start = std::chrono::steady_clock::now();
        pt_camera c = to_c(&world);
        const size_t n = image_width * image_height;
        std::vector<double> accum(n * 3, 0.0);
        pt_render_stats st;
        pt_render_opts ro;
        std::memset(&ro, 0, sizeof ro);
        ro.profile = 1u;   // (print_stats: every launch is timed, so K2's and K3's milliseconds are known)
        if (pt_render(world.scene, &c, seed, 0, (uint32_t)samples_per_pixel, accum.data(), print_stats ? &ro : nullptr, &st) != 0) panic("Camera::render");
        develop(world, filename, accum, (uint32_t)samples_per_pixel, nullptr, "Camera::render");
        double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        std::fprintf(stderr, "[camera.rs:125] start.elapsed().as_secs_f64() = %.6f (render kernel time %.3f s, %.2f Msamples/s)\n", secs,
                     st.ms_total * 1e-3, (double)st.samples / (st.ms_total * 1e-3) * 1e-6);
        if (print_stats)
            std::printf("{\"samples\": %llu, \"segments\": %llu, \"ms_total\": %.4f, \"ms_extend\": %.4f, \"ms_shade\": %.4f, \"launches_extend\": %llu, \"launches_shade\": %llu, "
                        "\"extend_variant\": %u, \"shade_variant\": %u, \"motion\": %d}\n",
                        (unsigned long long)st.samples, (unsigned long long)st.segments, st.ms_total, st.ms_extend, st.ms_shade, (unsigned long long)st.launches_extend,
                        (unsigned long long)st.launches_shade, st.extend_variant, st.shade_variant, pt_scene_motion(world.scene));
        if (stats_out) *stats_out = st;
    }
    // not in the reference: render to a noise target (pt_render_adaptive) with samples_per_pixel as the cap; each pixel is
    // resolved with its own sample count (pt_resolve_u8_counts); prints the mean samples per pixel
    void render_adaptive(World& world, const std::string& filename, double threshold, uint32_t min_spp, uint64_t seed = 1) const {
        auto start = std::chrono::steady_clock::now();
        pt_camera c = to_c(&world);
        const size_t n = image_width * image_height;
        std::vector<double> accum(n * 3, 0.0);
        std::vector<uint32_t> counts(n, 0);
        pt_adaptive_opts ao;
        std::memset(&ao, 0, sizeof ao);
        ao.min_spp = min_spp;
        ao.max_spp = (uint32_t)samples_per_pixel;
        ao.threshold = threshold;
        pt_render_stats st;
        if (pt_render_adaptive(world.scene, &c, seed, &ao, accum.data(), counts.data(), &st) != 0) panic(std::string("Camera::render_adaptive: ") + pt_last_error());
        develop(world, filename, accum, 0, counts.data(), "Camera::render_adaptive");
        double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        std::fprintf(stderr, "adaptive: threshold %g, min spp %u, max spp %u: mean spp %.2f (%llu samples) in %.6f s\n", threshold, min_spp,
                     (uint32_t)samples_per_pixel, (double)st.samples / (double)n, (unsigned long long)st.samples, secs);
    }
    // not in the reference: render samples [0, s/2) and [s/2, s) into two sums, the first-hit AOVs over [0, min(aov_spp, s)),
    // denoise (pt_denoise, default options) and save the denoised means; needs samples_per_pixel >= 2
    void render_denoised(World& world, const std::string& filename, uint32_t aov_spp, uint64_t seed = 1) const {
        auto start = std::chrono::steady_clock::now();
        pt_camera c = to_c(&world);
        const size_t n = image_width * image_height;
        const uint32_t s = (uint32_t)samples_per_pixel, half = s / 2, n_aov = std::min(aov_spp, s);
        std::vector<double> sum_a(n * 3, 0.0), sum_b(n * 3, 0.0), aov(n * 8, 0.0), out(n * 3);
        pt_render_stats sa, sb;
        if (pt_render(world.scene, &c, seed, 0, half, sum_a.data(), nullptr, &sa) != 0 ||
            pt_render(world.scene, &c, seed, half, s, sum_b.data(), nullptr, &sb) != 0)
            panic(std::string("Camera::render_denoised: ") + pt_last_error());
        if (pt_render_aovs(world.scene, &c, seed, 0, n_aov, aov.data(), nullptr) != 0) panic(std::string("Camera::render_denoised: ") + pt_last_error());
        pt_ctx* ctx = pt_scene_ctx(world.scene);
        if (pt_denoise(ctx, (uint32_t)image_width, (uint32_t)image_height, sum_a.data(), half, sum_b.data(), s - half, aov.data(), n_aov, nullptr,
                       out.data()) != 0)
            panic(std::string("Camera::render_denoised: ") + pt_last_error());
        develop(world, filename, out, 1, nullptr, "Camera::render_denoised");   // out holds means: n = 1
        double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        std::fprintf(stderr, "denoise: %u spp as %u + %u, aov %u spp: %.6f s (render kernel time %.3f s)\n", s, half, s - half, n_aov, secs,
                     (sa.ms_total + sb.ms_total) * 1e-3);
    }
};

inline int ImageTexture::emit(Emitter& e) const {
    auto it = e.done.find(this);
    if (it != e.done.end()) return it->second;
    // key relative to the asset dir ("assets/bricks/color.png" -> "bricks/color.png")
    std::string key = filename;
    const std::string prefix = "assets/";
    if (key.compare(0, prefix.size(), prefix) == 0) key = key.substr(prefix.size());
    int h = pt_find_registered_image(e.scene, key.c_str());
    if (h >= 0) return e.done[this] = h;
    const std::string path = e.asset_dir + "/" + key;
    uint8_t* rgb = nullptr;
    uint32_t w = 0, hh = 0;
    if (key.size() > 4 && key.substr(key.size() - 4) == ".hdr" && pt_scene_float_hdr(e.scene)) {   // the float-HDR option: no to_rgb8()
        float* rgbf = nullptr;
        if (pt_load_hdr_rgbf32(path.c_str(), &rgbf, &w, &hh) != 0) panic("ImageTexture::new(" + filename + ")");
        h = pt_tex_image_rgbf32(e.scene, w, hh, rgbf);
        pt_free(rgbf);
    } else if (key.size() > 4 && key.substr(key.size() - 4) == ".hdr") {
        if (pt_load_hdr_rgb8(path.c_str(), &rgb, &w, &hh) != 0) panic("ImageTexture::new(" + filename + ")");
        h = pt_tex_image_rgb8(e.scene, w, hh, rgb);
        pt_free(rgb);
    } else if (key.size() > 4 && key.substr(key.size() - 4) == ".png") {
        if (pt_load_png_rgb8(path.c_str(), &rgb, &w, &hh) != 0) panic("ImageTexture::new(" + filename + ")");
        h = pt_tex_image_rgb8(e.scene, w, hh, rgb);
        pt_free(rgb);
    } else if ((key.size() > 4 && key.substr(key.size() - 4) == ".jpg") || (key.size() > 5 && key.substr(key.size() - 5) == ".jpeg")) {
        if (pt_load_jpeg_rgb8(path.c_str(), &rgb, &w, &hh) != 0) panic("ImageTexture::new(" + filename + ")");
        h = pt_tex_image_rgb8(e.scene, w, hh, rgb);
        pt_free(rgb);
    } else {
        std::ifstream in(path + ".rgb8", std::ios::binary);
        std::string magic;
        if (!in || !(in >> magic >> w >> hh) || magic != "PTRGB8")
            throw std::runtime_error("ImageTexture::new(" + filename + "): no decoder for this format in the host library; run tools/prepare_assets.py "
                                     "(writes " + path + ".rgb8) or hand the decoded pixels over with pt_register_image");
        in.get();
        std::vector<uint8_t> px((size_t)w * hh * 3);
        in.read((char*)px.data(), (std::streamsize)px.size());
        if (!in) throw std::runtime_error("ImageTexture::new(" + filename + "): truncated sidecar");
        h = pt_tex_image_rgb8(e.scene, w, hh, px.data());
    }
    if (h < 0) panic("ImageTexture::new");
    return e.done[this] = h;
}

}  // namespace path_tracer
