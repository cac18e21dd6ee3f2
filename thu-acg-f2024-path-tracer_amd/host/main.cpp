// CLI with the reference's two flags (src/main.rs:620-645): -q/--quality toggles
// 1920 px @ 4000 spp vs 600 px @ 100 spp, -s/--scene N picks the scene script. Extra,
// explicit overrides (not in the reference): --width, --spp, --seed, --out, --assets, --device, --float-hdr
// (.hdr environments keep their f32 samples instead of the reference's .to_rgb8() squash, texture.rs:67),
// --adaptive T [--min-spp M] (adaptive sampling to the noise target T, pt_render_adaptive; --spp is then the cap),
// --denoise [--aov-spp N] (two half-frames + first-hit AOVs over min(N, spp) samples through pt_denoise; N defaults to 16),
// --fog DENSITY[,R,G,B[,G]] (the built world's bounds, grown by 1 %, become the boundary of a homogeneous medium of that density,
// albedo (default 1,1,1) and Henyey-Greenstein g (default 0); the camera starts inside it when look_from lies inside),
// --smoke SCALE[,R,G,B[,G]] (a fixed closed-form plume, smoke_plume below, sampled into a 64^3 grid over the box --fog would build, as an
// unbounded grid-density camera medium of extinction SCALE * V),
// --isosurface ISO[,GRID_N] (the same plume sampled into GRID_N^3 cells over the same box and meshed on the GPU where it crosses ISO:
// pt_mesh_isosurface),
// --mesh-smoke SCALE[,GRID_N[,RAMP_CELLS]] (scene 6: spot, sampled on the GPU into a density grid of its shape, replaces its surface as an
// unbounded camera medium: pt_mesh_sdf), --remesh OFFSET[,GRID_N] (scene 6: spot and cow go through a signed distance grid and
// come back as the level set OFFSET * E outside their surface: pt_mesh_sdf, then pt_mesh_isosurface),
// --simplify GRID_N[,quadric|mean] (scene 6's meshes and the surface of --isosurface clustered on the GPU into cubic cells, GRID_N along the
// longest extent: pt_mesh_simplify) and --weld (vertices of equal position become one: the same stage's mode 0),
// --interior DENSITY[,R,G,B[,G[,AR,AG,AB]]] (every glass material of the scene script is filled with a homogeneous medium of that density,
// albedo, g and absorption per channel; density 0 with an absorption > 0 is a clear tinted body),
// --dispersion ABBE (every glass material of the scene script disperses: its ior is n_d, ABBE > 0 its Abbe number V_d),
// --exposure EV, --tonemap reference|srgb|reinhard|aces, --white W, --bloom S[,THRESHOLD[,SIGMA[,LEVELS]]] (the film stage between the
// accumulator and the PNG: the image scaled by 2^EV, glare of strength S around pixels brighter than THRESHOLD, a tone curve; pt_film_develop,
// DESIGN.md §17; without them the PNG is the reference's) and --out-hdr FILE (the scene-linear image after exposure and glare as f32:
// .pfm, or Radiance .hdr for any other extension).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <vector>

#include "scenes.hpp"

using namespace path_tracer;

// The plume of --smoke at the normalised position (x, y, z) in [0, 1]^3 of the box, y up: a column that rises from the floor's centre,
// sways, widens and thins:  cx = 0.5 + 0.08 sin(3 pi y),  cz = 0.5 + 0.08 cos(2 pi y),  r = 0.06 + 0.22 y,
//   V = (1 - 0.7 y) * exp(-((x - cx)^2 + (z - cz)^2) / r^2)
static double smoke_plume(double x, double y, double z) {
    const double pi = 3.14159265358979323846;
    const double cx = 0.5 + 0.08 * std::sin(3.0 * pi * y), cz = 0.5 + 0.08 * std::cos(2.0 * pi * y), r = 0.06 + 0.22 * y;
    return (1.0 - 0.7 * y) * std::exp(-((x - cx) * (x - cx) + (z - cz) * (z - cz)) / (r * r));
}
// STRENGTH[,R,G,B[,G]] of --fog / --smoke: one, four or five numbers, each parsed whole; strength > 0, albedo in [0, 1], |G| < 1
static bool parse_medium(const std::string& v, double out[5]) {
    std::vector<double> f;
    bool ok = !v.empty();
    for (size_t pos = 0; ok && pos <= v.size();) {
        const size_t comma = std::min(v.find(',', pos), v.size());
        const std::string tok = v.substr(pos, comma - pos);
        char* end = nullptr;
        const double x = strtod(tok.c_str(), &end);
        ok = !tok.empty() && end == tok.c_str() + tok.size();
        f.push_back(x);
        pos = comma + 1;
    }
    ok = ok && (f.size() == 1 || f.size() == 4 || f.size() == 5);
    for (size_t k = 0; ok && k < f.size(); ++k) out[k] = f[k];
    ok = ok && out[0] > 0.0 && out[0] < std::numeric_limits<double>::infinity() && std::fabs(out[4]) < 1.0;
    for (int k = 1; k <= 3; ++k) ok = ok && out[k] >= 0.0 && out[k] <= 1.0;
    return ok;
}
// DENSITY[,R,G,B[,G[,AR,AG,AB]]] of --interior: one, four, five or eight numbers, each parsed whole; density >= 0, albedo in [0, 1], |G| < 1,
// absorption >= 0, density + the largest absorption > 0
static bool parse_interior(const std::string& v, double out[8]) {
    std::vector<double> f;
    bool ok = !v.empty();
    for (size_t pos = 0; ok && pos <= v.size();) {
        const size_t comma = std::min(v.find(',', pos), v.size());
        const std::string tok = v.substr(pos, comma - pos);
        char* end = nullptr;
        const double x = strtod(tok.c_str(), &end);
        ok = !tok.empty() && end == tok.c_str() + tok.size();
        f.push_back(x);
        pos = comma + 1;
    }
    ok = ok && (f.size() == 1 || f.size() == 4 || f.size() == 5 || f.size() == 8);
    for (size_t k = 0; ok && k < f.size(); ++k) out[k] = f[k];
    const double inf = std::numeric_limits<double>::infinity();
    ok = ok && out[0] >= 0.0 && out[0] < inf && std::fabs(out[4]) < 1.0;
    for (int k = 1; k <= 3; ++k) ok = ok && out[k] >= 0.0 && out[k] <= 1.0;
    for (int k = 5; k <= 7; ++k) ok = ok && out[k] >= 0.0 && out[k] < inf;
    return ok && out[0] + std::max(out[5], std::max(out[6], out[7])) > 0.0;
}

// S[,THRESHOLD[,SIGMA[,LEVELS]]] of --bloom: one to four numbers, each parsed whole (LEVELS a whole number); the ranges are pt_film_opts_check's
static bool parse_bloom(const std::string& v, Film& film) {
    std::vector<double> f;
    for (size_t pos = 0; pos <= v.size();) {
        const size_t comma = std::min(v.find(',', pos), v.size());
        const std::string tok = v.substr(pos, comma - pos);
        char* end = nullptr;
        const double x = strtod(tok.c_str(), &end);
        if (tok.empty() || end != tok.c_str() + tok.size()) return false;
        f.push_back(x);
        pos = comma + 1;
    }
    if (f.empty() || f.size() > 4) return false;
    if (f.size() > 3 && !(f[3] >= 0.0 && f[3] <= 1e6 && f[3] == std::floor(f[3]))) return false;
    film.bloom_strength = f[0];
    if (f.size() > 1) film.bloom_threshold = f[1];
    if (f.size() > 2) film.bloom_sigma = f[2];
    if (f.size() > 3) film.bloom_levels = (uint32_t)f[3];
    return true;
}
// a whole-string number, any value: the film options' ranges are checked once, by pt_film_opts_check
static bool parse_number(const std::string& v, double& out) {
    char* end = nullptr;
    out = strtod(v.c_str(), &end);
    return !v.empty() && end == v.c_str() + v.size();
}
// `n_min` to `n_max` comma-separated finite numbers, each parsed whole (--shutter, --motion)
static bool parse_numbers(const std::string& v, size_t n_min, size_t n_max, std::vector<double>& x) {
    x.clear();
    for (size_t pos = 0; pos <= v.size();) {
        const size_t comma = std::min(v.find(',', pos), v.size());
        const std::string tok = v.substr(pos, comma - pos);
        char* end = nullptr;
        const double d = strtod(tok.c_str(), &end);
        if (tok.empty() || !end || *end != 0 || !std::isfinite(d)) return false;
        x.push_back(d);
        pos = comma + 1;
    }
    return x.size() >= n_min && x.size() <= n_max;
}
// X,Y,Z,RADIUS[,R,G,B] of --mesh-light: four or seven numbers, each parsed whole; radius > 0, emission >= 0
static bool parse_mesh_light(const std::string& v, double out[7]) {
    std::vector<double> x;
    size_t pos = 0;
    while (pos <= v.size()) {
        const size_t comma = std::min(v.find(',', pos), v.size());
        const std::string tok = v.substr(pos, comma - pos);
        char* end = nullptr;
        const double d = strtod(tok.c_str(), &end);
        if (tok.empty() || !end || *end != 0 || !std::isfinite(d)) return false;
        x.push_back(d);
        pos = comma + 1;
    }
    if (x.size() != 4 && x.size() != 7) return false;
    if (!(x[3] > 0.0)) return false;
    for (size_t i = 4; i < x.size(); ++i)
        if (!(x[i] >= 0.0)) return false;
    for (size_t i = 0; i < x.size(); ++i) out[i] = x[i];
    return true;
}
// A unit icosahedron subdivided `level` times (20 * 4^level triangles), its vertices pushed out to `radius` around `centre`
static Mesh icosphere(int level, Vec3 centre, double radius) {
    const double t = (1.0 + std::sqrt(5.0)) / 2.0;
    std::vector<Vec3> v = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t}, {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
    std::vector<uint32_t> f = {0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
                               3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1};
    auto unit = [](Vec3 p) { const double l = std::sqrt(p.x * p.x + p.y * p.y + p.z * p.z); return Vec3{p.x / l, p.y / l, p.z / l}; };
    for (Vec3& p : v) p = unit(p);
    for (int l = 0; l < level; ++l) {
        std::map<uint64_t, uint32_t> cache;
        auto mid = [&](uint32_t a, uint32_t b) {
            const uint64_t key = ((uint64_t)std::min(a, b) << 32) | std::max(a, b);
            auto it = cache.find(key);
            if (it != cache.end()) return it->second;
            v.push_back(unit(Vec3{v[a].x + v[b].x, v[a].y + v[b].y, v[a].z + v[b].z}));
            return cache[key] = (uint32_t)v.size() - 1;
        };
        std::vector<uint32_t> nf;
        for (size_t i = 0; i < f.size(); i += 3) {
            const uint32_t a = f[i], b = f[i + 1], c = f[i + 2], ab = mid(a, b), bc = mid(b, c), ca = mid(c, a);
            for (uint32_t k : {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca}) nf.push_back(k);
        }
        f = nf;
    }
    Mesh m;
    for (const Vec3& p : v)
        for (double c : {centre.x + radius * p.x, centre.y + radius * p.y, centre.z + radius * p.z}) m.positions.push_back((float)c);
    m.indices = f;
    return m;
}

// --displace: the Quad of the scene whose material carries a normal map gives way to a tessellated, displaced grid mesh of the same q, u, v
// with the same base colour and no normal map. v = SCALE[, LEVELS[, MIDLEVEL]].
static void displace_brick_wall(World& world, pt_ctx* ctx, const std::string& file, const std::string& asset_dir, const std::vector<double>& v, bool weld) {
    std::string path = file;
    if (!std::ifstream(path)) {   // "assets/bricks/color.png" the way the scene scripts name their images: relative to --assets
        const std::string prefix = "assets/";
        path = asset_dir + "/" + (file.compare(0, prefix.size(), prefix) == 0 ? file.substr(prefix.size()) : file);
    }
    uint8_t* rgb = nullptr;
    uint32_t w = 0, h = 0;
    const bool jpeg = (path.size() > 4 && path.substr(path.size() - 4) == ".jpg") || (path.size() > 5 && path.substr(path.size() - 5) == ".jpeg");
    if ((jpeg ? pt_load_jpeg_rgb8(path.c_str(), &rgb, &w, &h) : pt_load_png_rgb8(path.c_str(), &rgb, &w, &h)) != 0) panic("--displace " + file);
    std::vector<float> height((size_t)w * h);
    pt_height_from_rgb8(w, h, rgb, height.data());
    pt_free(rgb);
    pt_tess_opts o;
    pt_tess_opts_default(&o);
    o.levels = v.size() > 1 ? (uint32_t)v[1] : 2u;
    o.height_w = w;
    o.height_h = h;
    o.height = height.data();
    o.scale = v[0];
    if (v.size() > 2) o.midlevel = v[2];
    for (auto& obj : world.objects) {
        auto quad = std::dynamic_pointer_cast<Quad>(obj);
        auto mat = quad ? std::dynamic_pointer_cast<DiffuseBRDF>(quad->material) : nullptr;
        if (!mat || !mat->normal_map) continue;
        Mesh grid = Mesh::grid(quad->q, quad->u, quad->v, 64, 64);
        if (weld) {   // (a grid shares its vertices already: the pass is the identity but for the normals, which it recomputes)
            pt_simplify_opts wo;
            pt_simplify_opts_default(&wo);
            wo.mode = 0;
            grid = grid.simplified(ctx, wo);
        }
        obj = TriangleMesh::from_obj(1.0, grid.tessellated(ctx, o), DiffuseBRDF::from_textures(mat->base_color, nullptr));
        return;
    }
    throw std::runtime_error("--displace: the scene has no wall with a normal-mapped material");
}

// --subdivide: the three OBJ meshes of scene 6 (bunny, spot, cow: coarse control cages) become Loop subdivision surfaces: LEVELS levels on the
// GPU, pushed to the limit surface, with smooth normals. v = LEVELS[, CREASE_DEG[, CORNER_DEG]].
static const char* const SUBDIVIDE_FILES[3] = {"bunny.obj", "spot.obj", "cow.obj"};
static const uint64_t SUBDIVIDE_MAX_FACES = 1ull << 19;   // the default device-BVH threshold: from there on the LBVH can be too deep

static pt_subdiv_opts subdivide_opts(const std::vector<double>& v) {
    pt_subdiv_opts o;
    pt_subdiv_opts_default(&o);
    const double rad = 3.14159265358979323846 / 180.0;
    o.levels = (uint32_t)v[0];
    if (v.size() > 1) o.crease_cos = std::cos(v[1] * rad);
    if (v.size() > 2) o.corner_cos = std::cos(v[2] * rad);
    o.limit = 1;
    return o;
}

static void subdivide_meshes(World& world, pt_ctx* ctx, const std::vector<double>& v) {
    const pt_subdiv_opts o = subdivide_opts(v);
    size_t done = 0;
    for (auto& obj : world.objects) {
        auto inst = std::dynamic_pointer_cast<Instance>(obj);
        auto mesh = inst ? std::dynamic_pointer_cast<TriangleMesh>(inst->object) : nullptr;
        if (!mesh) continue;
        inst->object = TriangleMesh::from_obj(mesh->scale, mesh->mesh.subdivided(ctx, o), mesh->material);
        ++done;
    }
    if (done != 3) throw std::runtime_error("--subdivide: the scene does not hold its three meshes");
}

// --simplify GRID_N[,quadric|mean]: a mesh clustered on the GPU into cubic cells, GRID_N along its longest extent (pt_mesh_simplify,
// DESIGN.md section 31). A mesh that came with normals gets smooth ones back, one without stays flat-shaded. --weld: mode 0 of the same
// stage: vertices of equal position become one, so that a mesh whose vertices are duplicated along seams subdivides and displaces as one surface.
static Mesh simplified_mesh(const Mesh& m, pt_ctx* ctx, uint32_t grid_n, int placement) {
    pt_simplify_opts o;
    pt_simplify_opts_default(&o);
    o.grid_n = grid_n;
    o.placement = placement;
    o.normals = m.normals.empty() ? 1 : 0;
    return m.simplified(ctx, o);
}

static void simplify_meshes(World& world, pt_ctx* ctx, uint32_t grid_n, int placement, bool weld) {
    for (auto& obj : world.objects) {
        auto inst = std::dynamic_pointer_cast<Instance>(obj);
        auto mesh = inst ? std::dynamic_pointer_cast<TriangleMesh>(inst->object) : nullptr;
        if (!mesh) continue;
        const Mesh r = weld ? mesh->mesh.welded(ctx) : simplified_mesh(mesh->mesh, ctx, grid_n, placement);
        if (r.indices.empty()) throw std::runtime_error("--simplify: nothing is left of a mesh at that GRID_N");
        inst->object = TriangleMesh::from_obj(mesh->scale, r, mesh->material);
    }
}

// --isosurface ISO[,GRID_N]: the plume of --smoke, sampled into GRID_N^3 cells over the box --fog would fill, meshed on the GPU where it
// crosses ISO (closed, gradient normals) and added to the world as a white diffuse body.
static void add_isosurface(World& world, pt_ctx* ctx, const std::vector<double>& v, Vec3 lo, Vec3 hi, uint32_t simplify_n, int placement) {
    const uint32_t N = v.size() > 1 ? (uint32_t)v[1] : 64u;
    std::vector<float> f((size_t)N * N * N);
    for (uint32_t k = 0; k < N; ++k)
        for (uint32_t j = 0; j < N; ++j)
            for (uint32_t i = 0; i < N; ++i) f[((size_t)k * N + j) * N + i] = (float)smoke_plume((i + 0.5) / N, (j + 0.5) / N, (k + 0.5) / N);
    pt_iso_opts o;
    pt_iso_opts_default(&o);
    o.iso = v[0];
    o.closed = 1;
    Mesh m = Mesh::isosurface(ctx, o, N, N, N, f, lo, hi);
    if (m.indices.empty()) throw std::runtime_error("--isosurface: the plume does not cross that level");
    if (simplify_n) {
        m = simplified_mesh(m, ctx, simplify_n, placement);
        if (m.indices.empty()) throw std::runtime_error("--simplify: nothing is left of the isosurface at that GRID_N");
    }
    world.add_object(TriangleMesh::from_obj(1.0, m, DiffuseBRDF::from_rgb(Vec3{0.73, 0.73, 0.73})));
}

// --mesh-smoke and --remesh work on the OBJ meshes of scene 6, which the scene adds in the order of SUBDIVIDE_FILES: bunny, spot, cow
static std::vector<std::shared_ptr<Instance>> obj_instances(World& world, const char* flag) {
    std::vector<std::shared_ptr<Instance>> out;
    for (auto& obj : world.objects) {
        auto inst = std::dynamic_pointer_cast<Instance>(obj);
        if (inst && std::dynamic_pointer_cast<TriangleMesh>(inst->object)) out.push_back(inst);
    }
    if (out.size() != 3) throw std::runtime_error(std::string(flag) + ": the scene does not hold its three meshes");
    return out;
}

// The mesh of an instance where the scene puts it: scaled, turned about the instance's axis (Rodrigues, as Instance::bounds), translated
static Mesh placed_mesh(const Instance& inst) {
    const auto tm = std::dynamic_pointer_cast<TriangleMesh>(inst.object);
    Mesh m;
    m.indices = tm->mesh.indices;
    m.positions.resize(tm->mesh.positions.size());
    const double c = std::cos(inst.angle), s = std::sin(inst.angle);
    const Vec3 a = inst.axis, t = inst.translation;
    for (size_t i = 0; i + 2 < m.positions.size(); i += 3) {
        const Vec3 p{tm->mesh.positions[i] * tm->scale, tm->mesh.positions[i + 1] * tm->scale, tm->mesh.positions[i + 2] * tm->scale};
        const double d = a.x * p.x + a.y * p.y + a.z * p.z;
        const Vec3 x{a.y * p.z - a.z * p.y, a.z * p.x - a.x * p.z, a.x * p.y - a.y * p.x};
        m.positions[i] = (float)(p.x * c + x.x * s + a.x * d * (1.0 - c) + t.x);
        m.positions[i + 1] = (float)(p.y * c + x.y * s + a.y * d * (1.0 - c) + t.y);
        m.positions[i + 2] = (float)(p.z * c + x.z * s + a.z * d * (1.0 - c) + t.z);
    }
    return m;
}

// --mesh-smoke SCALE[,GRID_N[,RAMP_CELLS]]: spot leaves the scene as a surface and comes back as a cloud of its shape: its mesh, where the
// scene puts it, sampled on the GPU into a density that rises from 0 at the surface to 1 RAMP_CELLS cells inside (pt_mesh_sdf, what = 3;
// DESIGN.md section 30) over cubic cells fitted around it, GRID_N along its longest extent; the grid is the camera's unbounded medium, as --smoke's is.
static void mesh_smoke_cloud(World& world, pt_ctx* ctx, const std::vector<double>& v) {
    const auto spot = obj_instances(world, "--mesh-smoke")[1];
    const Mesh m = placed_mesh(*spot);
    const Grid shape = Grid::fit(m, v.size() > 1 ? (uint32_t)v[1] : 64u, 2.0);
    pt_sdf_opts o;
    pt_sdf_opts_default(&o);
    o.what = 3;
    o.ramp = (v.size() > 2 ? v[2] : 2.0) * shape.cell();
    Grid g = Grid::from_mesh(ctx, o, m, shape);
    for (size_t i = 0; i < world.objects.size(); ++i)
        if (world.objects[i] == spot) {
            world.objects.erase(world.objects.begin() + (std::ptrdiff_t)i);
            break;
        }
    world.camera_medium = HeterogeneousVolume::from_grid(nullptr, v[0], Vec3{1.0, 1.0, 1.0}, 0.0, g.nx, g.ny, g.nz, std::move(g.values), g.lo, g.hi);
}

// --remesh OFFSET[,GRID_N]: spot and cow are sampled into signed distance grids (pt_mesh_sdf, what = 0, GRID_N cubic cells along the longest
// extent E) and meshed again where the depth is -OFFSET * E (pt_mesh_isosurface, closed): the body grown by OFFSET * E (shrunk when negative),
// uniformly tessellated, with its material and placement. The bunny is an open mesh, whose sign means nothing, and stays as it is.
static void remesh_meshes(World& world, pt_ctx* ctx, const std::vector<double>& v) {
    const auto inst = obj_instances(world, "--remesh");
    const double N = v.size() > 1 ? v[1] : 64.0, grow = std::fabs(v[0]);
    const double margin = std::ceil((grow * N + 2.0) / (1.0 + 2.0 * grow));   // cells: two past the grown body on either side
    for (size_t k = 1; k < 3; ++k) {
        const auto tm = std::dynamic_pointer_cast<TriangleMesh>(inst[k]->object);
        const Grid shape = Grid::fit(tm->mesh, (uint32_t)N, margin);
        const double h = shape.cell(), E = h * (N - 2.0 * margin);
        pt_sdf_opts o;
        pt_sdf_opts_default(&o);
        o.band = grow * E + 4.0 * h;
        const Grid g = Grid::from_mesh(ctx, o, tm->mesh, shape);
        pt_iso_opts io;
        pt_iso_opts_default(&io);
        io.iso = -v[0] * E;
        io.closed = 1;
        io.outside = (float)-o.band;
        const Mesh r = Mesh::isosurface(ctx, io, g.nx, g.ny, g.nz, g.values, g.lo, g.hi);
        if (r.indices.empty()) throw std::runtime_error("--remesh: nothing is left of a mesh at that offset");
        inst[k]->object = TriangleMesh::from_obj(tm->scale, r, tm->material);
    }
}

int main(int argc, char** argv) {
    bool quality = false, float_hdr = false;
    int scene = 1, device = 0;
    long width = -1, spp = -1, min_spp = 16;
    double adaptive = 0.0, env_sampling = 0.0;
    bool use_adaptive = false, use_denoise = false;
    int sampler = 0;
    bool fog = false;
    double fog_v[5] = {0.0, 1.0, 1.0, 1.0, 0.0};   // density, albedo r g b, g
    bool smoke = false;
    double smoke_v[5] = {0.0, 1.0, 1.0, 1.0, 0.0};   // scale, albedo r g b, g
    bool interior = false;
    double interior_v[8] = {0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0};   // density, albedo r g b, g, absorption r g b
    double dispersion = 0.0;   // the Abbe number of --dispersion, 0: not given
    int projection = 0;        // --projection: pt_scene_set_projection's kind
    double shutter[2] = {0.0, 1.0};   // --shutter OPEN,CLOSE
    bool motion = false;              // --motion DX,DY,DZ[,DEGREES]
    bool stats = false;               // --stats: the render's statistics as one JSON line on stdout
    double motion_v[4] = {0.0, 0.0, 0.0, 0.0};
    int light_sampling = -1;   // -1: not given (--mesh-light then implies exact)
    bool mesh_light = false;
    std::vector<std::vector<double>> point_lights, spot_lights, suns;   // --point-light, --spot-light, --sun: repeatable
    double punctual_fraction = 0.5;                                      // --punctual-fraction F
    int punctual_selection = 0;                                          // --punctual-selection uniform|grid[,NX,NY,NZ]: the light grid
    uint32_t punctual_grid[3] = {0u, 0u, 0u};
    bool light_shafts = false;                                           // --light-shafts: the punctual lights light --fog / --smoke
    double mesh_light_v[7] = {0.0, 0.0, 0.0, 0.0, 10.0, 10.0, 10.0};   // centre x y z, radius, emission r g b
    long aov_spp = 16;
    Film film;   // --exposure, --tonemap, --white, --bloom, --out-hdr
    bool sky = false, sky_no_disc = false;   // --sky ELEVATION_DEG,AZIMUTH_DEG[,TURBIDITY[,WIDTH]], --sky-no-disc
    std::vector<double> sky_v;
    bool displace = false;                   // --displace FILE,SCALE[,LEVELS[,MIDLEVEL]]
    std::string displace_file;
    std::vector<double> displace_v;
    bool subdivide = false;                  // --subdivide LEVELS[,CREASE_DEG[,CORNER_DEG]]
    std::vector<double> subdivide_v;
    bool isosurface = false;                 // --isosurface ISO[,GRID_N]
    std::vector<double> isosurface_v;
    bool mesh_smoke = false;                 // --mesh-smoke SCALE[,GRID_N[,RAMP_CELLS]]
    std::vector<double> mesh_smoke_v;
    bool simplify = false, weld = false;     // --simplify GRID_N[,quadric|mean]; --weld
    uint32_t simplify_n = 0;
    int simplify_placement = 0;
    bool remesh = false;                     // --remesh OFFSET[,GRID_N]
    std::vector<double> remesh_v;
    uint64_t seed = 1;
    std::string out, assets = "assets";
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) { std::cerr << "missing value for " << a << "\n"; exit(2); }
            return argv[++i];
        };
        if (a == "-q" || a == "--quality") quality = true;
        else if (a == "-s" || a == "--scene") scene = atoi(next());
        else if (a == "--width") width = atol(next());
        else if (a == "--spp") spp = atol(next());
        else if (a == "--seed") seed = strtoull(next(), nullptr, 10);
        else if (a == "--out") out = next();
        else if (a == "--assets") assets = next();
        else if (a == "--device") device = atoi(next());
        else if (a == "--float-hdr") float_hdr = true;
        else if (a == "--env-sampling") {
            env_sampling = atof(next());
            if (!(env_sampling >= 0.0 && env_sampling < 1.0)) { std::cerr << "--env-sampling must be in [0, 1)\n"; return 2; }
        }
        else if (a == "--sampler") {
            const std::string v = next();
            if (v == "independent") sampler = 0;
            else if (v == "sobol") sampler = 1;
            else { std::cerr << "--sampler must be independent or sobol\n"; return 2; }
        }
        else if (a == "--fog") {
            if (!parse_medium(next(), fog_v)) { std::cerr << "--fog must be DENSITY[,R,G,B[,G]]: density > 0, albedo channels in [0, 1], |G| < 1\n"; return 2; }
            fog = true;
        }
        else if (a == "--smoke") {
            if (!parse_medium(next(), smoke_v)) { std::cerr << "--smoke must be SCALE[,R,G,B[,G]]: scale > 0, albedo channels in [0, 1], |G| < 1\n"; return 2; }
            smoke = true;
        }
        else if (a == "--interior") {
            if (!parse_interior(next(), interior_v)) {
                std::cerr << "--interior must be DENSITY[,R,G,B[,G[,AR,AG,AB]]]: density >= 0, albedo channels in [0, 1], |G| < 1, absorption >= 0, density or an absorption > 0\n";
                return 2;
            }
            interior = true;
        }
        else if (a == "--dispersion") {
            const std::string v = next();
            char* end = nullptr;
            dispersion = strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || !(dispersion > 0.0) || !std::isfinite(dispersion)) {
                std::cerr << "--dispersion must be ABBE: the Abbe number V_d of the scene's glass, finite and > 0\n";
                return 2;
            }
        }
        else if (a == "--light-sampling") {
            const std::string v = next();
            if (v == "reference") light_sampling = 0;
            else if (v == "exact") light_sampling = 1;
            else { std::cerr << "--light-sampling must be reference or exact\n"; return 2; }
        }
        else if (a == "--projection") {
            const std::string v = next();
            if (v == "perspective") projection = 0;
            else if (v == "orthographic") projection = 1;
            else if (v == "fisheye") projection = 2;
            else if (v == "panorama") projection = 3;
            else { std::cerr << "--projection must be perspective, orthographic, fisheye or panorama\n"; return 2; }
        }
        else if (a == "--stats") stats = true;
        else if (a == "--shutter") {
            std::vector<double> x;
            if (!parse_numbers(next(), 2, 2, x) || !(0.0 <= x[0] && x[0] <= x[1] && x[1] <= 1.0)) {
                std::cerr << "--shutter must be OPEN,CLOSE with 0 <= OPEN <= CLOSE <= 1\n";
                return 2;
            }
            shutter[0] = x[0]; shutter[1] = x[1];
        }
        else if (a == "--motion") {
            std::vector<double> x;
            if (!parse_numbers(next(), 3, 4, x)) { std::cerr << "--motion must be DX,DY,DZ[,DEGREES]: finite numbers\n"; return 2; }
            for (size_t k = 0; k < x.size(); ++k) motion_v[k] = x[k];
            motion = true;
        }
        else if (a == "--point-light") {
            std::vector<double> x;
            if (!parse_numbers(next(), 6, 6, x)) { std::cerr << "--point-light must be X,Y,Z,R,G,B: finite numbers\n"; return 2; }
            point_lights.push_back(x);
        }
        else if (a == "--spot-light") {
            std::vector<double> x;
            if (!parse_numbers(next(), 11, 11, x)) { std::cerr << "--spot-light must be X,Y,Z,TX,TY,TZ,INNER,OUTER,R,G,B: finite numbers\n"; return 2; }
            spot_lights.push_back(x);
        }
        else if (a == "--sun") {
            std::vector<double> x;
            if (!parse_numbers(next(), 6, 6, x)) { std::cerr << "--sun must be DX,DY,DZ,R,G,B: finite numbers\n"; return 2; }
            suns.push_back(x);
        }
        else if (a == "--punctual-fraction") {
            if (!parse_number(next(), punctual_fraction) || !(punctual_fraction > 0.0 && punctual_fraction < 1.0)) { std::cerr << "--punctual-fraction must be a number F with 0 < F < 1\n"; return 2; }
        }
        else if (a == "--punctual-selection") {
            const std::string v = next();
            bool ok = v == "uniform" || v == "grid";
            punctual_selection = v == "uniform" ? 0 : 1;
            if (!ok && v.rfind("grid,", 0) == 0) {
                std::vector<double> x;
                ok = parse_numbers(v.substr(5), 3, 3, x);
                for (size_t k = 0; ok && k < 3; ++k) {
                    ok = x[k] >= 1.0 && x[k] <= 64.0 && x[k] == std::floor(x[k]);
                    if (ok) punctual_grid[k] = (uint32_t)x[k];
                }
            }
            if (!ok) { std::cerr << "--punctual-selection must be uniform, grid or grid,NX,NY,NZ with whole numbers 1..64\n"; return 2; }
        }
        else if (a == "--light-shafts") light_shafts = true;
        else if (a == "--mesh-light") {
            if (!parse_mesh_light(next(), mesh_light_v)) { std::cerr << "--mesh-light must be X,Y,Z,RADIUS[,R,G,B]: radius > 0, emission >= 0\n"; return 2; }
            mesh_light = true;
        }
        else if (a == "--exposure") {
            if (!parse_number(next(), film.exposure_ev)) { std::cerr << "--exposure must be a number (EV)\n"; return 2; }
        }
        else if (a == "--tonemap") {
            const std::string v = next();
            if (v == "reference") film.tonemap = 0;
            else if (v == "srgb") film.tonemap = 1;
            else if (v == "reinhard") film.tonemap = 2;
            else if (v == "aces") film.tonemap = 3;
            else { std::cerr << "--tonemap must be reference, srgb, reinhard or aces\n"; return 2; }
        }
        else if (a == "--white") {
            if (!parse_number(next(), film.white)) { std::cerr << "--white must be a number\n"; return 2; }
        }
        else if (a == "--bloom") {
            if (!parse_bloom(next(), film)) { std::cerr << "--bloom must be S[,THRESHOLD[,SIGMA[,LEVELS]]]: numbers, LEVELS a whole one\n"; return 2; }
        }
        else if (a == "--out-hdr") film.hdr_filename = next();
        else if (a == "--sky") {
            if (!parse_numbers(next(), 2, 4, sky_v)) {
                pt_set_error_message("--sky must be ELEVATION_DEG,AZIMUTH_DEG[,TURBIDITY[,WIDTH]]: finite numbers");
                std::cerr << pt_last_error() << "\n";
                return 2;
            }
            sky = true;
        }
        else if (a == "--sky-no-disc") sky_no_disc = true;
        else if (a == "--displace") {
            const std::string v = next();
            const size_t comma = v.find(',');
            displace_file = v.substr(0, comma);
            if (comma == std::string::npos || displace_file.empty() || !parse_numbers(v.substr(comma + 1), 1, 3, displace_v) ||
                (displace_v.size() > 1 && (displace_v[1] < 0.0 || displace_v[1] > 12.0 || displace_v[1] != std::floor(displace_v[1])))) {
                std::cerr << "--displace must be FILE,SCALE[,LEVELS[,MIDLEVEL]]: finite numbers, LEVELS a whole one in 0..12\n";
                return 2;
            }
            displace = true;
        }
        else if (a == "--subdivide") {
            if (!parse_numbers(next(), 1, 3, subdivide_v) || subdivide_v[0] < 0.0 || subdivide_v[0] > 12.0 || subdivide_v[0] != std::floor(subdivide_v[0])) {
                std::cerr << "--subdivide must be LEVELS[,CREASE_DEG[,CORNER_DEG]]: finite numbers, LEVELS a whole one in 0..12\n";
                return 2;
            }
            if (subdivide_v.size() > 1 && !(subdivide_v[1] >= 0.0 && subdivide_v[1] <= 180.0)) { std::cerr << "--subdivide: CREASE_DEG must lie in 0..180\n"; return 2; }
            if (subdivide_v.size() > 2 && !(subdivide_v[2] >= 0.0 && subdivide_v[2] <= 180.0)) { std::cerr << "--subdivide: CORNER_DEG must lie in 0..180\n"; return 2; }
            subdivide = true;
        }
        else if (a == "--isosurface") {
            if (!parse_numbers(next(), 1, 2, isosurface_v) || (isosurface_v.size() > 1 && (isosurface_v[1] < 2.0 || isosurface_v[1] > 512.0 || isosurface_v[1] != std::floor(isosurface_v[1])))) {
                std::cerr << "--isosurface must be ISO[,GRID_N]: finite numbers, GRID_N a whole one in 2..512\n";
                return 2;
            }
            isosurface = true;
        }
        else if (a == "--mesh-smoke") {
            const auto grid_n = [](double n) { return n >= 8.0 && n <= 256.0 && n == std::floor(n); };
            if (!parse_numbers(next(), 1, 3, mesh_smoke_v) || !(mesh_smoke_v[0] > 0.0) || (mesh_smoke_v.size() > 1 && !grid_n(mesh_smoke_v[1])) ||
                (mesh_smoke_v.size() > 2 && !(mesh_smoke_v[2] > 0.0))) {
                std::cerr << "--mesh-smoke must be SCALE[,GRID_N[,RAMP_CELLS]]: finite numbers, SCALE > 0, GRID_N a whole one in 8..256, RAMP_CELLS > 0\n";
                return 2;
            }
            mesh_smoke = true;
        }
        else if (a == "--remesh") {
            if (!parse_numbers(next(), 1, 2, remesh_v) || !(std::fabs(remesh_v[0]) <= 0.25) ||
                (remesh_v.size() > 1 && !(remesh_v[1] >= 8.0 && remesh_v[1] <= 256.0 && remesh_v[1] == std::floor(remesh_v[1])))) {
                std::cerr << "--remesh must be OFFSET[,GRID_N]: finite numbers, OFFSET in -0.25..0.25, GRID_N a whole one in 8..256\n";
                return 2;
            }
            remesh = true;
        }
        else if (a == "--simplify") {
            const std::string v = next();
            const size_t comma = v.find(',');
            const std::string how = comma == std::string::npos ? "quadric" : v.substr(comma + 1);
            std::vector<double> n;
            if (!parse_numbers(v.substr(0, comma), 1, 1, n) || !(n[0] >= 1.0 && n[0] <= 4096.0 && n[0] == std::floor(n[0])) || (how != "quadric" && how != "mean")) {
                std::cerr << "--simplify must be GRID_N[,quadric|mean]: GRID_N a whole number in 1..4096\n";
                return 2;
            }
            simplify = true;
            simplify_n = (uint32_t)n[0];
            simplify_placement = how == "mean" ? 1 : 0;
        }
        else if (a == "--weld") weld = true;
        else if (a == "--adaptive") { adaptive = atof(next()); use_adaptive = true; }
        else if (a == "--min-spp") min_spp = atol(next());
        else if (a == "--denoise") use_denoise = true;
        else if (a == "--aov-spp") aov_spp = atol(next());
        else if (a == "-h" || a == "--help") {
            std::cout << "usage: pt_render [-q] [-s N] [--width W] [--spp S] [--seed K] [--out file.png] [--assets DIR] [--device D] [--float-hdr] [--env-sampling F] [--sampler independent|sobol] [--fog DENSITY[,R,G,B[,G]]] [--smoke SCALE[,R,G,B[,G]]] [--interior DENSITY[,R,G,B[,G[,AR,AG,AB]]]] [--dispersion ABBE] [--light-sampling reference|exact] [--mesh-light X,Y,Z,RADIUS[,R,G,B]] [--projection perspective|orthographic|fisheye|panorama] [--shutter OPEN,CLOSE] [--motion DX,DY,DZ[,DEGREES]] [--point-light X,Y,Z,R,G,B]... [--spot-light X,Y,Z,TX,TY,TZ,INNER,OUTER,R,G,B]... [--sun DX,DY,DZ,R,G,B]... [--punctual-fraction F] [--punctual-selection uniform|grid[,NX,NY,NZ]] [--light-shafts] [--stats] [--adaptive T [--min-spp M]] [--denoise [--aov-spp N]] [--exposure EV] [--tonemap reference|srgb|reinhard|aces] [--white W] [--bloom S[,THRESHOLD[,SIGMA[,LEVELS]]]] [--out-hdr file.hdr|file.pfm] [--sky ELEVATION_DEG,AZIMUTH_DEG[,TURBIDITY[,WIDTH]] [--sky-no-disc]] [--displace FILE,SCALE[,LEVELS[,MIDLEVEL]]] [--subdivide LEVELS[,CREASE_DEG[,CORNER_DEG]]] [--isosurface ISO[,GRID_N]] [--mesh-smoke SCALE[,GRID_N[,RAMP_CELLS]]] [--remesh OFFSET[,GRID_N]] [--simplify GRID_N[,quadric|mean]] [--weld]\n"
                         "  --simplify: scene 6's meshes (after --remesh, before --subdivide) and the surface of --isosurface are clustered on the GPU into cubic cells,\n"
                         "           GRID_N along the mesh's longest extent: the vertices of a cell become one, placed where the planes of the faces around them meet\n"
                         "           (quadric, the default) or at their mean; faces that lose a corner go. Fewer triangles for the BVH and for K2\n"
                         "  --weld: vertices of equal position become one, on the GPU: scene 6's meshes before --subdivide, the wall's grid before --displace\n"
                         "  --mesh-smoke: scene 6 only: spot leaves the scene as a surface and comes back as a cloud of its shape: an unbounded grid-density camera\n"
                         "           medium of extinction SCALE * V, as --smoke's, V the density pt_mesh_sdf samples on the GPU over cubic cells fitted around spot (GRID_N\n"
                         "           along its longest extent, default 64, two cells of margin): 0 outside, rising to 1 RAMP_CELLS cells (default 2) below the surface.\n"
                         "           White, isotropic. Not with whatever --smoke is refused with, nor with --smoke, --isosurface, --subdivide or --remesh\n"
                         "  --remesh: scene 6 only: spot and cow are sampled into signed distance grids on the GPU (GRID_N cubic cells along the longest extent E, default\n"
                         "           64) and meshed again by --isosurface's marching tetrahedra at the distance OFFSET * E outside the surface (inside when negative):\n"
                         "           grown, shrunk or (0) merely tessellated evenly; material and placement stay. The bunny is open and stays. Not with --subdivide\n"
                         "  --isosurface: the plume of --smoke as a surface: V is sampled at the centres of GRID_N^3 cells (default 64) over the box --fog would fill,\n"
                         "           meshed on the GPU by marching tetrahedra where it crosses ISO (0 < ISO < 1; closed where it leaves the box) and added to the\n"
                         "           scene as a white diffuse body. Not with --smoke or --fog\n"
                         "  --subdivide: scene 6 only: bunny, spot and cow, coarse control cages, become Loop subdivision surfaces: LEVELS levels on the GPU (each makes\n"
                         "           four triangles of one; at most 2^19 a mesh), the vertices pushed to the limit surface, smooth normals. An edge whose two faces'\n"
                         "           normals differ by more than CREASE_DEG stays sharp (default: none does; 0 keeps every edge, the cage itself); a crease vertex whose\n"
                         "           two sharp edges meet at less than CORNER_DEG stays a corner (default: none does). Boundary edges are always sharp\n"
                         "  --displace: scene 7 only: the wall that carries the normal-mapped bricks becomes a 64 x 64 grid mesh, subdivided LEVELS times (default 2) on\n"
                         "           the GPU and pushed along its normal by SCALE * (luminance of the PNG or JPEG image FILE - MIDLEVEL) (MIDLEVEL default 0.5): real relief\n"
                         "           with a silhouette and shadows; the wall keeps the brick colours and drops the normal map\n"
                         "  --sky: the scene's environment becomes a physical sky (Preetham daylight, a ground below the horizon and the sun's disc) baked on the GPU\n"
                         "           into a WIDTH x WIDTH/2 float map (default 2048): the sun stands ELEVATION_DEG above the horizon at AZIMUTH_DEG from +x towards +z,\n"
                         "           TURBIDITY 1.7 (clear) .. 10 (hazy), default 3. Works with --env-sampling (which finds the disc), --exposure, --tonemap, --out-hdr.\n"
                         "           --sky-no-disc leaves the disc out of the map and prints the --sun argument that brings the same sun back as a punctual light\n"
                         "  --projection: orthographic frames the rectangle the scene's camera sees on its focal plane; fisheye is equidistant with the scene's vfov\n"
                         "           across the image height; panorama is an equirectangular image of everything around the camera position, in world axes: loaded as\n"
                         "           an environment map (--out-hdr, then --float-hdr) it lights another scene. fisheye and panorama have no lens: the scene's\n"
                         "           defocus_angle is set to 0 for them\n"
                         "  --motion: every instance of the scene moves by (DX, DY, DZ) and turns by DEGREES about its own axis while the shutter is open, and blurs;\n"
                         "           --shutter: the part of that unit interval the camera's shutter is open for (default 0,1; OPEN = CLOSE freezes the scene at that\n"
                         "           instant; moving spheres follow it too). Not with --env-sampling, --fog, --smoke, --interior, --dispersion, --light-sampling exact\n"
                         "           or --mesh-light\n"
                         "  --point-light, --spot-light, --sun: lights without geometry, each flag repeatable: a point light of power R,G,B (W) at X,Y,Z; a spot light at\n"
                         "           X,Y,Z aimed at TX,TY,TZ with on-axis intensity R,G,B (W/sr), full inside INNER degrees from the axis and fading to zero at OUTER; a sun\n"
                         "           whose light travels along DX,DY,DZ with irradiance R,G,B. --punctual-fraction: the share F of a bounce's one sample they get (default\n"
                         "           0.5). They are invisible to the camera and every surface shadows them, glass included. Not with --env-sampling, --fog, --smoke,\n"
                         "           --interior, --dispersion, --light-sampling exact, --mesh-light or --motion. --light-shafts: the lights also light --fog and\n"
                         "           --smoke (a spot light's cone in haze, sun beams through a plume), which they are refused with otherwise; max_depth is at most 255 then\n"
                         "           --punctual-selection grid: the branch picks its light by importance per cell of a grid over the scene (NX,NY,NZ cells, each 1..64;\n"
                         "           automatic without them) instead of uniformly: for scenes with many lamps\n"
                         "  --stats: every kernel launch of a plain render is timed and its statistics are printed as one JSON line (tools/motion_eval.py reads it)\n"
                         "  --exposure, --tonemap, --white, --bloom: the film stage between the accumulator and the PNG: the image is scaled by 2^EV, light above the\n"
                         "           luminance THRESHOLD (default 1) spreads as glare of strength S (LEVELS Gaussians of SIGMA, 2 SIGMA, ... pixels; defaults 5 and 2),\n"
                         "           then the tone curve (reinhard maps the luminance W, default 4, to white). --out-hdr: the linear image after exposure and glare, f32\n"
                         "  --dispersion ABBE: every glass of the scene disperses light; its ior is read as n_d (587.56 nm), ABBE = V_d = (n_d - 1) / (n_F - n_C)\n"
                         "           (crown glass about 60, flint 30, diamond 55; smaller = more colour). Not with --env-sampling, --fog, --smoke, --interior,\n"
                         "           --light-sampling exact or --mesh-light\n"
                         "  --smoke: an unbounded grid-density camera medium of extinction SCALE * V over the world's bounds grown by 1 % (the box --fog fills),\n"
                         "           V sampled at the centres of 64^3 cells; at the normalised position (x, y, z) of the box, y up:\n"
                         "           cx = 0.5 + 0.08 sin(3 pi y), cz = 0.5 + 0.08 cos(2 pi y), r = 0.06 + 0.22 y,\n"
                         "           V = (1 - 0.7 y) exp(-((x - cx)^2 + (z - cz)^2) / r^2)\n";
            return 0;
        } else { std::cerr << "unknown argument " << a << "\n"; return 2; }
    }
    size_t w = quality ? 1920 : 600, s = quality ? 4000 : 100;   // main.rs:633
    if (width > 0) w = (size_t)width;
    if (spp > 0) s = (size_t)spp;
    if (use_denoise && use_adaptive) { std::cerr << "--denoise and --adaptive cannot be combined\n"; return 2; }
    if (use_denoise && s < 2) { std::cerr << "--denoise needs at least 2 samples per pixel\n"; return 2; }
    if (use_denoise && aov_spp < 1) { std::cerr << "--aov-spp must be positive\n"; return 2; }
    if (fog && env_sampling > 0.0) { std::cerr << "--fog and --env-sampling cannot be combined\n"; return 2; }
    if (smoke && env_sampling > 0.0) { std::cerr << "--smoke and --env-sampling cannot be combined\n"; return 2; }
    if (smoke && fog) { std::cerr << "--smoke and --fog cannot be combined\n"; return 2; }
    if (isosurface && (smoke || fog)) { std::cerr << "--isosurface cannot be combined with --smoke or --fog\n"; return 2; }
    if (mesh_smoke && (smoke || fog || isosurface || env_sampling > 0.0 || interior || mesh_light || dispersion > 0.0 || motion ||
                       ((!point_lights.empty() || !spot_lights.empty() || !suns.empty()) && !light_shafts))) {
        std::cerr << "--mesh-smoke cannot be combined with --smoke, --fog, --isosurface, --env-sampling, --interior, --mesh-light, --dispersion, --motion, "
                     "or --point-light, --spot-light and --sun without --light-shafts (whatever --smoke is refused with)\n";
        return 2;
    }
    if ((mesh_smoke || remesh) && subdivide) { std::cerr << (mesh_smoke ? "--mesh-smoke" : "--remesh") << " and --subdivide cannot be combined\n"; return 2; }
    if (mesh_smoke && remesh) { std::cerr << "--mesh-smoke and --remesh cannot be combined\n"; return 2; }
    if (interior && env_sampling > 0.0) { std::cerr << "--interior and --env-sampling cannot be combined\n"; return 2; }
    if (interior && (fog || smoke)) { std::cerr << "--interior cannot be combined with --fog or --smoke (that would nest media)\n"; return 2; }
    if (mesh_light && (env_sampling > 0.0 || fog || smoke || interior)) {
        std::cerr << "--mesh-light cannot be combined with --env-sampling, --fog, --smoke or --interior (exact light sampling runs without them)\n";
        return 2;
    }
    if (light_sampling < 0) light_sampling = mesh_light ? 1 : 0;
    if (dispersion > 0.0 && (env_sampling > 0.0 || fog || smoke || interior || light_sampling == 1)) {
        std::cerr << "--dispersion cannot be combined with --env-sampling, --fog, --smoke, --interior, --light-sampling exact or --mesh-light\n";
        return 2;
    }
    if (motion && (env_sampling > 0.0 || fog || smoke || interior || dispersion > 0.0 || light_sampling == 1)) {
        std::cerr << "--motion cannot be combined with --env-sampling, --fog, --smoke, --interior, --dispersion, --light-sampling exact or --mesh-light\n";
        return 2;
    }
    if ((!point_lights.empty() || !spot_lights.empty() || !suns.empty()) && (env_sampling > 0.0 || ((fog || smoke) && !light_shafts) || interior || dispersion > 0.0 || light_sampling == 1 || mesh_light || motion)) {
        std::cerr << "--point-light, --spot-light and --sun cannot be combined with --env-sampling, --fog, --smoke (unless --light-shafts is given), --interior, --dispersion, --light-sampling exact, --mesh-light or --motion\n";
        return 2;
    }
    {   // the film options' ranges: the library's own test, before anything is rendered
        const pt_film_opts fo = film.to_c();
        if (pt_film_opts_check(&fo) != 0) {
            std::cerr << "--exposure / --tonemap / --white / --bloom: " << pt_last_error() << "\n";
            return 2;
        }
    }
    if (simplify && scene != 6 && !isosurface) { std::cerr << "--simplify works on scene 6 (bunny, spot and cow) and with --isosurface only\n"; return 2; }
    if (weld && scene != 6 && !displace) { std::cerr << "--weld works on scene 6 (bunny, spot and cow) and with --displace only\n"; return 2; }
    if (displace && scene != 7) { std::cerr << "--displace works on scene 7 only (the wall with the normal-mapped bricks)\n"; return 2; }
    if (mesh_smoke && scene != 6) { std::cerr << "--mesh-smoke works on scene 6 only (spot)\n"; return 2; }
    if (remesh && scene != 6) { std::cerr << "--remesh works on scene 6 only (spot and cow)\n"; return 2; }
    if (subdivide && scene != 6) { std::cerr << "--subdivide works on scene 6 only (bunny, spot and cow)\n"; return 2; }
    if (subdivide) {   // the size of the result, from the files alone: before a context is made
        const uint64_t grow = 1ull << (2 * (uint32_t)subdivide_v[0]);
        for (const char* file : SUBDIVIDE_FILES) {
            float *pos, *uv;
            uint32_t *idx, np, ni, nuv;
            if (pt_load_obj((assets + "/" + file).c_str(), &pos, &np, &idx, &ni, &uv, &nuv) != 0) { std::cerr << "--subdivide: " << pt_last_error() << "\n"; return 2; }
            pt_free(pos); pt_free(idx); pt_free(uv);
            if ((uint64_t)(ni / 3) * grow > SUBDIVIDE_MAX_FACES) {
                std::cerr << "--subdivide: LEVELS " << (uint32_t)subdivide_v[0] << " takes " << file << " (" << ni / 3 << " triangles) past 2^19 triangles\n";
                return 2;
            }
        }
    }
    pt_sky_opts sky_opts;
    uint32_t sky_width = 2048;
    pt_sky_opts_default(&sky_opts);
    if (sky_no_disc && !sky) { std::cerr << "--sky-no-disc needs --sky\n"; return 2; }
    if (sky) {   // the sky options' ranges: the library's own test, before anything is rendered
        const double rad = 3.14159265358979323846 / 180.0;
        const double el = sky_v[0] * rad, az = sky_v[1] * rad;
        sky_opts.sun_dir[0] = std::cos(el) * std::cos(az);
        sky_opts.sun_dir[1] = std::sin(el);
        sky_opts.sun_dir[2] = std::cos(el) * std::sin(az);
        if (sky_v.size() > 2) sky_opts.turbidity = sky_v[2];
        int bad = pt_sky_opts_check(&sky_opts);
        if (bad == 0 && sky_v.size() > 3) {
            if (!(sky_v[3] >= 2.0 && sky_v[3] <= 8192.0) || sky_v[3] != std::floor(sky_v[3])) bad = pt_set_error_message("WIDTH must be a whole number in 2..8192");
            else sky_width = (uint32_t)sky_v[3];
        }
        if (bad != 0) {
            std::cerr << "--sky: " << pt_last_error() << "\n";
            return 2;
        }
        if (sky_no_disc) {
            double e[3];
            if (pt_sky_sun_irradiance(&sky_opts, e) != 0) { std::cerr << "--sky: " << pt_last_error() << "\n"; return 2; }
            std::printf("--sun %.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n", -sky_opts.sun_dir[0], -sky_opts.sun_dir[1], -sky_opts.sun_dir[2], e[0], e[1], e[2]);
            std::fflush(stdout);
            sky_opts.sun_scale = 0.0;
        }
    }
    if (scene < 1 || scene > 7) return 0;   // `_ => ()` main.rs:643
    pt_ctx* ctx = nullptr;
    if (pt_ctx_create(device, &ctx) != 0) {
        std::cerr << "fatal: " << pt_last_error() << "\n";
        return 1;
    }
    try {
        SceneSetup setup = make_scene(scene, w, s, assets, 1);
        setup.world.float_hdr = float_hdr;
        if (displace) {
            displace_brick_wall(setup.world, ctx, displace_file, assets, displace_v, weld);
            // the wall goes to the host's SAH builder at every size: from 2^19 triangles on it would get the device's LBVH, whose depth under the
            // scene's other entries can pass the traversal stack
            setup.world.device_bvh_threshold = 0;
        }
        if (remesh) remesh_meshes(setup.world, ctx, remesh_v);
        if (weld && scene == 6) simplify_meshes(setup.world, ctx, 0, 0, true);
        if (simplify && scene == 6) simplify_meshes(setup.world, ctx, simplify_n, simplify_placement, false);
        if (subdivide) subdivide_meshes(setup.world, ctx, subdivide_v);
        if (mesh_smoke) mesh_smoke_cloud(setup.world, ctx, mesh_smoke_v);
        if (sky) setup.camera.environment = EnvironmentType::Map(Sky::new_(sky_opts, sky_width, sky_width / 2));
        setup.world.env_sampling = env_sampling;
        setup.world.sampler = sampler;
        setup.world.light_sampling = light_sampling;
        setup.world.projection = projection;
        setup.world.shutter[0] = shutter[0]; setup.world.shutter[1] = shutter[1];
        setup.world.instance_motion = motion;
        for (int k = 0; k < 3; ++k) setup.world.motion[k] = motion_v[k];
        setup.world.motion[3] = motion_v[3] * (3.14159265358979323846 / 180.0);
        for (const auto& x : point_lights) setup.world.add_punctual(PointLight::new_(Vec3{x[0], x[1], x[2]}, Vec3{x[3], x[4], x[5]}));
        for (const auto& x : spot_lights) setup.world.add_punctual(SpotLight::new_(Vec3{x[0], x[1], x[2]}, Vec3{x[3], x[4], x[5]}, x[6], x[7], Vec3{x[8], x[9], x[10]}));
        for (const auto& x : suns) setup.world.add_punctual(DirectionalLight::new_(Vec3{x[0], x[1], x[2]}, Vec3{x[3], x[4], x[5]}));
        setup.world.punctual_fraction = punctual_fraction;
        setup.world.punctual_media = light_shafts;
        setup.world.punctual_selection = punctual_selection;
        for (int k = 0; k < 3; ++k) setup.world.punctual_grid[k] = punctual_grid[k];
        if (projection >= 2) setup.camera.defocus_angle = 0.0;   // the library refuses a lens there (pt_scene_set_projection's rule)
        if (mesh_light) {   // an emissive level-4 icosphere (5120 triangles), in the world and in the lights list
            auto ball = TriangleMesh::from_obj(1.0, icosphere(4, Vec3{mesh_light_v[0], mesh_light_v[1], mesh_light_v[2]}, mesh_light_v[3]),
                                               DiffuseLight::from_rgb(Vec3{mesh_light_v[4], mesh_light_v[5], mesh_light_v[6]}));
            setup.world.add_object(ball);
            setup.world.add_light(ball);
        }
        if (fog || smoke || isosurface) {
            const double inf = std::numeric_limits<double>::infinity();
            Vec3 lo{inf, inf, inf}, hi{-inf, -inf, -inf};
            setup.world.bounds(lo, hi);
            const Vec3 grow{0.005 * (hi.x - lo.x), 0.005 * (hi.y - lo.y), 0.005 * (hi.z - lo.z)};   // 1 % larger, about its centre
            lo = Vec3{lo.x - grow.x, lo.y - grow.y, lo.z - grow.z};
            hi = Vec3{hi.x + grow.x, hi.y + grow.y, hi.z + grow.z};
            if (isosurface) {
                add_isosurface(setup.world, ctx, isosurface_v, lo, hi, simplify ? simplify_n : 0u, simplify_placement);
            } else if (fog) {
                auto vol = HomogeneousVolume::from_albedo(Cuboid::new_(lo, hi, nullptr), fog_v[0], Vec3{fog_v[1], fog_v[2], fog_v[3]}, fog_v[4]);
                setup.world.add_object(vol);
                const Vec3 c = setup.camera.look_from;
                if (c.x > lo.x && c.x < hi.x && c.y > lo.y && c.y < hi.y && c.z > lo.z && c.z < hi.z) setup.world.camera_medium = vol;
            } else {   // no boundary: the density is 0 outside the box, so the grid serves as the medium of all space
                constexpr uint32_t N = 64;
                std::vector<float> v((size_t)N * N * N);
                for (uint32_t k = 0; k < N; ++k)
                    for (uint32_t j = 0; j < N; ++j)
                        for (uint32_t i = 0; i < N; ++i) v[((size_t)k * N + j) * N + i] = (float)smoke_plume((i + 0.5) / N, (j + 0.5) / N, (k + 0.5) / N);
                setup.world.camera_medium = HeterogeneousVolume::from_grid(nullptr, smoke_v[0], Vec3{smoke_v[1], smoke_v[2], smoke_v[3]}, smoke_v[4], N, N, N, std::move(v), lo, hi);
            }
        }
        setup.world.glass_dispersion = dispersion;
        if (interior)
            setup.world.glass_interior = HomogeneousVolume::tinted(nullptr, interior_v[0], Vec3{interior_v[1], interior_v[2], interior_v[3]}, interior_v[4],
                                                                   Vec3{interior_v[5], interior_v[6], interior_v[7]});
        setup.world.build_bvh(ctx, setup.camera.environment.is_map ? setup.camera.environment.map : nullptr);
        setup.camera.init();
        setup.camera.film = film;
        setup.camera.print_stats = stats;
        std::cerr << "rendering production\n";   // camera.rs:101
        if (use_adaptive) {
            const uint32_t m = (uint32_t)std::max(2L, std::min(min_spp, (long)s));
            setup.camera.render_adaptive(setup.world, out.empty() ? setup.output : out, adaptive, m, seed);
        } else if (use_denoise) {
            setup.camera.render_denoised(setup.world, out.empty() ? setup.output : out, (uint32_t)aov_spp, seed);
        } else {
            setup.camera.render(setup.world, out.empty() ? setup.output : out, seed);
        }
        setup.world.release();
    } catch (const std::exception& e) {
        std::cerr << "panic: " << e.what() << "\n";   // the reference unwrap()s asset errors
        pt_ctx_destroy(ctx);
        return 101;
    }
    pt_ctx_destroy(ctx);
    return 0;
}
