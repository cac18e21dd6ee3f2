// The scene graph and the flattener (csrc/pt_graph.cpp, csrc/pt_flatten.cpp) as a stand-alone program, for a run under the host sanitizers:
//   P=thu-acg-f2024-path-tracer_amd; g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/scene_host_check.cpp $P/csrc/pt_error.cpp $P/csrc/pt_graph.cpp $P/csrc/pt_flatten.cpp $P/csrc/pt_assets.cpp $P/csrc/pt_jpeg.cpp \
//       $P/host/scenes.cpp -lz -o scene_host_check && ./scene_host_check assets
// It flattens the seven built-in scenes (through pt_build_scene, on a stack pt_scene) and hand-made graphs at the smallest shapes where the
// flattener can go wrong, checks the structure of every result (child references, triangle ranges, leaf order, primitive indices, the
// walk order, stack depth, f32 boxes around f64 boxes), prints one FNV checksum per scene (pt::flat_checksum, the number the library prints
// under PT_VERBOSE) and walks the refusals. No GPU, no Python: pt_world_build here is pt::flatten without a device builder, so the
// sanitizers see every load and store between the C ABI and the arrays the library would upload.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/pt_amd.h"
#include "../thu-acg-f2024-path-tracer_amd/csrc/pt_flatten.h"

using namespace pt;

static FlatScene g_flat;
static int g_breaches = 0;

// the library's two are in pt_scene_upload.cpp (they reach the device)
extern "C" int pt_world_build(pt_scene* s) {
    s->built = false;
    if (flatten(*s, nullptr, g_flat) != 0) return -1;
    finish_build(*s, g_flat);
    return 0;
}
extern "C" int pt_scene_set_punctual_fraction(pt_scene* s, double f) {
    s->punctual_f = f;
    return 0;
}

static void breach(const char* scene, const char* what) {
    printf("BREACH %s: %s\n", scene, what);
    ++g_breaches;
}
// the triangles (positions in `tris`) below `ref`, and the deepest level; false on a reference out of range
static bool walk(const FlatScene& f, uint32_t ref, int depth, int& deepest, std::vector<uint32_t>* leaves, std::vector<uint32_t>* entries) {
    deepest = std::max(deepest, depth);
    if (depth > 64) return false;
    const uint32_t type = ref & REF_TYPE_MASK;
    if (type == REF_TRIS) {
        const uint32_t first = ref & 0x07FFFFFFu, count = ((ref >> 27) & 7u) + 1u;
        if ((uint64_t)first + count > f.tris.size() || !leaves) return false;
        for (uint32_t k = 0; k < count; ++k) leaves->push_back(first + k);
        return true;
    }
    if (type == REF_ENTRY) {
        if ((ref & ~REF_TYPE_MASK) >= f.entries.size() || !entries) return false;
        entries->push_back(ref & ~REF_TYPE_MASK);
        return true;
    }
    if (type != REF_NODE || ref >= f.nodes.size()) return false;
    return walk(f, f.nodes[ref].child0, depth + 1, deepest, leaves, entries) && walk(f, f.nodes[ref].child1, depth + 1, deepest, leaves, entries);
}
static bool is_permutation(std::vector<uint32_t> v) {
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] != i) return false;
    return true;
}
static void check(const char* name, const pt_scene& s) {
    const FlatScene& f = g_flat;
    const size_t n = f.entries.size();
    int top_depth = 0, mesh_depth = 0;
    std::vector<uint32_t> reached;
    if (!walk(f, f.tlas_root, 0, top_depth, nullptr, &reached) || reached.size() != n || !is_permutation(reached)) breach(name, "the top level does not reach every entry once");
    for (const Entry& e : f.entries) {
        if ((uint64_t)e.first_prim + e.n_prims > f.prims.size()) breach(name, "an entry's primitives lie outside prims");
        if (e.inst >= (int32_t)f.insts.size()) breach(name, "an entry's instance is out of range");
        if (e.kind != ENTRY_MESH) continue;
        std::vector<uint32_t> leaves, faces;
        int d = 0;
        if (!walk(f, e.blas_root, 0, d, &leaves, nullptr)) { breach(name, "a mesh tree holds a reference out of range"); continue; }
        mesh_depth = std::max(mesh_depth, d);
        for (uint32_t pos : leaves) faces.push_back(f.tri_gid[pos]);
        if (faces.size() != e.n_prims || !is_permutation(faces)) breach(name, "a mesh's leaf order is no permutation of its faces");
    }
    if (top_depth > f.tlas_depth || mesh_depth > f.max_blas_depth || f.tlas_depth + 1 + f.max_blas_depth + 1 > TRAVERSAL_STACK || s.stack_need > (uint32_t)TRAVERSAL_STACK ||
        s.stack_need_extend2 > s.stack_need)
        breach(name, "the trees are deeper than recorded or than the traversal stack");
    for (const PrimRef& p : f.prims) {
        const uint32_t k = p.kind & 0xFFu;
        const size_t limit = k == PRIM_SPHERE ? f.spheres.size() : k == PRIM_QUAD ? f.quads.size() : k == PRIM_TRI ? f.tris.size() : 0;
        if (p.index >= limit || p.mat >= f.mats.size() || p.inst >= (int32_t)f.insts.size()) breach(name, "a PrimRef is out of range");
    }
    for (uint32_t l : f.lights)
        if (l >= n) breach(name, "a light is no entry");
    if (f.tri_gid.size() != f.tris.size() || (f.any_attr && f.tri_attr.size() != f.tris.size()) || f.inst_motion.size() != f.insts.size() || f.entry_box.size() != n ||
        f.cuboid_box.size() != n || s.entry_at.size() != n || s.entry_boxes.size() != 6 * n || s.entry_shadeable.size() != n)
        breach(name, "parallel arrays differ in length");
    else if (!is_permutation(s.entry_at)) breach(name, "entry_at is no permutation");
    else
        for (size_t i = 0; i < n; ++i) {
            const EntryBox& eb = f.entry_box[s.entry_at[i]];
            const double* b = &s.entry_boxes[6 * i];
            bool inside = eb.entry == i;
            for (int a = 0; a < 3; ++a) inside = inside && (double)eb.lo[a] <= b[a] && (double)eb.hi[a] >= b[3 + a];
            if (!inside) breach(name, "an entry's f32 box does not hold its f64 box");
        }
    printf("scene %s: %zu entries, %zu prims, %zu nodes, flat %u, checksum %016llx\n", name, n, f.prims.size(), f.nodes.size(), f.tlas_flat, (unsigned long long)flat_checksum(f));
}
static void build(const char* name, pt_scene& s) {
    if (pt_world_build(&s) != 0) {
        printf("unexpected refusal of %s: %s\n", name, pt_last_error());
        ++g_breaches;
    } else check(name, s);
}
static void refused(const char* name, pt_scene& s) {
    if (pt_world_build(&s) == 0) breach(name, "built, but must be refused");
    else printf("refused %s: %s\n", name, pt_last_error());
}

// ---- hand-made graphs -----------------------------------------------------------------------------------------------------------------------
static int grey(pt_scene& s) { return pt_mat_diffuse(&s, pt_tex_solid_rgb(&s, 0.5, 0.5, 0.5), -1); }
static int sphere(pt_scene& s, double x, double r, int mat) {
    const double p[3] = {x, 0.25 * x, -x};
    return pt_sphere(&s, r, p, p, mat);
}
static int strip(pt_scene& s, uint32_t n_tris, int mat, bool attrs = false) {   // a zigzag strip: n_tris + 2 vertices
    std::vector<float> pos, nrm, uv;
    std::vector<uint32_t> idx;
    for (uint32_t j = 0; j < n_tris + 2; ++j) {
        pos.insert(pos.end(), {0.5f * j, (float)(j & 1u), 0.1f * j});
        nrm.insert(nrm.end(), {0.0f, 0.0f, 1.0f});
        uv.insert(uv.end(), {0.1f * j, (float)(j & 1u)});
    }
    for (uint32_t k = 0; k < n_tris; ++k) idx.insert(idx.end(), {k, k + 1, k + 2});
    const uint32_t nv = attrs ? n_tris + 2 : 0;
    return pt_mesh(&s, 1.5, n_tris + 2, pos.data(), (uint32_t)idx.size(), idx.data(), nv, nrm.data(), nv, uv.data(), mat);
}
static const double AXIS[3] = {0.0, 1.0, 0.0}, T0[3] = {1.0, 2.0, 3.0}, T1[3] = {-2.0, 2.5, 3.0};
static void add(pt_scene& s, int obj, bool light = false) {
    if (obj < 0 || (light ? pt_world_add_light(&s, obj) : pt_world_add_object(&s, obj)) != 0) {
        printf("unexpected graph error: %s\n", pt_last_error());
        ++g_breaches;
    }
}
static void hand_made() {
    { pt_scene s; add(s, sphere(s, 1.0, 0.5, grey(s))); build("one-sphere", s); }
    { pt_scene s; add(s, strip(s, 1, grey(s))); build("one-triangle", s); }
    { pt_scene s; add(s, strip(s, 5, grey(s), true)); build("five-triangles", s); }
    {   // one mesh object placed three times, once also as a light
        pt_scene s;
        const int m = strip(s, 9, pt_mat_light(&s, pt_tex_solid_rgb(&s, 4.0, 4.0, 4.0)));
        const int i1 = pt_instance(&s, m, AXIS, 0.7, T0), i2 = pt_instance(&s, i1, AXIS, -0.3, T1);
        add(s, m); add(s, i1); add(s, i2); add(s, i1, true);
        build("shared-mesh", s);
    }
    {   // a translating-only instance of a mesh, and a spinning one
        pt_scene s;
        const int m = strip(s, 6, grey(s));
        add(s, pt_instance_moving(&s, m, AXIS, 0.4, 0.4, T0, T1)); add(s, pt_instance_moving(&s, m, AXIS, 0.0, 1.1, T0, T1));
        build("moving-mesh", s);
    }
    {
        pt_scene s;
        const double a[3] = {0.0, 0.0, 0.0}, b[3] = {1.0, 2.0, 3.0};
        add(s, pt_instance(&s, pt_cuboid(&s, a, b, grey(s)), AXIS, 0.5, T0));
        build("cuboid-instance", s);
    }
    for (uint32_t n : {TLAS_FLAT_MAX, TLAS_FLAT_MAX + 1}) {   // both top-level forms
        pt_scene s;
        const int mat = grey(s);
        for (uint32_t i = 0; i < n; ++i) add(s, sphere(s, 1.0 + 2.0 * i, 0.75, mat));
        build(n == TLAS_FLAT_MAX ? "flat-top-level" : "tree-top-level", s);
        if (g_flat.tlas_flat != (n == TLAS_FLAT_MAX ? 1u : 0u)) breach("top-level", "the flat walk's threshold moved");
    }
    {   // a checker of two solids, a checker of an image
        pt_scene s;
        const uint8_t px[12] = {255, 0, 0, 0, 255, 0, 0, 0, 255, 9, 9, 9};
        const int a = pt_tex_solid_rgb(&s, 0.1, 0.2, 0.3), b = pt_tex_solid_rgb(&s, 0.9, 0.8, 0.7), img = pt_tex_image_rgb8(&s, 2, 2, px);
        add(s, sphere(s, 1.0, 0.5, pt_mat_diffuse(&s, pt_tex_checker(&s, 0.3, a, b), -1)));
        add(s, sphere(s, 3.0, 0.5, pt_mat_diffuse(&s, pt_tex_checker(&s, 0.3, img, b), -1)));
        build("checkers", s);
    }
    {
        pt_scene s;
        const int d = grey(s), m = pt_mat_metal(&s, pt_tex_solid_rgb(&s, 0.9, 0.9, 0.9), pt_tex_solid_f(&s, 0.1));
        add(s, sphere(s, 1.0, 0.5, pt_mat_mix(&s, 0.5, pt_mat_mix(&s, 0.25, d, m), pt_mat_mix(&s, 0.75, m, d))));
        build("mix-of-mixes", s);
    }
    {
        pt_scene s;
        const double absorb[3] = {0.1, 0.5, 1.0};
        const int med = pt_mat_medium_tinted(&s, 0.2, 0.9, 0.9, 0.9, 0.0, absorb), glass = pt_mat_glass(&s, pt_tex_solid_rgb(&s, 1.0, 1.0, 1.0), pt_tex_solid_f(&s, 0.0), 0.0, 1.5);
        if (pt_mat_glass_set_interior(&s, glass, med) != 0) ++g_breaches;
        add(s, sphere(s, 1.0, 0.5, glass));
        build("glass-interior", s);
    }
    {
        pt_scene s;
        const float vals[12] = {0.0f, 1.0f, 0.5f, 0.25f, 2.0f, 0.0f, 0.0f, 1.5f, 0.75f, 0.1f, 0.2f, 0.3f};
        const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 2.0, 3.0};
        add(s, pt_cuboid(&s, lo, hi, pt_mat_medium_grid(&s, 0.5, 0.8, 0.8, 0.8, 0.2, 2, 3, 2, vals, lo, hi)));
        add(s, sphere(s, 4.0, 0.5, grey(s)));
        build("grid-medium", s);
    }
    for (int given = 0; given < 2; ++given) {   // three punctual lights under grid selection
        pt_scene s;
        add(s, sphere(s, 1.0, 0.5, grey(s))); add(s, sphere(s, 6.0, 1.5, grey(s)));
        const double pos[3] = {0.0, 5.0, 0.0}, to[3] = {1.0, 0.0, 1.0}, down[3] = {0.0, -1.0, 0.0}, c[3] = {10.0, 10.0, 10.0};
        if (pt_light_point(&s, pos, c) < 0 || pt_light_spot(&s, pos, to, 10.0, 20.0, c) < 0 || pt_light_directional(&s, down, c) < 0 || pt_scene_set_punctual_selection(&s, 1) != 0 ||
            (given && pt_scene_set_punctual_grid(&s, 3, 2, 4, nullptr) != 0))
            ++g_breaches;
        build(given ? "light-grid-given" : "light-grid-auto", s);
        if (g_flat.grid.cells == 0u || s.grid_built.cells != g_flat.grid.cells || (given && g_flat.grid.cells != 24u)) breach("light-grid", "the grid is not in effect as set");
    }
}
static void refusals() {
    { pt_scene s; refused("empty-world", s); }
    { pt_scene s; add(s, pt_mesh(&s, 1.0, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, grey(s))); refused("empty-mesh", s); }
    {
        pt_scene s;
        int o = sphere(s, 1.0, 0.5, grey(s));
        for (int k = 0; k < 66; ++k) o = pt_instance(&s, o, AXIS, 0.01, T0);
        add(s, o);
        refused("deep-chain", s);
    }
    for (int over = 0; over < 2; ++over) {   // a light grid over an infinite box; a table over 2^25 entries
        pt_scene s;
        add(s, sphere(s, 1.0, over ? 0.5 : std::numeric_limits<double>::infinity(), grey(s)));
        const double pos[3] = {0.0, 5.0, 0.0}, c[3] = {1.0, 1.0, 1.0};
        for (int k = 0; k < (over ? 129 : 1); ++k)
            if (pt_light_point(&s, pos, c) < 0) ++g_breaches;
        if (pt_scene_set_punctual_selection(&s, 1) != 0 || (over && pt_scene_set_punctual_grid(&s, 64, 64, 64, nullptr) != 0)) ++g_breaches;
        refused(over ? "grid-table-too-large" : "grid-infinite-box", s);
        if (over) {   // the setting corrected: the same graph builds
            if (pt_scene_set_punctual_grid(&s, 4, 4, 4, nullptr) != 0) ++g_breaches;
            build("grid-corrected", s);
        }
    }
}

int main(int argc, char** argv) {
    const char* assets = argc > 1 ? argv[1] : "assets";
    for (int id = 1; id <= 7; ++id) {
        pt_scene s;
        pt_camera cam;
        const std::string name = "builtin-" + std::to_string(id);
        if (pt_build_scene(&s, id, 480, 16, assets, 1, &cam) != 0) {
            printf("unexpected refusal of %s: %s\n", name.c_str(), pt_last_error());
            return 1;
        }
        check(name.c_str(), s);
    }
    hand_made();
    refusals();
    printf("scene_host_check: %d breaches\n", g_breaches);
    return g_breaches == 0 ? 0 : 1;
}
