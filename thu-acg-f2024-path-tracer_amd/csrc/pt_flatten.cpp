// The flattener and the BVH builder (host-only). See pt_flatten.h.
#include "pt_flatten.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

using namespace pt;
using namespace pt::host;

// ----------------------------------------------------------------------------------------
// BVH builder: top-down binned SAH (16 bins) over item boxes, depth-limited (falls back to
// object-median splits when the remaining depth budget is tight) so that the traversal
// kernel's LDS stack (TRAVERSAL_STACK levels) can never overflow. The reference's O(n^2)
// full-sweep SAH (bvh.rs:54-120) is NOT reproduced: closest-hit results do not depend on the
// tree, only on the canonical tie rule both sides share.
// ----------------------------------------------------------------------------------------
namespace {
struct BuildItem {
    Box box;
    D3 c;
    uint32_t ref_payload;   // original index
};
struct Builder {
    std::vector<BvhNode>& nodes;
    std::vector<BuildItem>& items;
    int leaf_max, max_depth;
    bool tri_leaves;                       // leaf = REF_TRIS range, else REF_ENTRY single
    std::vector<uint32_t>* order;          // BLAS: output permutation (leaf order)
    uint32_t leaf_base = 0;                // BLAS: index of this mesh's first triangle in the global array
    int depth_reached = 0;
    int n_bins = 16;                       // SAH bins per axis (<= MAX_BINS)
    size_t sweep_below = 0;                // ranges of at most this many items are split by the exact SAH sweep (every split position of every axis)
    static constexpr int MAX_BINS = 64;

    static float down(double v) {
        float f = (float)v;
        if ((double)f > v) f = std::nextafterf(f, -INFINITY);
        return f;
    }
    static float up(double v) {
        float f = (float)v;
        if ((double)f < v) f = std::nextafterf(f, INFINITY);
        return f;
    }
    static void store_box(const Box& b, float* lo, float* hi) {
        // pad, then round outward to f32: strictly conservative for the f64 slab test
        double m = 1e-3;
        const double v[6] = {b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z};
        for (double x : v) m = std::fmax(m, std::fabs(x));
        double pad = 1e-7 * m;
        lo[0] = down(b.lo.x - pad); lo[1] = down(b.lo.y - pad); lo[2] = down(b.lo.z - pad);
        hi[0] = up(b.hi.x + pad); hi[1] = up(b.hi.y + pad); hi[2] = up(b.hi.z + pad);
    }
    static double axis_of(D3 v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; }

    uint32_t make_leaf(size_t begin, size_t end) {
        if (tri_leaves) {
            uint32_t first = leaf_base + (uint32_t)order->size();
            for (size_t i = begin; i < end; ++i) order->push_back(items[i].ref_payload);
            return REF_TRIS | ((uint32_t)(end - begin - 1) << 27) | first;
        }
        return REF_ENTRY | items[begin].ref_payload;
    }
    // returns child reference; `out_box` = bounds of the subtree
    uint32_t build(size_t begin, size_t end, int depth, Box& out_box) {
        depth_reached = std::max(depth_reached, depth);
        Box box, cbox;
        for (size_t i = begin; i < end; ++i) { box.grow(items[i].box); cbox.grow(items[i].c); }
        out_box = box;
        const size_t n = end - begin;
        if (n <= (size_t)leaf_max) return make_leaf(begin, end);
        // depth budget: levels still needed with perfect median splits
        int needed = 0;
        for (size_t cap = (size_t)leaf_max; cap < n; cap *= 2) ++needed;
        const bool force_median = needed >= max_depth - depth;
        D3 ext = cbox.hi - cbox.lo;
        int axis = ext.x >= ext.y && ext.x >= ext.z ? 0 : (ext.y >= ext.z ? 1 : 2);
        size_t mid = begin + n / 2;
        bool done = false;
        if (!force_median && n <= sweep_below) {
            // exact sweep: the items sorted along each axis, every position between two neighbours a candidate
            double best_cost = INFINITY;
            int best_axis = -1;
            size_t best_pos = 0;
            std::vector<BuildItem> tmp(items.begin() + begin, items.begin() + end);
            std::vector<double> right_area(n);
            for (int a = 0; a < 3; ++a) {
                std::stable_sort(tmp.begin(), tmp.end(), [&](const BuildItem& x, const BuildItem& y) { return axis_of(x.c, a) < axis_of(y.c, a); });
                Box acc;
                for (size_t i = n; i-- > 1;) { acc.grow(tmp[i].box); right_area[i] = acc.half_area(); }
                acc = Box();
                for (size_t i = 0; i + 1 < n; ++i) {
                    acc.grow(tmp[i].box);
                    const double cost = acc.half_area() * (double)(i + 1) + right_area[i + 1] * (double)(n - i - 1);
                    if (cost < best_cost) { best_cost = cost; best_axis = a; best_pos = i + 1; }
                }
            }
            if (best_axis >= 0) {
                std::stable_sort(items.begin() + begin, items.begin() + end,
                                 [&](const BuildItem& x, const BuildItem& y) { return axis_of(x.c, best_axis) < axis_of(y.c, best_axis); });
                mid = begin + best_pos;
                done = true;
            }
        }
        if (!force_median && !done) {
            const int NB = n_bins;
            double best_cost = INFINITY;
            int best_axis = -1, best_bin = -1;
            for (int a = 0; a < 3; ++a) {
                double lo = axis_of(cbox.lo, a), hi = axis_of(cbox.hi, a);
                if (!(hi > lo)) continue;
                Box bb[MAX_BINS];
                size_t bc[MAX_BINS] = {0};
                double k = (double)NB / (hi - lo);
                for (size_t i = begin; i < end; ++i) {
                    int b = (int)((axis_of(items[i].c, a) - lo) * k);
                    b = std::min(std::max(b, 0), NB - 1);
                    bb[b].grow(items[i].box);
                    ++bc[b];
                }
                Box right_acc[MAX_BINS];
                size_t right_cnt[MAX_BINS];
                Box acc;
                size_t cnt = 0;
                for (int b = NB - 1; b > 0; --b) {
                    acc.grow(bb[b]);
                    cnt += bc[b];
                    right_acc[b] = acc;
                    right_cnt[b] = cnt;
                }
                acc = Box();
                cnt = 0;
                for (int b = 0; b < NB - 1; ++b) {
                    acc.grow(bb[b]);
                    cnt += bc[b];
                    if (cnt == 0 || right_cnt[b + 1] == 0) continue;
                    double cost = acc.half_area() * (double)cnt + right_acc[b + 1].half_area() * (double)right_cnt[b + 1];
                    if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = b; }
                }
            }
            if (best_axis >= 0) {
                double lo = axis_of(cbox.lo, best_axis), hi = axis_of(cbox.hi, best_axis);
                double k = (double)NB / (hi - lo);
                auto it = std::stable_partition(items.begin() + begin, items.begin() + end, [&](const BuildItem& it_) {
                    int b = (int)((axis_of(it_.c, best_axis) - lo) * k);
                    b = std::min(std::max(b, 0), NB - 1);
                    return b <= best_bin;
                });
                mid = (size_t)(it - items.begin());
                done = mid > begin && mid < end;
            }
        }
        if (!done) {
            mid = begin + n / 2;
            std::stable_sort(items.begin() + begin, items.begin() + end,
                             [&](const BuildItem& a, const BuildItem& b) { return axis_of(a.c, axis) < axis_of(b.c, axis); });
        }
        uint32_t me = (uint32_t)nodes.size();
        nodes.emplace_back();
        Box lb, rb;
        uint32_t l = build(begin, mid, depth + 1, lb);
        uint32_t r = build(mid, end, depth + 1, rb);
        BvhNode& nd = nodes[me];
        store_box(lb, nd.lo0, nd.hi0);
        store_box(rb, nd.lo1, nd.hi1);
        nd.child0 = l;
        nd.child1 = r;
        nd.pad0 = nd.pad1 = 0;
        return REF_NODE | me;
    }
};
// max |coordinate| of a subtree's bounds, as the f32 slab test's error margin needs it: padded like
// the stored boxes and rounded up
float box_extent(const Box& b) {
    double m = 1e-3;
    const double v[6] = {b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z};
    for (double x : v) m = std::fmax(m, std::fabs(x));
    return std::nextafterf((float)(m * 1.000001), INFINITY);
}
Box sphere_box(const SphereD& s) {
    Box b;
    D3 r{s.r, s.r, s.r};
    b.grow(d3(s.p1) - r); b.grow(d3(s.p1) + r);
    b.grow(d3(s.p2) - r); b.grow(d3(s.p2) + r);
    return b;
}
Box quad_box(const QuadD& q) {
    Box b;
    D3 o = d3(q.q), u = d3(q.u), v = d3(q.v);
    b.grow(o); b.grow(o + u); b.grow(o + v); b.grow(o + u + v);
    return b;
}
struct SharedBlas {   // one tree and one triangle range per MESH OBJECT, however many placements it has
    uint32_t root, tri_base;
    float extent;
    Box local;
    std::vector<uint32_t> face_pos;   // face -> position in BLAS (leaf) order
    int depth = 0;                    // of the tree
    uint32_t cdf_ofs = 0xFFFFFFFFu;   // its area table in light_cdf, once a placement of it is a light
};
struct Flattening {   // one run: the graph, the result, and what the steps hand each other
    pt_scene& s;
    const BlasHook& device_blas;
    FlatScene& f;
    std::map<int, SharedBlas> blas_of;
    std::vector<BuildItem> tlas_items;   // item i is entry i, until build_top_level permutes them
    std::vector<Box> entry_boxes;        // the f64 world box of every entry (order_entries)
};

// ---- place_entries: one Entry per placement, its primitives, its world box --------------------------------------------------------------
// The placement's instance chain, outermost first, down to the object it finally wraps: that object's index, or -1 with the error set
int instance_chain(Flattening& w, int oi, std::vector<int>& chain) {
    FlatScene& f = w.f;
    for (int guard = 0; w.s.objs[oi].kind == OBJ_INSTANCE; ++guard) {
        if (guard > 64) return set_error("pt_world_build: instance chain too deep");
        chain.push_back((int)f.insts.size());
        f.insts.push_back(w.s.objs[oi].xf);
        f.inst_motion.push_back(w.s.objs[oi].motion);
        f.any_moving = f.any_moving || w.s.objs[oi].motion.moves != 0u;
        oi = w.s.objs[oi].child;
    }
    for (size_t k = 0; k < chain.size(); ++k) {
        f.insts[chain[k]].outer = k == 0 ? -1 : chain[k - 1];
        f.insts[chain[k]].inner = k + 1 < chain.size() ? chain[k + 1] : -1;
    }
    return oi;
}
// A large mesh: depth-bounded LBVH through the hook (pt_bvh_device.hip); true when it built the tree. Only a HIP failure — or no hook —
// leaves the mesh to the host builder.
bool device_tree(Flattening& w, const HostObj& o, int leaf_max, SharedBlas& sb, std::vector<uint32_t>& perm) {
    pt_scene& s = w.s;
    if (!w.device_blas || s.device_bvh_min_tris == 0 || o.tris.size() < s.device_bvh_min_tris) return false;
    DeviceBlas db;
    const double lo[3] = {sb.local.lo.x, sb.local.lo.y, sb.local.lo.z}, hi[3] = {sb.local.hi.x, sb.local.hi.y, sb.local.hi.z};
    // depth budget: eight levels above a perfectly balanced tree — the radix tree of 1.3 M triangles comes out 27 deep, and
    // every level the bound takes away bends Morton splits (measured on that mesh, K2 per launch: 27 levels 1.78 ms,
    // 23: 1.83, 21: 2.19, 20: 2.50; the host's SAH tree 1.50) — within what the traversal stacks cover (k_extend2's
    // largest LDS stack holds 32 entries; TRAVERSAL_STACK bounds top level + mesh tree)
    int bal = 0;
    for (size_t cap = (size_t)leaf_max; cap < o.tris.size(); cap *= 2) ++bal;
    int dev_depth = std::min(29, std::max((int)MAX_BLAS_DEPTH, bal + 8));
    if (const char* ev = exp_env("PT_LBVH_DEPTH")) dev_depth = std::min(29, std::max(bal, atoi(ev)));
    uint32_t median_below = 0;
    if (const char* ev = exp_env("PT_LBVH_MEDIAN")) median_below = (uint32_t)atoi(ev);
    if (!w.device_blas(o.tris.data(), (uint32_t)o.tris.size(), lo, hi, (uint32_t)leaf_max, (uint32_t)dev_depth, median_below, db)) return false;
    const uint32_t node_base = (uint32_t)w.f.nodes.size();
    auto fix = [&](uint32_t ref) {
        if ((ref & REF_TYPE_MASK) == REF_NODE) return REF_NODE | (node_base + ref);
        return (ref & ~0x07FFFFFFu) | (sb.tri_base + (ref & 0x07FFFFFFu));     // REF_TRIS: count bits kept
    };
    for (BvhNode nd : db.nodes) {
        nd.child0 = fix(nd.child0);
        nd.child1 = fix(nd.child1);
        w.f.nodes.push_back(nd);
    }
    sb.root = REF_NODE | node_base;
    perm = db.order;
    sb.depth = db.depth;
    ++s.n_device_blas;
    s.device_blas_depth = std::max<uint32_t>(s.device_blas_depth, (uint32_t)db.depth);
    return true;
}
// The tree and the triangle range of mesh object `oi`, built at its first placement; null with the error set
SharedBlas* shared_blas_of(Flattening& w, int oi, const HostObj& o) {
    FlatScene& f = w.f;
    auto it = w.blas_of.find(oi);
    if (it != w.blas_of.end()) return &it->second;
    std::vector<BuildItem> items(o.tris.size());
    SharedBlas sb;
    for (size_t i = 0; i < o.tris.size(); ++i) {
        Box b;
        b.grow(d3(o.tris[i].v0)); b.grow(d3(o.tris[i].v1)); b.grow(d3(o.tris[i].v2));
        items[i] = BuildItem{b, b.centroid(), (uint32_t)i};
        sb.local.grow(b);
    }
    std::vector<uint32_t> perm;
    sb.tri_base = (uint32_t)f.tris.size();
    if ((size_t)sb.tri_base + o.tris.size() > 0x07FFFFFFu) {
        set_error("pt_world_build: too many triangles");
        return nullptr;
    }
    int leaf_max = 4;   // PT_LEAF_MAX: experiments only (smaller leaves were slower on scene 6)
    if (const char* ev = exp_env("PT_LEAF_MAX")) leaf_max = std::min(8, std::max(1, atoi(ev)));
    Box bb = sb.local;
    if (!device_tree(w, o, leaf_max, sb, perm)) {
        Builder bl{f.nodes, items, leaf_max, MAX_BLAS_DEPTH, true, &perm, sb.tri_base};
        if (const char* ev = exp_env("PT_SAH_BINS")) bl.n_bins = std::min((int)Builder::MAX_BINS, std::max(2, atoi(ev)));
        if (const char* ev = exp_env("PT_SAH_SWEEP")) bl.sweep_below = (size_t)std::max(0, atoi(ev));
        sb.root = bl.build(0, items.size(), 0, bb);
        sb.depth = bl.depth_reached;
    }
    f.max_blas_depth = std::max(f.max_blas_depth, sb.depth);
    sb.extent = box_extent(bb);
    sb.face_pos.resize(perm.size());
    for (size_t k = 0; k < perm.size(); ++k) {
        const uint32_t face = perm[k];
        sb.face_pos[face] = (uint32_t)k;
        f.tris.push_back(o.tris[face]);
        f.tri_gid.push_back(face);                 // face index inside the mesh; the kernels add Entry::first_prim
        if (f.any_attr) f.tri_attr.push_back(o.tri_attr.empty() ? TriAttr{} : o.tri_attr[face]);
    }
    return &w.blas_of.emplace(oi, std::move(sb)).first->second;
}
// Exact light sampling's table of a light mesh (the rule in pt_amd.h), built whatever the kind: C[0] = 0, C[i + 1] = C[i] + A_i in face order,
// A_i = 0.5 |cross(v1 - v0, v2 - v0)| of the local-space vertices — instance chains are rigid, so every placement shares it. 0, or -1.
int light_table(Flattening& w, SharedBlas& sb, const HostObj& o) {
    pt_scene& s = w.s;
    std::vector<double>& light_cdf = w.f.light_cdf;
    if (sb.cdf_ofs == 0xFFFFFFFFu) {
        if (light_cdf.size() + o.tris.size() + 1 > 0xFFFFFFF0ull) return set_error("pt_world_build: too many light triangles");
        sb.cdf_ofs = (uint32_t)light_cdf.size();
        double c = 0.0;
        light_cdf.push_back(c);
        for (const TriD& t : o.tris) {
            const D3 v0 = d3(t.v0);
            c = c + 0.5 * length(cross(d3(t.v1) - v0, d3(t.v2) - v0));
            light_cdf.push_back(c);
        }
    }
    const double A = light_cdf[sb.cdf_ofs + o.tris.size()];
    s.light_mesh_bad_area = s.light_mesh_bad_area || !(A > 0.0 && std::isfinite(A));
    s.light_blas_depth = std::max<uint32_t>(s.light_blas_depth, (uint32_t)sb.depth);
    return 0;
}
// A mesh placement: its (shared) tree, its light table, one PrimRef per placed triangle. 0, or -1.
int place_mesh(Flattening& w, int oi, const HostObj& o, bool is_light, int inst, Entry& e, Box& local) {
    e.kind = ENTRY_MESH;
    if (o.tris.empty()) return set_error("pt_world_build: empty mesh");
    SharedBlas* sb = shared_blas_of(w, oi, o);
    if (!sb) return -1;
    if (is_light) {
        if (light_table(w, *sb, o) != 0) return -1;
        e.pad[0] = sb->cdf_ofs;
    }
    e.blas_root = sb->root;
    e.extent = sb->extent;
    local = sb->local;
    const uint32_t flags = PRIM_TRI | (o.has_normals ? PRIM_HAS_NORMALS : 0u) | (o.has_uvs ? PRIM_HAS_UVS : 0u);
    for (size_t face = 0; face < o.tris.size(); ++face)   // one PrimRef per PLACED triangle: ids are per placement
        w.f.prims.push_back(PrimRef{flags, sb->tri_base + sb->face_pos[face], (uint32_t)o.mat, inst});
    return 0;
}
// The world box of a placement from its object-space box: box of the box per instance (aabb.rs:50-76), a moving level by the box rule over
// [0, 1] (swept_box), and for meshes the two tighter rules below
Box world_box_of(const Flattening& w, const HostObj& o, const std::vector<int>& chain, const Box& local) {
    const FlatScene& f = w.f;
    Box world = local;
    bool chain_moves = false;
    for (size_t k = chain.size(); k-- > 0;) {
        const InstMotionD& mk = f.inst_motion[chain[k]];
        chain_moves = chain_moves || mk.moves != 0u;
        world = mk.moves ? swept_box(world, mk) : xform_box(world, f.insts[chain[k]]);
    }
    if (chain.size() == 1 && chain_moves && !f.inst_motion[chain[0]].spins && o.kind == OBJ_MESH) {
        // a mesh under ONE instance that translates only: the bounds of its transformed vertices at times 0 and 1, as below — every
        // vertex is R p + tr(t) with tr(t) monotone in t component by component, so the two ends hold every time in between
        InstD m0, m1;
        pose_of_keys(f.inst_motion[chain[0]], 0.0, m0);
        pose_of_keys(f.inst_motion[chain[0]], 1.0, m1);
        Box tight;
        for (const TriD& t : o.tris)
            for (const double* v : {t.v0, t.v1, t.v2}) {
                tight.grow(xform_point(d3(m0.c0), d3(m0.c1), d3(m0.c2), d3(m0.t), d3(v)));
                tight.grow(xform_point(d3(m1.c0), d3(m1.c1), d3(m1.c2), d3(m1.t), d3(v)));
            }
        world = tight;
    }
    if (!chain.empty() && o.kind == OBJ_MESH && !chain_moves) {
        // an instanced mesh gets the bounds of its TRANSFORMED VERTICES, not the box of its transformed box
        // (aabb.rs:50-76 does the latter): a mesh turned by ~50 degrees has a third less box to enter, and
        // every ray that enters costs a trip through the mesh pass. Any conservative box gives the same
        // closest hit; store_box pads by 1e-7 relative, far above the rounding of the transform.
        Box tight;
        for (const TriD& t : o.tris)
            for (const double* v : {t.v0, t.v1, t.v2}) {
                D3 p = d3(v);   // object space -> world: innermost instance first
                for (size_t k = chain.size(); k-- > 0;) {
                    const InstD& m = f.insts[chain[k]];
                    p = xform_point(d3(m.c0), d3(m.c1), d3(m.c2), d3(m.t), p);
                }
                tight.grow(p);
            }
        world = tight;
    }
    return world;
}
int place_entries(Flattening& w) {
    pt_scene& s = w.s;
    FlatScene& f = w.f;
    s.lights_have_mesh_or_sphere = s.light_mesh_bad_area = false;
    s.light_blas_depth = 0;
    for (auto& o : s.objs) f.any_attr = f.any_attr || !o.tri_attr.empty();
    // canonical global primitive ids: lights list first, then objects, insertion order
    std::vector<int> order = s.world_lights;
    order.insert(order.end(), s.world_objects.begin(), s.world_objects.end());
    if (order.empty()) return set_error("pt_world_build: the world is empty");
    s.n_device_blas = s.device_blas_depth = 0;
    for (size_t wi = 0; wi < order.size(); ++wi) {
        std::vector<int> chain;
        const int oi = instance_chain(w, order[wi], chain);
        if (oi < 0) return -1;
        const int inst = chain.empty() ? -1 : chain.front();
        const HostObj& o = s.objs[oi];
        const bool is_light = wi < s.world_lights.size();
        if (is_light) f.lights.push_back((uint32_t)f.entries.size());   // any hittable may be a light (world.rs:18-20)
        if (is_light && (o.kind == OBJ_MESH || o.kind == OBJ_SPHERE)) s.lights_have_mesh_or_sphere = true;
        Entry e{};
        memset(&e, 0, sizeof e);
        e.first_prim = (uint32_t)f.prims.size();
        e.inst = inst;
        e.blas_root = REF_EMPTY;
        Box local;
        switch (o.kind) {
        case OBJ_SPHERE:
            e.kind = ENTRY_SPHERE;
            f.prims.push_back(PrimRef{PRIM_SPHERE, (uint32_t)f.spheres.size(), (uint32_t)o.mat, inst});
            f.spheres.push_back(o.sphere);
            local = sphere_box(o.sphere);
            break;
        case OBJ_QUAD:
        case OBJ_CUBOID:
            e.kind = o.kind == OBJ_QUAD ? ENTRY_QUAD : ENTRY_CUBOID;
            for (const QuadD& q : o.quads) {
                f.prims.push_back(PrimRef{PRIM_QUAD, (uint32_t)f.quads.size(), (uint32_t)o.mat, inst});
                f.quads.push_back(q);
                local.grow(quad_box(q));
            }
            break;
        case OBJ_MESH:
            if (place_mesh(w, oi, o, is_light, inst, e, local) != 0) return -1;
            break;
        default:
            return set_error("pt_world_build: unsupported object kind");
        }
        e.n_prims = (uint32_t)f.prims.size() - e.first_prim;
        const Box world = world_box_of(w, o, chain, local);
        w.tlas_items.push_back(BuildItem{world, world.centroid(), (uint32_t)f.entries.size()});
        f.entries.push_back(e);
    }
    if (f.prims.size() >= (size_t)HIT_ID_MASK - 4) return set_error("pt_world_build: too many primitives (28-bit ids)");
    return 0;
}

// ---- mark_prims: the material's kind into every PrimRef, and what the world's materials put in effect ---------------------------------------
// PRIM_NEEDS_UV (pt_types.h): can this material read HitD::u / v? A normal map, an image texture in the colour texture's tree
// (through checker children), or a mix with such a child, at both nesting levels. An index out of range counts as "can".
bool tex_reads_uv(const pt_scene& s, int32_t t, int depth) {
    if (t < 0) return false;
    if ((size_t)t >= s.tex.size() || depth > 16) return true;
    const TexD& T = s.tex[t].d;
    if (T.kind == TEX_IMAGE || T.kind == TEX_IMAGE_F32) return true;
    return T.kind == TEX_CHECKER && (tex_reads_uv(s, (int32_t)T.t1, depth + 1) || tex_reads_uv(s, (int32_t)T.t2, depth + 1));
}
bool mat_reads_uv(const pt_scene& s, int32_t mi, int depth) {
    if (mi < 0 || (size_t)mi >= s.mats.size() || depth > 2) return true;   // (pt_mat_mix admits two levels)
    const MatD& m = s.mats[mi];
    if (m.nmap_tex >= 0) return true;
    if (m.kind == MAT_MIX) return mat_reads_uv(s, m.color_tex, depth + 1) || mat_reads_uv(s, m.rough_tex, depth + 1);   // (a mix keeps its children there)
    return tex_reads_uv(s, m.color_tex, 0);
}
void mark_prims(Flattening& w) {
    pt_scene& s = w.s;
    // (a medium's boundary sorts with glass — the other kind that sends the ray on — so that K2's result word keeps its classes: pt_types.h)
    s.world_has_medium = s.world_has_grid_medium = s.world_has_interior = s.world_has_dispersion = false;
    for (PrimRef& pr : w.f.prims) {
        const uint32_t kind = s.mats[pr.mat].kind;
        if ((pr.kind & 0xFFu) == PRIM_SPHERE && mat_reads_uv(s, (int32_t)pr.mat, 0)) pr.kind |= PRIM_NEEDS_UV;
        s.world_has_medium = s.world_has_medium || kind == MAT_MEDIUM;
        s.world_has_grid_medium = s.world_has_grid_medium || (kind == MAT_MEDIUM && s.mats[pr.mat].p[6] != 0.0);
        // a glass with an interior, or a tinted medium's boundary
        s.world_has_interior = s.world_has_interior || (kind == MAT_GLASS && s.mats[pr.mat].p[0] != 0.0) || (kind == MAT_MEDIUM && s.mats[pr.mat].p[10] != 0.0);
        s.world_has_dispersion = s.world_has_dispersion || (kind == MAT_GLASS && s.mats[pr.mat].p[3] != 0.0);   // a dispersive glass
        pr.kind |= (kind == MAT_MEDIUM ? MEDIUM_SORT_KIND : kind) << PRIM_MAT_KIND_SHIFT;
    }
}

// ---- pick_shadeable: the short-path pass's entries (pt_k_short.hip shades them itself) -----------------------------------
// a world-level sphere or quad, no instance chain, still, a diffuse material without a normal map (fetch_tex looks up whatever colour
// texture it has)
void pick_shadeable(Flattening& w) {
    pt_scene& s = w.s;
    const FlatScene& f = w.f;
    s.entry_shadeable.assign(f.entries.size(), 0);
    s.shade_prims.clear();
    s.shade_self_ok.clear();
    s.shade_entry.clear();
    for (size_t i = 0; i < f.entries.size(); ++i) {
        const Entry& e = f.entries[i];
        if ((e.kind != ENTRY_SPHERE && e.kind != ENTRY_QUAD) || e.inst >= 0 || e.n_prims != 1u) continue;
        const PrimRef& pr = f.prims[e.first_prim];
        const MatD& m = s.mats[pr.mat];
        if (pr.inst >= 0 || m.kind != MAT_DIFFUSE || m.nmap_tex >= 0) continue;
        if ((pr.kind & 0xFFu) == PRIM_SPHERE) {
            const SphereD& sp = f.spheres[pr.index];
            if (!(sp.p1[0] == sp.p2[0] && sp.p1[1] == sp.p2[1] && sp.p1[2] == sp.p2[2])) continue;
        } else if ((pr.kind & 0xFFu) != PRIM_QUAD) continue;
        s.entry_shadeable[i] = 1;
        s.shade_prims.push_back(e.first_prim);
        s.shade_entry.push_back((uint32_t)i);
        //  a quad whose numbers keep the proof's bound: finite, |coordinates| <= 1e6, the stored normal of unit length
        bool self_ok = (pr.kind & 0xFFu) == PRIM_QUAD;
        if (self_ok) {
            const QuadD& q = f.quads[pr.index];
            for (int a = 0; a < 3; ++a)
                for (double x : {q.q[a], q.q[a] + q.u[a], q.q[a] + q.v[a], q.q[a] + q.u[a] + q.v[a], q.n[a]}) self_ok = self_ok && std::fabs(x) <= 1e6;
            const double n2 = (q.n[0] * q.n[0] + q.n[1] * q.n[1]) + q.n[2] * q.n[2];
            self_ok = self_ok && std::fabs(q.d) <= 2e6 && std::fabs(n2 - 1.0) <= 1e-9;   // (a NaN fails every comparison)
        }
        s.shade_self_ok.push_back(self_ok ? 1 : 0);
    }
}

// ---- order_entries: the place of every entry in SceneD::entry_box, and the f64 boxes pt_world_entry_box hands out -----------------------------
void order_entries(Flattening& w) {
    pt_scene& s = w.s;
    const std::vector<Entry>& entries = w.f.entries;
    // the order the flat top level's loop runs in (walk_records: non-mesh entries first, each kind in entry order)
    s.entry_at.assign(entries.size(), 0);
    uint32_t at = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t i = 0; i < entries.size(); ++i)
            if ((entries[i].kind == ENTRY_MESH) == (pass == 1)) s.entry_at[i] = at++;
    w.entry_boxes.resize(w.tlas_items.size());
    for (const BuildItem& it : w.tlas_items) w.entry_boxes[it.ref_payload] = it.box;
    s.entry_boxes.clear();   // pt_world_entry_box: the f64 boxes, before the f32 rounding
    for (const Box& b : w.entry_boxes)
        for (double x : {b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z}) s.entry_boxes.push_back(x);
}

// ---- plan_light_grid: its box and dims are settled, and their refusals made, before the top level is built -------------------
int plan_light_grid(Flattening& w) {
    pt_scene& s = w.s;
    PunctualGridBuild& gb = w.f.grid;
    gb = PunctualGridBuild{};
    s.grid_built = gb;
    if (s.punctual_selection != 1 || s.punctual.empty()) return 0;
    const uint64_t n = s.punctual.size();
    if (s.grid_box_given) memcpy(gb.box, s.grid_box_set, sizeof gb.box);
    else {
        Box u;
        for (const Box& b : w.entry_boxes) { u.grow(b.lo); u.grow(b.hi); }
        const double ub[6] = {u.lo.x, u.lo.y, u.lo.z, u.hi.x, u.hi.y, u.hi.z};
        if (w.entry_boxes.empty() || !grid_box_ok(ub)) return set_error("pt_world_build: the light grid needs a finite box and the world's bounds are not finite: give one (pt_scene_set_punctual_grid)");
        memcpy(gb.box, ub, sizeof gb.box);
    }
    if (s.grid_dims_set[0] != 0u) {
        memcpy(gb.dims, s.grid_dims_set, sizeof gb.dims);
        if ((uint64_t)gb.dims[0] * gb.dims[1] * gb.dims[2] * n > PLT_GRID_MAX_ENTRIES)
            return set_error("pt_world_build: the light grid's table would hold more than 2^25 entries (cells x lights): take fewer cells (pt_scene_set_punctual_grid)");
    } else {
        const double ext[3] = {gb.box[3] - gb.box[0], gb.box[4] - gb.box[1], gb.box[5] - gb.box[2]};
        const double ext_max = std::max(ext[0], std::max(ext[1], ext[2]));
        for (uint32_t R = PLT_GRID_AUTO_RES;; R /= 2u) {
            for (int ax = 0; ax < 3; ++ax) {
                const double c = ext[ax] > 0.0 ? std::ceil((double)R * ext[ax] / ext_max) : 1.0;   // (the longest axis: exactly R)
                gb.dims[ax] = (uint32_t)(c < 1.0 ? 1.0 : (c > (double)R ? (double)R : c));
            }
            if ((uint64_t)gb.dims[0] * gb.dims[1] * gb.dims[2] * n <= PLT_GRID_MAX_ENTRIES || R == 1u) break;
        }
    }
    gb.cells = gb.dims[0] * gb.dims[1] * gb.dims[2];
    return 0;
}

// ---- build_top_level: the tree over world entries (one entry per leaf) -------------------------------------------------------------------
int build_top_level(Flattening& w) {
    FlatScene& f = w.f;
    Builder tl{f.nodes, w.tlas_items, 1, MAX_TLAS_DEPTH, false, nullptr};
    Box wb;
    f.tlas_root = tl.build(0, w.tlas_items.size(), 0, wb);
    f.tlas_extent = box_extent(wb);
    f.tlas_depth = tl.depth_reached;
    if (tl.depth_reached + 1 + f.max_blas_depth + 1 > TRAVERSAL_STACK) return set_error("pt_world_build: BVH too deep for the traversal stack");
    w.s.stack_need = (uint32_t)(tl.depth_reached + 1 + f.max_blas_depth + 1);
    return 0;
}

// ---- fold_textures_and_materials: the atlases, flat checkers, solid textures' values into the material records --------------------------------
void fold_textures_and_materials(Flattening& w) {
    const pt_scene& s = w.s;
    FlatScene& f = w.f;
    std::vector<TexD>& tex = f.tex;
    tex.resize(s.tex.size());
    for (size_t i = 0; i < s.tex.size(); ++i) {
        tex[i] = s.tex[i].d;
        if (tex[i].kind == TEX_IMAGE) {
            tex[i].ofs = f.atlas.size();
            f.atlas.insert(f.atlas.end(), s.tex[i].image.begin(), s.tex[i].image.end());
        } else if (tex[i].kind == TEX_IMAGE_F32) {
            tex[i].ofs = f.atlas_f.size();
            f.atlas_f.insert(f.atlas_f.end(), s.tex[i].image_f.begin(), s.tex[i].image_f.end());
        }
    }
    for (TexD& t : tex)   // checkers of two solid children carry the children's values
        if (t.kind == TEX_CHECKER) {
            const TexD &a = tex[t.t1], &b = tex[t.t2];
            const bool solid = (a.kind == TEX_SOLID_RGB || a.kind == TEX_SOLID_F) && (b.kind == TEX_SOLID_RGB || b.kind == TEX_SOLID_F);
            t.flat = solid ? 1u : 0u;
            for (int c = 0; c < 3; ++c) { t.c1[c] = solid ? a.v[c] : 0.0; t.c2[c] = solid ? b.v[c] : 0.0; }
        }
    std::vector<MatD>& mats = f.mats;
    mats = s.mats;
    for (const PrimRef& pr : f.prims)   // a medium that bounds something in the world (MatD::p[5], pt_dev_medium.h)
        if (mats[pr.mat].kind == MAT_MEDIUM) mats[pr.mat].p[5] = 1.0;
        else if (mats[pr.mat].kind == MAT_GLASS && mats[pr.mat].p[0] != 0.0) mats[(size_t)mats[pr.mat].p[0] - 1].p[5] = 1.0;   // ... or fills a glass object
    for (MatD& m : mats) {   // solid textures' values into the material records (MatD::color_solid)
        m.color_solid = m.rough_solid = 0u;
        const bool has_color = m.kind == MAT_DIFFUSE || m.kind == MAT_METAL || m.kind == MAT_PRINCIPLED || m.kind == MAT_LIGHT;
        const bool has_rough = m.kind == MAT_METAL || m.kind == MAT_GLASS;
        if (has_color && m.color_tex >= 0 && (size_t)m.color_tex < tex.size() && tex[m.color_tex].kind == TEX_SOLID_RGB && !exp_env("PT_NO_SOLID_IN_MAT")) {
            m.color_solid = 1u;
            for (int c = 0; c < 3; ++c) m.color_v[c] = tex[m.color_tex].v[c];
        }
        if (has_rough && m.rough_tex >= 0 && (size_t)m.rough_tex < tex.size() && tex[m.rough_tex].kind == TEX_SOLID_F && !exp_env("PT_NO_SOLID_IN_MAT")) {
            m.rough_solid = 1u;
            m.rough_v = tex[m.rough_tex].v[0];
        }
    }
}

// ---- walk_records: the flat walk's EntryBox / CuboidBox list, and whether the walk runs ------------------------------------------------------
void walk_records(Flattening& w) {
    FlatScene& f = w.f;
    for (int pass = 0; pass < 2; ++pass)   // spheres / quads / cuboids first: their hits trim the mesh boxes
        for (size_t i = 0; i < w.entry_boxes.size(); ++i) {
            if ((f.entries[i].kind == ENTRY_MESH) != (pass == 1)) continue;
            EntryBox eb{};
            const Entry& e = f.entries[i];
            Builder::store_box(w.entry_boxes[i], eb.lo, eb.hi);
            eb.entry = (uint32_t)i;
            eb.kind = e.kind;
            eb.first_prim = e.first_prim;
            eb.inst = e.inst;
            eb.blas_root = e.blas_root;
            eb.extent = e.extent;
            eb.n_prims = e.n_prims;
            eb.prim_kind = ENTRYBOX_VIA_PRIMREF;
            if (e.kind != ENTRY_MESH) {   // one kind, consecutive records: the walk addresses them without prims[]
                const PrimRef& p0 = f.prims[e.first_prim];
                bool direct = true;
                for (uint32_t k = 0; k < e.n_prims; ++k) {
                    const PrimRef& pk = f.prims[e.first_prim + k];
                    direct = direct && (pk.kind & 0xFFu) == (p0.kind & 0xFFu) && pk.index == p0.index + k && pk.inst == e.inst;
                }
                if (direct && !exp_env("PT_ENTRYBOX_VIA_PRIMREF")) {
                    eb.prim_kind = p0.kind & 0xFFu;
                    eb.prim_index = p0.index;
                }
            }
            CuboidBox cb{};
            if (e.kind == ENTRY_CUBOID && eb.prim_kind == PRIM_QUAD) {   // object-space box of the six faces (they are consecutive QuadD records)
                Box local;
                for (uint32_t k = 0; k < 6; ++k) local.grow(quad_box(f.quads[eb.prim_index + k]));
                Builder::store_box(local, cb.lo, cb.hi);
                eb.extent = box_extent(local);
            }
            f.cuboid_box.push_back(cb);
            f.entry_box.push_back(eb);
        }
    uint32_t flat_max = TLAS_FLAT_MAX;
    if (const char* ev = exp_env("PT_FLAT_MAX")) flat_max = (uint32_t)atoi(ev);
    bool pair_ids_fit = true;   // the flat walk packs (primitive id, lane) into one word: ids of spheres / quads / cuboid faces below 2^26
    for (const Entry& e : f.entries) pair_ids_fit = pair_ids_fit && (e.kind == ENTRY_MESH || (uint64_t)e.first_prim + e.n_prims <= (1ull << 26));
    f.tlas_flat = f.entries.size() <= flat_max && pair_ids_fit && !exp_env("PT_NO_FLAT_TLAS") ? 1u : 0u;
    f.flat_pairs = 0;
    for (const Entry& e : f.entries) f.flat_pairs |= (f.tlas_flat && e.kind == ENTRY_CUBOID && !exp_env("PT_NO_FLAT_PAIRS")) ? 1u : 0u;
}

// ---- pack_grids: the grid-density media's table and their samples, one array --------------------------------------------------------------
void pack_grids(Flattening& w) {
    for (const HostGrid& hg : w.s.grids) {
        w.f.grids.push_back(hg.d);
        w.f.grids.back().ofs = w.f.grid_vals.size();
        w.f.grid_vals.insert(w.f.grid_vals.end(), hg.vals.begin(), hg.vals.end());
    }
}

struct Fnv {   // FNV-1a, 64 bit, over the bytes of arithmetic fields
    uint64_t h = 14695981039346656037ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    }
    template <class T>
    std::enable_if_t<std::is_arithmetic<T>::value> one(const T& v) { bytes(&v, sizeof v); }
    template <class T, size_t N>
    void one(const T (&a)[N]) { for (const T& x : a) one(x); }
    template <class... A>
    void operator()(const A&... a) { (one(a), ...); }
    template <class T, class F>
    void each(const std::vector<T>& v, F fields) {   // the length, then every element through `fields`
        (*this)((uint64_t)v.size());
        for (const T& x : v) fields(x);
    }
};
}  // namespace

int pt::flatten(pt_scene& s, const BlasHook& device_blas, FlatScene& out) {
    out = FlatScene{};
    Flattening w{s, device_blas, out};
    if (place_entries(w) != 0) return -1;
    mark_prims(w);
    pick_shadeable(w);
    order_entries(w);
    if (plan_light_grid(w) != 0) return -1;
    if (build_top_level(w) != 0) return -1;
    fold_textures_and_materials(w);
    walk_records(w);
    pack_grids(w);
    return 0;
}

// What a finished build leaves on the scene. Its caller makes it the last step — scene_build once the upload has succeeded — so a build
// that fails anywhere before keeps these fields of the build before it.
void pt::finish_build(pt_scene& s, const FlatScene& f) {
    s.grid_built = f.grid;
    s.stack_need_extend2 = f.tlas_flat ? (uint32_t)(f.max_blas_depth + 1) : s.stack_need;
    s.n_prims = (uint32_t)f.prims.size();
    s.n_mesh_entries = 0;
    s.n_punctual_built = (uint32_t)s.punctual.size();
    s.has_moving_instance = f.any_moving;
    s.motionless = !f.any_moving;   // (a moving instance: a ray's time reaches its pose)
    for (const SphereD& sp : f.spheres)
        for (int i = 0; i < 3; ++i) s.motionless = s.motionless && sp.p1[i] == sp.p2[i];
    for (const Entry& e : f.entries) s.n_mesh_entries += e.kind == ENTRY_MESH ? 1u : 0u;
    s.built = true;
}

uint64_t pt::flat_checksum(const FlatScene& f) {
    Fnv h;
    h.each(f.nodes, [&](const BvhNode& x) { h(x.lo0, x.hi0, x.lo1, x.hi1, x.child0, x.child1, x.pad0, x.pad1); });
    h.each(f.entries, [&](const Entry& x) { h(x.kind, x.first_prim, x.inst, x.blas_root, x.extent, x.n_prims, x.pad); });
    h.each(f.prims, [&](const PrimRef& x) { h(x.kind, x.index, x.mat, x.inst); });
    h.each(f.spheres, [&](const SphereD& x) { h(x.r, x.p1, x.p2); });
    h.each(f.quads, [&](const QuadD& x) { h(x.q, x.u, x.v, x.w, x.n, x.d); });
    h.each(f.tris, [&](const TriD& x) { h(x.v0, x.v1, x.v2); });
    h.each(f.tri_gid, [&](uint32_t x) { h(x); });
    h.each(f.insts, [&](const InstD& x) { h(x.c0, x.c1, x.c2, x.t, x.i0, x.i1, x.i2, x.it, x.inner, x.outer); });
    h.each(f.tex, [&](const TexD& x) { h(x.kind, x.t1, x.t2, x.w, x.h, x.flat, x.ofs, x.v, x.inv_scale, x.c1, x.c2); });
    h.each(f.mats, [&](const MatD& x) { h(x.kind, x.color_tex, x.rough_tex, x.nmap_tex, x.ior, x.p, x.lobe_w, x.lobe_p, x.alpha_g, x.color_solid, x.rough_solid, x.color_v, x.rough_v); });
    h.each(f.atlas, [&](uint8_t x) { h(x); });
    h.each(f.atlas_f, [&](float x) { h(x); });
    h.each(f.lights, [&](uint32_t x) { h(x); });
    h.each(f.entry_box, [&](const EntryBox& x) { h(x.lo, x.hi, x.entry, x.kind, x.first_prim, x.inst, x.blas_root, x.extent, x.n_prims, x.prim_kind, x.prim_index, x.pad); });
    h.each(f.cuboid_box, [&](const CuboidBox& x) { h(x.lo, x.hi, x.pad); });
    h.each(f.light_cdf, [&](double x) { h(x); });
    h.each(f.tri_attr, [&](const TriAttr& x) { h(x.n, x.uv); });
    h.each(f.inst_motion, [&](const InstMotionD& x) { h(x.axis, x.angle0, x.dangle, x.tr0, x.dtr, x.moves, x.spins); });
    h.each(f.grids, [&](const GridD& x) { h(x.nx, x.ny, x.nz, x.pad, x.ofs, x.lo, x.hi, x.cells, x.scale, x.mu); });
    h.each(f.grid_vals, [&](float x) { h(x); });
    h(f.tlas_root, f.tlas_extent, f.tlas_flat, f.flat_pairs, f.grid.box, f.grid.dims, f.grid.cells, (uint32_t)f.any_attr, (uint32_t)f.any_moving, (int32_t)f.max_blas_depth);
    return h.h;
}
