// Closest-hit traversal shared by K2 (pt_k2_extend.h), k_probe and k_aov / k_aov_qmc (pt_k3.hip, pt_k3_qmc.hip), and at its end the
// first-hit feature walk of those two (pt_render_aovs).
#pragma once
#include "pt_k_common.h"

namespace pt {

// ---------------------------------------------------------------------------------------
// Closest-hit traversal. Two-level BVH2 walked with one per-lane stack held in LDS
// (stack[level][lane]: a wave touches 64 consecutive dwords per level -> conflict free).
// The result is tree-independent: minimum t; on an exact tie the larger global primitive id
// wins, so any builder/visit order gives the reference's hit.
// ---------------------------------------------------------------------------------------
struct Closest {
    double t;
    uint32_t id;
};
PT_DEV void consider(Closest& best, double t, uint32_t id) {
    if (t < best.t || (t == best.t && id > best.id)) {
        best.t = t;
        best.id = id;
    }
}
// K2's result word for a slot (pt_types.h, PoolD::hit_prim): id | class << 28. `id` may be one of the sentinels.
PT_DEV uint32_t hit_word(const SceneD& sc, uint32_t id) {
    if (id >= HIT_SLOT_DEAD) {
        const uint32_t cls = id == HIT_NONE ? CLASS_MISS : id == HIT_SLOT_IDLE ? CLASS_IDLE : CLASS_DEAD;
        return (cls << HIT_CLASS_SHIFT) | HIT_ID_MASK;
    }
    const uint32_t mat_kind = (sc.prims[id].kind >> PRIM_MAT_KIND_SHIFT) & 0xFFu;
    return ((1u + mat_kind) << HIT_CLASS_SHIFT) | id;
}
PT_DEV uint32_t dead_or_idle(uint32_t bounce) { return bounce == SLOT_IDLE ? HIT_SLOT_IDLE : HIT_SLOT_DEAD; }

// ---- conservative f32 slab test -----------------------------------------------------------------
// Per ray and per space (world / instance-local) the f64 ray is reduced to idf = fl32(1/d),
// oif = fl32(o/d) and t' = fma32(b, idf, -oif) for a box bound b. Error analysis (u = 2^-24):
//   t' = (b*id*(1+da) - oi*(1+db))*(1+dc)  =>  |t' - t| <= 2u (|b||id| + |oi|) <= 2u (S|id| + |oi|)
// with S = max |coordinate| of the boxes of the tree being walked (SceneD::tlas_extent /
// Entry::extent). 1/d itself is a fast f32 reciprocal of fl32(d) (<= 3u relative error: the slabs
// of a ray tilted by 3u, another 3u (S|id| + |oi|)). Every axis interval is widened by
// e = 8u (S|id| + |oi|), which also covers the rounding of e itself and of the +-e — so a box the
// exact ray touches inside [t_min, t_best] is never rejected. 1/d is clamped to +-1e30 so that an exactly axis-parallel ray
// (they occur: a direction sampled inside the plane of an axis-aligned light has d.y == 0) yields
// finite products: the axis then behaves as "parallel" — everything when the origin is inside the
// slab, nothing when it is outside. Box tests never influence WHICH hit wins, only how much work
// it takes to find it; the primitive tests keep the reference's f64 arithmetic.
struct RayF {
    float idx, idy, idz, oix, oiy, oiz, ex, ey, ez;
};
PT_DEV void rayf_axis(double o, double d, float S, float& idf, float& oif, float& e) {
    // idf: f32 reciprocal of fl32(d) (relative error <= 3u against 1/d), clamped to +-1e30; the slab
    // parameters are then those of a ray whose direction differs by <= 3u — absorbed by the margin
    float df = (float)d;
    float id = __frcp_rn(df);
    if (!(fabsf(id) <= 1e30f)) id = copysignf(1e30f, df);
    idf = id;
    oif = (float)(o * (double)id);
    e = (S * fabsf(id) + fabsf(oif)) * 4.7683716e-07f;   // 8u >= (2u arithmetic + 3u reciprocal) with slack
}
PT_DEV RayF make_rayf(V3 o, V3 d, float S) {
    RayF f;
    rayf_axis(o.x, d.x, S, f.idx, f.oix, f.ex);
    rayf_axis(o.y, d.y, S, f.idy, f.oiy, f.ey);
    rayf_axis(o.z, d.z, S, f.idz, f.oiz, f.ez);
    return f;
}
PT_DEV bool slab_f32(const float* lo, const float* hi, const RayF& f, float t_min, float t_max, float& t_near) {
    const float t1x = __builtin_fmaf(lo[0], f.idx, -f.oix), t2x = __builtin_fmaf(hi[0], f.idx, -f.oix);
    const float t1y = __builtin_fmaf(lo[1], f.idy, -f.oiy), t2y = __builtin_fmaf(hi[1], f.idy, -f.oiy);
    const float t1z = __builtin_fmaf(lo[2], f.idz, -f.oiz), t2z = __builtin_fmaf(hi[2], f.idz, -f.oiz);
    const float nx = fminf(t1x, t2x) - f.ex, fx = fmaxf(t1x, t2x) + f.ex;
    const float ny = fminf(t1y, t2y) - f.ey, fy = fmaxf(t1y, t2y) + f.ey;
    const float nz = fminf(t1z, t2z) - f.ez, fz = fmaxf(t1z, t2z) + f.ez;
    const float tn = fmaxf(fmaxf(nx, ny), fmaxf(nz, t_min));
    const float tf = fminf(fminf(fx, fy), fminf(fz, t_max));
    t_near = tn;
    return tn <= tf;
}
// Cuboid face culling (flat top level). `f` = the OBJECT-space ray reduced like any other (make_rayf with the box's extent), lo / hi =
// the cuboid's object-space box. A face's exact f64 quad test (quad.rs:40-59) can only accept a hit with t in [t_min, t_best] at
// a point of the box's surface, and such a point satisfies, for every axis, t_near_axis <= t <= t_far_axis. With the proven
// slab bound |t' - t| <= e per axis (above): the face on plane b of axis a stays a candidate iff t'_b + e_a >= max over the
// axes of (near' - e) and t'_b - e_a <= min over the axes of (far' + e) — the ray's ENTRY and EXIT faces, plus whatever the margin
// cannot tell apart at an edge. Bits follow pt_cuboid's face order (cuboid.rs:18-52): 0 +z front, 1 +x right, 2 -z back,
// 3 -x left, 4 +y top, 5 -y bottom. Conservative only: which hit wins is still decided by the f64 tests of the faces kept.
PT_DEV uint32_t cuboid_face_mask(const float* lo, const float* hi, const RayF& f, float t_min, float t_max) {
    const float lx = __builtin_fmaf(lo[0], f.idx, -f.oix), hx = __builtin_fmaf(hi[0], f.idx, -f.oix);
    const float ly = __builtin_fmaf(lo[1], f.idy, -f.oiy), hy = __builtin_fmaf(hi[1], f.idy, -f.oiy);
    const float lz = __builtin_fmaf(lo[2], f.idz, -f.oiz), hz = __builtin_fmaf(hi[2], f.idz, -f.oiz);
    const float tn = fmaxf(fmaxf(fminf(lx, hx) - f.ex, fminf(ly, hy) - f.ey), fmaxf(fminf(lz, hz) - f.ez, t_min));
    const float tf = fminf(fminf(fmaxf(lx, hx) + f.ex, fmaxf(ly, hy) + f.ey), fminf(fmaxf(lz, hz) + f.ez, t_max));
    if (!(tn <= tf)) return 0u;
    auto cand = [&](float t, float e) -> uint32_t { return (t + e >= tn && t - e <= tf) ? 1u : 0u; };
    return cand(hz, f.ez) | (cand(hx, f.ex) << 1) | (cand(lz, f.ez) << 2) | (cand(lx, f.ex) << 3) | (cand(hy, f.ey) << 4) | (cand(ly, f.ey) << 5);
}
// one BVH2 node: both children tested, near-first order; returns the number of children to visit
PT_DEV int visit_node(const BvhNode* nd, const RayF& f, float t_min, float t_max, uint32_t& first, uint32_t& second) {
    const float4 q0 = ((const float4*)nd)[0], q1 = ((const float4*)nd)[1], q2 = ((const float4*)nd)[2];
    const uint4 q3 = ((const uint4*)nd)[3];
    const float lo0[3] = {q0.x, q0.y, q0.z}, hi0[3] = {q0.w, q1.x, q1.y};
    const float lo1[3] = {q1.z, q1.w, q2.x}, hi1[3] = {q2.y, q2.z, q2.w};
    float tn0, tn1;
    const bool h0 = slab_f32(lo0, hi0, f, t_min, t_max, tn0);
    const bool h1 = slab_f32(lo1, hi1, f, t_min, t_max, tn1);
    if (h0 && h1) {
        const bool swap = tn1 < tn0;
        first = swap ? q3.y : q3.x;
        second = swap ? q3.x : q3.y;
        return 2;
    }
    first = h0 ? q3.x : q3.y;
    return (h0 || h1) ? 1 : 0;
}
PT_DEV float t_max_f32(double t) { return __double2float_ru(t); }   // rounded UP: conservative upper end

// One triangle leaf (<= 8 triangles, BLAS order first .. first+count-1) for the ray of this lane.
// (Tried in round 2 and removed: a two-pass form — a division-free, exactly equivalent screen of every triangle, then
// the full test for the survivors only, so that a wave runs the expensive pass once or twice instead of `count` times.
// Bit-exact, but 1.5 % SLOWER on scene 6: the screen repeats two thirds of the test's arithmetic and the full pass still
// runs once for almost every leaf.)
PT_DEV void test_leaf(const SceneD& sc, uint32_t first, uint32_t count, const RayD& r, double t_min, uint32_t first_prim, Closest& best) {
    for (uint32_t i = first; i < first + count; ++i) {
        double t, u, v;
        if (hit_tri(sc.tris[i], r, t_min, t, u, v)) consider(best, t, first_prim + sc.tri_gid[i]);
    }
}

// U: `gid` is wave-uniform (the flat top-level walk) -> the primitive's record arrives by scalar loads (ldu)
template <bool U = false>
PT_DEV void test_world_prim(const SceneD& sc, const RayD& r, double t_min, uint32_t gid, Closest& best) {
    PrimRef pr;
    if constexpr (U) pr = ldu(&sc.prims[gid]); else pr = sc.prims[gid];
    if ((pr.kind & 0xFFu) == PRIM_SPHERE) {
        double t;
        V3 c;
        bool h;
        if constexpr (U) { const SphereD sp = ldu(&sc.spheres[pr.index]); h = hit_sphere(sp, r, t_min, t, c); }
        else h = hit_sphere(sc.spheres[pr.index], r, t_min, t, c);
        if (h) consider(best, t, gid);
    } else {
        double t, a, b;
        bool h;
        if constexpr (U) { const QuadD qd = ldu(&sc.quads[pr.index]); h = hit_quad(qd, r, t_min, t, a, b); }
        else h = hit_quad(sc.quads[pr.index], r, t_min, t, a, b);
        if (h) consider(best, t, gid);
    }
}

template <bool MOT = false>   // MOT: instances are posed at the ray's time (inst_at)
PT_DEV Closest closest_hit(const SceneD& sc, const RayD& wray, double t_min, uint32_t* stk /* &stack[0][lane] */) {
    Closest best{D_INF, HIT_NONE};
    RayD r = wray;
    const RayF fw = make_rayf(wray.o, wray.d, sc.tlas_extent);   // world-space reduction, kept across instances
    RayF f = fw;
    const float t_min_f = __double2float_rd(t_min);
    float t_max_f = t_max_f32(best.t);
    int sp = 0;
    uint32_t cur = sc.tlas_root;
    uint32_t mesh_first_prim = 0;   // Entry::first_prim of the mesh instance being walked
    for (;;) {
        if ((cur & REF_TYPE_MASK) == REF_NODE) {
            const BvhNode* nd = &sc.nodes[cur];
            uint32_t c0, c1;
            const int n = visit_node(nd, f, t_min_f, t_max_f, c0, c1);
            if (n == 2 && sp < TRAVERSAL_STACK) stk[(sp++) * BLOCK] = c1;
            if (n > 0) {
                cur = c0;
                continue;
            }
        } else if ((cur & REF_TYPE_MASK) == REF_TRIS) {
            const uint32_t first = cur & 0x07FFFFFFu, count = ((cur >> 27) & 7u) + 1u;
            test_leaf(sc, first, count, r, t_min, mesh_first_prim, best);
            t_max_f = t_max_f32(best.t);
        } else if ((cur & REF_TYPE_MASK) == REF_ENTRY) {
            const Entry e = sc.entries[cur & 0x3FFFFFFFu];
            const RayD lr = ray_to_local_chain<false, MOT>(sc, e.inst, wray);
            if (e.kind == ENTRY_MESH) {
                r = lr;
                mesh_first_prim = e.first_prim;
                f = make_rayf(r.o, r.d, e.extent);
                if (sp < TRAVERSAL_STACK) stk[(sp++) * BLOCK] = REF_LEAVE_INSTANCE;
                cur = e.blas_root;
                continue;
            }
            const uint32_t n = e.kind == ENTRY_CUBOID ? 6u : 1u;   // cuboid.rs: six quads, linear
            for (uint32_t i = 0; i < n; ++i) test_world_prim(sc, lr, t_min, e.first_prim + i, best);
            t_max_f = t_max_f32(best.t);
        } else if (cur == REF_LEAVE_INSTANCE) {
            r = wray;
            f = fw;
        }
        if (sp == 0) break;
        cur = stk[(--sp) * BLOCK];
    }
    return best;
}

template <int STRIDE = BLOCK, bool MOT = false>   // STRIDE: threads per block = distance of a lane's consecutive stack entries in LDS
PT_DEV void blas_pass(const SceneD& sc, const RayD& wray, const Entry& e, double t_min, float t_min_f, uint32_t* stk, int cap, Closest& best) {
    const RayD r = ray_to_local_chain<false, MOT>(sc, e.inst, wray);
    const RayF f = make_rayf(r.o, r.d, e.extent);
    float t_max_f = t_max_f32(best.t);
    int sp = 0;
    uint32_t cur = e.blas_root;
    // "while-while" traversal: every lane first descends until it HOLDS a triangle leaf (cheap f32 box
    // tests; lanes that already found theirs idle), then the wave runs the expensive f64 triangle
    // tests together. Interleaving the two per iteration made almost every iteration pay for a leaf.
    for (;;) {
        while ((cur & REF_TYPE_MASK) == REF_NODE) {
            uint32_t c0, c1;
            const int n = visit_node(&sc.nodes[cur], f, t_min_f, t_max_f, c0, c1);
            if (n == 2 && sp < cap) stk[(sp++) * STRIDE] = c1;
            if (n > 0) cur = c0;
            else if (sp > 0) cur = stk[(--sp) * STRIDE];
            else cur = REF_EMPTY;
        }
        if ((cur & REF_TYPE_MASK) != REF_TRIS) break;             // REF_EMPTY: nothing left
        const uint32_t first = cur & 0x07FFFFFFu, count = ((cur >> 27) & 7u) + 1u;
        test_leaf(sc, first, count, r, t_min, e.first_prim, best);
        t_max_f = t_max_f32(best.t);
        if (sp == 0) break;
        cur = stk[(--sp) * STRIDE];
    }
}

// First-hit feature buffers (pt_render_aovs; no counterpart in the reference). The colour the first bounce multiplies by:
// the colour texture of diffuse / metal / principled, sheen's base colour, (1, 1, 1) for glass (Q4: its base colour reaches
// no radiance), clearcoat and lights; a mix weights its children as mix.rs's pdf / eval do, down the MIX_MAX_DEPTH levels.
PT_DEV V3 aov_albedo(const SceneD& sc, const MatD& m, const HitD& h) {
    const V3 one{1.0, 1.0, 1.0};
    auto leaf = [&](const MatD& l) -> V3 {
        if (l.kind == MAT_DIFFUSE || l.kind == MAT_METAL || l.kind == MAT_PRINCIPLED) return fetch_tex(sc, l, h).color;
        if (l.kind == MAT_SHEEN) return V3{l.p[0], l.p[1], l.p[2]};
        return one;
    };
    auto child = [&](const MatD& c) -> V3 {   // a mix's child: a leaf, or a mix of leaves
        if (c.kind != MAT_MIX) return leaf(c);
        return (1.0 - c.p[0]) * leaf(sc.mats[c.color_tex]) + c.p[0] * leaf(sc.mats[c.rough_tex]);
    };
    if (m.kind != MAT_MIX) return leaf(m);
    return (1.0 - m.p[0]) * child(sc.mats[m.color_tex]) + m.p[0] * child(sc.mats[m.rough_tex]);
}
// One thread per pixel walks samples [spp_begin, spp_end) in order; sample s's camera ray is k_init's for (pixel, s) — same Rng,
// same generate_ray — and its closest hit is the one K2 finds (tree-independent). Adds (overwrite: stores) the
// sums aov[8 * pixel + k]: albedo rgb, shading normal xyz, depth, hits. No atomics: every pixel has one writer.
template <bool QMC, bool MOT = false>
PT_DEV void aov_pixels(const SceneD& sc, const CamD& cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov, uint32_t overwrite) {
    __shared__ uint32_t stack[TRAVERSAL_STACK * BLOCK];
    const uint32_t n_pixels = cam.width * cam.height;
    for (uint32_t p = blockIdx.x * BLOCK + threadIdx.x; p < n_pixels; p += gridDim.x * BLOCK) {
        uint32_t row, col;
        divmod_u31(p, cam.width, row, col);
        V3 alb{0.0, 0.0, 0.0}, nrm{0.0, 0.0, 0.0};
        double depth = 0.0, hits = 0.0;
        for (uint32_t s = spp_begin; s < spp_end; ++s) {
            std::conditional_t<QMC, RngQ, Rng> rng{(uint32_t)seed, (uint32_t)(seed >> 32), p, s, 0u};
            const RayD r = generate_ray<MOT>(cam, row, col, rng);
            const Closest c = closest_hit<MOT>(sc, r, 1e-3, &stack[threadIdx.x]);
            HitD h;
            if (c.id != HIT_NONE && reconstruct_hit<true, MOT>(sc, r, c.id, 1e-3, h)) {
                alb = alb + aov_albedo(sc, sc.mats[h.mat], h);
                nrm = nrm + h.sn;
                depth = depth + h.dist;
                hits = hits + 1.0;
            } else {
                alb = alb + V3{1.0, 1.0, 1.0};   // a miss: environment radiance is not reflected light
            }
        }
        double* o = aov + 8 * (size_t)p;
        const double v[8] = {alb.x, alb.y, alb.z, nrm.x, nrm.y, nrm.z, depth, hits};
        for (int k = 0; k < 8; ++k) o[k] = overwrite ? v[k] : o[k] + v[k];
    }
}

}  // namespace pt
