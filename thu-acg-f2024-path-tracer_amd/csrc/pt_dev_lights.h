// Exact light sampling (pt_scene_set_light_sampling kind 1; the rule is in include/pt_amd.h): lights.sample / lights.pdf
// of k_shade's LSE forms and of the light probe. A mesh entry is sampled uniformly by AREA (a binary search over the running area sums
// of SceneD::light_cdf, then a uniform point of the face) and its pdf is the solid-angle density of that sampler, summed over EVERY face
// the direction meets: an all-hits walk of the mesh's own BVH. A sphere entry is sampled over the cone it subtends. Quad and cuboid
// entries, the light-index draw and the instance chain are pt_dev_geom.h's, operation by operation.
#pragma once
#include "pt_k_trace.h"

namespace pt {

// the largest double below a positive finite a
PT_DEV double below(double a) { return __longlong_as_double(__double_as_longlong(a) - 1ll); }

// the term of one face met at distance t: the density of a uniform point of a surface of area A, per solid angle, with the face's
// GEOMETRIC normal
PT_DEV double mesh_pdf_term(const TriD& tr, const RayD& r, double t, double A) {
    const V3 v0 = ld3(tr.v0);
    const V3 c = cross(ld3(tr.v1) - v0, ld3(tr.v2) - v0);
    return (t * t) / (fabs(dot(r.d, normalize(c))) * A);
}

// All-hits walk of one mesh tree for the local-space ray r: blas_pass's node format and slab margin over [0, +inf), no closest-hit
// pruning and no ordering — every leaf whose box the ray meets is tested with hit_tri and every accepted face adds its term. The sum's
// order is the tree's. stk = &stack[0][lane] of an LDS stack[level][lane] with STRIDE lanes; the host refuses a tree deeper than `cap`.
template <int STRIDE>
PT_DEV double mesh_pdf_walk(const SceneD& sc, const RayD& r, uint32_t root, float extent, double A, uint32_t* stk, int cap) {
    const RayF f = make_rayf(r.o, r.d, extent);
    const float t_max_f = __builtin_huge_valf();
    double sum = 0.0;
    int sp = 0;
    uint32_t cur = root;
    for (;;) {
        while ((cur & REF_TYPE_MASK) == REF_NODE) {
            uint32_t c0, c1;
            const int n = visit_node(&sc.nodes[cur], f, 0.0f, t_max_f, c0, c1);
            if (n == 2 && sp < cap) stk[(sp++) * STRIDE] = c1;
            if (n > 0) cur = c0;
            else if (sp > 0) cur = stk[(--sp) * STRIDE];
            else cur = REF_EMPTY;
        }
        if ((cur & REF_TYPE_MASK) != REF_TRIS) break;             // REF_EMPTY: nothing left (at once when the ray misses the root's boxes)
        const uint32_t first = cur & 0x07FFFFFFu, count = ((cur >> 27) & 7u) + 1u;
        for (uint32_t i = first; i < first + count; ++i) {
            double t, u, v;
            const TriD& tr = sc.tris[i];
            if (hit_tri(tr, r, 0.0, t, u, v)) sum += mesh_pdf_term(tr, r, t, A);
        }
        if (sp == 0) break;
        cur = stk[(--sp) * STRIDE];
    }
    return sum;
}

// the cone a sphere of squared radius r2 subtends from squared distance d2 > r2: k = 1 - cos(theta_max), without the cancellation
PT_DEV double sphere_cone_k(double r2, double d2) {
    const double x = r2 / d2;
    const double cm = sqrt(1.0 - x);
    return x / (1.0 + cm);
}

// lights.sample, kind 1. light / face (the probe's columns): the index drawn and, for a mesh entry, the face chosen (else -1).
template <class R>
PT_DEV V3 lights_sample_exact(const SceneD& sc, V3 origin_w, double time, R& rng, uint32_t* light = nullptr, int32_t* face = nullptr) {
    const uint32_t i = rng_index(rng, sc.n_lights);
    if (light) *light = i;
    if (face) *face = -1;
    const Entry e = sc.entries[sc.lights[i]];
    V3 origin = origin_w;
    int32_t innermost = -1;
    for (int32_t k = e.inst; k >= 0;) {                                           // instance.rs:64-66, outermost instance first
        const InstD& m = sc.insts[k];
        origin = xform_point(m.i0, m.i1, m.i2, m.it, origin);
        innermost = k;
        k = m.inner;
    }
    V3 dir;
    if (e.kind == ENTRY_QUAD) {
        dir = sample_quad_dir(sc.quads[sc.prims[e.first_prim].index], origin, rng);
    } else if (e.kind == ENTRY_CUBOID) {
        const uint32_t j = rng_index(rng, 6u);
        dir = sample_quad_dir(sc.quads[sc.prims[e.first_prim + j].index], origin, rng);
    } else if (e.kind == ENTRY_MESH) {
        const double* C = sc.light_cdf + e.pad[0];
        const double A = C[e.n_prims];
        double x = rng_f64(rng) * A;
        if (x >= A) x = below(A);
        uint32_t lo = 0u, hi = e.n_prims - 1u;                                    // the smallest j with x < C[j + 1]
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (x < C[mid + 1u]) hi = mid; else lo = mid + 1u;
        }
        if (face) *face = (int32_t)lo;
        uint64_t ua, ub;
        rng_u64x2(rng, ua, ub);
        const double s = sqrt(u64_to_unit(ua)), u2 = u64_to_unit(ub);
        const double b0 = 1.0 - s, b1 = s * (1.0 - u2), b2 = s * u2;
        const TriD& tr = sc.tris[sc.prims[e.first_prim + lo].index];
        const V3 point = ld3(tr.v0) * b0 + ld3(tr.v1) * b1 + ld3(tr.v2) * b2;
        dir = normalize(point - origin);
    } else {
        const SphereD& s = sc.spheres[sc.prims[e.first_prim].index];
        const V3 center = ld3(s.p1) + (ld3(s.p2) - ld3(s.p1)) * time;
        const V3 L = center - origin;
        const double d2 = length_squared(L), r2 = s.r * s.r;
        uint64_t ua, ub;
        rng_u64x2(rng, ua, ub);
        const double u1 = u64_to_unit(ua), u2 = u64_to_unit(ub);
        const bool inside = d2 <= r2;
        const double cos_t = inside ? 1.0 - 2.0 * u1 : 1.0 - u1 * sphere_cone_k(r2, d2);
        const double sin_t = sqrt(fmax(0.0, 1.0 - cos_t * cos_t));
        const double phi = 2.0 * D_PI * u2;
        const SinCos sc_phi = dev_sincos(phi);
        const V3 local{sin_t * sc_phi.c, sin_t * sc_phi.s, cos_t};
        dir = inside ? local : to_world(frame_to_z(normalize(L)), local);         // around normalize(L), as hg_sample goes around its axis
    }
    for (int32_t k = innermost; k >= 0;) {                                        // instance.rs:67-68 (not re-normalised)
        const InstD& m = sc.insts[k];
        dir = xform_vector(m.c0, m.c1, m.c2, dir);
        k = m.outer;
    }
    return dir;
}

// lights.pdf, kind 1. The light index is wave-uniform: entry, chain, tree root and table base arrive by scalar loads (ldu). The caller's
// lanes without a direction are not here; a lane whose ray misses the root's boxes leaves the walk at its first step.
template <int STRIDE>
PT_DEV double lights_pdf_exact(const SceneD& sc, V3 origin_w, V3 direction_w, double time, uint32_t* stk) {
    if (sc.n_lights == 0) return 0.0;
    double sum = 0.0;
    for (uint32_t i = 0; i < sc.n_lights; ++i) {
        const Entry e = ldu(&sc.entries[ldu(&sc.lights[i])]);
        V3 origin = origin_w, direction = direction_w;
        for (int32_t k = e.inst; k >= 0;) {                                       // instance.rs:71-75, outermost instance first
            const InstD m = ldu(&sc.insts[k]);
            origin = xform_point(m.i0, m.i1, m.i2, m.it, origin);
            direction = xform_vector(m.i0, m.i1, m.i2, direction);
            k = m.inner;
        }
        double pdf = 0.0;
        if (e.kind == ENTRY_QUAD) {
            const PrimRef pr = ldu(&sc.prims[e.first_prim]);
            const QuadD qd = ldu(&sc.quads[pr.index]);
            pdf = pdf_quad(sc, qd, pr.mat, origin, direction, time);
        } else if (e.kind == ENTRY_CUBOID) {                                      // list.rs:86-96 over the six sides
            double s6 = 0.0;
            for (uint32_t j = 0; j < 6u; ++j) {
                const PrimRef pr = ldu(&sc.prims[e.first_prim + j]);
                const QuadD qd = ldu(&sc.quads[pr.index]);
                s6 += pdf_quad(sc, qd, pr.mat, origin, direction, time);
            }
            pdf = s6 / 6.0;
        } else if (e.kind == ENTRY_MESH) {
            const double A = ldu(sc.light_cdf + e.pad[0] + e.n_prims);
            pdf = mesh_pdf_walk<STRIDE>(sc, make_ray(origin, direction, time), e.blas_root, e.extent, A, stk, LIGHT_STACK);
        } else {
            const PrimRef pr = ldu(&sc.prims[e.first_prim]);
            const SphereD s = ldu(&sc.spheres[pr.index]);
            const V3 center = ld3(s.p1) + (ld3(s.p2) - ld3(s.p1)) * time;
            const double d2 = length_squared(center - origin), r2 = s.r * s.r;
            if (d2 <= r2) {
                pdf = 1.0 / (4.0 * D_PI);
            } else {
                const RayD r = make_ray(origin, direction, time);
                double t;
                V3 c;
                if (hit_sphere(s, r, 0.0, t, c)) pdf = 1.0 / (2.0 * D_PI * sphere_cone_k(r2, d2));
            }
        }
        sum += pdf;
    }
    return sum / (double)sc.n_lights;
}

}  // namespace pt
