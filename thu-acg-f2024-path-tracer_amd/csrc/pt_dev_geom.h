// Device-side primitive intersection (sphere / quad / triangle, optionally under a rigid
// instance), hit-record reconstruction, light-list sampling and camera-ray generation.
// Formulas and comparison strictness follow hittable/{sphere,quad,mesh,instance,hit_info}.rs
// and camera.rs:133-168 operation by operation (see pt_dev_math.h for the contract).
#pragma once
#include "pt_dev_bsdf.h"

namespace pt {

struct RayD {
    V3 o, d;   // d normalised (ray.rs:23-29)
    double time;
};
PT_DEV V3 ray_at(const RayD& r, double t) { return r.o + r.d * t; }
PT_DEV RayD make_ray(V3 o, V3 d, double time) { return RayD{o, normalize(d), time}; }
// instance.rs:36-38 with the analytic rigid inverse
PT_DEV RayD ray_to_local(const InstD& m, const RayD& r) {
    return make_ray(xform_point(m.i0, m.i1, m.i2, m.it, r.o), xform_vector(m.i0, m.i1, m.i2, r.d), r.time);
}

// The pose of a moving instance at `time` (pt_instance_moving's rule, pt_amd.h): pt_instance's operation sequence (pt_graph.cpp
// make_pose) on angle0 + dangle * time and tr0 + dtr * time, so the record equals the static instance's of those two values bit for
// bit. A key pair that does not spin keeps the stored rotation columns and makes no sincos call.
PT_DEV void pose_at(const InstMotionD& k, double time, InstD& m) {
    if (k.spins) {
        const double angle = k.angle0 + k.dangle * time;
        const SinCos h = dev_sincos(angle * 0.5);
        const V3 v = ld3(k.axis) * h.s;
        const double qx = v.x, qy = v.y, qz = v.z, qw = h.c;
        const double x2 = qx + qx, y2 = qy + qy, z2 = qz + qz;
        const double xx = qx * x2, xy = qx * y2, xz = qx * z2;
        const double yy = qy * y2, yz = qy * z2, zz = qz * z2;
        const double wx = qw * x2, wy = qw * y2, wz = qw * z2;
        m.c0[0] = 1.0 - (yy + zz); m.c0[1] = xy + wz; m.c0[2] = xz - wy;
        m.c1[0] = xy - wz; m.c1[1] = 1.0 - (xx + zz); m.c1[2] = yz + wx;
        m.c2[0] = xz + wy; m.c2[1] = yz - wx; m.c2[2] = 1.0 - (xx + yy);
        m.i0[0] = m.c0[0]; m.i0[1] = m.c1[0]; m.i0[2] = m.c2[0];
        m.i1[0] = m.c0[1]; m.i1[1] = m.c1[1]; m.i1[2] = m.c2[1];
        m.i2[0] = m.c0[2]; m.i2[1] = m.c1[2]; m.i2[2] = m.c2[2];
    }
    const V3 t = ld3(k.tr0) + ld3(k.dtr) * time;
    const V3 it = -xform_vector(m.i0, m.i1, m.i2, t);
    m.t[0] = t.x; m.t[1] = t.y; m.t[2] = t.z;
    m.it[0] = it.x; m.it[1] = it.y; m.it[2] = it.z;
}
// Instance record `i` as a ray of time `time` sees it. MOT = false: the stored record — a scalar load when U says the index is
// wave-uniform, else each lane's own. MOT = true (the MOT forms of K2 / K3, the probes): the pose at `time` where the instance
// moves. The record is wave-uniform wherever it was; the pose is per lane, because `time` is.
// Only inst_at<true, U> is ever instantiated: the chain walks below call it in their MOT forms only and keep their statements as they were
// otherwise (MOT = false here says what those statements are: today's load, nothing else) — routed through this function's
// by-value record, four of k_shade's and k_aov's non-MOT kernels came out with other SGPR spill counts, and a scene
// without motion must run the kernels it ran before.
template <bool MOT, bool U = false>
PT_DEV InstD inst_at(const SceneD& sc, int32_t i, double time) {
    InstD m;
    if constexpr (U) m = ldu(&sc.insts[i]); else m = sc.insts[i];
    if constexpr (MOT) {
        if (sc.inst_motion) {   // (null: the scene's motion is its spheres' and the shutter's)
            InstMotionD k;
            if constexpr (U) k = ldu(&sc.inst_motion[i]); else k = sc.inst_motion[i];
            if (k.moves) pose_at(k, time, m);
        }
    }
    return m;
}

// Ray into the object space of a placement: Instance::intersects' transform (instance.rs:36-38, Ray::new re-normalises)
// of every instance of the chain, outermost first, every level at the ray's time. U: the chain is wave-uniform (scalar loads).
// `innermost` receives the last index visited (the start of the way back: to_world_chain).
template <bool U = false, bool MOT = false>
PT_DEV RayD ray_to_local_chain(const SceneD& sc, int32_t outermost, RayD r, int32_t* innermost = nullptr) {
    int32_t last = -1;
    for (int32_t i = outermost; i >= 0;) {
        last = i;
        if constexpr (MOT) {
            const InstD m = inst_at<true, U>(sc, i, r.time);
            r = ray_to_local(m, r);
            i = m.inner;
        } else if constexpr (U) {
            const InstD m = ldu(&sc.insts[i]);
            r = ray_to_local(m, r);
            i = m.inner;
        } else {
            const InstD& m = sc.insts[i];
            r = ray_to_local(m, r);
            i = m.inner;
        }
    }
    if (innermost) *innermost = last;
    return r;
}

// sphere.rs:64-87 — open interval (t_min, +inf)
PT_DEV bool hit_sphere(const SphereD& s, const RayD& r, double t_min, double& t, V3& center) {
    center = ld3(s.p1) + (ld3(s.p2) - ld3(s.p1)) * r.time;
    V3 l = center - r.o;
    double sd = dot(l, r.d);
    double l2 = length_squared(l);
    double r2 = s.r * s.r;
    if (sd < 0.0 && l2 > r2) return false;
    double d2 = l2 - sd * sd;
    if (d2 > r2) return false;
    double q = sqrt(r2 - d2);
    t = l2 > r2 ? sd - q : sd + q;
    if (t <= t_min || t >= D_INF) return false;
    return true;
}
// quad.rs:40-59 — closed interval [t_min, +inf]
PT_DEV bool hit_quad(const QuadD& qd, const RayD& r, double t_min, double& t, double& alpha, double& beta) {
    V3 n = ld3(qd.n);
    double nd = dot(n, r.d);
    if (fabs(nd) < 1e-8) return false;
    t = (qd.d - dot(n, r.o)) / nd;
    if (!(t_min <= t && t <= D_INF)) return false;
    V3 p = ray_at(r, t) - ld3(qd.q);
    V3 w = ld3(qd.w);
    alpha = dot(w, cross(p, ld3(qd.v)));
    beta = dot(w, cross(ld3(qd.u), p));
    if (!(alpha >= 0.0 && alpha <= 1.0) || !(beta >= 0.0 && beta <= 1.0)) return false;
    return true;
}
// mesh.rs:50-82 Moeller-Trumbore — closed interval
PT_DEV bool hit_tri(const TriD& tr, const RayD& r, double t_min, double& t, double& u, double& v) {
    V3 v0 = ld3(tr.v0);
    V3 edge1 = ld3(tr.v1) - v0, edge2 = ld3(tr.v2) - v0;
    V3 h = cross(r.d, edge2);
    double a = dot(edge1, h);
    if (fabs(a) < 1e-8) return false;
    double f = 1.0 / a;
    V3 s = r.o - v0;
    u = f * dot(s, h);
    if (!(u >= 0.0 && u <= 1.0)) return false;
    V3 q = cross(s, edge1);
    v = f * dot(r.d, q);
    if (v < 0.0 || u + v > 1.0) return false;
    t = f * dot(edge2, q);
    if (!(t_min <= t && t <= D_INF)) return false;
    return true;
}

// hit_info.rs:57-67
PT_DEV void tangent_basis(V3 n, V3& tangent, V3& bitangent) {
    V3 a = fabs(n.x) > 0.9 ? V3{0.0, 1.0, 0.0} : V3{1.0, 0.0, 0.0};
    tangent = normalize(cross(n, a));
    bitangent = cross(n, tangent);
}
// HitInfo::new hit_info.rs:16-55
// UM: `mat` is wave-uniform (lights.pdf walks the lights list in step): the material's normal-map handle arrives by a scalar load —
// a vector load there would make the pure-arithmetic stretch of k_shade wait for the record prefetch it is meant to hide.
template <bool UM = false>
PT_DEV void finish_hit(const SceneD& sc, const RayD& r, V3 point, V3 normal, double dist, uint32_t mat, double u,
                       double v, HitD& h) {
    h.front = dot(r.d, normal) < 0.0;
    V3 nn = normalize(normal);
    h.gn = h.front ? nn : -nn;
    int32_t nm;
    if constexpr (UM) nm = ldu(&sc.mats[mat].nmap_tex); else nm = sc.mats[mat].nmap_tex;
    if (nm >= 0) {
        V3 m = 2.0 * tex_image(sc, sc.tex[nm], u, v) - splat(1.0);
        V3 t, b;
        tangent_basis(h.gn, t, b);
        h.sn = normalize(m.x * t + m.y * b + m.z * h.gn);
    } else {
        h.sn = h.gn;
    }
    h.point = point;
    h.dist = dist;
    h.mat = mat;
    h.u = u;
    h.v = v;
}

// Rebuilds the reference's HitInfo for the primitive of record `pr`, known to be hit by `world_ray`.
// Re-runs that one primitive's intersection (same arithmetic as the traversal kernel, so the
// same t/u/v bits), then applies Instance::intersects' world transform (instance.rs:43-53, Q1).
// UV = false (k_shade): a sphere whose record lacks PRIM_NEEDS_UV gets u = v = 0 — the host has proved that nothing reads them
// (pt_types.h) — and neither dev_acos, dev_atan2 nor the two divisions are computed. UV = true (probe, AOV walk): always computed.
// U: `pr` is wave-uniform and no triangle (k_shade's single-primitive groups): the instance chain, the sphere / quad record and the
// material's normal-map handle arrive by scalar loads instead of a chain of dependent per-lane gathers of the same bytes.
template <bool UV = true, bool U = false, bool MOT = false>
PT_DEV bool reconstruct_hit_prim(const SceneD& sc, const RayD& world_ray, const PrimRef& pr, double t_min, HitD& h) {
    int32_t innermost = -1;
    const RayD r = ray_to_local_chain<U, MOT>(sc, pr.inst, world_ray, &innermost);
    const uint32_t kind = pr.kind & 0xFFu;
    if (kind == PRIM_SPHERE) {
        double t;
        V3 c;
        bool ok;
        if constexpr (U) ok = hit_sphere(ldu(&sc.spheres[pr.index]), r, t_min, t, c);
        else ok = hit_sphere(sc.spheres[pr.index], r, t_min, t, c);
        if (!ok) return false;
        V3 point = ray_at(r, t);
        V3 normal = normalize(point - c);
        double u = 0.0, v = 0.0;
        if (UV || (pr.kind & PRIM_NEEDS_UV)) {
            double theta = dev_acos(-normal.y);                   // sphere.rs:52-56
            double phi = dev_atan2(-normal.z, normal.x) + D_PI;
            u = phi / (2.0 * D_PI);
            v = theta / D_PI;
        }
        finish_hit<U>(sc, r, point, normal, t, pr.mat, u, v, h);
    } else if (U || kind == PRIM_QUAD) {
        double t, a, b;
        if constexpr (U) {
            const QuadD q = ldu(&sc.quads[pr.index]);
            if (!hit_quad(q, r, t_min, t, a, b)) return false;
            finish_hit<true>(sc, r, ray_at(r, t), ld3(q.n), t, pr.mat, a, b, h);
        } else {
            const QuadD& q = sc.quads[pr.index];
            if (!hit_quad(q, r, t_min, t, a, b)) return false;
            finish_hit(sc, r, ray_at(r, t), ld3(q.n), t, pr.mat, a, b, h);
        }
    } else {
        double t, u, v;
        const TriD& tr = sc.tris[pr.index];
        if (!hit_tri(tr, r, t_min, t, u, v)) return false;
        V3 v0 = ld3(tr.v0);
        V3 edge1 = ld3(tr.v1) - v0, edge2 = ld3(tr.v2) - v0;
        double w = 1.0 - u - v;
        V3 normal;
        double tu = u, tv = v;
        if (pr.kind & PRIM_HAS_NORMALS) {                    // mesh.rs:85-87
            const TriAttr& at = sc.tri_attr[pr.index];
            normal = normalize(ld3(at.n[0]) * w + ld3(at.n[1]) * u + ld3(at.n[2]) * v);
        } else {
            normal = normalize(cross(edge1, edge2));          // flat shading :88
        }
        if (pr.kind & PRIM_HAS_UVS) {                        // mesh.rs:91-99
            const TriAttr& at = sc.tri_attr[pr.index];
            tu = at.uv[0][0] * w + at.uv[1][0] * u + at.uv[2][0] * v;
            tv = at.uv[0][1] * w + at.uv[1][1] * u + at.uv[2][1] * v;
        }
        finish_hit(sc, r, ray_at(r, t), normal, t, pr.mat, tu, tv, h);
    }
    for (int32_t i = innermost; i >= 0;) {                                       // instance.rs:43-53, innermost instance first
        if constexpr (MOT) {
            const InstD m = inst_at<true, U>(sc, i, world_ray.time);
            h.point = xform_point(m.c0, m.c1, m.c2, m.t, h.point);
            h.gn = normalize(xform_vector(m.c0, m.c1, m.c2, h.gn));
            i = m.outer;
        } else if constexpr (U) {
            const InstD m = ldu(&sc.insts[i]);
            h.point = xform_point(m.c0, m.c1, m.c2, m.t, h.point);
            h.gn = normalize(xform_vector(m.c0, m.c1, m.c2, h.gn));
            i = m.outer;
        } else {
            const InstD& m = sc.insts[i];
            h.point = xform_point(m.c0, m.c1, m.c2, m.t, h.point);
            h.gn = normalize(xform_vector(m.c0, m.c1, m.c2, h.gn));
            i = m.outer;
        }
    }
    return true;
}
// ... for primitive `gid`, each lane its own
template <bool UV = true, bool MOT = false>
PT_DEV bool reconstruct_hit(const SceneD& sc, const RayD& world_ray, uint32_t gid, double t_min, HitD& h) {
    const PrimRef pr = sc.prims[gid];
    return reconstruct_hit_prim<UV, false, MOT>(sc, world_ray, pr, t_min, h);
}

// ---- lights list: Hittable::sample / pdf for every kind of object (list.rs:78-96, quad.rs:80-98,
// sphere.rs:110-135, mesh.rs:122-141, cuboid.rs:78-84, instance.rs:64-75) ---------------------------
template <class R>
PT_DEV V3 sample_quad_dir(const QuadD& q, V3 origin, R& rng) {                  // quad.rs:80-86
    uint64_t ua, ub;
    rng_u64x2(rng, ua, ub);                                                        // two consecutive draws: one Philox block when they share it
    double a = u64_to_unit(ua), b = u64_to_unit(ub);
    V3 point = ld3(q.q) + ld3(q.u) * a + ld3(q.v) * b;
    return normalize(point - origin);
}
PT_DEV double pdf_quad(const SceneD& sc, const QuadD& q, uint32_t mat, V3 origin, V3 direction, double time) {   // quad.rs:88-98
    RayD r = make_ray(origin, direction, time);
    double t, al, be;
    if (!hit_quad(q, r, 0.0, t, al, be)) return 0.0;
    HitD h;
    finish_hit<true>(sc, r, ray_at(r, t), ld3(q.n), t, mat, al, be, h);   // (every caller hands a wave-uniform material: lights_pdf)
    double area = length(cross(ld3(q.u), ld3(q.v)));
    double cos_theta = fabs(dot(r.d, h.sn));
    return (h.dist * h.dist) / (cos_theta * area);
}
// ONE: the lights list has a single entry (the Cornell box, scene 7): the index draw still happens (list.rs:82 draws it), but the
// light is the same for every lane, so its entry, transform chain and quad / sphere record arrive by scalar loads instead of four
// DEPENDENT vector gathers (lights[i] -> entries -> prims -> quads, ~700 cycles each in k_shade).
template <bool ONE, bool MOT, class R>
PT_DEV V3 lights_sample_impl(const SceneD& sc, V3 origin_w, double time, R& rng) {
    uint32_t i = rng_index(rng, sc.n_lights);
    Entry e;
    if constexpr (ONE) e = ldu(&sc.entries[ldu(&sc.lights[0])]); else e = sc.entries[sc.lights[i]];
    V3 origin = origin_w;
    int32_t innermost = -1;
    for (int32_t k = e.inst; k >= 0;) {                                           // instance.rs:64-66, outermost instance first
        if constexpr (MOT) {
            const InstD m = inst_at<true, ONE>(sc, k, time);   // the pose at the path's time
            origin = xform_point(m.i0, m.i1, m.i2, m.it, origin);
            innermost = k;
            k = m.inner;
        } else if constexpr (ONE) {
            const InstD m = ldu(&sc.insts[k]);
            origin = xform_point(m.i0, m.i1, m.i2, m.it, origin);
            innermost = k;
            k = m.inner;
        } else {
            const InstD& m = sc.insts[k];
            origin = xform_point(m.i0, m.i1, m.i2, m.it, origin);
            innermost = k;
            k = m.inner;
        }
    }
    V3 dir;
    if (e.kind == ENTRY_QUAD) {
        if constexpr (ONE) {
            const PrimRef pr = ldu(&sc.prims[e.first_prim]);
            const QuadD qd = ldu(&sc.quads[pr.index]);
            dir = sample_quad_dir(qd, origin, rng);
        } else {
            dir = sample_quad_dir(sc.quads[sc.prims[e.first_prim].index], origin, rng);
        }
    } else if (e.kind == ENTRY_CUBOID) {                                          // cuboid.rs:78-80 -> list.rs:78-84
        uint32_t j = rng_index(rng, 6u);
        dir = sample_quad_dir(sc.quads[sc.prims[e.first_prim + j].index], origin, rng);
    } else if (e.kind == ENTRY_MESH) {                                            // mesh.rs:207-209 -> :122-129
        uint32_t j = rng_index(rng, e.n_prims);
        const TriD& tr = sc.tris[sc.prims[e.first_prim + j].index];
        double u = rng_f64(rng), v = rng_f64(rng);
        double w = 1.0 - u - v;
        V3 point = ld3(tr.v0) * w + ld3(tr.v1) * u + ld3(tr.v2) * v;
        dir = normalize(point - origin);
    } else {                                                                      // sphere.rs:110-122
        const SphereD& s = sc.spheres[sc.prims[e.first_prim].index];
        double a = rng_f64(rng), b = rng_f64(rng);
        double theta = 2.0 * D_PI * a;
        double phi = dev_acos(2.0 * b - 1.0);
        const SinCos scp = dev_sincos(phi), sct = dev_sincos(theta);
        const double sp = scp.s, cp = scp.c, st = sct.s, ct = sct.c;
        V3 center = ld3(s.p1) + (ld3(s.p2) - ld3(s.p1)) * time;
        V3 point = center + V3{sp * ct, sp * st, cp} * s.r;
        dir = normalize(point - origin);
    }
    for (int32_t k = innermost; k >= 0;) {                                        // instance.rs:67-68 (not re-normalised)
        if constexpr (MOT) {
            const InstD m = inst_at<true, false>(sc, k, time);
            dir = xform_vector(m.c0, m.c1, m.c2, dir);
            k = m.outer;
        } else {
            const InstD& m = sc.insts[k];
            dir = xform_vector(m.c0, m.c1, m.c2, dir);
            k = m.outer;
        }
    }
    return dir;
}
template <bool MOT = false, class R>
PT_DEV V3 lights_sample(const SceneD& sc, V3 origin_w, double time, R& rng) {
    if (sc.n_lights == 1u) return lights_sample_impl<true, MOT>(sc, origin_w, time, rng);
    return lights_sample_impl<false, MOT>(sc, origin_w, time, rng);
}
template <bool MOT = false>
PT_DEV double lights_pdf(const SceneD& sc, V3 origin_w, V3 direction_w, double time) {
    if (sc.n_lights == 0) return 0.0;
    double sum = 0.0;
    for (uint32_t i = 0; i < sc.n_lights; ++i) {                                  // the light index is wave-uniform: scalar loads (ldu)
        const Entry e = ldu(&sc.entries[ldu(&sc.lights[i])]);
        V3 origin = origin_w, direction = direction_w;
        for (int32_t k = e.inst; k >= 0;) {                                       // instance.rs:71-75, outermost instance first
            if constexpr (MOT) {
                const InstD m = inst_at<true, true>(sc, k, time);
                origin = xform_point(m.i0, m.i1, m.i2, m.it, origin);
                direction = xform_vector(m.i0, m.i1, m.i2, direction);
                k = m.inner;
            } else {
                const InstD m = ldu(&sc.insts[k]);
                origin = xform_point(m.i0, m.i1, m.i2, m.it, origin);
                direction = xform_vector(m.i0, m.i1, m.i2, direction);
                k = m.inner;
            }
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
        } else if (e.kind == ENTRY_MESH) {                                        // list.rs:86-96 over ALL triangles (O(n), like the reference)
            double sn = 0.0;
            RayD r = make_ray(origin, direction, time);
            for (uint32_t j = 0; j < e.n_prims; ++j) {
                const PrimRef pr = sc.prims[e.first_prim + j];
                const TriD& tr = sc.tris[pr.index];
                double t, u, v, p = 0.0;
                if (hit_tri(tr, r, 0.0, t, u, v)) {                               // mesh.rs:131-141
                    V3 v0 = ld3(tr.v0);
                    V3 edge1 = ld3(tr.v1) - v0, edge2 = ld3(tr.v2) - v0;
                    double w = 1.0 - u - v;
                    V3 normal;
                    double tu = u, tv = v;
                    if (pr.kind & PRIM_HAS_NORMALS) {
                        const TriAttr& at = sc.tri_attr[pr.index];
                        normal = normalize(ld3(at.n[0]) * w + ld3(at.n[1]) * u + ld3(at.n[2]) * v);
                    } else {
                        normal = normalize(cross(edge1, edge2));
                    }
                    if (pr.kind & PRIM_HAS_UVS) {
                        const TriAttr& at = sc.tri_attr[pr.index];
                        tu = at.uv[0][0] * w + at.uv[1][0] * u + at.uv[2][0] * v;
                        tv = at.uv[0][1] * w + at.uv[1][1] * u + at.uv[2][1] * v;
                    }
                    HitD h;
                    finish_hit(sc, r, ray_at(r, t), normal, t, pr.mat, tu, tv, h);
                    double area = 0.5 * length(cross(edge1, edge2));
                    double cos_theta = fabs(dot(direction, h.sn));            // `direction`, not the normalised ray (mesh.rs:136)
                    p = h.dist * h.dist / (cos_theta * area);
                }
                sn += p;
            }
            pdf = sn / (double)e.n_prims;
        } else {                                                                  // sphere.rs:124-135
            const SphereD& s = sc.spheres[sc.prims[e.first_prim].index];
            RayD r = make_ray(origin, direction, time);
            double t;
            V3 c;
            if (hit_sphere(s, r, 0.0, t, c)) {
                double r2 = s.r * s.r;
                V3 center = ld3(s.p1) + (ld3(s.p2) - ld3(s.p1)) * time;
                double solid_angle = 2.0 * D_PI * sqrt(1.0 - r2 / length_squared(center - origin));
                pdf = 1.0 / solid_angle;
            }
        }
        sum += pdf;
    }
    return sum / (double)sc.n_lights;
}

// ---- camera.rs:133-168 -----------------------------------------------------------------
template <class R>
PT_DEV void random_offsets(R& rng, double& ox, double& oy) {
    uint64_t a, b;
    rng_u64x2(rng, a, b);
    double radius = sqrt(u64_to_unit(a));
    double angle = u64_to_unit(b) * 2.0 * D_PI;
    const SinCos sc_angle = dev_sincos(angle);
    const double sn = sc_angle.s, cs = sc_angle.c;
    ox = radius * cs;
    oy = radius * sn;
}
// The directions of the fisheye and panorama projections (pt_scene_set_projection kinds 2 and 3; the rule is in include/pt_amd.h,
// DESIGN.md §18) for the continuous pixel coordinates fy = row + bx, fx = col + by.
// z: a zero the compiler cannot see through. The CamD fields that only kinds 1-3 read are loaded at field[z]: a plain load of a kernel
// argument is hoisted to the kernel's entry, and 30 more SGPRs live across every call of K1 / K3 cost the perspective camera's kernels
// registers and scratch; a load whose address depends on an instruction of the cold branch stays in it.
PT_DEV V3 projected_direction(const CamD& cam, double fy, double fx) {
    uint32_t z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    const double W = (&cam.fw)[z], H = (&cam.fh)[z];
    if (cam.projection == PROJ_FISHEYE) {
        const double xn = (2.0 * (fx + 0.5) - W) / H, yn = (H - 2.0 * (fy + 0.5)) / H;
        const double rho = sqrt((xn * xn) + (yn * yn));
        const SinCos t = dev_sincos(fmin(rho * (&cam.th)[z], D_PI));
        const double a = rho > 0.0 ? t.s / rho : 0.0;
        return (ld3(cam.right + z) * (xn * a)) + (ld3(cam.up + z) * (yn * a)) - (ld3(cam.forward + z) * t.c);
    }
    // PROJ_PANORAMA: sample_environment's convention, in world axes
    const double phi = -D_PI + ((2.0 * D_PI) * (fx + 0.5)) / W;
    const double theta = fmin(fmax((D_PI * (fy + 0.5)) / H, 0.0), D_PI);
    const SinCos t = dev_sincos(theta), p = dev_sincos(phi);
    return V3{t.s * p.c, t.c, t.s * p.s};
}
// The branches on cam.projection are wave-uniform (cam is a kernel argument) and not taken by the perspective camera (kind 0), whose
// arithmetic below is the reference's; every kind makes kind 0's draws in kind 0's order.
// MOT (the MOT forms of K1 / K3, and the probes when motion is in effect): the shutter maps the time draw u to open + span * u — with the
// default (0, 1) those are u's bits. The number and order of draws are the same.
template <bool MOT = false, class R>
PT_DEV RayD generate_ray(const CamD& cam, uint32_t row, uint32_t col, R& rng) {
    double bx, by;
    random_offsets(rng, bx, by);
    bx = bx * cam.blur_strength;
    by = by * cam.blur_strength;
    V3 sample_location = ld3(cam.pixel00) + (ld3(cam.pixel_dv) * ((double)row + bx)) + (ld3(cam.pixel_du) * ((double)col + by));
    if (cam.projection >= PROJ_FISHEYE)   // fisheye, panorama: the ray's direction w takes the sample location's place
        sample_location = projected_direction(cam, (double)row + bx, (double)col + by);
    V3 origin = ld3(cam.center);
    if (cam.projection == PROJ_ORTHOGRAPHIC) {   // O = S + forward * F, in the plane through center (z: see projected_direction)
        uint32_t z;
        asm volatile("s_mov_b32 %0, 0" : "=s"(z));
        origin = sample_location + (ld3(cam.forward + z) * (&cam.focal_length)[z]);
    }
    if (cam.lens_zero) {
        rng_skip2(rng);   // the two lens draws are made all the same (camera.rs:160); their products with a zero radius add nothing
    } else {
        double px, py;
        random_offsets(rng, px, py);
        origin = origin + (ld3(cam.dof_right) * px) + (ld3(cam.dof_up) * py);
    }
    double time = 0.0;
    if (cam.motionless) ++rng.draw;   // drawn all the same (camera.rs:165); no result depends on it (CamD::motionless), so its Philox block is not computed
    else time = rng_f64(rng);
    if constexpr (MOT) time = cam.shutter_open + cam.shutter_span * time;
    return make_ray(origin, cam.projection >= PROJ_FISHEYE ? sample_location : sample_location - origin, time);
}
// camera.rs:140-151
PT_DEV V3 sample_environment(const SceneD& sc, const CamD& cam, V3 d) {
    if (!cam.env_is_map) return ld3(cam.env_color);
    double theta = dev_acos(d.y);
    double phi = dev_atan2(d.z, d.x);
    double u = (phi + D_PI) / (2.0 * D_PI);
    double v = 1.0 - theta / D_PI;
    return tex_image(sc, ldu(&sc.tex[cam.env_tex]), u, v);   // the environment's descriptor is the same for every lane
}

}  // namespace pt
