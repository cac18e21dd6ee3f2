// Device-side participating media (the rules are in include/pt_amd.h). Homogeneous (pt_mat_medium): the free-flight
// distance and the Henyey-Greenstein phase function. Grid density (pt_mat_medium_grid): the trilinear density, the
// clip of a segment to the grid's box and the delta-tracking loop. Called by k_shade's MED / HET forms and by the probe behind
// pt_medium_probe — the same functions, so what the probe returns is what a path computes. Interior media and chromatic absorption
// (pt_mat_glass_set_interior, pt_mat_medium_tinted): the absorption coefficients of a medium's record and the
// Beer-Lambert attenuation of a segment, called by k_shade's INT forms.
#pragma once
#include "pt_dev_math.h"
#include "pt_types.h"

namespace pt {

// a real function like dev_log2 (pt_dev_math.h): k_shade's MED forms hold the logarithm once
PT_DM_CALL double dev_log(double x) { return detmath::log(x); }

// the medium record of a path's medium word (PoolD bounce word >> MEDIUM_SHIFT = material index + 1)
struct MediumD {
    double density, g;
    V3 albedo;
    bool bounded;   // some world object carries this material: a ray that left the scene cannot be inside it
};
PT_DEV MediumD load_medium(const SceneD& sc, uint32_t med) {
    const MatD& m = sc.mats[med - 1u];
    return MediumD{m.p[0], m.p[1], V3{m.p[2], m.p[3], m.p[4]}, m.p[5] != 0.0};
}
// pt_mat_medium_tinted's absorption coefficients (MatD::p[7..9]; zero for every other medium) — read by the INT forms only, where they
// are used, so that they do not stay live across the free flight
PT_DEV V3 load_absorption(const SceneD& sc, uint32_t med) {
    const MatD& m = sc.mats[med - 1u];
    return V3{m.p[7], m.p[8], m.p[9]};
}

// a real function like dev_log: k_shade's INT forms hold the exponential once
PT_DM_CALL double dev_exp(double x) { return detmath::exp(x); }
// Beer-Lambert along a segment of length l (+inf on a miss) in a medium with absorption a: thr_c *= exp(-(a_c * l)), the product formed
// first; a channel with a_c == 0 is not touched (no 0 * inf)
PT_DEV V3 medium_absorb(V3 a, V3 thr, double l) {
    if (a.x > 0.0) thr.x = thr.x * dev_exp(-(a.x * l));
    if (a.y > 0.0) thr.y = thr.y * dev_exp(-(a.y * l));
    if (a.z > 0.0) thr.z = thr.z * dev_exp(-(a.z * l));
    return thr;
}

// d = -log(1 - u) / density, u in [0, 1)
PT_DEV double medium_free_flight(double u, double density) { return -dev_log(1.0 - u) / density; }

// ph(c) = (1 - g^2) / (4 pi s sqrt(s)), s = 1 + g^2 - 2 g c, c = the cosine between the propagation direction and the new one
PT_DEV double hg_phase(double g, double c) {
    const double s = 1.0 + g * g - 2.0 * g * c;
    return (1.0 - g * g) / (4.0 * D_PI * s * sqrt(s));
}
// The direction two unit draws give: cos_t by the inverse of HG's CDF (isotropic below |g| = 1e-3), phi = 2 pi u2, expressed in the
// shading frame built around `axis` (frame_to_z) — `axis` is the propagation direction, g > 0 scatters forward.
PT_DEV V3 hg_sample(double g, double u1, double u2, V3 axis) {
    double cos_t;
    if (fabs(g) < 1e-3) {
        cos_t = 1.0 - 2.0 * u1;
    } else {
        const double q = (1.0 - g * g) / (1.0 - g + 2.0 * g * u1);
        cos_t = (1.0 + g * g - q * q) / (2.0 * g);
    }
    cos_t = clampd(cos_t, -1.0, 1.0);
    const double sin_t = sqrt(fmax(0.0, 1.0 - cos_t * cos_t));
    const double phi = 2.0 * D_PI * u2;
    const SinCos sc_phi = dev_sincos(phi);
    const Frame f = frame_to_z(axis);
    return to_world(f, V3{sin_t * sc_phi.c, sin_t * sc_phi.s, cos_t});
}


// ---- grid-density media (pt_mat_medium_grid) ----------------------------------------------------------------------------------
// sigma(x) = scale * V(x); 0 outside the box (a NaN coordinate counts as outside). Per axis q = (x - lo) * cells - 0.5 clamped to
// [0, n - 1], i = min(floor(q), n - 2), f = q - i; V blends the eight corners x pairs first, then y, then z, each as a + f * (b - a).
// The eight loads are issued together, before the first use.
PT_DEV double grid_sigma(const GridD& g, const float* vals, V3 x) {
    if (!(x.x >= g.lo[0] && x.x <= g.hi[0] && x.y >= g.lo[1] && x.y <= g.hi[1] && x.z >= g.lo[2] && x.z <= g.hi[2])) return 0.0;
    const double qx = clampd((x.x - g.lo[0]) * g.cells[0] - 0.5, 0.0, (double)(g.nx - 1u));
    const double qy = clampd((x.y - g.lo[1]) * g.cells[1] - 0.5, 0.0, (double)(g.ny - 1u));
    const double qz = clampd((x.z - g.lo[2]) * g.cells[2] - 0.5, 0.0, (double)(g.nz - 1u));
    uint32_t ix = (uint32_t)qx, iy = (uint32_t)qy, iz = (uint32_t)qz;          // q >= 0: truncation is floor
    if (ix > g.nx - 2u) ix = g.nx - 2u;
    if (iy > g.ny - 2u) iy = g.ny - 2u;
    if (iz > g.nz - 2u) iz = g.nz - 2u;
    const double fx = qx - (double)ix, fy = qy - (double)iy, fz = qz - (double)iz;
    const float* p0 = vals + g.ofs + ((uint64_t)iz * g.ny + iy) * g.nx + ix;     // corner (ix, iy, iz); the host checked nx*ny*nz <= 2^28
    const float* p1 = p0 + (uint64_t)g.nx * g.ny;
    const float a000 = p0[0], a100 = p0[1], a010 = p0[g.nx], a110 = p0[g.nx + 1u];
    const float a001 = p1[0], a101 = p1[1], a011 = p1[g.nx], a111 = p1[g.nx + 1u];
    const double v000 = a000, v100 = a100, v010 = a010, v110 = a110, v001 = a001, v101 = a101, v011 = a011, v111 = a111;
    const double c00 = v000 + fx * (v100 - v000), c10 = v010 + fx * (v110 - v010);
    const double c01 = v001 + fx * (v101 - v001), c11 = v011 + fx * (v111 - v011);
    const double c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    return g.scale * (c0 + fz * (c1 - c0));
}

// The part [t0, t1] of the segment o + s * d, 0 <= s <= t, inside the grid's box, by the slab test: per axis with d_a != 0,
// ta = (lo_a - o_a) * (1 / d_a), tb = (hi_a - o_a) * (1 / d_a), near = the smaller, far = the larger; an axis with d_a == 0 bounds
// nothing when lo_a <= o_a <= hi_a and empties the interval otherwise. t0 = max(largest near, 0), t1 = min(smallest far, t).
// False — nothing to track — unless t0 < t1 and t1 is finite; a non-finite component of o or d gives false.
PT_DEV bool grid_clip(const GridD& g, V3 o, V3 d, double t, double& t0, double& t1) {
    const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    double tn = 0.0, tf = t;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ok = ok && fabs(oo[a]) < D_INF && fabs(dd[a]) < D_INF;                 // (false for NaN)
        if (dd[a] == 0.0) {
            ok = ok && oo[a] >= g.lo[a] && oo[a] <= g.hi[a];
        } else {
            const double inv = 1.0 / dd[a];
            const double ta = (g.lo[a] - oo[a]) * inv, tb = (g.hi[a] - oo[a]) * inv;
            const double near = ta < tb ? ta : tb, far = ta < tb ? tb : ta;
            if (near > tn) tn = near;
            if (far < tf) tf = far;
        }
    }
    t0 = tn;
    t1 = tf;
    return ok && tn < tf && tf < D_INF;
}

// Delta (Woodcock) tracking along the clipped segment at the majorant mu: s = t0; then a single draw u, s += -log(1 - u) / mu;
// s >= t1: no collision; else a single draw v: a collision at o + s * d when v * mu < sigma(o + s * d), else on. `trips` counts the
// tentative collisions (the v draws). The expected trip count is mu * (t1 - t0), which the host bounds by 4096 for a unit direction
// (pt_mat_medium_grid); every step is finite and t1 is finite, so the loop ends.
// A real function like dev_sincos: k_shade's HET forms hold the loop once, outside the allocation of the bounce around it.
struct GridTrack {
    double s;               // the collision's ray parameter (0 without one)
    uint32_t collided, draw, trips;   // draw: the generator's draw index after the loop
};
template <class R> PT_DM_CALL GridTrack grid_track(const GridD* gp, const float* vals, V3 o, V3 d, double t, R rng) {
    const GridD g = *gp;
    GridTrack out{0.0, 0u, rng.draw, 0u};
    double s, t1;
    if (!grid_clip(g, o, d, t, s, t1)) return out;
    for (;;) {
        s += -dev_log(1.0 - rng_f64(rng)) / g.mu;
        if (!(s < t1)) break;
        const double v = rng_f64(rng);
        ++out.trips;
        if (v * g.mu < grid_sigma(g, vals, o + d * s)) {
            out.collided = 1u;
            out.s = s;
            break;
        }
    }
    out.draw = rng.draw;
    return out;
}

}  // namespace pt
