// Punctual lights (the rule: include/pt_amd.h): what a light of the list sends to a point, and how far a shadow ray's
// origin is from it. Plain f64 on arrays of doubles, one rounding per written operation, compiled for the device (k_shade's PLT forms,
// k_punctual_probe) and for the host (pt_punctual_eval): the same function on both sides, so a CPU test holds what the kernels run.
#pragma once
#include "pt_detmath.h"
#include "pt_types.h"

#define PT_PL PT_DM   // host and device under hipcc, host elsewhere

namespace pt {

// w: the unit direction from the point to the light; D: the distance (+inf for a directional light); d2 = D * D before the root (1 for a
// directional light: never an ending); E: what arrives per unit area facing the light.
struct PunctualEval {
    double w[3], D, d2, E[3];
};
PT_PL PunctualEval punctual_eval(const PunctualD& L, const double x[3]) {
    PunctualEval r;
    if (L.kind == 2u) {
        r.w[0] = -L.axis[0]; r.w[1] = -L.axis[1]; r.w[2] = -L.axis[2];
        r.D = __builtin_huge_val();
        r.d2 = 1.0;
        r.E[0] = L.I[0]; r.E[1] = L.I[1]; r.E[2] = L.I[2];
        return r;
    }
    const double lx = L.pos[0] - x[0], ly = L.pos[1] - x[1], lz = L.pos[2] - x[2];
    const double d2 = (lx * lx) + (ly * ly) + (lz * lz);
    const double D = __builtin_sqrt(d2);
    r.w[0] = lx / D; r.w[1] = ly / D; r.w[2] = lz / D;
    r.D = D;
    r.d2 = d2;
    if (L.kind == 1u) {
        const double c = -((r.w[0] * L.axis[0]) + (r.w[1] * L.axis[1]) + (r.w[2] * L.axis[2]));
        double s;
        if (L.cos_i > L.cos_o) {
            s = (c - L.cos_o) / (L.cos_i - L.cos_o);
            if (s < 0.0) s = 0.0;
            if (s > 1.0) s = 1.0;
        } else {
            s = c >= L.cos_o ? 1.0 : 0.0;
        }
        const double fall = (s * s) * (3.0 - 2.0 * s);
        r.E[0] = (L.I[0] * fall) / d2; r.E[1] = (L.I[1] * fall) / d2; r.E[2] = (L.I[2] * fall) / d2;
    } else {
        r.E[0] = L.I[0] / d2; r.E[1] = L.I[1] / d2; r.E[2] = L.I[2] / d2;
    }
    return r;
}
// D' of a SHADOW segment: from the stored ray origin o to the light; +inf for a directional light
PT_PL double punctual_shadow_distance(const PunctualD& L, const double o[3]) {
    if (L.kind == 2u) return __builtin_huge_val();
    const double lx = L.pos[0] - o[0], ly = L.pos[1] - o[1], lz = L.pos[2] - o[2];
    return __builtin_sqrt((lx * lx) + (ly * ly) + (lz * lz));
}

// ---- the light grid (the rule: include/pt_amd.h "the light grid") ----
// The same functions build a row on the device (k_punctual_grid, pt_k3_plt.hip) and on the host (pt_punctual_grid_row), and pick a light
// in k_shade's PLT / light-shaft forms, the probe and pt_punctual_grid_select.
struct PunctualCell {
    double a[3], b[3], m[3], rc2;   // the cell's corners, its centre, its squared half-diagonal
};
PT_PL uint32_t punctual_grid_axis(double x, double lo, double inv, uint32_t n) {
    const double q = (x - lo) * inv;
    return q >= 0.0 ? (q < (double)n ? (uint32_t)q : n - 1u) : 0u;   // (a NaN takes cell 0)
}
PT_PL uint32_t punctual_grid_cell(const PunctualGridD& g, const double x[3]) {
    const uint32_t ix = punctual_grid_axis(x[0], g.lo[0], g.inv[0], g.n[0]), iy = punctual_grid_axis(x[1], g.lo[1], g.inv[1], g.n[1]),
                   iz = punctual_grid_axis(x[2], g.lo[2], g.inv[2], g.n[2]);
    return (iz * g.n[1] + iy) * g.n[0] + ix;
}
PT_PL PunctualCell punctual_grid_geometry(const double box[6], const uint32_t dims[3], uint32_t cell) {
    const uint32_t i[3] = {cell % dims[0], (cell / dims[0]) % dims[1], cell / (dims[0] * dims[1])};
    PunctualCell c;
    double h[3];
    for (int ax = 0; ax < 3; ++ax) {
        const double s = (box[3 + ax] - box[ax]) / (double)dims[ax];
        c.a[ax] = box[ax] + (double)i[ax] * s;
        c.b[ax] = box[ax] + (double)(i[ax] + 1u) * s;
        c.m[ax] = (c.a[ax] + c.b[ax]) * 0.5;
        h[ax] = (c.b[ax] - c.a[ax]) * 0.5;
    }
    c.rc2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    return c;
}
// the importance of light L for the cell: its luminous sum over the squared distance to the cell (the half-diagonal keeps it finite inside),
// zero for a spot whose outer cone misses the cell's bounding sphere
PT_PL double punctual_grid_weight(const PunctualD& L, const PunctualCell& c) {
    const double Y = (L.I[0] + L.I[1]) + L.I[2];
    if (L.kind == 2u) return Y;
    double t[3];
    for (int ax = 0; ax < 3; ++ax) {
        const double p = L.pos[ax];
        t[ax] = p < c.a[ax] ? c.a[ax] - p : (p > c.b[ax] ? p - c.b[ax] : 0.0);
    }
    const double dmin2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    double w = Y / (dmin2 + c.rc2);
    if (L.kind == 1u) {
        const double vx = c.m[0] - L.pos[0], vy = c.m[1] - L.pos[1], vz = c.m[2] - L.pos[2];
        const double d2 = (vx * vx + vy * vy) + vz * vz;
        if (d2 > c.rc2) {
            const double d = __builtin_sqrt(d2);
            const double sa = __builtin_sqrt(c.rc2) / d, ca = __builtin_sqrt(1.0 - sa * sa);
            const double c_m = ((vx * L.axis[0] + vy * L.axis[1]) + vz * L.axis[2]) / d;
            const double s2 = 1.0 - L.cos_o * L.cos_o;
            const double so = __builtin_sqrt(s2 > 0.0 ? s2 : 0.0);
            const double c_far = L.cos_o * ca - so * sa;
            if (L.cos_o > -ca && c_m < c_far - 1e-9) w = 0.0;
        }
    }
    return w;
}
// One row: light(k) hands out record k, put(k, C) takes C[k]; both run in ascending k, the weights are formed twice (sum, then CDF) so
// that no row is read back.
template <class Light, class Put> PT_PL void punctual_grid_row(Light&& light, uint32_t n, const PunctualCell& c, Put&& put) {
    double W = 0.0;
    for (uint32_t k = 0; k < n; ++k) W = W + punctual_grid_weight(light(k), c);
    const bool by_weight = W > 0.0 && W - W == 0.0;   // (finite and positive)
    const double u = 1.0 / (double)n, floor_p = 0.125 / (double)n;
    double C = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        const double p = by_weight ? 0.875 * (punctual_grid_weight(light(k), c) / W) + floor_p : u;
        C = C + p;
        put(k, k + 1u == n ? 1.0 : C);
    }
}
// the smallest k with u < C[k] (C[n - 1] = 1 > u), and p = C[k] - C[k - 1]
PT_PL uint32_t punctual_select(const double* row, uint32_t n, double u, double& p) {
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (u < row[mid]) hi = mid;
        else lo = mid + 1u;
    }
    p = row[lo] - (lo > 0u ? row[lo - 1u] : 0.0);
    return lo;
}

}  // namespace pt
