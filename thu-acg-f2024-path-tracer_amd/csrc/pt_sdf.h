// Mesh voxelisation: signed distance, occupancy and density grids from a triangle mesh (the rule in include/pt_amd.h): the
// per-element arithmetic, written once for host and device. pt_mesh_sdf_host runs it from plain C++ loops, the kernels of pt_sdf.hip run
// it per triangle, per column and per sample, and the unit is built with -ffp-contract=off on both sides, so the two execute the same
// sequence of IEEE operations (+ - * / sqrt on f64, one rounding to f32 per output) and agree bit for bit. The sign is an integer count
// per sample, the distance a minimum of f64 values: neither depends on the order the triangles are visited in.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_tess.h"   // tess_finite

#if defined(__HIPCC__)
#define PT_SDF_HD __host__ __device__ inline
#else
#define PT_SDF_HD inline
#endif

namespace pt {

// The grid of a call and what is written into it
struct SdfGrid {
    uint32_t nx, ny, nz;
    double lo[3], h[3];   // the box's low corner and the spacing (hi - lo) / n per axis
    int what;             // 0 depth, 1 distance, 2 occupancy, 3 density
    int fill;             // 0 non-zero, 1 odd
    int negate;
    double band;          // 0: exact everywhere
    double ramp;          // what = 3
};

// The centre of cell i along an axis
PT_SDF_HD double sdf_coord(const SdfGrid& g, int axis, uint32_t i) { return g.lo[axis] + ((double)i + 0.5) * g.h[axis]; }

// The number of i in 0 .. n - 1 with coord(i) < x: the coordinates never decrease with i, so a bisection finds it
PT_SDF_HD uint32_t sdf_count_below(const SdfGrid& g, int axis, uint32_t n, double x) {
    uint32_t a = 0, b = n;   // coord(i) < x for i < a, not for i >= b
    while (a < b) {
        const uint32_t m = a + (b - a) / 2u;
        if (sdf_coord(g, axis, m) < x) a = m + 1u;
        else b = m;
    }
    return a;
}
// The number of i in 0 .. n - 1 with coord(i) <= x
PT_SDF_HD uint32_t sdf_count_not_above(const SdfGrid& g, int axis, uint32_t n, double x) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2u;
        if (sdf_coord(g, axis, m) <= x) a = m + 1u;
        else b = m;
    }
    return a;
}

// ---- the sign ----
// The side of the column P = (Py, Pz) of the directed edge U -> V of a projected triangle, +1 or -1, and the directed edge value
PT_SDF_HD int sdf_edge_side(double Uy, double Uz, double Vy, double Vz, double Py, double Pz, double& value) {
    const bool swapped = Vy < Uy || (Vy == Uy && Vz < Uz);
    if (swapped) {
        double t = Uy; Uy = Vy; Vy = t;
        t = Uz; Uz = Vz; Vz = t;
    }
    const double dy = Vy - Uy, dz = Vz - Uz;
    const double e = dy * (Pz - Uz) - dz * (Py - Uy);
    // the tie: P moved by (+eps, +eps^2); an edge that projects to a point (dy == dz == 0) gets -1
    const int s = (e > 0.0 || (e == 0.0 && (dz < 0.0 || (dz == 0.0 && dy > 0.0)))) ? 1 : -1;
    value = swapped ? -e : e;
    return swapped ? -s : s;
}

// The columns j0 .. j1 - 1, k0 .. k1 - 1 whose centre lies in the closed (y, z) bounding box of a triangle
PT_SDF_HD void sdf_columns(const SdfGrid& g, const double A[3], const double B[3], const double C[3], uint32_t& j0, uint32_t& j1, uint32_t& k0, uint32_t& k1) {
    const double ylo = A[1] < B[1] ? (A[1] < C[1] ? A[1] : C[1]) : (B[1] < C[1] ? B[1] : C[1]);
    const double yhi = A[1] > B[1] ? (A[1] > C[1] ? A[1] : C[1]) : (B[1] > C[1] ? B[1] : C[1]);
    const double zlo = A[2] < B[2] ? (A[2] < C[2] ? A[2] : C[2]) : (B[2] < C[2] ? B[2] : C[2]);
    const double zhi = A[2] > B[2] ? (A[2] > C[2] ? A[2] : C[2]) : (B[2] > C[2] ? B[2] : C[2]);
    j0 = sdf_count_below(g, 1, g.ny, ylo);
    j1 = sdf_count_not_above(g, 1, g.ny, yhi);
    k0 = sdf_count_below(g, 2, g.nz, zlo);
    k1 = sdf_count_not_above(g, 2, g.nz, zhi);
}

// Does the column (j, k) cross the triangle? Then o = +1 / -1 and m = the number of samples of the column before the crossing
PT_SDF_HD bool sdf_crossing(const SdfGrid& g, const double A[3], const double B[3], const double C[3], uint32_t j, uint32_t k, int& o, uint32_t& m) {
    const double Py = sdf_coord(g, 1, j), Pz = sdf_coord(g, 2, k);
    double wa, wb, wc;
    const int sc = sdf_edge_side(A[1], A[2], B[1], B[2], Py, Pz, wc);
    const int sa = sdf_edge_side(B[1], B[2], C[1], C[2], Py, Pz, wa);
    const int sb = sdf_edge_side(C[1], C[2], A[1], A[2], Py, Pz, wb);
    if (sa != sb || sb != sc) return false;
    const double den = (wa + wb) + wc;
    if (den == 0.0) return false;
    const double x = ((wa * A[0] + wb * B[0]) + wc * C[0]) / den;
    if (!tess_finite(x)) return false;
    o = sa;
    m = sdf_count_below(g, 0, g.nx, x);
    return true;
}

PT_SDF_HD bool sdf_inside(int fill, int32_t winding) { return fill == 0 ? winding != 0 : (winding & 1) != 0; }

// ---- the distance ----
// A triangle of the distance pass: A, B - A, C - A in f64, and the box of its three f32 positions
struct SdfRecord {
    double A[3], ab[3], ac[3];
};
constexpr size_t SDF_RECORD_DOUBLES = 9, SDF_BOX_FLOATS = 6;   // 72 + 24 = 96 B a triangle

PT_SDF_HD double sdf_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The record of a triangle; false when it is dropped from the distance pass (a repeated index, or n.n == 0 for n = (B - A) x (C - A))
PT_SDF_HD bool sdf_record(const float* pos, uint32_t ia, uint32_t ib, uint32_t ic, double rec[9], float box[6]) {
    const float *a = pos + 3 * (size_t)ia, *b = pos + 3 * (size_t)ib, *c = pos + 3 * (size_t)ic;
    for (int d = 0; d < 3; ++d) {
        rec[d] = (double)a[d];
        rec[3 + d] = (double)b[d] - (double)a[d];
        rec[6 + d] = (double)c[d] - (double)a[d];
        const float lo = a[d] < b[d] ? (a[d] < c[d] ? a[d] : c[d]) : (b[d] < c[d] ? b[d] : c[d]);
        const float hi = a[d] > b[d] ? (a[d] > c[d] ? a[d] : c[d]) : (b[d] > c[d] ? b[d] : c[d]);
        box[d] = lo;
        box[3 + d] = hi;
    }
    if (ia == ib || ib == ic || ic == ia) return false;
    const double* ab = rec + 3;
    const double* ac = rec + 6;
    const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    return sdf_dot(n, n) != 0.0;
}

// The squared distance from P to the triangle of a record: the closest point by Voronoi region, in the header's order
PT_SDF_HD double sdf_dist2(const double rec[9], const double P[3]) {
    const double* A = rec;
    const double* ab = rec + 3;
    const double* ac = rec + 6;
    const double ap[3] = {P[0] - A[0], P[1] - A[1], P[2] - A[2]};
    const double d1 = sdf_dot(ab, ap), d2 = sdf_dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return sdf_dot(ap, ap);                                  // vertex A
    const double bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]};
    const double d3 = sdf_dot(ab, bp), d4 = sdf_dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return sdf_dot(bp, bp);                                   // vertex B
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                                           // edge AB
        const double v = d1 / (d1 - d3);
        const double q[3] = {ap[0] - ab[0] * v, ap[1] - ab[1] * v, ap[2] - ab[2] * v};
        return sdf_dot(q, q);
    }
    const double cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
    const double d5 = sdf_dot(ab, cp), d6 = sdf_dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return sdf_dot(cp, cp);                                   // vertex C
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                                           // edge AC
        const double w = d2 / (d2 - d6);
        const double q[3] = {ap[0] - ac[0] * w, ap[1] - ac[1] * w, ap[2] - ac[2] * w};
        return sdf_dot(q, q);
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {                             // edge BC
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        const double q[3] = {bp[0] - (ac[0] - ab[0]) * w, bp[1] - (ac[1] - ab[1]) * w, bp[2] - (ac[2] - ab[2]) * w};
        return sdf_dot(q, q);
    }
    const double den = (va + vb) + vc;                                                   // the face
    const double v = vb / den, w = vc / den;
    const double q[3] = {ap[0] - (ab[0] * v + ac[0] * w), ap[1] - (ab[1] * v + ac[1] * w), ap[2] - (ab[2] * v + ac[2] * w)};
    return sdf_dot(q, q);
}

// A lower bound of the squared distance between the boxes [alo, ahi] and [blo, bhi] (a point is a box with alo == ahi), up to its own
// rounding: three gaps, each exact up to one rounding, their squares summed. The culls compare it through sdf_cull_far.
PT_SDF_HD double sdf_box_gap2(const double alo[3], const double ahi[3], const float box[6]) {
    double s = 0.0;
    for (int d = 0; d < 3; ++d) {
        const double below = (double)box[d] - ahi[d], above = alo[d] - (double)box[3 + d];
        const double gap = below > 0.0 ? below : (above > 0.0 ? above : 0.0);
        s += gap * gap;
    }
    return s;
}
// May a triangle whose box lies gap2 from the samples be skipped when the largest squared distance it would have to beat is `best`?
// The margin, 2^-20, errs towards testing: DESIGN.md section 30 has the bound it covers.
PT_SDF_HD bool sdf_cull_far(double gap2, double best) { return gap2 * (1.0 - 9.5367431640625e-07) > best; }
// The best a banded search starts from: just above band^2, so that everything at least `band` away reads exactly `band`
PT_SDF_HD double sdf_seed(double band) { return (band * band) * (1.0 + 9.5367431640625e-07); }

// The output of a sample from its least squared distance and its inside flag
PT_SDF_HD float sdf_output(const SdfGrid& g, double best2, bool inside) {
    if (g.what == 2) return inside ? 1.0f : 0.0f;
    double d = __builtin_sqrt(best2);
    if (g.what == 3) {
        if (!inside) return 0.0f;
        return (float)((d < g.ramp ? d : g.ramp) / g.ramp);
    }
    if (g.band > 0.0 && !(d < g.band)) d = g.band;
    if (g.what == 1) return (float)d;
    const double depth = inside ? d : -d;
    return (float)(g.negate ? -depth : depth);
}
// What a search may start from without changing a result: the cap the output applies anyway
PT_SDF_HD double sdf_start(const SdfGrid& g) {
    const double inf = __builtin_inf();
    if (g.what == 3) return sdf_seed(g.ramp);
    return g.band > 0.0 ? sdf_seed(g.band) : inf;
}

// ---- host side only: what pt_mesh_sdf and pt_mesh_sdf_host share (pt_sdf_host.cpp) ----
constexpr uint64_t SDF_MAX_TRIANGLES = 0x07FFFFFFull;   // pt_mesh's cap
// Every refusal of the rule, in one place: 0 and a filled grid, or -1 with the error set under `who`. Touches no device.
int sdf_check(const char* who, const void* opts /* pt_sdf_opts or NULL */, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t nx, uint32_t ny,
              uint32_t nz, const double* box_lo, const double* box_hi, const float* out_values, SdfGrid& grid);

}  // namespace pt
