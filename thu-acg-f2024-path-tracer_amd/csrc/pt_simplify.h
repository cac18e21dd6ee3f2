// Mesh welding and simplification by quadric vertex clustering (the rule in include/pt_amd.h): the per-element
// arithmetic, written once for host and device. pt_mesh_simplify_host runs it from plain C++ loops, the kernels of pt_simplify.hip run
// it per lane, and the unit is built with -ffp-contract=off on both sides, so the two execute the same sequence of IEEE operations
// (+ - * / floor on f64, one rounding to f32 per written attribute) and agree bit for bit. Which vertex lands in which cluster, which
// cluster gets which index and the order of every sum follow from sorts of integer keys, never from the order threads arrive in.
#pragma once
#include <stdint.h>

#include "pt_tess.h"   // tess_finite, PT_TESS_HD

namespace pt {

constexpr uint32_t SIMP_NONE = 0xFFFFFFFFu;        // no cluster, no output vertex
constexpr uint64_t SIMP_NO_KEY = ~0ull;            // the cell key of an unreferenced vertex: sorts last (a real key has 63 bits)
constexpr uint64_t SIMP_MAX_FACES = 0x07FFFFFFull; // pt_mesh's cap
constexpr int SIMP_TILE = 16;                      // TSUM's tile

// The grid of mode 1: the lower corner of the referenced positions and the edge of a cell
struct SimpGrid {
    double lo[3];
    double cell;
};

// One f32 position component for the weld key: -0 and +0 are the same value
PT_TESS_HD uint32_t simp_weld_bits(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return b.u == 0x80000000u ? 0u : b.u;
}

// c_a = floor(((double)p_a - lo_a) / cell) per axis; key = (c_z << 42) | (c_y << 21) | c_x. simplify_check bounds every c_a below 2^21.
PT_TESS_HD uint64_t simp_cell_key(const SimpGrid& g, const float* p) {
    uint64_t c[3];
    for (int a = 0; a < 3; ++a) c[a] = (uint64_t)__builtin_floor(((double)p[a] - g.lo[a]) / g.cell);
    return (c[2] << 42) | (c[1] << 21) | c[0];
}

// o_a = lo_a + ((double)c_a + 0.5) * cell: the centre of the key's cell
PT_TESS_HD void simp_cell_origin(const SimpGrid& g, uint64_t key, double o[3]) {
    const uint64_t c[3] = {key & 0x1FFFFFull, (key >> 21) & 0x1FFFFFull, (key >> 42) & 0x1FFFFFull};
    for (int a = 0; a < 3; ++a) o[a] = g.lo[a] + ((double)c[a] + 0.5) * g.cell;
}

// A tile's value: the balanced pairwise tree over its sixteen entries (the host's form; sixteen lanes take it as four xor-butterfly
// steps, which add the same pairs: f64 addition is commutative bit for bit)
PT_TESS_HD double simp_tile_tree(double* s /* 16 entries, overwritten */) {
    for (int w = SIMP_TILE / 2; w >= 1; w /= 2)
        for (int i = 0; i < w; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}

// The nine terms of one corner of face (i0, i1, i2): its plane n . x = d about the origin o, as n n^T (upper triangle) and n d
PT_TESS_HD void simp_corner_terms(const float* pos, const uint32_t* tri, const double o[3], double t[9]) {
    double p[3][3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = (double)pos[3 * (size_t)tri[k] + a] - o[a];
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double d = (n[0] * p[0][0] + n[1] * p[0][1]) + n[2] * p[0][2];
    t[0] = n[0] * n[0]; t[1] = n[0] * n[1]; t[2] = n[0] * n[2];
    t[3] = n[1] * n[1]; t[4] = n[1] * n[2]; t[5] = n[2] * n[2];
    t[6] = n[0] * d; t[7] = n[1] * d; t[8] = n[2] * d;
}

// The regularised minimiser of the cluster's quadric about its cell centre: q = (a00 a01 a02 a11 a12 a22 b0 b1 b2), m the members'
// mean. x = m where the quadric is unusable or the optimum leaves the cell by more than half a cell.
PT_TESS_HD void simp_solve(const double q[9], const double m[3], double reg, double cell, double x[3]) {
    x[0] = m[0]; x[1] = m[1]; x[2] = m[2];
    const double T = (q[0] + q[3]) + q[5];
    if (!(tess_finite(T) && T > 0.0)) return;
    const double lam = reg * T;
    const double a00 = q[0] + lam, a01 = q[1], a02 = q[2], a11 = q[3] + lam, a12 = q[4], a22 = q[5] + lam;
    const double r0 = q[6] + lam * m[0], r1 = q[7] + lam * m[1], r2 = q[8] + lam * m[2];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    if (!(det > 0.0)) return;
    const double s0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    const double s1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    const double s2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
    if (!(tess_finite(s0) && tess_finite(s1) && tess_finite(s2))) return;
    if (!(__builtin_fabs(s0) <= cell && __builtin_fabs(s1) <= cell && __builtin_fabs(s2) <= cell)) return;
    x[0] = s0; x[1] = s1; x[2] = s2;
}

// Face (A, B, C) of cluster ids, no two equal: the sorted triple and whether (A, B, C) is an odd permutation of it
PT_TESS_HD bool simp_sorted_triple(uint32_t A, uint32_t B, uint32_t C, uint32_t& lo, uint32_t& mid, uint32_t& hi) {
    bool odd = false;
    if (A > B) { const uint32_t t = A; A = B; B = t; odd = !odd; }
    if (B > C) { const uint32_t t = B; B = C; C = t; odd = !odd; }
    if (A > B) { const uint32_t t = A; A = B; B = t; odd = !odd; }
    lo = A; mid = B; hi = C;
    return odd;
}

// ---- host side only: what pt_mesh_simplify and pt_mesh_simplify_host share (pt_simplify_host.cpp) ----
struct SimpPlan {
    uint32_t n, F;       // the input's vertices and faces
    bool has_uv;
    int mode;            // 0 weld, 1 cluster
    bool quadric;        // mode 1: quadric placement (else the mean)
    bool dedup;
    bool normals;        // smooth normals are written
    bool want_map;
    double reg;
    SimpGrid grid;       // mode 1
};
struct SimpIn {
    uint32_t n_pos; const float* pos;
    uint32_t n_idx; const uint32_t* idx;
    uint32_t n_uv; const float* uv;
};
struct SimpOut {
    float** pos; uint32_t* n_pos;
    uint32_t** idx; uint32_t* n_idx;
    float** nrm; float** uv; uint32_t** map;
};
// Every refusal of the rule, in one place: 0 and a filled plan (the grid included: the bounds are taken here, before any device
// work, because three refusals depend on them), or -1 with the error set under `who`. Touches no device.
int simplify_check(const char* who, const void* opts /* pt_simplify_opts or NULL */, const SimpIn& in, const SimpOut& out, SimpPlan& plan);

}  // namespace pt
