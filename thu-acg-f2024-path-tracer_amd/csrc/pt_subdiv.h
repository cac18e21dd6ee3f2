// Loop subdivision with creases, corners and limit projection (the rule in include/pt_amd.h): the per-element arithmetic,
// written once for host and device, as pt_tess.h is for tessellation. pt_mesh_subdivide_host runs it from plain C++ loops, the kernels of
// pt_subdiv.hip run it one lane per element, and the unit is built with -ffp-contract=off on both sides: the same sequence of IEEE
// operations (+ - * / sqrt on f64, one rounding to f32 per written attribute), the same bits. No trigonometry: angles arrive as cosines.
// The structures the functions read are made by integer sorts on both sides:
//   edges : the sorted (edge key, slot 3f + k) pairs of §27; a key's run is its slots in ascending order
//   rays  : per distinct key (A, B) with A != B of rank r, the two pairs ((A << 32) | B, r) and ((B << 32) | A, r), sorted by key: the
//           run of vertex v lists its neighbours in ascending order
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_tess.h"

namespace pt {

PT_TESS_HD double subdiv_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// c = (p1 - p0) x (p2 - p0) of face f
PT_TESS_HD void subdiv_face_cross(const float* pos, const uint32_t* idx, size_t f, double c[3]) {
    const float *p0 = pos + 3 * (size_t)idx[3 * f], *p1 = pos + 3 * (size_t)idx[3 * f + 1], *p2 = pos + 3 * (size_t)idx[3 * f + 2];
    const double e1[3] = {(double)p1[0] - (double)p0[0], (double)p1[1] - (double)p0[1], (double)p1[2] - (double)p0[2]};
    const double e2[3] = {(double)p2[0] - (double)p0[0], (double)p2[1] - (double)p0[1], (double)p2[2] - (double)p0[2]};
    c[0] = e1[1] * e2[2] - e1[2] * e2[1];
    c[1] = e1[2] * e2[0] - e1[0] * e2[2];
    c[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// Creasing by angle: the faces f0, f1 of a two-slot edge fold more sharply than crease_cos allows (false for NaN)
PT_TESS_HD bool subdiv_fold(const float* pos, const uint32_t* idx, size_t f0, size_t f1, double crease_cos) {
    double c0[3], c1[3];
    subdiv_face_cross(pos, idx, f0, c0);
    subdiv_face_cross(pos, idx, f1, c1);
    return subdiv_dot(c0, c1) < crease_cos * __builtin_sqrt(subdiv_dot(c0, c0) * subdiv_dot(c1, c1));
}

// What an edge's run says: its length, whether any slot is flagged, the vertices opposite its first and second slot
struct SubdivEdge {
    bool sharp, flagged;
    uint32_t C, D;
};

// slots[0 .. len): the run of key (A, B); crease: one byte per slot of the mesh
PT_TESS_HD SubdivEdge subdiv_edge(uint32_t A, uint32_t B, const uint32_t* slots, size_t len, const uint32_t* idx, const uint8_t* crease) {
    SubdivEdge e;
    e.flagged = false;
    for (size_t j = 0; j < len; ++j) e.flagged = e.flagged || crease[slots[j]] != 0;
    e.sharp = len != 2 || A == B || e.flagged;
    const size_t s0 = slots[0], s1 = slots[len > 1 ? 1 : 0];
    e.C = idx[3 * (s0 / 3) + (s0 % 3 + 2) % 3];
    e.D = idx[3 * (s1 / 3) + (s1 % 3 + 2) % 3];
    return e;
}

// The odd vertex of an edge, n components (positions 3, texcoords 2)
PT_TESS_HD void subdiv_odd(const float* A, const float* B, const float* C, const float* D, int n, bool sharp, float* out) {
    for (int c = 0; c < n; ++c) {
        if (sharp) out[c] = (float)(((double)A[c] + (double)B[c]) * 0.5);
        else out[c] = (float)(((double)A[c] + (double)B[c]) * 0.375 + ((double)C[c] + (double)D[c]) * 0.125);
    }
}

// The even vertex v (limit = false) or its limit position (limit = true). rays[0 .. k) / rank[0 .. k): v's run, neighbours ascending;
// sharp: one byte per edge rank. uv / out_uv NULL: no texcoords. Reads the level's input values only.
PT_TESS_HD void subdiv_even(const float* pos, const float* uv, size_t v, const uint64_t* rays, const uint32_t* rank, size_t k, const uint8_t* sharp,
                            double corner_cos, bool limit, float* out_pos, float* out_uv) {
    const float* P = pos + 3 * v;
    const float* T = uv ? uv + 2 * v : nullptr;
    double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    size_t s = 0, w0 = 0, w1 = 0;
    for (size_t r = 0; r < k; ++r) {
        const size_t w = (size_t)(rays[r] & 0xFFFFFFFFu);
        if (sharp[rank[r]]) {
            if (s == 0) w0 = w;
            else if (s == 1) w1 = w;
            ++s;
        }
        for (int c = 0; c < 3; ++c) S[c] += (double)pos[3 * w + c];
        if (uv)
            for (int c = 0; c < 2; ++c) S[3 + c] += (double)uv[2 * w + c];
    }
    int mask = 0;   // 0 kept, 1 crease, 2 smooth
    if (k != 0 && s <= 1) mask = 2;
    else if (k != 0 && s == 2) {
        const float *Q0 = pos + 3 * w0, *Q1 = pos + 3 * w1;
        const double d0[3] = {(double)Q0[0] - (double)P[0], (double)Q0[1] - (double)P[1], (double)Q0[2] - (double)P[2]};
        const double d1[3] = {(double)Q1[0] - (double)P[0], (double)Q1[1] - (double)P[1], (double)Q1[2] - (double)P[2]};
        const bool corner = subdiv_dot(d0, d1) > corner_cos * __builtin_sqrt(subdiv_dot(d0, d0) * subdiv_dot(d1, d1));
        mask = corner ? 0 : 1;
    }
    if (mask == 0) {
        for (int c = 0; c < 3; ++c) out_pos[c] = P[c];
        if (uv)
            for (int c = 0; c < 2; ++c) out_uv[c] = T[c];
    } else if (mask == 1) {
        const double own = limit ? 2.0 / 3.0 : 0.75, other = limit ? 1.0 / 6.0 : 0.125;
        for (int c = 0; c < 3; ++c) out_pos[c] = (float)((double)P[c] * own + ((double)pos[3 * w0 + c] + (double)pos[3 * w1 + c]) * other);
        if (uv)
            for (int c = 0; c < 2; ++c) out_uv[c] = (float)((double)T[c] * own + ((double)uv[2 * w0 + c] + (double)uv[2 * w1 + c]) * other);
    } else {
        const double kd = (double)k;
        const double beta = limit ? (k == 3 ? 0.2 : 0.5 / kd) : (k == 3 ? 0.1875 : 0.375 / kd);
        const double own = 1.0 - kd * beta;
        for (int c = 0; c < 3; ++c) out_pos[c] = (float)((double)P[c] * own + S[c] * beta);
        if (uv)
            for (int c = 0; c < 2; ++c) out_uv[c] = (float)((double)T[c] * own + S[3 + c] * beta);
    }
}

// ---- host side only: what pt_mesh_subdivide and pt_mesh_subdivide_host share (pt_subdiv_host.cpp) ----
struct SubdivPlan {
    uint32_t levels;
    uint32_t n, F;
    bool has_uv, has_crease, limit, normals, want_crease;
    double crease_cos, corner_cos;
};
struct SubdivIn {
    uint32_t n_pos; const float* pos;
    uint32_t n_idx; const uint32_t* idx;
    uint32_t n_uv; const float* uv;
    const uint8_t* crease;
};
struct SubdivOut {
    float** pos; uint32_t* n_pos;
    uint32_t** idx; uint32_t* n_idx;
    float** nrm; float** uv;
    uint8_t** crease;   // may be NULL: not wanted
};
// Every refusal of the rule, in one place: 0 and a filled plan, or -1 with the error set under `who`. Touches no device.
int subdiv_check(const char* who, const void* opts /* pt_subdiv_opts or NULL */, const SubdivIn& in, const SubdivOut& out, SubdivPlan& plan);

}  // namespace pt
