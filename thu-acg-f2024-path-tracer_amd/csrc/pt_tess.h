// Mesh tessellation and displacement (the rule in include/pt_amd.h): the per-element arithmetic, written once for host
// and device. pt_mesh_tessellate_host runs it from plain C++ loops, the kernels of pt_tess.hip run it one lane per element, and the unit
// is built with -ffp-contract=off on both sides, so the two execute the same sequence of IEEE operations (+ - * / sqrt floor on f64,
// one rounding to f32 per written attribute) and agree bit for bit. Which element gets which index is decided by sorts of integer
// keys, never by the order threads arrive in.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_TESS_HD __host__ __device__ inline
#else
#define PT_TESS_HD inline
#endif

namespace pt {

// The height image and how it is read. The pixels travel beside it (a device pointer in the kernels, the caller's on the host).
struct TessDisp {
    uint32_t w, h;
    int wrap;   // 0 clamp, 1 repeat
    double scale, midlevel;
};

PT_TESS_HD bool tess_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }   // false for NaN and the infinities

PT_TESS_HD uint64_t tess_edge_key(uint32_t a, uint32_t b) { return a < b ? ((uint64_t)a << 32) | b : ((uint64_t)b << 32) | a; }

// (A + B) * 0.5 per component: positions (n = 3) and texcoords (n = 2)
PT_TESS_HD void tess_mid_lin(const float* A, const float* B, int n, float* out) {
    for (int c = 0; c < n; ++c) out[c] = (float)(((double)A[c] + (double)B[c]) * 0.5);
}

// L = sqrt(s.x^2 + s.y^2 + s.z^2) summed left to right; s / L when L is finite and > 0 (true), else nothing is written (false)
PT_TESS_HD bool tess_normalise(const double s[3], float* out) {
    const double L = __builtin_sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    if (!(tess_finite(L) && L > 0.0)) return false;
    out[0] = (float)(s[0] / L);
    out[1] = (float)(s[1] / L);
    out[2] = (float)(s[2] / L);
    return true;
}

// The midpoint's normal; A belongs to the endpoint with the smaller index
PT_TESS_HD void tess_mid_normal(const float* A, const float* B, float* out) {
    const double s[3] = {(double)A[0] + (double)B[0], (double)A[1] + (double)B[1], (double)A[2] + (double)B[2]};
    if (!tess_normalise(s, out)) {
        out[0] = A[0]; out[1] = A[1]; out[2] = A[2];
    }
}

// c_f = (p1 - p0) x (p2 - p0), added into sum componentwise
PT_TESS_HD void tess_add_face_cross(const float* p0, const float* p1, const float* p2, double sum[3]) {
    const double e1[3] = {(double)p1[0] - (double)p0[0], (double)p1[1] - (double)p0[1], (double)p1[2] - (double)p0[2]};
    const double e2[3] = {(double)p2[0] - (double)p0[0], (double)p2[1] - (double)p0[1], (double)p2[2] - (double)p0[2]};
    sum[0] = sum[0] + (e1[1] * e2[2] - e1[2] * e2[1]);
    sum[1] = sum[1] + (e1[2] * e2[0] - e1[0] * e2[2]);
    sum[2] = sum[2] + (e1[0] * e2[1] - e1[1] * e2[0]);
}

// The smooth normal of vertex v: its corners 3f + k in ascending order (corners[0 .. n_corners), already in that order). prev: the
// normal the vertex had, or NULL.
PT_TESS_HD void tess_smooth_normal(const float* pos, const uint32_t* idx, const uint32_t* corners, size_t n_corners, const float* prev, float* out) {
    double sum[3] = {0.0, 0.0, 0.0};
    for (size_t r = 0; r < n_corners; ++r) {
        const size_t f = corners[r] / 3u;
        const uint32_t* t = idx + 3 * f;
        tess_add_face_cross(pos + 3 * (size_t)t[0], pos + 3 * (size_t)t[1], pos + 3 * (size_t)t[2], sum);
    }
    if (tess_normalise(sum, out)) return;
    if (prev) {
        out[0] = prev[0]; out[1] = prev[1]; out[2] = prev[2];
    } else {
        out[0] = 0.0f; out[1] = 1.0f; out[2] = 0.0f;
    }
}

// One image coordinate: the two texel indices and the weight of the second. t is u (flip = false) or v (flip = true: row 0 at v = 1).
PT_TESS_HD void tess_axis(double t, uint32_t n, int wrap, bool flip, uint32_t& k0, uint32_t& k1, double& w) {
    if (wrap) t = t - __builtin_floor(t);
    else t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double x = (flip ? 1.0 - t : t) * (double)n - 0.5;
    const double fl = __builtin_floor(x);
    w = x - fl;
    const int64_t i0 = (int64_t)fl, i1 = i0 + 1, m = (int64_t)n;   // |x| <= n + 1: no overflow
    if (wrap) {
        k0 = (uint32_t)(((i0 % m) + m) % m);
        k1 = (uint32_t)(((i1 % m) + m) % m);
    } else {
        k0 = (uint32_t)(i0 < 0 ? 0 : (i0 > m - 1 ? m - 1 : i0));
        k1 = (uint32_t)(i1 < 0 ? 0 : (i1 > m - 1 ? m - 1 : i1));
    }
}

// d = scale * (h(u, v) - midlevel), the bilinear height; 0 when u, v or h is not finite
PT_TESS_HD double tess_height(const TessDisp& D, const float* img, double u, double v) {
    if (!(tess_finite(u) && tess_finite(v))) return 0.0;
    uint32_t i0, i1, j0, j1;
    double tx, ty;
    tess_axis(u, D.w, D.wrap, false, i0, i1, tx);
    tess_axis(v, D.h, D.wrap, true, j0, j1, ty);
    const double h00 = (double)img[(size_t)j0 * D.w + i0], h10 = (double)img[(size_t)j0 * D.w + i1];
    const double h01 = (double)img[(size_t)j1 * D.w + i0], h11 = (double)img[(size_t)j1 * D.w + i1];
    const double h = (h00 * (1.0 - tx) + h10 * tx) * (1.0 - ty) + (h01 * (1.0 - tx) + h11 * tx) * ty;
    if (!tess_finite(h)) return 0.0;
    return D.scale * (h - D.midlevel);
}

// p' = p + N * d per component, in place
PT_TESS_HD void tess_displace(float* p, const float* N, double d) {
    for (int c = 0; c < 3; ++c) p[c] = (float)((double)p[c] + (double)N[c] * d);
}

// ---- host side only: what pt_mesh_tessellate and pt_mesh_tessellate_host share (pt_tess_host.cpp) ----
struct TessPlan {
    uint32_t levels;
    uint32_t n, F;         // the input's vertices and faces
    bool has_nrm, has_uv;  // the input carries normals / texcoords
    bool displace;
    int out_normals;       // what is written: 0 none, 1 the carried normals, 2 smooth normals of the final positions
    TessDisp disp;
};
struct TessIn {
    uint32_t n_pos; const float* pos;
    uint32_t n_idx; const uint32_t* idx;
    uint32_t n_nrm; const float* nrm;
    uint32_t n_uv; const float* uv;
};
struct TessOut {
    float** pos; uint32_t* n_pos;
    uint32_t** idx; uint32_t* n_idx;
    float** nrm; float** uv;
};
// Every refusal of the rule, in one place: 0 and a filled plan, or -1 with the error set under `who`. Touches no device.
int tess_check(const char* who, const void* opts /* pt_tess_opts or NULL */, const TessIn& in, const TessOut& out, TessPlan& plan);
// malloc'd copies for the caller (pt_free), nrm / uv NULL where there is none; -1 with everything freed when malloc fails
int tess_hand_over(const char* who, const TessOut& out, uint32_t n, uint32_t n_idx, const float* pos, const uint32_t* idx, const float* nrm, const float* uv);

}  // namespace pt
