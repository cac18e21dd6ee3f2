// Mesh tessellation and displacement, the host side (include/pt_amd.h has the rule): the refusals both entry points
// share, pt_mesh_tessellate_host (the GPU stage's twin: std::sort where the device sorts by radix, the same pt_tess.h functions per
// element), pt_mesh_grid and pt_height_from_rgb8. Plain C++: nothing here touches a device.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_tess.h"

namespace pt {

int set_error(const std::string& msg);   // pt_error.cpp; returns -1

int tess_check(const char* who, const void* opts_, const TessIn& in, const TessOut& out, TessPlan& plan) {
    const std::string p = std::string(who) + ": ";
    pt_tess_opts o;
    if (opts_) o = *(const pt_tess_opts*)opts_;
    else pt_tess_opts_default(&o);
    if (!out.pos || !out.n_pos || !out.idx || !out.n_idx || !out.nrm || !out.uv) return set_error(p + "null output pointer");
    *out.pos = nullptr; *out.idx = nullptr; *out.nrm = nullptr; *out.uv = nullptr;
    *out.n_pos = 0; *out.n_idx = 0;
    if ((in.n_pos && !in.pos) || (in.n_idx && !in.idx) || (in.n_nrm && !in.nrm) || (in.n_uv && !in.uv)) return set_error(p + "null input array");
    if (in.n_idx % 3 != 0) return set_error(p + "index count must be a multiple of 3");
    if (o.wrap != 0 && o.wrap != 1) return set_error(p + "wrap must be 0 (clamp) or 1 (repeat)");
    if (o.normals < 0 || o.normals > 3) return set_error(p + "normals must be 0 (auto), 1 (keep), 2 (smooth) or 3 (none)");
    if (o.levels > 12) return set_error(p + "levels must be at most 12");
    if (o.height && in.n_uv == 0) return set_error(p + "a height image needs texcoords");
    if (o.height && (o.height_w == 0 || o.height_h == 0)) return set_error(p + "height_w and height_h must be positive");
    const uint64_t F = in.n_idx / 3, grow = 1ull << (2 * o.levels);   // 4^levels <= 2^24
    if (F * grow > 0x07FFFFFFull) return set_error(p + "too many triangles: 4^levels * faces must be at most 0x07FFFFFF");
    if ((uint64_t)in.n_pos + (grow - 1) * F > 0xFFFFFFFFull) return set_error(p + "too many vertices: the vertex count passes 32 bits");
    for (uint32_t i = 0; i < in.n_idx; ++i) {
        if (in.idx[i] >= in.n_pos) return set_error(p + "position index out of range");
        if (in.n_nrm && in.idx[i] >= in.n_nrm) return set_error(p + "normal index out of range");
        if (in.n_uv && in.idx[i] >= in.n_uv) return set_error(p + "texcoord index out of range");
    }
    plan.levels = o.levels;
    plan.n = in.n_pos;
    plan.F = (uint32_t)F;
    plan.has_nrm = in.n_nrm != 0;
    plan.has_uv = in.n_uv != 0;
    plan.displace = o.height != nullptr;
    const bool carried = plan.has_nrm || plan.displace;
    switch (o.normals) {
        case 0: plan.out_normals = plan.displace ? 2 : (plan.has_nrm ? 1 : 0); break;
        case 1: plan.out_normals = carried ? 1 : 0; break;
        case 2: plan.out_normals = 2; break;
        default: plan.out_normals = 0; break;
    }
    plan.disp.w = o.height_w;
    plan.disp.h = o.height_h;
    plan.disp.wrap = o.wrap;
    plan.disp.scale = o.scale;
    plan.disp.midlevel = o.midlevel;
    return 0;
}

namespace {
template <class T>
T* dup(const T* v, size_t n) {
    T* q = (T*)malloc(n * sizeof(T) + sizeof(T));   // (never a zero-byte request: an empty array still has a pointer)
    if (q && n) memcpy(q, v, n * sizeof(T));
    return q;
}
}  // namespace

int tess_hand_over(const char* who, const TessOut& out, uint32_t n, uint32_t n_idx, const float* pos, const uint32_t* idx, const float* nrm, const float* uv) {
    float* P = dup(pos, (size_t)n * 3);
    uint32_t* I = dup(idx, (size_t)n_idx);
    float* N = nrm ? dup(nrm, (size_t)n * 3) : nullptr;
    float* T = uv ? dup(uv, (size_t)n * 2) : nullptr;
    if (!P || !I || (nrm && !N) || (uv && !T)) {
        free(P); free(I); free(N); free(T);
        return set_error(std::string(who) + ": out of host memory");
    }
    *out.pos = P; *out.n_pos = n;
    *out.idx = I; *out.n_idx = n_idx;
    *out.nrm = N; *out.uv = T;
    return 0;
}

namespace {

// Smooth normals of (pos, idx): the corners of each vertex in ascending order by a sort of (vertex, corner) pairs
void smooth_normals(const std::vector<float>& pos, const std::vector<uint32_t>& idx, const float* prev, std::vector<float>& out) {
    const size_t n = pos.size() / 3, M = idx.size();
    std::vector<std::pair<uint32_t, uint32_t>> vc(M);
    for (size_t c = 0; c < M; ++c) vc[c] = {idx[c], (uint32_t)c};
    std::sort(vc.begin(), vc.end());
    std::vector<uint32_t> corners(M);
    for (size_t i = 0; i < M; ++i) corners[i] = vc[i].second;
    out.assign(n * 3, 0.0f);
    size_t i = 0;
    for (size_t v = 0; v < n; ++v) {
        const size_t first = i;
        while (i < M && vc[i].first == v) ++i;
        tess_smooth_normal(pos.data(), idx.data(), corners.data() + first, i - first, prev ? prev + 3 * v : nullptr, out.data() + 3 * v);
    }
}

}  // namespace
}  // namespace pt

using namespace pt;

extern "C" int pt_tess_opts_default(pt_tess_opts* o) {
    if (!o) return set_error("pt_tess_opts_default: null options");
    memset(o, 0, sizeof *o);
    o->levels = 1;
    o->scale = 1.0;
    o->midlevel = 0.5;
    return 0;
}

extern "C" int pt_mesh_tessellate_host(const pt_tess_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t n_nrm,
                                       const float* nrm, uint32_t n_uv, const float* uv, float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx,
                                       uint32_t* out_n_idx, float** out_nrm, float** out_uv) {
    const char* who = "pt_mesh_tessellate_host";
    const TessIn in{n_pos, pos, n_idx, idx, n_nrm, nrm, n_uv, uv};
    const TessOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm, out_uv};
    TessPlan plan;
    if (tess_check(who, opts, in, out, plan) != 0) return -1;
    size_t n = plan.n, F = plan.F;
    std::vector<float> P(pos, pos + n * 3), N, T;
    std::vector<uint32_t> I(idx, idx + F * 3);
    if (plan.has_nrm) {
        N.assign(n * 3, 0.0f);
        memcpy(N.data(), nrm, std::min<size_t>(n, n_nrm) * 3 * sizeof(float));
    }
    if (plan.has_uv) {
        T.assign(n * 2, 0.0f);
        memcpy(T.data(), uv, std::min<size_t>(n, n_uv) * 2 * sizeof(float));
    }
    for (uint32_t level = 0; level < plan.levels; ++level) {
        const size_t M = 3 * F;
        std::vector<std::pair<uint64_t, uint32_t>> ks(M);
        for (size_t f = 0; f < F; ++f)
            for (uint32_t k = 0; k < 3; ++k) ks[3 * f + k] = {tess_edge_key(I[3 * f + k], I[3 * f + (k + 1) % 3]), (uint32_t)(3 * f + k)};
        std::sort(ks.begin(), ks.end());
        std::vector<uint32_t> mid(M);
        size_t E = 0;
        for (size_t i = 0; i < M; ++i) {
            if (i == 0 || ks[i].first != ks[i - 1].first) {
                const size_t a = (size_t)(ks[i].first >> 32), b = (size_t)(ks[i].first & 0xFFFFFFFFu), m = n + E;
                ++E;
                P.resize(3 * (m + 1));
                tess_mid_lin(&P[3 * a], &P[3 * b], 3, &P[3 * m]);
                if (plan.has_nrm) {
                    N.resize(3 * (m + 1));
                    tess_mid_normal(&N[3 * a], &N[3 * b], &N[3 * m]);
                }
                if (plan.has_uv) {
                    T.resize(2 * (m + 1));
                    tess_mid_lin(&T[2 * a], &T[2 * b], 2, &T[2 * m]);
                }
            }
            mid[ks[i].second] = (uint32_t)(n + E - 1);
        }
        std::vector<uint32_t> J(12 * F);
        for (size_t f = 0; f < F; ++f) {
            const uint32_t a = I[3 * f], b = I[3 * f + 1], c = I[3 * f + 2], ab = mid[3 * f], bc = mid[3 * f + 1], ca = mid[3 * f + 2];
            const uint32_t ch[12] = {a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca};
            memcpy(&J[12 * f], ch, sizeof ch);
        }
        I.swap(J);
        n += E;
        F *= 4;
    }
    if (plan.displace) {
        if (!plan.has_nrm) smooth_normals(P, I, nullptr, N);
        const pt_tess_opts& o = *opts;
        for (size_t v = 0; v < n; ++v) tess_displace(&P[3 * v], &N[3 * v], tess_height(plan.disp, o.height, (double)T[2 * v], (double)T[2 * v + 1]));
    }
    const bool carried = plan.has_nrm || plan.displace;
    if (plan.out_normals == 2) {
        std::vector<float> S;
        smooth_normals(P, I, carried ? N.data() : nullptr, S);
        N.swap(S);
    }
    static const float none[1] = {0.0f};   // an empty array that is there is not NULL (an empty vector's data() may be)
    return tess_hand_over(who, out, (uint32_t)n, (uint32_t)(3 * F), P.data(), I.data(), plan.out_normals ? (n ? N.data() : none) : nullptr,
                          plan.has_uv ? (n ? T.data() : none) : nullptr);
}

extern "C" int pt_mesh_grid(const double q[3], const double u[3], const double v[3], uint32_t nu, uint32_t nv, float** out_pos, uint32_t* out_n_pos,
                            uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm, float** out_uv) {
    const char* who = "pt_mesh_grid";
    if (!q || !u || !v) return set_error("pt_mesh_grid: null vector");
    if (!out_pos || !out_n_pos || !out_idx || !out_n_idx || !out_nrm || !out_uv) return set_error("pt_mesh_grid: null output pointer");
    *out_pos = nullptr; *out_idx = nullptr; *out_nrm = nullptr; *out_uv = nullptr;
    *out_n_pos = 0; *out_n_idx = 0;
    if (nu == 0 || nv == 0) return set_error("pt_mesh_grid: nu and nv must be positive");
    if (2ull * nu * nv > 0x07FFFFFFull) return set_error("pt_mesh_grid: too many triangles");
    const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    float nrm[3];
    if (!tess_normalise(c, nrm)) return set_error("pt_mesh_grid: cross(u, v) must have a finite length above 0");
    const size_t row = (size_t)nu + 1, n = row * ((size_t)nv + 1);
    std::vector<float> P(n * 3), N(n * 3), T(n * 2);
    std::vector<uint32_t> I((size_t)6 * nu * nv);
    for (size_t j = 0; j <= nv; ++j)
        for (size_t i = 0; i <= nu; ++i) {
            const size_t k = j * row + i;
            const double s = (double)i / (double)nu, t = (double)j / (double)nv;
            for (int a = 0; a < 3; ++a) {
                P[3 * k + a] = (float)((q[a] + u[a] * s) + v[a] * t);
                N[3 * k + a] = nrm[a];
            }
            T[2 * k] = (float)s;
            T[2 * k + 1] = (float)t;
        }
    size_t w = 0;
    for (size_t j = 0; j < nv; ++j)
        for (size_t i = 0; i < nu; ++i) {
            const uint32_t v00 = (uint32_t)(j * row + i), v10 = v00 + 1, v01 = (uint32_t)((j + 1) * row + i), v11 = v01 + 1;
            const uint32_t t6[6] = {v00, v10, v11, v00, v11, v01};
            memcpy(&I[w], t6, sizeof t6);
            w += 6;
        }
    const TessOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm, out_uv};
    return tess_hand_over(who, out, (uint32_t)n, (uint32_t)I.size(), P.data(), I.data(), N.data(), T.data());
}

extern "C" int pt_height_from_rgb8(uint32_t w, uint32_t h, const uint8_t* rgb, float* out) {
    const size_t n = (size_t)w * h;
    if (n && (!rgb || !out)) return set_error("pt_height_from_rgb8: null buffer");
    for (size_t k = 0; k < n; ++k)
        out[k] = (float)(((0.2126 * (double)rgb[3 * k] + 0.7152 * (double)rgb[3 * k + 1]) + 0.0722 * (double)rgb[3 * k + 2]) / 255.0);
    return 0;
}
