// Mesh welding and simplification, the host side (include/pt_amd.h has the rule): the refusals both entry points share
// and pt_mesh_simplify_host, the GPU stage's twin: std::stable_sort where the device sorts by radix, running sums where it scans, the
// same pt_simplify.h functions per element, the same passes in the same order. Plain C++: nothing here touches a device.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_simplify.h"

namespace pt {

int set_error(const std::string& msg);   // pt_error.cpp; returns -1

int simplify_check(const char* who, const void* opts_, const SimpIn& in, const SimpOut& out, SimpPlan& plan) {
    const std::string p = std::string(who) + ": ";
    pt_simplify_opts o;
    if (opts_) o = *(const pt_simplify_opts*)opts_;
    else pt_simplify_opts_default(&o);
    if (!out.pos || !out.n_pos || !out.idx || !out.n_idx || !out.nrm || !out.uv) return set_error(p + "null output pointer");
    *out.pos = nullptr; *out.idx = nullptr; *out.nrm = nullptr; *out.uv = nullptr;
    *out.n_pos = 0; *out.n_idx = 0;
    if (out.map) *out.map = nullptr;
    if ((in.n_pos && !in.pos) || (in.n_idx && !in.idx) || (in.n_uv && !in.uv)) return set_error(p + "null input array");
    if (in.n_idx == 0 || in.n_idx % 3 != 0) return set_error(p + "index count must be a multiple of 3 above 0");
    if (in.n_idx / 3 > SIMP_MAX_FACES) return set_error(p + "too many triangles: at most 0x07FFFFFF");
    if (o.mode != 0 && o.mode != 1) return set_error(p + "mode must be 0 (weld) or 1 (cluster)");
    if (o.placement != 0 && o.placement != 1) return set_error(p + "placement must be 0 (quadric) or 1 (mean)");
    if (o.dedup != 0 && o.dedup != 1) return set_error(p + "dedup must be 0 or 1");
    if (o.normals != 0 && o.normals != 1) return set_error(p + "normals must be 0 (smooth) or 1 (none)");
    if (o.mode == 1) {
        if (!tess_finite(o.cell) || o.cell < 0.0) return set_error(p + "cell must be finite and not negative");
        if (o.cell == 0.0 && o.grid_n == 0) return set_error(p + "cell and grid_n cannot both be 0");
        if (!(o.reg >= 1e-6 && o.reg <= 1.0)) return set_error(p + "reg must lie in [1e-6, 1]");
    }
    for (uint32_t i = 0; i < in.n_idx; ++i) {
        if (in.idx[i] >= in.n_pos) return set_error(p + "position index out of range");
        if (in.n_uv && in.idx[i] >= in.n_uv) return set_error(p + "texcoord index out of range");
    }
    for (size_t i = 0; i < 3 * (size_t)in.n_pos; ++i)
        if (!tess_finite((double)in.pos[i])) return set_error(p + "every position must be finite");
    plan.n = in.n_pos;
    plan.F = in.n_idx / 3;
    plan.has_uv = in.n_uv != 0;
    plan.mode = o.mode;
    plan.quadric = o.mode == 1 && o.placement == 0;
    plan.dedup = o.dedup == 1;
    plan.normals = o.normals == 0;
    plan.want_map = out.map != nullptr;
    plan.reg = o.reg;
    plan.grid = SimpGrid{{0.0, 0.0, 0.0}, 0.0};
    if (o.mode == 1) {   // the bounds of the referenced positions (a minimum and a maximum: no order in them)
        double lo[3], hi[3];
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = (double)in.pos[3 * (size_t)in.idx[0] + a];
        for (uint32_t i = 1; i < in.n_idx; ++i)
            for (int a = 0; a < 3; ++a) {
                const double v = (double)in.pos[3 * (size_t)in.idx[i] + a];
                lo[a] = v < lo[a] ? v : lo[a];
                hi[a] = v > hi[a] ? v : hi[a];
            }
        double E = 0.0;
        for (int a = 0; a < 3; ++a) E = hi[a] - lo[a] > E ? hi[a] - lo[a] : E;
        if (E == 0.0) return set_error(p + "the referenced positions have no extent");
        const double cell = o.cell > 0.0 ? o.cell : E / (double)o.grid_n;
        if (!(tess_finite(cell) && cell > 0.0)) return set_error(p + "the cell has no usable size");
        for (int a = 0; a < 3; ++a)
            if (!(__builtin_floor((hi[a] - lo[a]) / cell) < 2097152.0)) return set_error(p + "too many cells: at most 2^21 along an axis");
        for (int a = 0; a < 3; ++a) plan.grid.lo[a] = lo[a];
        plan.grid.cell = cell;
    }
    return 0;
}

namespace {

template <class T>
T* dup(const T* v, size_t n) {
    T* q = (T*)malloc(n * sizeof(T) + sizeof(T));   // (never a zero-byte request: an empty array still has a pointer)
    if (q && n) memcpy(q, v, n * sizeof(T));
    return q;
}

// TSUM over term(0) .. term(L - 1), L >= 1
template <class Fn>
double tsum(size_t L, Fn term) {
    double acc = 0.0;
    for (size_t j = 0; j * SIMP_TILE < L; ++j) {
        double s[SIMP_TILE];
        for (size_t i = 0; i < (size_t)SIMP_TILE; ++i) s[i] = j * SIMP_TILE + i < L ? term(j * SIMP_TILE + i) : 0.0;
        const double t = simp_tile_tree(s);
        acc = j == 0 ? t : acc + t;
    }
    return acc;
}

}  // namespace
}  // namespace pt

using namespace pt;

extern "C" int pt_simplify_opts_default(pt_simplify_opts* o) {
    if (!o) return set_error("pt_simplify_opts_default: null options");
    memset(o, 0, sizeof *o);
    o->mode = 1;
    o->grid_n = 64;
    o->reg = 1e-3;
    o->dedup = 1;
    return 0;
}

extern "C" int pt_mesh_simplify_host(const pt_simplify_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t n_uv, const float* uv,
                                     float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm, float** out_uv, uint32_t** out_map) {
    const char* who = "pt_mesh_simplify_host";
    const SimpIn in{n_pos, pos, n_idx, idx, n_uv, uv};
    const SimpOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm, out_uv, out_map};
    SimpPlan plan;
    if (simplify_check(who, opts, in, out, plan) != 0) return -1;
    const size_t n = plan.n, F = plan.F, M = 3 * F;
    const SimpGrid& g = plan.grid;
    std::vector<float> T;   // the texcoords brought to n entries
    if (plan.has_uv) {
        T.assign(2 * n + 1, 0.0f);
        memcpy(T.data(), uv, std::min<size_t>(n, n_uv) * 2 * sizeof(float));
    }

    // 1, 2: the referenced vertices in ascending order, and their keys
    std::vector<uint8_t> ref(n + 1, 0);
    for (size_t s = 0; s < M; ++s) ref[idx[s]] = 1;
    std::vector<uint32_t> sv;
    for (size_t v = 0; v < n; ++v)
        if (ref[v]) sv.push_back((uint32_t)v);
    std::vector<uint64_t> key(plan.mode == 1 ? n + 1 : 0, SIMP_NO_KEY);
    auto wbits = [&](uint32_t v, int a) { return simp_weld_bits(pos[3 * (size_t)v + a]); };
    if (plan.mode == 1) {
        for (uint32_t v : sv) key[v] = simp_cell_key(g, pos + 3 * (size_t)v);
        std::stable_sort(sv.begin(), sv.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    } else {
        std::stable_sort(sv.begin(), sv.end(), [&](uint32_t a, uint32_t b) {
            for (int c = 0; c < 3; ++c)
                if (wbits(a, c) != wbits(b, c)) return wbits(a, c) < wbits(b, c);
            return false;
        });
    }
    auto same_key = [&](uint32_t a, uint32_t b) {
        return plan.mode == 1 ? key[a] == key[b] : (wbits(a, 0) == wbits(b, 0) && wbits(a, 1) == wbits(b, 1) && wbits(a, 2) == wbits(b, 2));
    };

    // 3: the runs; a cluster's id is the rank of its head among the heads, in vertex order
    const size_t nref = sv.size();
    std::vector<uint32_t> run_start;   // per run in key order, and nref at the end
    for (size_t i = 0; i < nref; ++i)
        if (i == 0 || !same_key(sv[i - 1], sv[i])) run_start.push_back((uint32_t)i);
    const size_t C = run_start.size();
    run_start.push_back((uint32_t)nref);
    std::vector<uint32_t> head_rank(n + 1, 0);
    {
        std::vector<uint8_t> is_head(n + 1, 0);
        for (size_t r = 0; r < C; ++r) is_head[sv[run_start[r]]] = 1;
        uint32_t sum = 0;
        for (size_t v = 0; v < n; ++v) {
            head_rank[v] = sum;
            sum += is_head[v];
        }
    }
    std::vector<uint32_t> vcl(n + 1, SIMP_NONE), crun(C + 1, 0);   // a vertex's cluster; a cluster's run
    for (size_t r = 0; r < C; ++r) {
        const uint32_t c = head_rank[sv[run_start[r]]];
        crun[c] = (uint32_t)r;
        for (size_t i = run_start[r]; i < run_start[r + 1]; ++i) vcl[sv[i]] = c;
    }

    // 6: a cluster's position and texcoord
    std::vector<float> cpos(3 * C + 1, 0.0f), cuv(plan.has_uv ? 2 * C + 1 : 0, 0.0f);
    std::vector<uint32_t> corner, corner_start;
    if (plan.quadric) {   // the (cluster, slot) pairs, slots ascending within a cluster
        corner.resize(M);
        std::iota(corner.begin(), corner.end(), 0u);
        std::stable_sort(corner.begin(), corner.end(), [&](uint32_t a, uint32_t b) { return vcl[idx[a]] < vcl[idx[b]]; });
        corner_start.assign(C + 1, (uint32_t)M);
        for (size_t i = M; i-- > 0;) corner_start[vcl[idx[corner[i]]]] = (uint32_t)i;   // (every cluster has a corner: its members are referenced)
    }
    for (size_t c = 0; c < C; ++c) {
        const size_t r = crun[c], first = run_start[r], count = run_start[r + 1] - first;
        const uint32_t* mem = sv.data() + first;
        if (plan.mode == 0) {
            memcpy(&cpos[3 * c], pos + 3 * (size_t)mem[0], 12);
            if (plan.has_uv) memcpy(&cuv[2 * c], &T[2 * (size_t)mem[0]], 8);
            continue;
        }
        double o[3], m[3], x[3];
        simp_cell_origin(g, key[mem[0]], o);
        for (int a = 0; a < 3; ++a) m[a] = tsum(count, [&](size_t i) { return ((double)pos[3 * (size_t)mem[i] + a] - o[a]) / (double)count; });
        if (plan.has_uv)
            for (int a = 0; a < 2; ++a) cuv[2 * c + a] = (float)(tsum(count, [&](size_t i) { return (double)T[2 * (size_t)mem[i] + a]; }) / (double)count);
        if (plan.quadric) {
            const size_t cf = corner_start[c], len = corner_start[c + 1] - cf;
            std::vector<double> terms(9 * len);
            for (size_t i = 0; i < len; ++i) simp_corner_terms(pos, idx + 3 * (size_t)(corner[cf + i] / 3u), o, &terms[9 * i]);
            double q[9];
            for (int k = 0; k < 9; ++k) q[k] = tsum(len, [&](size_t i) { return terms[9 * i + k]; });
            simp_solve(q, m, plan.reg, g.cell, x);
        } else {
            x[0] = m[0]; x[1] = m[1]; x[2] = m[2];
        }
        for (int a = 0; a < 3; ++a) cpos[3 * c + a] = (float)(o[a] + x[a]);
    }

    // 4: the faces that survive
    std::vector<uint8_t> keep(F + 1, 0);
    {
        std::vector<uint32_t> lo(F + 1), mid(F + 1), hi(F + 1), live;
        std::vector<uint8_t> odd(F + 1, 0);
        for (size_t f = 0; f < F; ++f) {
            const uint32_t A = vcl[idx[3 * f]], B = vcl[idx[3 * f + 1]], Cc = vcl[idx[3 * f + 2]];
            if (A == B || B == Cc || Cc == A) continue;
            if (!plan.dedup) {
                keep[f] = 1;
                continue;
            }
            odd[f] = simp_sorted_triple(A, B, Cc, lo[f], mid[f], hi[f]) ? 1 : 0;
            live.push_back((uint32_t)f);
        }
        std::stable_sort(live.begin(), live.end(), [&](uint32_t a, uint32_t b) {
            if (lo[a] != lo[b]) return lo[a] < lo[b];
            if (mid[a] != mid[b]) return mid[a] < mid[b];
            return hi[a] < hi[b];
        });
        for (size_t i = 0; i < live.size();) {
            size_t j = i, e = 0, od = 0;
            const uint32_t f0 = live[i];
            for (; j < live.size() && lo[live[j]] == lo[f0] && mid[live[j]] == mid[f0] && hi[live[j]] == hi[f0]; ++j) (odd[live[j]] ? od : e) += 1;
            const uint8_t want = od > e ? 1 : 0;
            size_t left = od > e ? od - e : e - od;
            for (size_t k = i; k < j && left; ++k)
                if (odd[live[k]] == want) {
                    keep[live[k]] = 1;
                    --left;
                }
            i = j;
        }
    }

    // 5: the clusters a surviving face names, in cluster order; the faces in face order
    std::vector<uint8_t> used(C + 1, 0);
    size_t Fo = 0;
    for (size_t f = 0; f < F; ++f)
        if (keep[f]) {
            ++Fo;
            for (int k = 0; k < 3; ++k) used[vcl[idx[3 * f + k]]] = 1;
        }
    std::vector<uint32_t> cout_(C + 1, 0);
    size_t no = 0;
    for (size_t c = 0; c < C; ++c) {
        cout_[c] = (uint32_t)no;
        no += used[c];
    }
    std::vector<float> P(3 * no + 1, 0.0f), U(plan.has_uv ? 2 * no + 1 : 0, 0.0f), N(plan.normals ? 3 * no + 1 : 0, 0.0f);
    std::vector<uint32_t> I(3 * Fo + 1, 0), map(plan.want_map ? n + 1 : 0, SIMP_NONE);
    for (size_t c = 0; c < C; ++c)
        if (used[c]) {
            memcpy(&P[3 * (size_t)cout_[c]], &cpos[3 * c], 12);
            if (plan.has_uv) memcpy(&U[2 * (size_t)cout_[c]], &cuv[2 * c], 8);
        }
    for (size_t f = 0, w = 0; f < F; ++f)
        if (keep[f])
            for (int k = 0; k < 3; ++k) I[w++] = cout_[vcl[idx[3 * f + k]]];
    if (plan.want_map)
        for (size_t v = 0; v < n; ++v)
            if (vcl[v] != SIMP_NONE && used[vcl[v]]) map[v] = cout_[vcl[v]];
    if (plan.normals) {   // section 27's smooth normals of the finished mesh
        const size_t Mo = 3 * Fo;
        std::vector<uint32_t> oc(Mo + 1);
        std::iota(oc.begin(), oc.begin() + Mo, 0u);
        std::stable_sort(oc.begin(), oc.begin() + Mo, [&](uint32_t a, uint32_t b) { return I[a] < I[b]; });
        size_t i = 0;
        for (size_t v = 0; v < no; ++v) {
            const size_t first = i;
            while (i < Mo && I[oc[i]] == v) ++i;
            tess_smooth_normal(P.data(), I.data(), oc.data() + first, i - first, nullptr, &N[3 * v]);
        }
    }
    float* rP = dup(P.data(), 3 * no);
    uint32_t* rI = dup(I.data(), 3 * Fo);
    float* rN = plan.normals ? dup(N.data(), 3 * no) : nullptr;
    float* rU = plan.has_uv ? dup(U.data(), 2 * no) : nullptr;
    uint32_t* rM = plan.want_map ? dup(map.data(), n) : nullptr;
    if (!rP || !rI || (plan.normals && !rN) || (plan.has_uv && !rU) || (plan.want_map && !rM)) {
        free(rP); free(rI); free(rN); free(rU); free(rM);
        return set_error(std::string(who) + ": out of host memory");
    }
    *out_pos = rP; *out_n_pos = (uint32_t)no;
    *out_idx = rI; *out_n_idx = (uint32_t)(3 * Fo);
    *out_nrm = rN; *out_uv = rU;
    if (out_map) *out_map = rM;
    return 0;
}
