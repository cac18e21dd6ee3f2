// Loop subdivision, the host side (include/pt_amd.h has the rule): the refusals both entry points share and
// pt_mesh_subdivide_host, the GPU stage's twin: std::sort where the device sorts by radix, the same pt_subdiv.h functions per element,
// the same passes in the same order. Plain C++: nothing here touches a device.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_subdiv.h"

namespace pt {

int set_error(const std::string& msg);   // pt_error.cpp; returns -1

int subdiv_check(const char* who, const void* opts_, const SubdivIn& in, const SubdivOut& out, SubdivPlan& plan) {
    const std::string p = std::string(who) + ": ";
    pt_subdiv_opts o;
    if (opts_) o = *(const pt_subdiv_opts*)opts_;
    else pt_subdiv_opts_default(&o);
    if (!out.pos || !out.n_pos || !out.idx || !out.n_idx || !out.nrm || !out.uv) return set_error(p + "null output pointer");
    *out.pos = nullptr; *out.idx = nullptr; *out.nrm = nullptr; *out.uv = nullptr;
    *out.n_pos = 0; *out.n_idx = 0;
    if (out.crease) *out.crease = nullptr;
    if ((in.n_pos && !in.pos) || (in.n_idx && !in.idx) || (in.n_uv && !in.uv)) return set_error(p + "null input array");
    if (in.n_idx % 3 != 0) return set_error(p + "index count must be a multiple of 3");
    if (o.limit != 0 && o.limit != 1) return set_error(p + "limit must be 0 or 1");
    if (o.normals != 0 && o.normals != 1) return set_error(p + "normals must be 0 (smooth) or 1 (none)");
    if (o.crease_cos != o.crease_cos || o.corner_cos != o.corner_cos) return set_error(p + "crease_cos and corner_cos must not be NaN");
    if (o.levels > 12) return set_error(p + "levels must be at most 12");
    const uint64_t F = in.n_idx / 3, grow = 1ull << (2 * o.levels);   // 4^levels <= 2^24
    if (F * grow > 0x07FFFFFFull) return set_error(p + "too many triangles: 4^levels * faces must be at most 0x07FFFFFF");
    if ((uint64_t)in.n_pos + (grow - 1) * F > 0xFFFFFFFFull) return set_error(p + "too many vertices: the vertex count passes 32 bits");
    for (uint32_t i = 0; i < in.n_idx; ++i) {
        if (in.idx[i] >= in.n_pos) return set_error(p + "position index out of range");
        if (in.n_uv && in.idx[i] >= in.n_uv) return set_error(p + "texcoord index out of range");
    }
    plan.levels = o.levels;
    plan.n = in.n_pos;
    plan.F = (uint32_t)F;
    plan.has_uv = in.n_uv != 0;
    plan.has_crease = in.crease != nullptr;
    plan.limit = o.limit == 1;
    plan.normals = o.normals == 0;
    plan.want_crease = out.crease != nullptr;
    plan.crease_cos = o.crease_cos;
    plan.corner_cos = o.corner_cos;
    return 0;
}

namespace {

struct HostMesh {
    std::vector<float> P, T;      // T empty: no texcoords
    std::vector<uint32_t> I;
    std::vector<uint8_t> Cr;      // one byte per slot, 0 or 1
    size_t n = 0, F = 0;
};

// The sorted (key, slot) pairs of a mesh and, per distinct key in ascending order, where its run begins
struct Edges {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> slots, rank, head;   // rank: of each sorted pair; head[r]: the first pair of rank r (head[E] = M)
    size_t E = 0;
};

void build_edges(const HostMesh& m, Edges& e) {
    const size_t M = 3 * m.F;
    std::vector<std::pair<uint64_t, uint32_t>> ks(M);
    for (size_t f = 0; f < m.F; ++f)
        for (uint32_t k = 0; k < 3; ++k) ks[3 * f + k] = {tess_edge_key(m.I[3 * f + k], m.I[3 * f + (k + 1) % 3]), (uint32_t)(3 * f + k)};
    std::sort(ks.begin(), ks.end());
    e.keys.resize(M); e.slots.resize(M); e.rank.resize(M); e.head.clear();
    for (size_t i = 0; i < M; ++i) {
        e.keys[i] = ks[i].first;
        e.slots[i] = ks[i].second;
        if (i == 0 || ks[i].first != ks[i - 1].first) e.head.push_back((uint32_t)i);
        e.rank[i] = (uint32_t)(e.head.size() - 1);
    }
    e.E = e.head.size();
    e.head.push_back((uint32_t)M);
}

void angle_pass(HostMesh& m, const Edges& e, double crease_cos) {
    for (size_t r = 0; r < e.E; ++r) {
        const size_t i = e.head[r], len = e.head[r + 1] - i;
        const uint64_t key = e.keys[i];
        if (len != 2 || (uint32_t)(key >> 32) == (uint32_t)key) continue;
        if (subdiv_fold(m.P.data(), m.I.data(), e.slots[i] / 3u, e.slots[i + 1] / 3u, crease_cos)) m.Cr[e.slots[i]] = m.Cr[e.slots[i + 1]] = 1;
    }
}

// Per edge rank: what its run says; and the sorted rays with each vertex's run
struct Rings {
    std::vector<SubdivEdge> edge;
    std::vector<uint8_t> sharp;
    std::vector<uint64_t> rays;
    std::vector<uint32_t> rank;
    std::vector<size_t> start;   // n + 1 entries
};

void build_rings(const HostMesh& m, const Edges& e, Rings& g) {
    g.edge.resize(e.E);
    g.sharp.resize(e.E + 1);
    std::vector<std::pair<uint64_t, uint32_t>> rr;
    rr.reserve(2 * e.E);
    for (size_t r = 0; r < e.E; ++r) {
        const size_t i = e.head[r];
        const uint32_t A = (uint32_t)(e.keys[i] >> 32), B = (uint32_t)e.keys[i];
        g.edge[r] = subdiv_edge(A, B, e.slots.data() + i, e.head[r + 1] - i, m.I.data(), m.Cr.data());
        g.sharp[r] = g.edge[r].sharp ? 1 : 0;
        if (A != B) {
            rr.push_back({((uint64_t)A << 32) | B, (uint32_t)r});
            rr.push_back({((uint64_t)B << 32) | A, (uint32_t)r});
        }
    }
    std::sort(rr.begin(), rr.end());
    g.rays.resize(rr.size() + 1);
    g.rank.resize(rr.size() + 1);
    g.start.assign(m.n + 1, 0);
    size_t i = 0;
    for (size_t v = 0; v < m.n; ++v) {
        g.start[v] = i;
        while (i < rr.size() && (rr[i].first >> 32) == v) ++i;
    }
    g.start[m.n] = i;
    for (size_t j = 0; j < rr.size(); ++j) {
        g.rays[j] = rr[j].first;
        g.rank[j] = rr[j].second;
    }
}

// Every even vertex of `a` (limit = false) or its limit position (limit = true) into P / T, which hold at least a.n entries
void even_pass(const HostMesh& a, const Rings& g, double corner_cos, bool limit, float* P, float* T) {
    const bool uv = !a.T.empty();
    for (size_t v = 0; v < a.n; ++v)
        subdiv_even(a.P.data(), uv ? a.T.data() : nullptr, v, g.rays.data() + g.start[v], g.rank.data() + g.start[v], g.start[v + 1] - g.start[v], g.sharp.data(),
                    corner_cos, limit, P + 3 * v, uv ? T + 2 * v : nullptr);
}

void level(const HostMesh& a, const Edges& e, double corner_cos, HostMesh& b) {
    const bool uv = !a.T.empty();
    Rings g;
    build_rings(a, e, g);
    b.n = a.n + e.E;
    b.F = 4 * a.F;
    b.P.assign(3 * b.n + 1, 0.0f);
    b.T.assign(uv ? 2 * b.n + 1 : 0, 0.0f);
    for (size_t r = 0; r < e.E; ++r) {
        const uint64_t key = e.keys[e.head[r]];
        const size_t A = (size_t)(key >> 32), B = (size_t)(key & 0xFFFFFFFFu), C = g.edge[r].C, D = g.edge[r].D, m = a.n + r;
        subdiv_odd(&a.P[3 * A], &a.P[3 * B], &a.P[3 * C], &a.P[3 * D], 3, g.edge[r].sharp, &b.P[3 * m]);
        if (uv) subdiv_odd(&a.T[2 * A], &a.T[2 * B], &a.T[2 * C], &a.T[2 * D], 2, g.edge[r].sharp, &b.T[2 * m]);
    }
    even_pass(a, g, corner_cos, false, b.P.data(), b.T.data());
    std::vector<uint32_t> mid(3 * a.F + 1);
    for (size_t i = 0; i < 3 * a.F; ++i) mid[e.slots[i]] = (uint32_t)(a.n + e.rank[i]);
    b.I.assign(12 * a.F + 1, 0);
    b.Cr.assign(12 * a.F + 1, 0);
    for (size_t f = 0; f < a.F; ++f) {
        const uint32_t va = a.I[3 * f], vb = a.I[3 * f + 1], vc = a.I[3 * f + 2], ab = mid[3 * f], bc = mid[3 * f + 1], ca = mid[3 * f + 2];
        const uint32_t ch[12] = {va, ab, ca, ab, vb, bc, ca, bc, vc, ab, bc, ca};
        memcpy(&b.I[12 * f], ch, sizeof ch);
        const uint8_t e0 = g.edge[ab - a.n].flagged, e1 = g.edge[bc - a.n].flagged, e2 = g.edge[ca - a.n].flagged;
        const uint8_t fl[12] = {e0, 0, e2, e0, e1, 0, 0, e1, e2, 0, 0, 0};
        memcpy(&b.Cr[12 * f], fl, sizeof fl);
    }
}

template <class T>
T* dup(const T* v, size_t n) {
    T* q = (T*)malloc(n * sizeof(T) + sizeof(T));   // (never a zero-byte request: an empty array still has a pointer)
    if (q && n) memcpy(q, v, n * sizeof(T));
    return q;
}

}  // namespace
}  // namespace pt

using namespace pt;

extern "C" int pt_subdiv_opts_default(pt_subdiv_opts* o) {
    if (!o) return set_error("pt_subdiv_opts_default: null options");
    memset(o, 0, sizeof *o);
    o->levels = 1;
    o->crease_cos = -2.0;
    o->corner_cos = 2.0;
    return 0;
}

extern "C" int pt_mesh_subdivide_host(const pt_subdiv_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t n_uv, const float* uv,
                                      const uint8_t* crease, float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm,
                                      float** out_uv, uint8_t** out_crease) {
    const char* who = "pt_mesh_subdivide_host";
    const SubdivIn in{n_pos, pos, n_idx, idx, n_uv, uv, crease};
    const SubdivOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm, out_uv, out_crease};
    SubdivPlan plan;
    if (subdiv_check(who, opts, in, out, plan) != 0) return -1;
    HostMesh m;
    m.n = plan.n;
    m.F = plan.F;
    m.P.assign(3 * m.n + 1, 0.0f);   // (one spare entry everywhere: data() of an empty vector may be NULL)
    if (m.n) memcpy(m.P.data(), pos, 3 * m.n * sizeof(float));
    m.I.assign(3 * m.F + 1, 0);
    if (m.F) memcpy(m.I.data(), idx, 3 * m.F * sizeof(uint32_t));
    if (plan.has_uv) {
        m.T.assign(2 * m.n + 1, 0.0f);
        memcpy(m.T.data(), uv, std::min<size_t>(m.n, n_uv) * 2 * sizeof(float));
    }
    m.Cr.assign(3 * m.F + 1, 0);
    if (crease)
        for (size_t i = 0; i < 3 * m.F; ++i) m.Cr[i] = crease[i] != 0 ? 1 : 0;

    Edges e;
    build_edges(m, e);
    angle_pass(m, e, plan.crease_cos);
    for (uint32_t l = 0; l < plan.levels; ++l) {
        HostMesh next;
        level(m, e, plan.corner_cos, next);
        m = std::move(next);
        if (l + 1 < plan.levels || plan.limit) build_edges(m, e);
    }
    if (plan.limit) {
        Rings g;
        build_rings(m, e, g);
        std::vector<float> P(3 * m.n + 1, 0.0f), T(m.T.empty() ? 0 : 2 * m.n + 1, 0.0f);
        even_pass(m, g, plan.corner_cos, true, P.data(), T.data());
        m.P.swap(P);
        m.T.swap(T);
    }
    std::vector<float> N;
    if (plan.normals) {
        const size_t M = 3 * m.F;
        std::vector<std::pair<uint32_t, uint32_t>> vc(M);
        for (size_t c = 0; c < M; ++c) vc[c] = {m.I[c], (uint32_t)c};
        std::sort(vc.begin(), vc.end());
        std::vector<uint32_t> corners(M + 1);
        for (size_t i = 0; i < M; ++i) corners[i] = vc[i].second;
        N.assign(3 * m.n + 1, 0.0f);
        size_t i = 0;
        for (size_t v = 0; v < m.n; ++v) {
            const size_t first = i;
            while (i < M && vc[i].first == v) ++i;
            tess_smooth_normal(m.P.data(), m.I.data(), corners.data() + first, i - first, nullptr, &N[3 * v]);
        }
    }
    float* rP = dup(m.P.data(), 3 * m.n);
    uint32_t* rI = dup(m.I.data(), 3 * m.F);
    float* rN = plan.normals ? dup(N.data(), 3 * m.n) : nullptr;
    float* rT = plan.has_uv ? dup(m.T.data(), 2 * m.n) : nullptr;
    uint8_t* rC = plan.want_crease ? dup(m.Cr.data(), 3 * m.F) : nullptr;
    if (!rP || !rI || (plan.normals && !rN) || (plan.has_uv && !rT) || (plan.want_crease && !rC)) {
        free(rP); free(rI); free(rN); free(rT); free(rC);
        return set_error(std::string(who) + ": out of host memory");
    }
    *out_pos = rP; *out_n_pos = (uint32_t)m.n;
    *out_idx = rI; *out_n_idx = (uint32_t)(3 * m.F);
    *out_nrm = rN; *out_uv = rT;
    if (out_crease) *out_crease = rC;
    return 0;
}
