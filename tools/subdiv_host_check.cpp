// The host twin of Loop subdivision (csrc/pt_subdiv_host.cpp) as a stand-alone program, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/subdiv_host_check.cpp thu-acg-f2024-path-tracer_amd/csrc/pt_subdiv_host.cpp -o subdiv_host_check && ./subdiv_host_check
// It walks the small shapes of tests/test_subdiv_cpu.py (and the refusals) through every level 0..3, with and without texcoords, flags,
// angle tests, limit projection and normals, feeds each result's flags into a further level, frees what comes back and prints a
// checksum. No GPU, no Python: the sanitizers see every load and store of the twin.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../include/pt_amd.h"

namespace pt {
static std::string g_err;
int set_error(const std::string& msg) { g_err = msg; return -1; }   // the library's is in pt_error.cpp
}  // namespace pt

struct Shape {
    std::vector<float> pos, uv;
    std::vector<uint32_t> idx;
    std::vector<uint8_t> crease;
};

static uint64_t g_sum = 0;
static int g_calls = 0, g_refused = 0;

static void mix(const void* p, size_t bytes) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) g_sum = (g_sum ^ b[i]) * 1099511628211ull;
}

// One call; `again`: the result goes through one more level with the flags it came with
static int run(const Shape& s, const pt_subdiv_opts& o, bool want_crease = true, bool again = false) {
    float *pos = nullptr, *nrm = nullptr, *uv = nullptr;
    uint32_t *idx = nullptr, np = 0, ni = 0;
    uint8_t* cr = nullptr;
    const int rc = pt_mesh_subdivide_host(&o, (uint32_t)(s.pos.size() / 3), s.pos.empty() ? nullptr : s.pos.data(), (uint32_t)s.idx.size(), s.idx.empty() ? nullptr : s.idx.data(),
                                          (uint32_t)(s.uv.size() / 2), s.uv.empty() ? nullptr : s.uv.data(), s.crease.empty() ? nullptr : s.crease.data(), &pos, &np, &idx, &ni,
                                          &nrm, &uv, want_crease ? &cr : nullptr);
    ++g_calls;
    if (rc != 0) {
        ++g_refused;
        if (pos || idx || nrm || uv || cr) { std::fprintf(stderr, "a refused call left an output behind\n"); std::exit(1); }
        return rc;
    }
    mix(pos, (size_t)np * 12);
    mix(idx, (size_t)ni * 4);
    if (nrm) mix(nrm, (size_t)np * 12);
    if (uv) mix(uv, (size_t)np * 8);
    if (cr) mix(cr, ni);
    for (uint32_t i = 0; i < ni; ++i) {
        if (idx[i] >= np) { std::fprintf(stderr, "index out of range in the output\n"); std::exit(1); }
        if (cr && cr[i] > 1) { std::fprintf(stderr, "a flag that is neither 0 nor 1\n"); std::exit(1); }
    }
    if (again && cr) {
        Shape t;
        t.pos.assign(pos, pos + 3 * (size_t)np);
        if (uv) t.uv.assign(uv, uv + 2 * (size_t)np);
        t.idx.assign(idx, idx + ni);
        t.crease.assign(cr, cr + ni);
        pt_subdiv_opts o1 = o;
        o1.levels = 1;
        if (run(t, o1) != 0) { std::fprintf(stderr, "the second call was refused: %s\n", pt::g_err.c_str()); std::exit(1); }
    }
    free(pos); free(idx); free(nrm); free(uv); free(cr);
    return 0;
}

static Shape grid(uint32_t nu, uint32_t nv) {
    Shape s;
    for (uint32_t j = 0; j <= nv; ++j)
        for (uint32_t i = 0; i <= nu; ++i) {
            const float x = (float)i, z = (float)j;
            s.pos.insert(s.pos.end(), {x, 0.1f * std::sin(1.3f * x + 0.7f * z), z});
            s.uv.insert(s.uv.end(), {x / (float)nu, z / (float)nv});
        }
    for (uint32_t j = 0; j < nv; ++j)
        for (uint32_t i = 0; i < nu; ++i) {
            const uint32_t v00 = j * (nu + 1) + i, v10 = v00 + 1, v01 = v00 + nu + 1, v11 = v01 + 1;
            s.idx.insert(s.idx.end(), {v00, v10, v11, v00, v11, v01});
        }
    return s;
}

static Shape fan(uint32_t valence, bool closed) {
    Shape s;
    s.pos = {0, 0.5f, 0};
    s.uv = {0.5f, 0.5f};
    for (uint32_t k = 0; k < valence; ++k) {
        const float t = 6.2831853f * (float)k / (float)valence;
        s.pos.insert(s.pos.end(), {std::cos(t), 0.2f * std::sin(3 * t), std::sin(t)});
        s.uv.insert(s.uv.end(), {0.5f + 0.5f * std::cos(t), 0.5f + 0.5f * std::sin(t)});
    }
    for (uint32_t k = 0; k < (closed ? valence : valence - 1); ++k) s.idx.insert(s.idx.end(), {0u, 1 + (k + 1) % valence, 1 + k});
    return s;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const std::vector<float> tri = {0, 0, 0, 1, 0, 0.25f, 0.3f, 1, 0}, tri_t = {0, 0, 1, 0, 0.3f, 1};
    const std::vector<float> quad = {0, 0, 0, 1, 0, 0, 1, 1, 0.5f, 0, 1, 0}, quad_t = {0, 0, 1, 0, 1, 1, 0, 1};
    const std::vector<float> tet = {1, 1, 1, 1, -1, -1, -1, 1, -1, -1, -1, 1};
    const std::vector<float> octa = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const std::vector<float> fin = {0, 0, 0, 0, 0, 1, 1, 0, 0, -1, 0.5f, 0, 0, -1, 0}, fin_t = {0, 0, 0, 0, 1, 0, -1, 0.5f, 0, -1};
    std::vector<float> cube;
    for (int z = 0; z < 2; ++z)
        for (int y = 0; y < 2; ++y)
            for (int x = 0; x < 2; ++x) cube.insert(cube.end(), {(float)x, (float)y, (float)z});
    const std::vector<uint32_t> cube_i = {0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5};
    std::vector<uint8_t> cube_c;
    for (int f = 0; f < 6; ++f) cube_c.insert(cube_c.end(), {1, 1, 0, 0, 1, 1});
    std::vector<Shape> shapes = {
        {tri, tri_t, {0, 1, 2}, {}},
        {quad, quad_t, {0, 1, 2, 0, 2, 3}, {}},
        {quad, quad_t, {0, 1, 2, 0, 2, 3}, {0, 0, 1, 0, 0, 0}},     // a crease flagged on one side only
        {quad, {}, {0, 1, 2, 3, 2, 0}, {}},                         // opposed winding
        {tet, {}, {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2}, {}},
        {octa, {}, {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5}, {}},
        {fin, fin_t, {0, 1, 2, 0, 1, 3, 1, 0, 4}, {}},              // an edge of three faces
        {tri, tri_t, {0, 0, 1, 0, 1, 2}, {}},                       // face (a, a, b)
        {{9, 9, 9, 0, 0, 0, 1, 0, 0.25f, 0.3f, 1, 0, 7, 7, 7}, {0, 0, 0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f, 1, 2, 2}, {1, 2, 3}, {}},   // unreferenced vertices, extra texcoords
        {tri, {}, {0, 1, 2, 0, 2, 1}, {}},
        {{nan, 0, 0, 1, inf, 0, 0, 1, 0}, {nan, 0, 0.5f, inf, 2.5f, -1.5f}, {0, 1, 2}, {}},
        {{}, {}, {}, {}},
        {cube, {}, cube_i, cube_c},
        {cube, {}, cube_i, {}},
        grid(1, 1), grid(3, 2), grid(8, 4), fan(40, true), fan(40, false),
    };
    for (const Shape& s : shapes)
        for (uint32_t levels = 0; levels <= 3; ++levels)
            for (int variant = 0; variant < 8; ++variant) {
                pt_subdiv_opts o;
                pt_subdiv_opts_default(&o);
                o.levels = levels;
                o.limit = variant & 1;
                o.normals = (variant >> 1) & 1;
                if (variant & 4) { o.crease_cos = std::cos(0.7); o.corner_cos = std::cos(1.8); }
                if (run(s, o, true, levels == 1) != 0 || run(s, o, false) != 0) { std::fprintf(stderr, "unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
                if (s.uv.empty()) continue;
                Shape bare = s;
                bare.uv.clear();
                if (run(bare, o) != 0) { std::fprintf(stderr, "unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
            }
    if (pt_mesh_subdivide_host(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != -1) return 1;
    // the refusals: nothing is read past what the counts allow, nothing is left allocated
    const int before = g_refused;
    pt_subdiv_opts o;
    pt_subdiv_opts_default(&o);
    Shape bad = shapes[0];
    bad.idx = {0, 1, 2, 0};
    run(bad, o);
    bad.idx = {0, 1, 3};
    run(bad, o);
    bad = shapes[0];
    bad.uv.resize(4);
    run(bad, o);
    o.levels = 13;
    run(shapes[0], o);
    o.levels = 12;
    bad = shapes[0];
    bad.idx = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2};
    run(bad, o);
    pt_subdiv_opts_default(&o);
    o.limit = 2;
    run(shapes[0], o);
    pt_subdiv_opts_default(&o);
    o.normals = 2;
    run(shapes[0], o);
    pt_subdiv_opts_default(&o);
    o.crease_cos = nan;
    run(shapes[0], o);
    pt_subdiv_opts_default(&o);
    o.corner_cos = nan;
    run(shapes[0], o);
    if (g_refused - before != 9) { std::fprintf(stderr, "%d of 9 bad calls were refused\n", g_refused - before); return 1; }
    std::printf("subdiv_host_check: %d calls (%d refused as they should be), checksum %016llx\n", g_calls, g_refused, (unsigned long long)g_sum);
    return 0;
}
