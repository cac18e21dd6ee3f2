// The host twin of mesh tessellation (csrc/pt_tess_host.cpp) as a stand-alone program, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/tess_host_check.cpp thu-acg-f2024-path-tracer_amd/csrc/pt_tess_host.cpp -o tess_host_check && ./tess_host_check
// It walks the small shapes of tests/test_tess_cpu.py (and the refusals) through every level 0..3, normals mode and wrap, frees what
// comes back and prints a checksum. No GPU, no Python: the sanitizers see every load and store of the twin.
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
    std::vector<float> pos, nrm, uv;
    std::vector<uint32_t> idx;
};

static uint64_t g_sum = 0;
static int g_calls = 0, g_refused = 0;

static void mix(const void* p, size_t bytes) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) g_sum = (g_sum ^ b[i]) * 1099511628211ull;
}

static int run(const Shape& s, const pt_tess_opts& o) {
    float *pos = nullptr, *nrm = nullptr, *uv = nullptr;
    uint32_t *idx = nullptr, np = 0, ni = 0;
    const int rc = pt_mesh_tessellate_host(&o, (uint32_t)(s.pos.size() / 3), s.pos.data(), (uint32_t)s.idx.size(), s.idx.data(), (uint32_t)(s.nrm.size() / 3),
                                           s.nrm.empty() ? nullptr : s.nrm.data(), (uint32_t)(s.uv.size() / 2), s.uv.empty() ? nullptr : s.uv.data(), &pos, &np, &idx, &ni,
                                           &nrm, &uv);
    ++g_calls;
    if (rc != 0) {
        ++g_refused;
        if (pos || idx || nrm || uv) { std::fprintf(stderr, "a refused call left an output behind\n"); std::exit(1); }
        return rc;
    }
    mix(pos, (size_t)np * 12);
    mix(idx, (size_t)ni * 4);
    if (nrm) mix(nrm, (size_t)np * 12);
    if (uv) mix(uv, (size_t)np * 8);
    for (uint32_t i = 0; i < ni; ++i)
        if (idx[i] >= np) { std::fprintf(stderr, "index out of range in the output\n"); std::exit(1); }
    free(pos); free(idx); free(nrm); free(uv);
    return 0;
}

static Shape grid(uint32_t nu, uint32_t nv) {
    const double q[3] = {-1.0, 0.25, 2.0}, u[3] = {2.0, 0.0, 0.5}, v[3] = {0.0, 0.1, -3.0};
    float *pos, *nrm, *uv;
    uint32_t *idx, np, ni;
    if (pt_mesh_grid(q, u, v, nu, nv, &pos, &np, &idx, &ni, &nrm, &uv) != 0) { std::fprintf(stderr, "pt_mesh_grid: %s\n", pt::g_err.c_str()); std::exit(1); }
    Shape s;
    s.pos.assign(pos, pos + 3 * (size_t)np);
    s.nrm.assign(nrm, nrm + 3 * (size_t)np);
    s.uv.assign(uv, uv + 2 * (size_t)np);
    s.idx.assign(idx, idx + ni);
    free(pos); free(idx); free(nrm); free(uv);
    return s;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const std::vector<float> tri = {0, 0, 0, 1, 0, 0.25f, 0.3f, 1, 0}, tri_n = {0, 0, 1, 0, 0, -1, 0, 1, 0}, tri_t = {0, 0, 1, 0, 0.3f, 1};
    const std::vector<float> quad = {0, 0, 0, 1, 0, 0, 1, 1, 0.5f, 0, 1, 0}, quad_t = {0, 0, 1, 0, 1, 1, 0, 1};
    const std::vector<float> tet = {1, 1, 1, 1, -1, -1, -1, 1, -1, -1, -1, 1};
    const std::vector<float> octa = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const std::vector<float> fin = {0, 0, 0, 0, 0, 1, 1, 0, 0, -1, 0.5f, 0, 0, -1, 0}, fin_t = {0, 0, 0, 0, 1, 0, -1, 0.5f, 0, -1};
    std::vector<Shape> shapes = {
        {tri, tri_n, tri_t, {0, 1, 2}},
        {quad, {}, quad_t, {0, 1, 2, 0, 2, 3}},
        {quad, {}, {}, {0, 1, 2, 3, 2, 0}},
        {tet, tet, {}, {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2}},
        {octa, {}, {}, {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5}},
        {fin, {}, fin_t, {0, 1, 2, 0, 1, 3, 1, 0, 4}},
        {tri, tri_n, tri_t, {0, 0, 1, 0, 1, 2}},
        {{9, 9, 9, 0, 0, 0, 1, 0, 0.25f, 0.3f, 1, 0, 7, 7, 7}, {1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1}, {0, 0, 0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f, 1, 2, 2}, {1, 2, 3}},
        {tri, tri_n, {}, {0, 1, 2, 0, 2, 1}},
        {{nan, 0, 0, 1, inf, 0, 0, 1, 0}, {}, {nan, 0, 0.5f, inf, 2.5f, -1.5f}, {0, 1, 2}},
        {{}, {}, {}, {}},
        grid(1, 1), grid(3, 2), grid(8, 4),
    };
    std::vector<float> img(7 * 5);
    for (size_t k = 0; k < img.size(); ++k) img[k] = 0.5f + 0.4f * std::sin(0.9f * (float)k);
    img[11] = inf;
    for (const Shape& s : shapes)
        for (uint32_t levels = 0; levels <= 3; ++levels)
            for (int normals = 0; normals <= 3; ++normals) {
                pt_tess_opts o;
                pt_tess_opts_default(&o);
                o.levels = levels;
                o.normals = normals;
                if (run(s, o) != 0) { std::fprintf(stderr, "unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
                if (s.uv.empty()) continue;
                for (int wrap = 0; wrap <= 1; ++wrap) {
                    o.height = img.data(); o.height_w = 7; o.height_h = 5; o.scale = 0.3; o.midlevel = 0.4; o.wrap = wrap;
                    if (run(s, o) != 0) { std::fprintf(stderr, "unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
                }
                o.height = nullptr;
            }
    // the refusals: nothing is read past what the counts allow, nothing is left allocated
    const int before = g_refused;
    pt_tess_opts o;
    pt_tess_opts_default(&o);
    Shape bad = shapes[0];
    bad.idx = {0, 1, 2, 0};
    run(bad, o);
    bad.idx = {0, 1, 3};
    run(bad, o);
    bad = shapes[0];
    bad.nrm.resize(6);
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
    pt_tess_opts_default(&o);
    o.wrap = 2;
    run(shapes[0], o);
    pt_tess_opts_default(&o);
    o.normals = 4;
    run(shapes[0], o);
    pt_tess_opts_default(&o);
    o.height = img.data(); o.height_w = 7; o.height_h = 5;
    run(shapes[2], o);   // a height without texcoords
    if (g_refused - before != 9) { std::fprintf(stderr, "%d of 9 bad calls were refused\n", g_refused - before); return 1; }
    std::vector<uint8_t> rgb(3 * 6 * 4);
    for (size_t k = 0; k < rgb.size(); ++k) rgb[k] = (uint8_t)(k * 37);
    std::vector<float> h(6 * 4);
    if (pt_height_from_rgb8(6, 4, rgb.data(), h.data()) != 0) return 1;
    mix(h.data(), h.size() * 4);
    std::printf("tess_host_check: %d calls (%d refused as they should be), checksum %016llx\n", g_calls, g_refused, (unsigned long long)g_sum);
    return 0;
}
