// The host twin of mesh welding and simplification (csrc/pt_simplify_host.cpp) as a stand-alone program, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/simplify_host_check.cpp thu-acg-f2024-path-tracer_amd/csrc/pt_simplify_host.cpp -o simplify_host_check && ./simplify_host_check
// It walks a cube, an octahedron, a finely gridded plane, a fan with a long corner run, a mesh with unreferenced vertices, repeated indices
// and coincident faces, and a mesh taken apart face by face through both modes, both placements, both dedup values, both normals values,
// with and without texcoords and with and without the vertex map, then the refusals, and prints a checksum. The arrays are exactly as
// large as the call says, so a read or write past them is one past the allocation. No GPU, no Python: the sanitizers see every load and
// store of the twin.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/pt_amd.h"

namespace pt {
static std::string g_err;
int set_error(const std::string& msg) { g_err = msg; return -1; }   // the library's is in pt_error.cpp
}  // namespace pt

extern "C" void pt_free(void* p) { free(p); }   // the library's is in pt_assets.cpp

struct M {
    std::vector<float> pos, uv;
    std::vector<uint32_t> idx;
};

static uint64_t g_sum = 0;
static int g_calls = 0, g_refused = 0;

static M cube(float x0, float y0, float z0, float x1, float y1, float z1) {
    M m;
    for (int b = 0; b < 8; ++b) {
        m.pos.push_back(b & 1 ? x1 : x0); m.pos.push_back(b & 2 ? y1 : y0); m.pos.push_back(b & 4 ? z1 : z0);
    }
    const uint32_t q[6][4] = {{0, 2, 3, 1}, {4, 5, 7, 6}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 4, 6, 2}, {1, 3, 7, 5}};
    for (auto& f : q)
        for (uint32_t c : {f[0], f[1], f[2], f[0], f[2], f[3]}) m.idx.push_back(c);
    return m;
}

static M octahedron(float cx, float cy, float cz, float r) {
    M m;
    const float v[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
    for (auto& p : v) { m.pos.push_back(cx + r * p[0]); m.pos.push_back(cy + r * p[1]); m.pos.push_back(cz + r * p[2]); }
    m.idx = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    return m;
}

static M plane(uint32_t nu, uint32_t nv) {
    M m;
    for (uint32_t j = 0; j <= nv; ++j)
        for (uint32_t i = 0; i <= nu; ++i) {
            const float u = (float)i / nu, v = (float)j / nv;
            m.pos.push_back(0.1f + 2.0f * u - 0.4f * v); m.pos.push_back(0.2f + 0.5f * u + 1.5f * v); m.pos.push_back(0.3f + 0.3f * u + 0.8f * v);
        }
    for (uint32_t j = 0; j < nv; ++j)
        for (uint32_t i = 0; i < nu; ++i) {
            const uint32_t a = j * (nu + 1) + i, b = a + 1, c = a + nu + 2, d = a + nu + 1;
            for (uint32_t k : {a, b, c, a, c, d}) m.idx.push_back(k);
        }
    return m;
}

static M fan(uint32_t corners) {   // a hub alone in its cell with `corners` corners
    M m;
    m.pos = {0.1f, 0.1f, 0.1f};
    for (uint32_t i = 0; i <= corners; ++i) { m.pos.push_back(2.0f + 1.5f * i); m.pos.push_back(1.0f + 0.5f * std::sin(0.37f * i)); m.pos.push_back(0.5f); }
    for (uint32_t i = 0; i < corners; ++i) { m.idx.push_back(0); m.idx.push_back(1 + i); m.idx.push_back(2 + i); }
    return m;
}

static M exploded(const M& a) {   // every face with vertices of its own; zero coordinates alternate -0 / +0
    M m;
    int flip = 0;
    for (size_t s = 0; s < a.idx.size(); ++s) {
        for (int c = 0; c < 3; ++c) {
            float v = a.pos[3 * a.idx[s] + c];
            if (v == 0.0f && (flip++ & 1)) v = -0.0f;
            m.pos.push_back(v);
        }
        m.idx.push_back((uint32_t)s);
    }
    return m;
}

static M junk() {   // unreferenced vertices at both ends and in the middle, repeated indices, copies of one face and flipped ones
    M m = octahedron(1.2f, 2.4f, 3.7f, 0.9f);
    m.pos.insert(m.pos.begin(), {100.0f, 100.0f, 100.0f});
    for (auto& i : m.idx) i += 1;
    m.pos.insert(m.pos.end(), {-50.0f, 0.0f, 3.0f, 7.0f, 7.0f, 7.0f});
    for (uint32_t i : {1u, 1u, 2u, 3u, 4u, 4u, 6u, 6u, 6u, 1u, 3u, 5u, 3u, 5u, 1u, 1u, 5u, 3u, 5u, 3u, 1u, 3u, 1u, 5u}) m.idx.push_back(i);
    return m;
}

static void with_uv(M& m) {
    m.uv.clear();
    for (size_t v = 0; v < m.pos.size() / 3; ++v) { m.uv.push_back(0.5f * m.pos[3 * v] + m.pos[3 * v + 2]); m.uv.push_back(m.pos[3 * v + 1] - 0.25f); }
}

static void mix(const void* p, size_t bytes) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < bytes; ++i) g_sum = g_sum * 1099511628211ull + b[i];
}

static int run(const M& m, const pt_simplify_opts* o, bool want_map, uint32_t* faces_out = nullptr) {
    float *pos = nullptr, *nrm = nullptr, *uv = nullptr;
    uint32_t *idx = nullptr, *map = nullptr, np = 0, ni = 0;
    const uint32_t n = (uint32_t)(m.pos.size() / 3);
    const int rc = pt_mesh_simplify_host(o, n, m.pos.data(), (uint32_t)m.idx.size(), m.idx.data(), (uint32_t)(m.uv.size() / 2), m.uv.empty() ? nullptr : m.uv.data(), &pos, &np,
                                         &idx, &ni, &nrm, &uv, want_map ? &map : nullptr);
    ++g_calls;
    if (rc != 0) {
        ++g_refused;
        if (pos || idx || nrm || uv || map) { printf("a refusal left an array behind\n"); exit(1); }
        return rc;
    }
    // shrink every array to its exact size, so that a checksum that reads past one is caught
    auto exact = [](void* p, size_t bytes) { void* q = malloc(bytes ? bytes : 1); if (bytes) memcpy(q, p, bytes); free(p); return q; };
    pos = (float*)exact(pos, (size_t)np * 12); idx = (uint32_t*)exact(idx, (size_t)ni * 4);
    mix(pos, (size_t)np * 12); mix(idx, (size_t)ni * 4);
    if (nrm) { nrm = (float*)exact(nrm, (size_t)np * 12); mix(nrm, (size_t)np * 12); }
    if (uv) { uv = (float*)exact(uv, (size_t)np * 8); mix(uv, (size_t)np * 8); }
    if (map) { map = (uint32_t*)exact(map, (size_t)n * 4); mix(map, (size_t)n * 4); }
    for (uint32_t i = 0; i < ni; ++i)
        if (idx[i] >= np) { printf("an output index is out of range\n"); exit(1); }
    if (faces_out) *faces_out = ni / 3;
    pt_free(pos); pt_free(idx); pt_free(nrm); pt_free(uv); pt_free(map);
    return 0;
}

int main() {
    std::vector<M> meshes = {cube(0.1f, 1.2f, 2.6f, 2.3f, 3.9f, 4.8f), octahedron(1.2f, 2.4f, 3.7f, 0.9f), plane(40, 33), fan(1), fan(17), fan(5000), junk(),
                             exploded(cube(-0.5f, 0.0f, -1.0f, 0.0f, 1.0f, 0.0f)), exploded(plane(9, 7))};
    for (M& m : meshes)
        for (int uv = 0; uv < 2; ++uv) {
            if (uv) with_uv(m);
            for (int mode = 0; mode < 2; ++mode)
                for (int placement = 0; placement < 2; ++placement)
                    for (int dedup = 0; dedup < 2; ++dedup)
                        for (int normals = 0; normals < 2; ++normals)
                            for (uint32_t grid_n : {1u, 2u, 5u, 17u}) {
                                if (mode == 0 && (placement || grid_n != 1)) continue;
                                pt_simplify_opts o;
                                pt_simplify_opts_default(&o);
                                o.mode = mode; o.placement = placement; o.dedup = dedup; o.normals = normals; o.grid_n = grid_n;
                                o.reg = grid_n == 5 ? 1.0 : (grid_n == 2 ? 1e-6 : 1e-3);
                                if (run(m, &o, (grid_n + dedup) % 2 == 0) != 0) { printf("unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
                                o.cell = 0.37; o.grid_n = 0;
                                if (mode == 1 && grid_n == 17 && run(m, &o, true) != 0) { printf("unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
                            }
        }
    uint32_t faces = 0;
    if (run(meshes[7], nullptr, true, &faces) != 0) return 1;                       // NULL options: the defaults
    pt_simplify_opts weld;
    pt_simplify_opts_default(&weld);
    weld.mode = 0;
    if (run(meshes[7], &weld, true, &faces) != 0 || faces != 12) { printf("the welded cube has %u faces\n", faces); return 1; }
    // refusals: nothing is read past what the arguments admit
    const int before = g_refused;
    pt_simplify_opts o;
    pt_simplify_opts_default(&o);
    const M& c = meshes[0];
    M bad = c;
    bad.idx.pop_back();
    run(bad, &o, true);
    bad.idx.clear();
    run(bad, &o, true);
    bad = c;
    bad.idx[7] = 8;
    run(bad, &o, true);
    bad = c;
    bad.pos[5] = std::numeric_limits<float>::infinity();
    run(bad, &o, true);
    bad.pos[5] = std::numeric_limits<float>::quiet_NaN();
    run(bad, &weld, true);
    bad = c;
    with_uv(bad);
    bad.uv.resize(10);   // five texcoords for eight vertices
    run(bad, &o, true);
    bad = c;
    for (size_t v = 0; v < 8; ++v) { bad.pos[3 * v] = 1.0f; bad.pos[3 * v + 1] = 2.0f; bad.pos[3 * v + 2] = 3.0f; }
    run(bad, &o, true);   // E == 0
    o.mode = 2; run(c, &o, true); o.mode = 1;
    o.placement = -1; run(c, &o, true); o.placement = 0;
    o.dedup = 2; run(c, &o, true); o.dedup = 1;
    o.normals = 2; run(c, &o, true); o.normals = 0;
    o.cell = -1.0; run(c, &o, true);
    o.cell = std::numeric_limits<double>::infinity(); run(c, &o, true);
    o.cell = 1e-7; run(c, &o, true);   // more than 2^21 cells along an axis
    o.cell = 0.0; o.grid_n = 0; run(c, &o, true); o.grid_n = 64;
    o.reg = 1e-7; run(c, &o, true);
    o.reg = 2.0; run(c, &o, true);
    o.reg = std::numeric_limits<double>::quiet_NaN(); run(c, &o, true);
    if (g_refused - before != 18) { printf("%d of 18 refusals\n", g_refused - before); return 1; }
    float* p = nullptr;
    uint32_t np = 0;
    if (pt_mesh_simplify_host(nullptr, 8, c.pos.data(), 36, c.idx.data(), 0, nullptr, &p, &np, nullptr, nullptr, nullptr, nullptr, nullptr) != -1) return 1;
    printf("simplify_host_check: %d calls, %d refused, checksum %016llx\n", g_calls, g_refused, (unsigned long long)g_sum);
    return 0;
}
