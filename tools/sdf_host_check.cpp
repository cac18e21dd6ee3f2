// The host twin of mesh voxelisation (csrc/pt_sdf_host.cpp) as a stand-alone program, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sdf_host_check.cpp thu-acg-f2024-path-tracer_amd/csrc/pt_sdf_host.cpp -o sdf_host_check && ./sdf_host_check
// It walks a cube, an octahedron, two overlapping cubes and a mesh with degenerate triangles through every mode, both fill rules, a band,
// boxes around, beside, inside and across the mesh and ragged grids, then pt_mesh_fit_grid and the refusals, and prints a checksum. The
// arrays are exactly as large as the call says, so a read or write past them is one past the allocation. No GPU, no Python: the
// sanitizers see every load and store of the twin.
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

struct M {
    std::vector<float> pos;
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

static M merged(const M& a, const M& b) {
    M m = a;
    m.pos.insert(m.pos.end(), b.pos.begin(), b.pos.end());
    for (uint32_t i : b.idx) m.idx.push_back(i + (uint32_t)(a.pos.size() / 3));
    return m;
}

static int run(const M& m, const pt_sdf_opts* o, uint32_t nx, uint32_t ny, uint32_t nz, const double lo[3], const double hi[3]) {
    const uint64_t cells = (uint64_t)nx * ny * nz;
    std::vector<float> out(cells <= (1u << 22) ? (size_t)cells : 1, 0.0f);
    const int rc = pt_mesh_sdf_host(o, (uint32_t)(m.pos.size() / 3), m.pos.data(), (uint32_t)m.idx.size(), m.idx.data(), nx, ny, nz, lo, hi, out.data());
    ++g_calls;
    if (rc != 0) { ++g_refused; return rc; }
    for (float v : out) {
        uint32_t bits;
        memcpy(&bits, &v, 4);
        g_sum = g_sum * 1099511628211ull + bits;
    }
    return 0;
}

int main() {
    const double LO[3] = {-1.0, 0.5, 2.0}, HI[3] = {3.5, 4.5, 5.5};
    M junk = octahedron(1.2f, 2.4f, 3.7f, 0.9f);
    for (uint32_t i : {0u, 0u, 1u, 2u, 3u, 3u, 5u, 5u, 5u}) junk.idx.push_back(i);   // repeated indices
    const M meshes[] = {cube(0.1f, 1.2f, 2.6f, 2.3f, 3.9f, 4.8f), octahedron(1.2f, 2.4f, 3.7f, 0.9f), merged(cube(0, 1, 2.5f, 2, 3, 4.5f), cube(1, 2, 3, 3, 4, 5)), junk,
                        cube(-50, -50, -50, 50, 50, 50), cube(10, 10, 10, 11, 11, 11)};
    const uint32_t dims[][3] = {{2, 2, 2}, {4, 4, 4}, {5, 3, 7}, {9, 6, 11}, {65, 4, 4}, {4, 4, 130}};
    for (const M& m : meshes)
        for (auto& d : dims)
            for (int what = 0; what < 4; ++what)
                for (int fill = 0; fill < 2; ++fill)
                    for (double band : {0.0, 0.3}) {
                        pt_sdf_opts o;
                        pt_sdf_opts_default(&o);
                        o.what = what; o.fill = fill; o.band = band; o.ramp = 0.25; o.negate = fill;
                        if (run(m, &o, d[0], d[1], d[2], LO, HI) != 0) { printf("unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
                    }
    if (run(meshes[0], nullptr, 6, 5, 4, LO, HI) != 0) return 1;
    // pt_mesh_fit_grid, and a call on what it returns
    uint32_t n[3];
    double lo[3], hi[3];
    if (pt_mesh_fit_grid((uint32_t)(meshes[1].pos.size() / 3), meshes[1].pos.data(), 12, 2.0, n, lo, hi) != 0 || run(meshes[1], nullptr, n[0], n[1], n[2], lo, hi) != 0) return 1;
    if (pt_mesh_fit_grid(6, meshes[1].pos.data(), 5, 2.0, n, lo, hi) != -1 || pt_mesh_fit_grid(1, meshes[1].pos.data(), 12, 2.0, n, lo, hi) != -1 ||
        pt_mesh_fit_grid(6, nullptr, 12, 2.0, n, lo, hi) != -1)
        return 1;
    // refusals: nothing is read past what the arguments admit
    const int before = g_refused;
    pt_sdf_opts o;
    pt_sdf_opts_default(&o);
    const M& c = meshes[0];
    run(c, &o, 1, 4, 4, LO, HI);
    run(c, &o, 1u << 16, 1u << 16, 1u << 16, LO, HI);
    run(c, &o, 4, 4, 4, HI, LO);
    M bad = c;
    bad.idx[7] = 8;
    run(bad, &o, 4, 4, 4, LO, HI);
    bad = c;
    bad.pos[5] = std::numeric_limits<float>::infinity();
    run(bad, &o, 4, 4, 4, LO, HI);
    bad = c;
    bad.idx.pop_back();
    run(bad, &o, 4, 4, 4, LO, HI);
    o.what = 3;
    run(c, &o, 4, 4, 4, LO, HI);   // no ramp
    o.what = 4;
    run(c, &o, 4, 4, 4, LO, HI);
    o.what = 0; o.band = -1.0;
    run(c, &o, 4, 4, 4, LO, HI);
    M flat = c;
    flat.idx = {0, 0, 1, 2, 2, 2};
    o.band = 0.0;
    run(flat, &o, 4, 4, 4, LO, HI);
    if (g_refused - before != 10) { printf("%d of 10 refusals\n", g_refused - before); return 1; }
    printf("sdf_host_check: %d calls, %d refused, checksum %016llx\n", g_calls, g_refused, (unsigned long long)g_sum);
    return 0;
}
