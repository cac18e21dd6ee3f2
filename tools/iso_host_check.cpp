// The host twin of isosurface extraction (csrc/pt_iso_host.cpp) as a stand-alone program, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/iso_host_check.cpp thu-acg-f2024-path-tracer_amd/csrc/pt_iso_host.cpp -o iso_host_check && ./iso_host_check
// It walks the shapes of tests/test_iso_cpu.py (all 256 corner patterns, a capped and a whole sphere, a torus, ties, noise, empty grids)
// through open and closed lattices and every normals mode, then the refusals, frees what comes back and prints a checksum. The value
// arrays are exactly as large as the grid says, so a read past the grid is a read past the allocation. No GPU, no Python: the
// sanitizers see every load and store of the twin.
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

struct Grid {
    uint32_t nx, ny, nz;
    std::vector<float> v;
};

static const double LO[3] = {-1.0, 0.5, 2.0}, HI[3] = {3.5, 4.5, 5.5};
static uint64_t g_sum = 0;
static int g_calls = 0, g_refused = 0;

static void mix(const void* p, size_t bytes) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) g_sum = (g_sum ^ b[i]) * 1099511628211ull;
}

static int call(const pt_iso_opts* o, uint32_t nx, uint32_t ny, uint32_t nz, const float* v, const double* lo, const double* hi, bool closed_mesh = false) {
    float *pos = nullptr, *nrm = nullptr;
    uint32_t *idx = nullptr, np = 0, ni = 0;
    const int rc = pt_mesh_isosurface_host(o, nx, ny, nz, v, lo, hi, &pos, &np, &idx, &ni, &nrm);
    ++g_calls;
    if (rc != 0) {
        ++g_refused;
        if (pos || idx || nrm || np || ni) { std::fprintf(stderr, "a refused call left an output behind\n"); std::exit(1); }
        return rc;
    }
    if (!pos || !idx || (nrm == nullptr) != (o && o->normals == 2)) { std::fprintf(stderr, "an output is missing\n"); std::exit(1); }
    mix(pos, (size_t)np * 12);
    mix(idx, (size_t)ni * 4);
    if (nrm) mix(nrm, (size_t)np * 12);
    std::vector<uint32_t> used(np, 0);
    for (uint32_t i = 0; i < ni; ++i) {
        if (idx[i] >= np) { std::fprintf(stderr, "index out of range in the output\n"); std::exit(1); }
        ++used[idx[i]];
    }
    for (uint32_t i = 0; i < np; ++i)
        if (!used[i]) { std::fprintf(stderr, "a vertex no triangle uses\n"); std::exit(1); }
    if (closed_mesh && 2 * (uint64_t)np != (uint64_t)(ni / 3) + 4) {   // V - E + F = 2 with E = 3F / 2
        std::fprintf(stderr, "a closed surface of genus 0 with %u vertices and %u triangles\n", np, ni / 3);
        std::exit(1);
    }
    free(pos); free(idx); free(nrm);
    return 0;
}

static int run(const Grid& g, const pt_iso_opts& o, bool closed_mesh = false) { return call(&o, g.nx, g.ny, g.nz, g.v.data(), LO, HI, closed_mesh); }

template <class F>
static Grid sample(uint32_t nx, uint32_t ny, uint32_t nz, F f) {
    Grid g{nx, ny, nz, {}};
    g.v.reserve((size_t)nx * ny * nz);
    for (uint32_t k = 0; k < nz; ++k)
        for (uint32_t j = 0; j < ny; ++j)
            for (uint32_t i = 0; i < nx; ++i)
                g.v.push_back((float)f(LO[0] + (i + 0.5) * (HI[0] - LO[0]) / nx, LO[1] + (j + 0.5) * (HI[1] - LO[1]) / ny, LO[2] + (k + 0.5) * (HI[2] - LO[2]) / nz, i, j, k));
    return g;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    pt_iso_opts o;
    // all 256 corner patterns, open and closed, every normals mode
    for (int bits = 0; bits < 256; ++bits) {
        const Grid g = sample(2, 2, 2, [&](double, double, double, uint32_t i, uint32_t j, uint32_t k) { return (bits >> (i + 2 * j + 4 * k)) & 1 ? 1.25 : -0.75; });
        for (int closed = 0; closed < 2; ++closed)
            for (int normals = 0; normals < 3; ++normals) {
                pt_iso_opts_default(&o);
                o.iso = 0.25; o.closed = closed; o.outside = -0.75f; o.normals = normals;
                if (run(g, o) != 0) { std::fprintf(stderr, "unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
            }
    }
    // the spheres (the small one larger than its grid and capped, the large one whole), a torus, ties, noise about a negative level
    auto ball = [](double cx, double cy, double cz, double r) {
        return [=](double x, double y, double z, uint32_t, uint32_t, uint32_t) { return r - std::sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz)); };
    };
    const Grid capped = sample(9, 8, 7, ball(3.5, 0.3, 5.5, 3.5)), whole = sample(24, 22, 20, ball(1.3, 2.55, 3.8, 1.27));
    const Grid torus = sample(22, 12, 20, [](double x, double y, double z, uint32_t, uint32_t, uint32_t) {
        const double q = std::sqrt((x - 1.25) * (x - 1.25) + (z - 3.75) * (z - 3.75)) - 1.2;
        return 0.45 - std::sqrt(q * q + (y - 2.5) * (y - 2.5));
    });
    const Grid ties = sample(6, 5, 4, [](double, double, double, uint32_t i, uint32_t j, uint32_t k) { return (double)((i + 2 * j + 3 * k) % 3); });
    const Grid noise = sample(7, 6, 5, [](double, double, double, uint32_t i, uint32_t j, uint32_t k) { return -5.0 + 4.0 * std::fabs(std::sin(12.9898 * i + 78.233 * j + 37.719 * k)); });
    const Grid ones = sample(5, 4, 3, [](double, double, double, uint32_t, uint32_t, uint32_t) { return 1.0; });
    for (int normals = 0; normals < 3; ++normals) {
        pt_iso_opts_default(&o);
        o.iso = 0.0; o.closed = 1; o.outside = -1.0f; o.normals = normals;
        if (run(capped, o, true) != 0 || run(whole, o, true) != 0 || run(torus, o) != 0) { std::fprintf(stderr, "unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
        o.closed = 0;
        if (run(capped, o) != 0 || run(whole, o, true) != 0 || run(torus, o) != 0) { std::fprintf(stderr, "unexpected refusal: %s\n", pt::g_err.c_str()); return 1; }
        o.iso = 1.0;
        if (run(ties, o) != 0) return 1;
        o.closed = 1; o.outside = 1.0f;
        if (run(ties, o) != 0) return 1;
        o.iso = -2.75; o.outside = -7.0f;
        if (run(noise, o) != 0) return 1;
        o.outside = 0.0f;   // above the level: the added layer is inside
        if (run(noise, o) != 0) return 1;
        for (double iso : {0.5, 1.0, 1.5}) {   // all inside, all inside by a tie, all outside: open, nothing; closed, the box or nothing
            o.iso = iso; o.closed = 0;
            if (run(ones, o) != 0) return 1;
            o.closed = 1; o.outside = 0.0f;
            if (run(ones, o, iso < 1.5) != 0) return 1;
        }
    }
    if (call(nullptr, capped.nx, capped.ny, capped.nz, capped.v.data(), LO, HI) != 0) return 1;   // NULL options: the defaults

    // the refusals: nothing is read past what the counts allow, nothing is left allocated
    const int before = g_refused;
    pt_iso_opts_default(&o);
    const Grid& g = noise;
    {
        float* pos = nullptr; float* nrm = nullptr; uint32_t* idx = nullptr; uint32_t np = 0, ni = 0;
        int bad = 0;
        bad += pt_mesh_isosurface_host(&o, g.nx, g.ny, g.nz, g.v.data(), LO, HI, nullptr, &np, &idx, &ni, &nrm) != -1;
        bad += pt_mesh_isosurface_host(&o, g.nx, g.ny, g.nz, g.v.data(), LO, HI, &pos, nullptr, &idx, &ni, &nrm) != -1;
        bad += pt_mesh_isosurface_host(&o, g.nx, g.ny, g.nz, g.v.data(), LO, HI, &pos, &np, nullptr, &ni, &nrm) != -1;
        bad += pt_mesh_isosurface_host(&o, g.nx, g.ny, g.nz, g.v.data(), LO, HI, &pos, &np, &idx, nullptr, &nrm) != -1;
        bad += pt_mesh_isosurface_host(&o, g.nx, g.ny, g.nz, g.v.data(), LO, HI, &pos, &np, &idx, &ni, nullptr) != -1;
        if (bad || pos || idx || nrm) { std::fprintf(stderr, "a NULL output pointer was accepted\n"); return 1; }
        if (pt_iso_opts_default(nullptr) != -1) return 1;
    }
    call(&o, g.nx, g.ny, g.nz, nullptr, LO, HI);
    call(&o, g.nx, g.ny, g.nz, g.v.data(), nullptr, HI);
    call(&o, g.nx, g.ny, g.nz, g.v.data(), LO, nullptr);
    call(&o, 1, g.ny, g.nz, g.v.data(), LO, HI);
    call(&o, g.nx, 1, g.nz, g.v.data(), LO, HI);
    call(&o, g.nx, g.ny, 0, g.v.data(), LO, HI);
    call(&o, 1u << 14, 1u << 14, 2, g.v.data(), LO, HI);                 // sizes are refused before a value is read
    call(&o, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, g.v.data(), LO, HI);
    call(&o, (1u << 28) + 1u, 2, 2, g.v.data(), LO, HI);
    o.closed = 1;
    call(&o, 1u << 26, 2, 2, g.v.data(), LO, HI);                        // 2^28 samples, but (2^26 + 2) * 16 lattice points
    pt_iso_opts_default(&o);
    for (float bad : {nan, inf, -inf}) {
        Grid b = g;
        b.v.back() = bad;
        run(b, o);
        pt_iso_opts q = o;
        q.iso = bad;
        run(g, q);
        q = o;
        q.outside = bad;
        run(g, q);
        for (int a = 0; a < 3; ++a) {
            double lo[3] = {LO[0], LO[1], LO[2]}, hi[3] = {HI[0], HI[1], HI[2]};
            lo[a] = bad;
            call(&o, g.nx, g.ny, g.nz, g.v.data(), lo, HI);
            hi[a] = bad;
            call(&o, g.nx, g.ny, g.nz, g.v.data(), LO, hi);
        }
    }
    for (int a = 0; a < 3; ++a) {
        double hi[3] = {HI[0], HI[1], HI[2]};
        hi[a] = LO[a];
        call(&o, g.nx, g.ny, g.nz, g.v.data(), LO, hi);
        hi[a] = LO[a] - 1.0;
        call(&o, g.nx, g.ny, g.nz, g.v.data(), LO, hi);
    }
    for (int v : {-1, 2}) { pt_iso_opts q = o; q.closed = v; run(g, q); }
    for (int v : {-1, 3}) { pt_iso_opts q = o; q.normals = v; run(g, q); }
    const int expected = 10 + 3 * 9 + 6 + 4;
    if (g_refused - before != expected) { std::fprintf(stderr, "%d of %d bad calls were refused\n", g_refused - before, expected); return 1; }
    std::printf("iso_host_check: %d calls (%d refused as they should be), checksum %016llx\n", g_calls, g_refused, (unsigned long long)g_sum);
    return 0;
}
