// Isosurface extraction, the host side (include/pt_amd.h has the rule): the refusals both entry points share and
// pt_mesh_isosurface_host, the GPU stage's twin: running sums where the device scans, the same pt_iso.h functions per lattice point, the
// same passes in the same order. Plain C++: nothing here touches a device.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_iso.h"

namespace pt {

int set_error(const std::string& msg);   // pt_error.cpp; returns -1

int iso_check(const char* who, const void* opts_, uint32_t nx, uint32_t ny, uint32_t nz, const float* values, const double* box_lo, const double* box_hi,
              const IsoOut& out, IsoPlan& plan) {
    const std::string p = std::string(who) + ": ";
    pt_iso_opts o;
    if (opts_) o = *(const pt_iso_opts*)opts_;
    else pt_iso_opts_default(&o);
    if (!out.pos || !out.n_pos || !out.idx || !out.n_idx || !out.nrm) return set_error(p + "null output pointer");
    *out.pos = nullptr; *out.idx = nullptr; *out.nrm = nullptr;
    *out.n_pos = 0; *out.n_idx = 0;
    if (!values) return set_error(p + "null values");
    if (!box_lo || !box_hi) return set_error(p + "null box");
    if (nx < 2 || ny < 2 || nz < 2) return set_error(p + "the grid needs at least 2 samples along every axis");
    if (o.closed != 0 && o.closed != 1) return set_error(p + "closed must be 0 or 1");
    if (o.normals < 0 || o.normals > 2) return set_error(p + "normals must be 0 (gradient), 1 (smooth) or 2 (none)");
    const uint64_t cells = (uint64_t)nx * ny * nz;   // (three 32-bit factors: test the partial product first)
    if ((uint64_t)nx * ny > (1ull << 28) || cells > (1ull << 28)) return set_error(p + "too many samples: nx ny nz must be at most 2^28");
    const uint64_t pad = o.closed ? 2u : 0u;
    if ((nx + pad) * (ny + pad) * (nz + pad) > (1ull << 29)) return set_error(p + "too many lattice points: at most 2^29 after padding");
    if (!tess_finite(o.iso)) return set_error(p + "iso must be finite");
    if (!tess_finite((double)o.outside)) return set_error(p + "outside must be finite");
    for (int a = 0; a < 3; ++a) {
        if (!tess_finite(box_lo[a]) || !tess_finite(box_hi[a])) return set_error(p + "the box must be finite");
        if (!(box_lo[a] < box_hi[a])) return set_error(p + "the box needs lo < hi along every axis");
    }
    for (uint64_t i = 0; i < cells; ++i)
        if (!tess_finite((double)values[i])) return set_error(p + "every value must be finite");
    IsoGrid& g = plan.grid;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.pad = o.closed ? 1u : 0u;
    g.NX = nx + 2u * g.pad; g.NY = ny + 2u * g.pad; g.NZ = nz + 2u * g.pad;
    g.outside = o.outside;
    g.iso = o.iso;
    const uint32_t n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = box_lo[a];
        g.h[a] = (box_hi[a] - box_lo[a]) / (double)n[a];
    }
    plan.normals = o.normals;
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
}  // namespace pt

using namespace pt;

extern "C" int pt_iso_opts_default(pt_iso_opts* o) {
    if (!o) return set_error("pt_iso_opts_default: null options");
    memset(o, 0, sizeof *o);
    o->iso = 0.5;
    return 0;
}

extern "C" int pt_mesh_isosurface_host(const pt_iso_opts* opts, uint32_t nx, uint32_t ny, uint32_t nz, const float* values, const double box_lo[3], const double box_hi[3],
                                       float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm) {
    const char* who = "pt_mesh_isosurface_host";
    const IsoOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm};
    IsoPlan plan;
    if (iso_check(who, opts, nx, ny, nz, values, box_lo, box_hi, out, plan) != 0) return -1;
    const IsoGrid& g = plan.grid;
    const size_t points = iso_points(g);

    // pass 1: per lattice point, the mask of its crossing edges and the triangles of its cube; the running sums are the device's scans
    std::vector<uint8_t> mask(points + 1, 0);
    std::vector<uint32_t> vbase(points + 1, 0), tbase(points + 1, 0);
    uint64_t n = 0, F = 0;
    {
        size_t p = 0;
        for (uint32_t k = 0; k < g.NZ; ++k)
            for (uint32_t j = 0; j < g.NY; ++j)
                for (uint32_t i = 0; i < g.NX; ++i, ++p) {
                    uint32_t have;
                    const uint32_t in8 = iso_corners(g, values, i, j, k, have);
                    mask[p] = (uint8_t)iso_edge_mask(in8, have);
                    vbase[p] = (uint32_t)n;
                    tbase[p] = (uint32_t)F;   // (wraps past 2^32 only where the count is refused below)
                    n += iso_popcount(mask[p]);
                    if (have == 255u) F += iso_cube_triangles(in8);
                }
    }
    if (F > ISO_MAX_TRIANGLES) return set_error(std::string(who) + ": too many triangles: the surface has more than 0x07FFFFFF");

    // passes 2 and 3: the vertices of every point, the triangles of every cube
    const bool gradient = plan.normals == 0;
    std::vector<float> P(3 * n + 1, 0.0f), N(plan.normals != 2 ? 3 * n + 1 : 0, 0.0f);
    std::vector<uint32_t> I(3 * F + 1, 0);
    {
        size_t p = 0;
        for (uint32_t k = 0; k < g.NZ; ++k)
            for (uint32_t j = 0; j < g.NY; ++j)
                for (uint32_t i = 0; i < g.NX; ++i, ++p) {
                    if (mask[p]) iso_emit_vertices(g, values, i, j, k, mask[p], vbase[p], P.data(), gradient ? N.data() : nullptr);
                    if (i + 1 < g.NX && j + 1 < g.NY && k + 1 < g.NZ && tbase[p + 1] != tbase[p]) {
                        uint32_t have;
                        const uint32_t in8 = iso_corners(g, values, i, j, k, have);
                        iso_emit_triangles(g, p, in8, mask.data(), vbase.data(), tbase[p], I.data());
                    }
                }
    }
    if (plan.normals == 1) {   // section 27's smooth normals of the finished mesh
        const size_t M = 3 * F;
        std::vector<std::pair<uint32_t, uint32_t>> vc(M);
        for (size_t c = 0; c < M; ++c) vc[c] = {I[c], (uint32_t)c};
        std::sort(vc.begin(), vc.end());
        std::vector<uint32_t> corners(M + 1);
        for (size_t i = 0; i < M; ++i) corners[i] = vc[i].second;
        size_t i = 0;
        for (size_t v = 0; v < n; ++v) {
            const size_t first = i;
            while (i < M && vc[i].first == v) ++i;
            tess_smooth_normal(P.data(), I.data(), corners.data() + first, i - first, nullptr, &N[3 * v]);
        }
    }
    float* rP = dup(P.data(), 3 * n);
    uint32_t* rI = dup(I.data(), 3 * F);
    float* rN = plan.normals != 2 ? dup(N.data(), 3 * n) : nullptr;
    if (!rP || !rI || (plan.normals != 2 && !rN)) {
        free(rP); free(rI); free(rN);
        return set_error(std::string(who) + ": out of host memory");
    }
    *out_pos = rP; *out_n_pos = (uint32_t)n;
    *out_idx = rI; *out_n_idx = (uint32_t)(3 * F);
    *out_nrm = rN;
    return 0;
}
