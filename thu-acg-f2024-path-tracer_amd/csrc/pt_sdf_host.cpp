// Mesh voxelisation, the host side (include/pt_amd.h has the rule): the refusals both entry points share, pt_mesh_fit_grid
// and pt_mesh_sdf_host, the GPU stage's twin: plain loops over triangles, columns and samples with the same pt_sdf.h functions. It has
// no brick cull: a sample skips a triangle by the bound of its own point against the triangle's box, and tries the triangle that won
// the sample before it first. The minimum of f64 values does not depend on either, which is what lets this twin prove the device's
// cull. Plain C++: nothing here touches a device.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_sdf.h"

namespace pt {

int set_error(const std::string& msg);   // pt_error.cpp; returns -1

int sdf_check(const char* who, const void* opts_, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t nx, uint32_t ny, uint32_t nz,
              const double* box_lo, const double* box_hi, const float* out_values, SdfGrid& g) {
    const std::string p = std::string(who) + ": ";
    pt_sdf_opts o;
    if (opts_) o = *(const pt_sdf_opts*)opts_;
    else pt_sdf_opts_default(&o);
    if (!out_values) return set_error(p + "null output pointer");
    if (!pos || !idx) return set_error(p + "null mesh");
    if (!box_lo || !box_hi) return set_error(p + "null box");
    if (n_idx == 0 || n_idx % 3u != 0) return set_error(p + "n_idx must be a positive multiple of 3");
    if ((uint64_t)(n_idx / 3u) > SDF_MAX_TRIANGLES) return set_error(p + "too many triangles: at most 0x07FFFFFF");
    if (nx < 2 || ny < 2 || nz < 2) return set_error(p + "the grid needs at least 2 samples along every axis");
    if ((uint64_t)nx * ny > (1ull << 28) || (uint64_t)nx * ny * nz > (1ull << 28)) return set_error(p + "too many samples: nx ny nz must be at most 2^28");
    if (o.what < 0 || o.what > 3) return set_error(p + "what must be 0 (depth), 1 (distance), 2 (occupancy) or 3 (density)");
    if (o.fill != 0 && o.fill != 1) return set_error(p + "fill must be 0 (non-zero) or 1 (odd)");
    if (!tess_finite(o.band) || o.band < 0.0) return set_error(p + "band must be finite and not negative");
    if (o.what == 3 && !(tess_finite(o.ramp) && o.ramp > 0.0)) return set_error(p + "density needs a finite ramp > 0");
    for (int a = 0; a < 3; ++a) {
        if (!tess_finite(box_lo[a]) || !tess_finite(box_hi[a])) return set_error(p + "the box must be finite");
        if (!(box_lo[a] < box_hi[a])) return set_error(p + "the box needs lo < hi along every axis");
    }
    for (uint32_t i = 0; i < n_idx; ++i)
        if (idx[i] >= n_pos) return set_error(p + "index out of range");
    for (size_t i = 0; i < (size_t)n_pos * 3; ++i)
        if (!tess_finite((double)pos[i])) return set_error(p + "every position must be finite");
    if (o.what != 2) {   // the distance pass needs a triangle
        bool any = false;
        double rec[SDF_RECORD_DOUBLES];
        float box[SDF_BOX_FLOATS];
        for (uint32_t t = 0; t < n_idx / 3u && !any; ++t) any = sdf_record(pos, idx[3 * (size_t)t], idx[3 * (size_t)t + 1], idx[3 * (size_t)t + 2], rec, box);
        if (!any) return set_error(p + "no triangle is left after the degenerate ones are dropped");
    }
    g.nx = nx; g.ny = ny; g.nz = nz;
    const uint32_t n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = box_lo[a];
        g.h[a] = (box_hi[a] - box_lo[a]) / (double)n[a];
    }
    g.what = o.what; g.fill = o.fill; g.negate = o.negate ? 1 : 0;
    g.band = o.band; g.ramp = o.ramp;
    return 0;
}

}  // namespace pt

using namespace pt;

extern "C" int pt_sdf_opts_default(pt_sdf_opts* o) {
    if (!o) return set_error("pt_sdf_opts_default: null options");
    memset(o, 0, sizeof *o);
    return 0;
}

extern "C" int pt_mesh_fit_grid(uint32_t n_pos, const float* pos, uint32_t n_longest, double margin_cells, uint32_t out_dims[3], double out_lo[3], double out_hi[3]) {
    const std::string p = "pt_mesh_fit_grid: ";
    if (!pos || !out_dims || !out_lo || !out_hi) return set_error(p + "null pointer");
    if (n_pos == 0) return set_error(p + "no positions");
    if (!tess_finite(margin_cells) || margin_cells < 0.0) return set_error(p + "margin_cells must be finite and not negative");
    if (!((double)n_longest > 2.0 * margin_cells + 1.0)) return set_error(p + "n_longest must exceed 2 margin_cells + 1");
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = (double)pos[a];
    for (size_t i = 0; i < (size_t)n_pos; ++i)
        for (int a = 0; a < 3; ++a) {
            const double v = (double)pos[3 * i + a];
            if (!tess_finite(v)) return set_error(p + "every position must be finite");
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
        }
    double ext[3], E = 0.0;
    for (int a = 0; a < 3; ++a) {
        ext[a] = hi[a] - lo[a];
        if (ext[a] > E) E = ext[a];
    }
    if (!(E > 0.0)) return set_error(p + "the mesh has no extent");
    const double h = E / ((double)n_longest - 2.0 * margin_cells);
    if (!(tess_finite(h) && h > 0.0)) return set_error(p + "the cell size is not a positive finite number");
    double n[3], cells = 1.0;
    for (int a = 0; a < 3; ++a) {
        n[a] = std::ceil(ext[a] / h + 2.0 * margin_cells);
        if (!(n[a] >= 2.0)) n[a] = 2.0;
        cells *= n[a];
    }
    if (!(cells <= 268435456.0)) return set_error(p + "too many samples: nx ny nz must be at most 2^28");
    for (int a = 0; a < 3; ++a) {
        const double c = lo[a] + 0.5 * ext[a], half = 0.5 * (n[a] * h);
        out_dims[a] = (uint32_t)n[a];
        out_lo[a] = c - half;
        out_hi[a] = c + half;
    }
    return 0;
}

extern "C" int pt_mesh_sdf_host(const pt_sdf_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t nx, uint32_t ny, uint32_t nz,
                                const double box_lo[3], const double box_hi[3], float* out_values) {
    SdfGrid g;
    if (sdf_check("pt_mesh_sdf_host", opts, n_pos, pos, n_idx, idx, nx, ny, nz, box_lo, box_hi, out_values, g) != 0) return -1;
    const size_t T = n_idx / 3u, rows = (size_t)ny * nz, samples = rows * nx;

    // the sign: a crossing adds its orientation at delta[row][m]; a sample's winding is the sum of its row's deltas past it
    std::vector<uint8_t> inside;
    if (g.what != 1) {
        std::vector<int32_t> delta(rows * ((size_t)nx + 1), 0);
        for (size_t t = 0; t < T; ++t) {
            double V[3][3];
            for (int c = 0; c < 3; ++c)
                for (int d = 0; d < 3; ++d) V[c][d] = (double)pos[3 * (size_t)idx[3 * t + c] + d];
            uint32_t j0, j1, k0, k1;
            sdf_columns(g, V[0], V[1], V[2], j0, j1, k0, k1);
            for (uint32_t k = k0; k < k1; ++k)
                for (uint32_t j = j0; j < j1; ++j) {
                    int o;
                    uint32_t m;
                    if (sdf_crossing(g, V[0], V[1], V[2], j, k, o, m)) delta[((size_t)k * ny + j) * ((size_t)nx + 1) + m] += o;
                }
        }
        inside.resize(samples);
        for (size_t r = 0; r < rows; ++r) {
            int32_t w = 0;
            for (uint32_t i = nx; i-- > 0;) {
                w += delta[r * ((size_t)nx + 1) + i + 1];
                inside[r * nx + i] = sdf_inside(g.fill, w) ? 1 : 0;
            }
        }
    }
    if (g.what == 2) {
        for (size_t s = 0; s < samples; ++s) out_values[s] = sdf_output(g, 0.0, inside[s] != 0);
        return 0;
    }

    // the distance: the least squared distance over the triangles that are not dropped
    std::vector<double> rec;
    std::vector<float> box;
    rec.reserve(T * SDF_RECORD_DOUBLES);
    box.reserve(T * SDF_BOX_FLOATS);
    for (size_t t = 0; t < T; ++t) {
        double r[SDF_RECORD_DOUBLES];
        float b[SDF_BOX_FLOATS];
        if (!sdf_record(pos, idx[3 * t], idx[3 * t + 1], idx[3 * t + 2], r, b)) continue;
        rec.insert(rec.end(), r, r + SDF_RECORD_DOUBLES);
        box.insert(box.end(), b, b + SDF_BOX_FLOATS);
    }
    const size_t K = box.size() / SDF_BOX_FLOATS;
    const double start = sdf_start(g);
    size_t last = 0;   // the triangle that won the previous sample: tried first
    size_t s = 0;
    for (uint32_t k = 0; k < nz; ++k)
        for (uint32_t j = 0; j < ny; ++j)
            for (uint32_t i = 0; i < nx; ++i, ++s) {
                const bool in = g.what == 1 ? false : inside[s] != 0;
                if (g.what == 3 && !in) {
                    out_values[s] = 0.0f;
                    continue;
                }
                const double P[3] = {sdf_coord(g, 0, i), sdf_coord(g, 1, j), sdf_coord(g, 2, k)};
                double best = start;
                {
                    const double d = sdf_dist2(&rec[last * SDF_RECORD_DOUBLES], P);
                    if (d < best) best = d;
                }
                for (size_t t = 0; t < K; ++t) {
                    if (sdf_cull_far(sdf_box_gap2(P, P, &box[t * SDF_BOX_FLOATS]), best)) continue;
                    const double d = sdf_dist2(&rec[t * SDF_RECORD_DOUBLES], P);
                    if (d < best) {
                        best = d;
                        last = t;
                    }
                }
                out_values[s] = sdf_output(g, best, in);
            }
    return 0;
}
