// Isosurface extraction by marching tetrahedra (the rule in include/pt_amd.h): the per-element arithmetic, written once
// for host and device. pt_mesh_isosurface_host runs it from plain C++ loops, the kernels of pt_iso.hip run it one lane per lattice point,
// and the unit is built with -ffp-contract=off on both sides, so the two execute the same sequence of IEEE operations (+ - * / sqrt on
// f64, one rounding to f32 per written attribute) and agree bit for bit. Which vertex gets which index follows from the lattice order
// alone: a point's crossing edges are a 7-bit mask, its first vertex an exclusive sum of the masks' populations.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_tess.h"   // tess_finite, tess_normalise

#if defined(__HIPCC__)
#define PT_ISO_HD __host__ __device__ inline
#else
#define PT_ISO_HD inline
#endif

namespace pt {

// The lattice of a call: the grid's sample centres, with one layer of `outside` around them when closed
struct IsoGrid {
    uint32_t nx, ny, nz;     // the grid
    uint32_t NX, NY, NZ;     // the lattice: n + 2 pad per axis
    uint32_t pad;            // 0 open, 1 closed
    float outside;
    double iso;
    double lo[3], h[3];      // the box's low corner and the spacing (hi - lo) / n per axis
};

PT_ISO_HD size_t iso_points(const IsoGrid& g) { return (size_t)g.NX * g.NY * g.NZ; }

// The sample of lattice point (i, j, k), lattice indices counted from the first layer
PT_ISO_HD float iso_value(const IsoGrid& g, const float* values, uint32_t i, uint32_t j, uint32_t k) {
    if (g.pad && (i == 0 || j == 0 || k == 0 || i == g.NX - 1 || j == g.NY - 1 || k == g.NZ - 1)) return g.outside;
    return values[((size_t)(k - g.pad) * g.ny + (j - g.pad)) * g.nx + (i - g.pad)];
}

PT_ISO_HD bool iso_inside(const IsoGrid& g, float v) { return (double)v >= g.iso; }

// lo + ((double)index + 0.5) * h with the index counted in the grid (-1 for the added layer)
PT_ISO_HD double iso_coord(const IsoGrid& g, int axis, uint32_t i) { return g.lo[axis] + ((double)((int64_t)i - (int64_t)g.pad) + 0.5) * g.h[axis]; }

// The case table of a tetrahedron (v0, v1, v2, v3) with det(v1 - v0, v2 - v0, v3 - v0) > 0. Row: bit l set when corner l is inside.
// A row: the number of triangles; then their vertices as edges of the tetrahedron: 0 = (0,1) 1 = (0,2) 2 = (0,3) 3 = (1,2) 4 = (1,3)
// 5 = (2,3). A tetrahedron of the other orientation swaps the second and third vertex of each triangle.
constexpr uint32_t iso_pack(uint32_t n, uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f) {
    return n | (a << 4) | (b << 7) | (c << 10) | (d << 13) | (e << 16) | (f << 19);
}
PT_ISO_HD uint32_t iso_row(uint32_t m) {
    constexpr uint32_t ROW[16] = {
        iso_pack(0, 0, 0, 0, 0, 0, 0),   // 0000
        iso_pack(1, 0, 1, 2, 0, 0, 0),   // 0001
        iso_pack(1, 0, 4, 3, 0, 0, 0),   // 0010
        iso_pack(2, 1, 2, 4, 1, 4, 3),   // 0011
        iso_pack(1, 1, 3, 5, 0, 0, 0),   // 0100
        iso_pack(2, 0, 5, 2, 0, 3, 5),   // 0101
        iso_pack(2, 0, 4, 5, 0, 5, 1),   // 0110
        iso_pack(1, 2, 4, 5, 0, 0, 0),   // 0111
        iso_pack(1, 2, 5, 4, 0, 0, 0),   // 1000
        iso_pack(2, 0, 1, 5, 0, 5, 4),   // 1001
        iso_pack(2, 0, 5, 3, 0, 2, 5),   // 1010
        iso_pack(1, 1, 5, 3, 0, 0, 0),   // 1011
        iso_pack(2, 1, 3, 4, 1, 4, 2),   // 1100
        iso_pack(1, 0, 3, 4, 0, 0, 0),   // 1101
        iso_pack(1, 0, 2, 1, 0, 0, 0),   // 1110
        iso_pack(0, 0, 0, 0, 0, 0, 0),   // 1111
    };
    return ROW[m];
}
PT_ISO_HD uint32_t iso_row_count(uint32_t row) { return row & 15u; }
PT_ISO_HD uint32_t iso_row_edge(uint32_t row, uint32_t k) { return (row >> (4u + 3u * k)) & 7u; }   // k = 3 * triangle + vertex

// The six tetrahedra of a cube as four cube corners each (4 bits a corner, v0 in the low bits), and which of them are positive
PT_ISO_HD uint32_t iso_tet(int t) {
    constexpr uint32_t TET[6] = {0x7310u, 0x7510u, 0x7320u, 0x7620u, 0x7540u, 0x7640u};
    return TET[t];
}
PT_ISO_HD bool iso_tet_positive(int t) { return (0x19u >> t) & 1u; }   // tetrahedra 0, 3 and 4

// The two corners (local, a < b) of a tetrahedron's edge 0..5
PT_ISO_HD void iso_edge_ends(uint32_t e, uint32_t& a, uint32_t& b) {
    a = e < 3u ? 0u : (e < 5u ? 1u : 2u);
    b = e < 3u ? e + 1u : (e < 5u ? e - 1u : 3u);
}

// The case of tetrahedron t from the cube's inside bits (bit c: corner c = x + 2y + 4z)
PT_ISO_HD uint32_t iso_case(uint32_t in8, int t) {
    const uint32_t T = iso_tet(t);
    return ((in8 >> (T & 15u)) & 1u) | (((in8 >> ((T >> 4) & 15u)) & 1u) << 1) | (((in8 >> ((T >> 8) & 15u)) & 1u) << 2) | (((in8 >> (T >> 12)) & 1u) << 3);
}

// The triangles of a cube: 0..12
PT_ISO_HD uint32_t iso_cube_triangles(uint32_t in8) {
    if (in8 == 0u || in8 == 255u) return 0u;
    uint32_t n = 0;
    for (int t = 0; t < 6; ++t) n += iso_row_count(iso_row(iso_case(in8, t)));
    return n;
}

// The inside bits of the corners of the cube anchored at (i, j, k) that lie in the lattice (the others read 0), and which do: bit c of
// `have`. A point that anchors a whole cube has have = 255.
PT_ISO_HD uint32_t iso_corners(const IsoGrid& g, const float* values, uint32_t i, uint32_t j, uint32_t k, uint32_t& have) {
    uint32_t in8 = 0;
    have = 0;
    for (uint32_t c = 0; c < 8u; ++c) {
        const uint32_t x = i + (c & 1u), y = j + ((c >> 1) & 1u), z = k + (c >> 2);
        if (x >= g.NX || y >= g.NY || z >= g.NZ) continue;
        have |= 1u << c;
        if (iso_inside(g, iso_value(g, values, x, y, z))) in8 |= 1u << c;
    }
    return in8;
}

// The crossing edges that start at a point: bit d - 1 for the edge to the point's corner d = dx + 2dy + 4dz
PT_ISO_HD uint32_t iso_edge_mask(uint32_t in8, uint32_t have) {
    const uint32_t differ = (in8 ^ ((in8 & 1u) ? 255u : 0u)) & have;
    return differ >> 1;
}

PT_ISO_HD uint32_t iso_popcount(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// The gradient at lattice point (i, j, k): per axis (v+ - v-) / (2 h), one-sided over h where a neighbour is not in the lattice
PT_ISO_HD void iso_gradient(const IsoGrid& g, const float* values, uint32_t i, uint32_t j, uint32_t k, double out[3]) {
    const uint32_t at[3] = {i, j, k}, N[3] = {g.NX, g.NY, g.NZ};
    for (int a = 0; a < 3; ++a) {
        uint32_t m[3] = {i, j, k}, p[3] = {i, j, k};
        const bool has_m = at[a] > 0u, has_p = at[a] + 1u < N[a];
        if (has_m) m[a] = at[a] - 1u;
        if (has_p) p[a] = at[a] + 1u;
        const double vm = (double)iso_value(g, values, m[0], m[1], m[2]), vp = (double)iso_value(g, values, p[0], p[1], p[2]);
        out[a] = has_m && has_p ? (vp - vm) / (2.0 * g.h[a]) : (vp - vm) / g.h[a];
    }
}

// The vertices of the crossing edges that start at lattice point (i, j, k) with mask `mask`, written from index `first` on
PT_ISO_HD void iso_emit_vertices(const IsoGrid& g, const float* values, uint32_t i, uint32_t j, uint32_t k, uint32_t mask, size_t first, float* pos, float* nrm) {
    const double a = (double)iso_value(g, values, i, j, k);
    const double PA[3] = {iso_coord(g, 0, i), iso_coord(g, 1, j), iso_coord(g, 2, k)};
    double gA[3] = {0.0, 0.0, 0.0};
    if (nrm) iso_gradient(g, values, i, j, k, gA);
    size_t v = first;
    for (uint32_t d = 1; d < 8u; ++d) {
        if (!((mask >> (d - 1u)) & 1u)) continue;
        const uint32_t x = i + (d & 1u), y = j + ((d >> 1) & 1u), z = k + (d >> 2);
        const double b = (double)iso_value(g, values, x, y, z);
        const double t = (g.iso - a) / (b - a);
        const double PB[3] = {iso_coord(g, 0, x), iso_coord(g, 1, y), iso_coord(g, 2, z)};
        for (int c = 0; c < 3; ++c) pos[3 * v + c] = (float)(PA[c] + (PB[c] - PA[c]) * t);
        if (nrm) {
            double gB[3];
            iso_gradient(g, values, x, y, z, gB);
            const double N[3] = {-(gA[0] + (gB[0] - gA[0]) * t), -(gA[1] + (gB[1] - gA[1]) * t), -(gA[2] + (gB[2] - gA[2]) * t)};
            if (!tess_normalise(N, nrm + 3 * v)) {
                nrm[3 * v] = 0.0f; nrm[3 * v + 1] = 1.0f; nrm[3 * v + 2] = 0.0f;
            }
        }
        ++v;
    }
}

// The triangles of the cube anchored at lattice point p = (k NY + j) NX + i with inside bits in8, written from triangle `first` on.
// mask / vbase: per lattice point, its crossing-edge mask and its first vertex.
PT_ISO_HD void iso_emit_triangles(const IsoGrid& g, size_t p, uint32_t in8, const uint8_t* mask, const uint32_t* vbase, size_t first, uint32_t* idx) {
    const size_t step[3] = {1, g.NX, (size_t)g.NX * g.NY};
    size_t f = first;
    for (int t = 0; t < 6; ++t) {
        const uint32_t row = iso_row(iso_case(in8, t));
        const uint32_t T = iso_tet(t);
        const bool pos_t = iso_tet_positive(t);
        for (uint32_t n = 0; n < iso_row_count(row); ++n) {
            uint32_t v[3];
            for (uint32_t c = 0; c < 3u; ++c) {
                uint32_t la, lb;
                iso_edge_ends(iso_row_edge(row, 3u * n + c), la, lb);
                const uint32_t ca = (T >> (4u * la)) & 15u, cb = (T >> (4u * lb)) & 15u, d = cb - ca;   // ca < cb, ca's bits among cb's
                const size_t A = p + (ca & 1u) * step[0] + ((ca >> 1) & 1u) * step[1] + (ca >> 2) * step[2];
                v[c] = vbase[A] + iso_popcount((uint32_t)mask[A] & ((1u << (d - 1u)) - 1u));
            }
            idx[3 * f] = v[0];
            idx[3 * f + 1] = pos_t ? v[1] : v[2];
            idx[3 * f + 2] = pos_t ? v[2] : v[1];
            ++f;
        }
    }
}

// ---- host side only: what pt_mesh_isosurface and pt_mesh_isosurface_host share (pt_iso_host.cpp) ----
struct IsoPlan {
    IsoGrid grid;
    int normals;   // 0 gradient, 1 smooth, 2 none
};
struct IsoOut {
    float** pos; uint32_t* n_pos;
    uint32_t** idx; uint32_t* n_idx;
    float** nrm;
};
constexpr uint64_t ISO_MAX_TRIANGLES = 0x07FFFFFFull;   // pt_mesh's cap
// Every refusal of the rule that needs no counting, in one place: 0 and a filled plan, or -1 with the error set under `who`. Touches no device.
int iso_check(const char* who, const void* opts /* pt_iso_opts or NULL */, uint32_t nx, uint32_t ny, uint32_t nz, const float* values, const double* box_lo,
              const double* box_hi, const IsoOut& out, IsoPlan& plan);

}  // namespace pt
