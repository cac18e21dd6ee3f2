// Isosurface extraction by marching tetrahedra on the GPU (include/pt_amd.h has the rule, pt_iso.h its arithmetic,
// pt_iso_host.cpp the host twin this stage matches byte for byte). One upload of the samples, four kernels and two scans on the
// context's stream, one download; between them only the two totals come back, to size the mesh.
//   k_iso_count     : one lane per lattice point, in tiles of 32 x 4 x 2 staged in LDS: the 7-bit mask of the crossing edges that start
//                     there, their number, and the number of triangles (0..12) of the cube anchored there; the block's triangles go into
//                     a 64-bit total with one integer atomic
//   hipcub exclusive sums of the two counts (in place): each point's first vertex, each cube's first triangle
//   k_iso_vertices  : one lane per lattice point writes the vertices (and gradient normals) of its crossing edges
//   k_iso_triangles : one lane per cube writes its triangles; a vertex's index is vbase[A] + popcount(mask[A] & lower kinds)
// In the emit kernels lanes run along i, so a wave reads 64 consecutive entries of a row. No sort, no floating-point atomic; every
// address is formed in size_t and a point's index fits 32 bits (at most 2^29 points).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/pt_amd.h"
#include "pt_scene_gpu.h"
#include "pt_iso.h"
#define PT_MESH_STAGE "isosurface"
#include "pt_tess_dev.h"

using namespace pt;

namespace pt {
namespace {

__device__ inline void iso_decode(const IsoGrid& g, size_t p, uint32_t& i, uint32_t& j, uint32_t& k) {
    const uint32_t q = (uint32_t)p / g.NX;   // p < 2^29
    i = (uint32_t)p - q * g.NX;
    k = q / g.NY;
    j = q - k * g.NY;
}

// A block takes tiles of 32 x 4 x 2 lattice points, one lane a point, and stages the 33 x 5 x 3 samples its cubes read in LDS first:
// a lane then forms its eight inside bits from LDS instead of through eight guarded global reads (DESIGN.md section 29 has the
// measurement: twice the direct form's rate). Tiles are numbered x fastest; a block strides over them.
constexpr uint32_t TX = 32, TY = 4, TZ = 2;                       // TX * TY * TZ == TB
constexpr uint32_t SX = TX + 1, SY = TY + 1, SZ = TZ + 1;
constexpr uint32_t COUNT_BLOCKS = 2048;                           // 8 blocks a CU; larger lattices are walked by stride
static_assert(TX * TY * TZ == TB, "one lane per lattice point of a tile");

__global__ __launch_bounds__(TB) void k_iso_count(const IsoGrid g, const float* __restrict__ values, uint32_t tiles_x, uint32_t tiles_y, uint32_t tiles,
                                                  uint8_t* __restrict__ mask, uint32_t* __restrict__ vcount, uint32_t* __restrict__ tcount,
                                                  unsigned long long* __restrict__ total) {
    __shared__ float tile[SZ][SY][SX];
    __shared__ uint8_t live[SZ][SY][SX];   // 1: the sample is a lattice point
    const uint32_t x = threadIdx.x % TX, y = (threadIdx.x / TX) % TY, z = threadIdx.x / (TX * TY);
    uint32_t tris = 0;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // (the same trip count for every lane of the block)
        const uint32_t tq = t / tiles_x;
        const uint32_t i0 = (t - tq * tiles_x) * TX, j0 = (tq % tiles_y) * TY, k0 = (tq / tiles_y) * TZ;
        for (uint32_t s = threadIdx.x; s < SX * SY * SZ; s += TB) {
            const uint32_t sx = s % SX, sy = (s / SX) % SY, sz = s / (SX * SY);
            const bool in = i0 + sx < g.NX && j0 + sy < g.NY && k0 + sz < g.NZ;
            tile[sz][sy][sx] = in ? iso_value(g, values, i0 + sx, j0 + sy, k0 + sz) : 0.0f;
            live[sz][sy][sx] = in ? 1 : 0;
        }
        __syncthreads();
        const uint32_t i = i0 + x, j = j0 + y, k = k0 + z;
        if (i < g.NX && j < g.NY && k < g.NZ) {
            uint32_t in8 = 0, have = 0;   // iso_corners, read from the tile
            for (uint32_t c = 0; c < 8u; ++c) {
                const uint32_t cx = x + (c & 1u), cy = y + ((c >> 1) & 1u), cz = z + (c >> 2);
                if (!live[cz][cy][cx]) continue;
                have |= 1u << c;
                if (iso_inside(g, tile[cz][cy][cx])) in8 |= 1u << c;
            }
            const uint32_t m = iso_edge_mask(in8, have);
            const uint32_t n = have == 255u ? iso_cube_triangles(in8) : 0u;
            const size_t p = ((size_t)k * g.NY + j) * g.NX + i;
            mask[p] = (uint8_t)m;
            vcount[p] = iso_popcount(m);
            tcount[p] = n;
            tris += n;   // (at most 12 a tile and 2^19 tiles a block: no overflow)
        }
        __syncthreads();   // the tile is read to the end before the next one is staged
    }
    // (every lane of the block reaches the reduction: nothing above returns)
    using Reduce = hipcub::BlockReduce<uint32_t, TB>;
    __shared__ typename Reduce::TempStorage tmp;
    const uint32_t sum = Reduce(tmp).Sum(tris);
    if (threadIdx.x == 0 && sum) atomicAdd(total, (unsigned long long)sum);
}

__global__ __launch_bounds__(TB) void k_iso_vertices(const IsoGrid g, const float* __restrict__ values, uint32_t points, const uint8_t* __restrict__ mask,
                                                     const uint32_t* __restrict__ vbase, float* __restrict__ pos, float* __restrict__ nrm) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= points) return;
    const uint32_t m = mask[p];
    if (!m) return;
    uint32_t i, j, k;
    iso_decode(g, p, i, j, k);
    iso_emit_vertices(g, values, i, j, k, m, vbase[p], pos, nrm);
}

__global__ __launch_bounds__(TB) void k_iso_triangles(const IsoGrid g, const float* __restrict__ values, uint32_t points, const uint8_t* __restrict__ mask,
                                                      const uint32_t* __restrict__ vbase, const uint32_t* __restrict__ tbase, uint32_t* __restrict__ idx) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= points) return;
    const uint32_t first = tbase[p];
    if (tbase[p + 1] == first) return;   // (tbase has points + 1 entries) no triangle: also every point that anchors no cube
    uint32_t i, j, k, have;
    iso_decode(g, p, i, j, k);
    const uint32_t in8 = iso_corners(g, values, i, j, k, have);
    iso_emit_triangles(g, p, in8, mask, vbase, first, idx);
}

bool scan_in_place(hipStream_t st, uint32_t* v, size_t count, DevMem& tmp) {
    size_t bytes = 0;
    return hip_ok(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, v, v, (int)count, st), "hipcub scan (isosurface)") && get(tmp, bytes) &&
           hip_ok(hipcub::DeviceScan::ExclusiveSum(tmp.as<void>(), bytes, v, v, (int)count, st), "hipcub scan (isosurface)");
}

}  // namespace
}  // namespace pt

extern "C" int pt_mesh_isosurface(pt_ctx* ctx, const pt_iso_opts* opts, uint32_t nx, uint32_t ny, uint32_t nz, const float* values, const double box_lo[3],
                                  const double box_hi[3], float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm) {
    const char* who = "pt_mesh_isosurface";
    if (!ctx) return set_error("pt_mesh_isosurface: null context");
    const IsoOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm};
    IsoPlan plan;
    if (iso_check(who, opts, nx, ny, nz, values, box_lo, box_hi, out, plan) != 0) return -1;
    const IsoGrid& g = plan.grid;
    const size_t points = iso_points(g), cells = (size_t)nx * ny * nz;   // points <= 2^29
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = ctx->stream;

    // the upload and the counting pass. The two count arrays have one entry more than there are points, 0, so that the exclusive sums
    // end in the totals
    DevMem vals, mask, vbase, tbase, total, tmp0, tmp1;
    if (!get(vals, cells * 4) || !get(mask, points) || !get(vbase, (points + 1) * 4) || !get(tbase, (points + 1) * 4) || !get(total, 8)) return -1;
    bool ok = hip_ok(hipMemcpyAsync(vals.as<void>(), values, cells * 4, hipMemcpyHostToDevice, st), "hipMemcpy(isosurface upload)") &&
              hip_ok(hipMemsetAsync(vbase.as<uint32_t>() + points, 0, 4, st), "hipMemset(isosurface)") &&
              hip_ok(hipMemsetAsync(tbase.as<uint32_t>() + points, 0, 4, st), "hipMemset(isosurface)") &&
              hip_ok(hipMemsetAsync(total.as<void>(), 0, 8, st), "hipMemset(isosurface)");
    if (!ok) {
        (void)hipStreamSynchronize(st);   // (the caller's array is pageable: nothing may still read it)
        return -1;
    }
    const uint32_t tiles_x = (g.NX + TX - 1) / TX, tiles_y = (g.NY + TY - 1) / TY, tiles_z = (g.NZ + TZ - 1) / TZ;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y * tiles_z;   // every tile holds a lattice point: at most 2^29 of them
    hipLaunchKernelGGL(k_iso_count, dim3((unsigned)std::min<uint64_t>(tiles, COUNT_BLOCKS)), dim3(TB), 0, st, g, vals.as<float>(), tiles_x, tiles_y, (uint32_t)tiles,
                       mask.as<uint8_t>(), vbase.as<uint32_t>(), tbase.as<uint32_t>(), total.as<unsigned long long>());
    ok = launched() && scan_in_place(st, vbase.as<uint32_t>(), points + 1, tmp0) && scan_in_place(st, tbase.as<uint32_t>(), points + 1, tmp1);
    uint32_t n32 = 0;
    unsigned long long F64 = 0;
    ok = ok && hip_ok(hipMemcpyAsync(&n32, vbase.as<uint32_t>() + points, 4, hipMemcpyDeviceToHost, st), "hipMemcpy(isosurface counts)") &&
         hip_ok(hipMemcpyAsync(&F64, total.as<void>(), 8, hipMemcpyDeviceToHost, st), "hipMemcpy(isosurface counts)");
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(isosurface counts)") || !ok) return -1;
    // (the 32-bit sum of the triangle counts can wrap; the 64-bit total cannot, and a total within the cap means no sum wrapped)
    if (F64 > ISO_MAX_TRIANGLES) return set_error(std::string(who) + ": too many triangles: the surface has more than 0x07FFFFFF");
    const size_t n = n32, F = (size_t)F64;

    // the mesh
    DevMesh m;
    m.n = n;
    m.F = F;
    DevMem nrm;
    const bool gradient = plan.normals == 0;
    if (!get(m.pos, n * 12) || !get(m.idx, F * 12) || (gradient && !get(nrm, n * 12))) return -1;
    if (n) {
        hipLaunchKernelGGL(k_iso_vertices, grid_for(points), dim3(TB), 0, st, g, vals.as<float>(), (uint32_t)points, mask.as<uint8_t>(), vbase.as<uint32_t>(), m.pos.as<float>(),
                           gradient ? nrm.as<float>() : nullptr);
        if (!launched()) return -1;
    }
    if (F) {
        hipLaunchKernelGGL(k_iso_triangles, grid_for(points), dim3(TB), 0, st, g, vals.as<float>(), (uint32_t)points, mask.as<uint8_t>(), vbase.as<uint32_t>(),
                           tbase.as<uint32_t>(), m.idx.as<uint32_t>());
        if (!launched()) return -1;
    }
    if (plan.normals == 1 && !smooth(st, m, nullptr, nrm)) return -1;

    // the download, straight into the arrays the caller gets (malloc'd: pt_free)
    struct HostOut {
        void* p = nullptr;
        ~HostOut() { free(p); }
        bool get(size_t bytes) { return (p = malloc(bytes + 8)) != nullptr; }
        void* give() { void* q = p; p = nullptr; return q; }
    } P, I, N;
    const bool has_nrm = plan.normals != 2;
    if (!P.get(n * 12) || !I.get(F * 12) || (has_nrm && !N.get(n * 12))) {
        (void)hipStreamSynchronize(st);   // (the device buffers go out of scope: the kernels that write them must be done first)
        return set_error(std::string(who) + ": out of host memory");
    }
    auto down = [&](void* h, const void* d, size_t bytes) { return bytes == 0 || hip_ok(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st), "hipMemcpy(isosurface download)"); };
    ok = down(P.p, m.pos.as<void>(), n * 12) && down(I.p, m.idx.as<void>(), F * 12) && (!has_nrm || down(N.p, nrm.as<void>(), n * 12));
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(isosurface download)") || !ok) return -1;
    *out_pos = (float*)P.give(); *out_n_pos = (uint32_t)n;
    *out_idx = (uint32_t*)I.give(); *out_n_idx = (uint32_t)(3 * F);
    *out_nrm = (float*)N.give();
    return 0;
}
