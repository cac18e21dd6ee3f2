// Mesh voxelisation on the GPU: signed distance, occupancy and density grids of a triangle mesh (include/pt_amd.h has the
// rule, pt_sdf.h its arithmetic, pt_sdf_host.cpp the host twin this stage matches byte for byte). One upload of the mesh, four kernels on
// the context's stream, one download of the grid.
//   k_sdf_prep   : one lane a triangle: the f64 record (A, B - A, C - A) and the f32 box of the distance pass, the boxes by component
//                  (box[c * T + t]) so that staging them is a straight copy; a dropped triangle gets an empty box (lo = +inf), which no
//                  search ever tests
//   k_sdf_raster : one wave a triangle, lanes stride over the columns of its (y, z) box; a crossing is one integer atomicAdd of +-1 into
//                  delta[(k ny + j)(nx + 1) + m]
//   k_sdf_rows   : one wave a row: the suffix sum of its nx + 1 deltas in chunks of 64 from the far end, then the fill rule; the inside
//                  flag of sample i replaces delta[i] of its row
//   k_sdf_dist   : one wave a 4 x 4 x 4 brick of samples, four bricks a block; the block stages 256 triangles at a time in LDS, each wave
//                  culls them 64 at a time (one lane a triangle: its box against the brick's, against the wave's largest best), and all
//                  lanes test the survivors one after another, each record read by every lane at once (an LDS broadcast)
// Integer atomics and a minimum of f64 values: nothing depends on the order anything arrives in. Every grid is a block-stride loop under
// a fixed cap, every address is formed in size_t.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/pt_amd.h"
#include "pt_scene_gpu.h"
#include "pt_sdf.h"

using namespace pt;

namespace pt {
namespace {

constexpr int TB = 256;                 // four waves a block
constexpr int WAVE = 64;
constexpr uint32_t MAX_BLOCKS = 4096;   // 16 blocks a CU; anything larger is walked by stride
constexpr uint32_t TILE = 256;          // triangles staged at a time: 256 x 96 B = 24 KiB of LDS
static_assert(TILE == TB, "the boxes of a tile are staged one lane a triangle");

#ifndef PT_SDF_CULL
#define PT_SDF_CULL 1                   // 0: a tool build that tests every triangle (tools/sdf_eval.py measures the two)
#endif

bool get(DevMem& m, size_t bytes) { return m.alloc(bytes, "hipMalloc(voxelisation)"); }
bool launched() { return hip_ok(hipGetLastError(), "kernel launch (voxelisation)"); }
dim3 blocks_for(uint64_t items, uint64_t per_block) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, MAX_BLOCKS))); }

__global__ __launch_bounds__(TB) void k_sdf_prep(const float* __restrict__ pos, const uint32_t* __restrict__ idx, uint32_t T, double* __restrict__ rec,
                                                 float* __restrict__ box) {
    for (size_t t = (size_t)blockIdx.x * TB + threadIdx.x; t < T; t += (size_t)gridDim.x * TB) {
        double r[SDF_RECORD_DOUBLES];
        float b[SDF_BOX_FLOATS];
        if (!sdf_record(pos, idx[3 * t], idx[3 * t + 1], idx[3 * t + 2], r, b)) {
            b[0] = b[1] = b[2] = __builtin_inff();
            b[3] = b[4] = b[5] = -__builtin_inff();
        }
        for (size_t c = 0; c < SDF_RECORD_DOUBLES; ++c) rec[t * SDF_RECORD_DOUBLES + c] = r[c];
        for (size_t c = 0; c < SDF_BOX_FLOATS; ++c) box[c * T + t] = b[c];
    }
}

__global__ __launch_bounds__(TB) void k_sdf_raster(const SdfGrid g, const float* __restrict__ pos, const uint32_t* __restrict__ idx, uint32_t T, int32_t* __restrict__ delta) {
    const uint32_t lane = threadIdx.x % WAVE, waves = TB / WAVE;
    for (size_t t = (size_t)blockIdx.x * waves + threadIdx.x / WAVE; t < T; t += (size_t)gridDim.x * waves) {
        double V[3][3];
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d) V[c][d] = (double)pos[3 * (size_t)idx[3 * t + c] + d];
        uint32_t j0, j1, k0, k1;
        sdf_columns(g, V[0], V[1], V[2], j0, j1, k0, k1);
        if (j1 <= j0 || k1 <= k0) continue;
        const uint32_t wj = j1 - j0;
        const uint64_t cols = (uint64_t)wj * (k1 - k0);   // at most ny nz <= 2^28
        for (uint64_t c = lane; c < cols; c += WAVE) {
            const uint32_t kk = (uint32_t)(c / wj), j = j0 + (uint32_t)(c - (uint64_t)kk * wj), k = k0 + kk;
            int o;
            uint32_t m;
            if (sdf_crossing(g, V[0], V[1], V[2], j, k, o, m)) atomicAdd(&delta[((size_t)k * g.ny + j) * ((size_t)g.nx + 1) + m], o);   // m <= nx
        }
    }
}

__global__ __launch_bounds__(TB) void k_sdf_rows(const SdfGrid g, uint32_t rows, int32_t* __restrict__ delta) {
    const uint32_t lane = threadIdx.x % WAVE, waves = TB / WAVE;
    const uint32_t len = g.nx + 1u, chunks = (len + WAVE - 1) / WAVE;
    for (size_t r = (size_t)blockIdx.x * waves + threadIdx.x / WAVE; r < rows; r += (size_t)gridDim.x * waves) {
        int32_t* row = delta + r * (size_t)len;
        int32_t carry = 0;   // the sum of every delta past this chunk
        for (uint32_t c = chunks; c-- > 0;) {
            const uint32_t p = c * WAVE + lane;
            const int32_t own = p < len ? row[p] : 0;
            int32_t s = own;   // becomes the sum of the chunk's deltas from this lane on
            for (int step = 1; step < WAVE; step *= 2) {
                const int32_t up = __shfl_down(s, step, WAVE);
                if (lane + step < WAVE) s += up;
            }
            const int32_t total = __shfl(s, 0, WAVE);
            if (p < g.nx) row[p] = sdf_inside(g.fill, (s - own) + carry) ? 1 : 0;   // the winding of sample p: the deltas past p
            carry += total;
        }
    }
}

__device__ inline double wave_max(double v) {
    for (int step = WAVE / 2; step > 0; step /= 2) {
        const double o = __shfl_xor(v, step, WAVE);
        v = o > v ? o : v;
    }
    return v;
}

// flags: the inside flags in the rows of nx + 1 words k_sdf_rows left, or NULL (distance only)
__global__ __launch_bounds__(TB) void k_sdf_dist(const SdfGrid g, const double* __restrict__ rec, const float* __restrict__ box, uint32_t T, const int32_t* __restrict__ flags,
                                                 uint32_t bx, uint32_t by, uint32_t groups, float* __restrict__ out, unsigned long long* __restrict__ tests) {
    __shared__ double s_rec[TILE][SDF_RECORD_DOUBLES];
    __shared__ float s_box[SDF_BOX_FLOATS][TILE];   // by component: the cull reads one component of 64 triangles at a time
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, waves = TB / WAVE;
    const uint64_t bricks = (uint64_t)bx * by * ((g.nz + 3u) / 4u);
    const double start = sdf_start(g);
#ifdef PT_SDF_COUNT
    unsigned long long counted = 0;
#endif
    for (uint32_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {   // (the same trip count for every lane of the block)
        const uint64_t b = (uint64_t)grp * waves + wave;
        const bool brick = b < bricks;
        uint32_t i = 0, j = 0, k = 0;
        bool live = false, in = false;
        double P[3] = {0.0, 0.0, 0.0}, lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
        if (brick) {
            const uint32_t q = (uint32_t)(b / bx), i0 = ((uint32_t)b - q * bx) * 4u, j0 = (q % by) * 4u, k0 = (q / by) * 4u;
            i = i0 + (lane & 3u); j = j0 + ((lane >> 2) & 3u); k = k0 + (lane >> 4);
            live = i < g.nx && j < g.ny && k < g.nz;
            if (live) {
                P[0] = sdf_coord(g, 0, i); P[1] = sdf_coord(g, 1, j); P[2] = sdf_coord(g, 2, k);
                if (flags) in = flags[((size_t)k * g.ny + j) * ((size_t)g.nx + 1) + i] != 0;
            }
            // the brick's box: its first and its last sample in the grid (the coordinates never decrease with the index)
            const uint32_t i1 = min(i0 + 3u, g.nx - 1u), j1 = min(j0 + 3u, g.ny - 1u), k1 = min(k0 + 3u, g.nz - 1u);
            lo[0] = sdf_coord(g, 0, i0); lo[1] = sdf_coord(g, 1, j0); lo[2] = sdf_coord(g, 2, k0);
            hi[0] = sdf_coord(g, 0, i1); hi[1] = sdf_coord(g, 1, j1); hi[2] = sdf_coord(g, 2, k1);
        }
        // a lane that writes no distance searches for nothing: a sample outside the grid, and with what = 3 one outside the body
        const bool seeks = live && !(g.what == 3 && !in);
        const bool wave_seeks = __any(seeks);
        double best = seeks ? start : 0.0;
#ifdef PT_SDF_COUNT
        const unsigned long long seekers = (unsigned long long)__popcll(__ballot(seeks));
#endif
        for (uint32_t t0 = 0; t0 < T; t0 += TILE) {
            const uint32_t n = min(TILE, T - t0);
            __syncthreads();   // the tile before is read to the end
            for (uint32_t c = threadIdx.x; c < n * (uint32_t)SDF_RECORD_DOUBLES; c += TB) (&s_rec[0][0])[c] = rec[(size_t)t0 * SDF_RECORD_DOUBLES + c];
            if (threadIdx.x < n)   // (TILE == TB: one lane a triangle, six coalesced rows)
                for (uint32_t c = 0; c < (uint32_t)SDF_BOX_FLOATS; ++c) s_box[c][threadIdx.x] = box[(size_t)c * T + t0 + threadIdx.x];
            __syncthreads();
            if (!wave_seeks) continue;   // (wave-uniform; the barriers above are reached by every wave)
            for (uint32_t c0 = 0; c0 < n; c0 += WAVE) {
                const uint32_t mine = c0 + lane;
                bool keep = false;
#if PT_SDF_CULL
                const double worst = wave_max(best);   // the largest best of the wave, refreshed once for 64 triangles (every lane takes part)
#endif
                if (mine < n) {
                    const float tb[SDF_BOX_FLOATS] = {s_box[0][mine], s_box[1][mine], s_box[2][mine], s_box[3][mine], s_box[4][mine], s_box[5][mine]};
                    keep = tb[0] <= tb[3];   // a dropped triangle has an empty box
#if PT_SDF_CULL
                    if (keep) keep = !sdf_cull_far(sdf_box_gap2(lo, hi, tb), worst);
#endif
                }
                unsigned long long todo = __ballot(keep);
#ifdef PT_SDF_COUNT
                if (lane == 0) counted += (unsigned long long)__popcll(todo) * seekers;
#endif
                while (todo) {   // wave-uniform: every lane tests the same triangle
                    const uint32_t t = c0 + (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1ull;
                    if (seeks) {
                        const double d = sdf_dist2(s_rec[t], P);
                        if (d < best) best = d;
                    }
                }
            }
        }
        if (live) out[((size_t)k * g.ny + j) * g.nx + i] = sdf_output(g, best, in);
    }
#ifdef PT_SDF_COUNT
    if (lane == 0 && counted) atomicAdd(tests, counted);
#endif
}

__global__ __launch_bounds__(TB) void k_sdf_occupancy(const SdfGrid g, const int32_t* __restrict__ flags, size_t samples, float* __restrict__ out) {
    for (size_t s = (size_t)blockIdx.x * TB + threadIdx.x; s < samples; s += (size_t)gridDim.x * TB) {
        const size_t r = s / g.nx;
        out[s] = sdf_output(g, 0.0, flags[r * ((size_t)g.nx + 1) + (s - r * g.nx)] != 0);
    }
}

}  // namespace
}  // namespace pt

#ifdef PT_SDF_COUNT
extern "C" {
unsigned long long pt_sdf_tests_counted = 0;   // tool build only: the point-triangle tests of the last call
}
#endif

extern "C" int pt_mesh_sdf(pt_ctx* ctx, const pt_sdf_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t nx, uint32_t ny, uint32_t nz,
                           const double box_lo[3], const double box_hi[3], float* out_values) {
    if (!ctx) return set_error("pt_mesh_sdf: null context");
    SdfGrid g;
    if (sdf_check("pt_mesh_sdf", opts, n_pos, pos, n_idx, idx, nx, ny, nz, box_lo, box_hi, out_values, g) != 0) return -1;
    const size_t T = n_idx / 3u, rows = (size_t)ny * nz, samples = rows * nx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = ctx->stream;

    DevMem d_pos, d_idx, d_rec, d_box, d_delta, d_out;
    unsigned long long* tests = nullptr;   // the counter of a tool build
#ifdef PT_SDF_COUNT
    DevMem d_tests;
    if (!get(d_tests, 8) || !hip_ok(hipMemsetAsync(d_tests.as<void>(), 0, 8, ctx->stream), "hipMemset(voxelisation)")) return -1;
    tests = d_tests.as<unsigned long long>();
#endif
    const bool sign = g.what != 1, dist = g.what != 2;
    if (!get(d_pos, (size_t)n_pos * 12) || !get(d_idx, (size_t)n_idx * 4) || !get(d_out, samples * 4)) return -1;
    if (dist && (!get(d_rec, T * SDF_RECORD_DOUBLES * 8) || !get(d_box, T * SDF_BOX_FLOATS * 4))) return -1;
    if (sign && !get(d_delta, rows * ((size_t)nx + 1) * 4)) return -1;
    bool ok = hip_ok(hipMemcpyAsync(d_pos.as<void>(), pos, (size_t)n_pos * 12, hipMemcpyHostToDevice, st), "hipMemcpy(voxelisation upload)") &&
              hip_ok(hipMemcpyAsync(d_idx.as<void>(), idx, (size_t)n_idx * 4, hipMemcpyHostToDevice, st), "hipMemcpy(voxelisation upload)") &&
              (!sign || hip_ok(hipMemsetAsync(d_delta.as<void>(), 0, rows * ((size_t)nx + 1) * 4, st), "hipMemset(voxelisation)"));
    if (ok && sign) {
        hipLaunchKernelGGL(k_sdf_raster, blocks_for(T, TB / WAVE), dim3(TB), 0, st, g, d_pos.as<float>(), d_idx.as<uint32_t>(), (uint32_t)T, d_delta.as<int32_t>());
        ok = launched();
        if (ok) {
            hipLaunchKernelGGL(k_sdf_rows, blocks_for(rows, TB / WAVE), dim3(TB), 0, st, g, (uint32_t)rows, d_delta.as<int32_t>());
            ok = launched();
        }
    }
    if (ok && dist) {
        hipLaunchKernelGGL(k_sdf_prep, blocks_for(T, TB), dim3(TB), 0, st, d_pos.as<float>(), d_idx.as<uint32_t>(), (uint32_t)T, d_rec.as<double>(), d_box.as<float>());
        ok = launched();
        if (ok) {
            const uint32_t bx = (nx + 3u) / 4u, by = (ny + 3u) / 4u, bz = (nz + 3u) / 4u;
            const uint64_t groups = ((uint64_t)bx * by * bz + TB / WAVE - 1) / (TB / WAVE);   // at most 2^28 samples: fits 32 bits
            hipLaunchKernelGGL(k_sdf_dist, blocks_for(groups, 1), dim3(TB), 0, st, g, d_rec.as<double>(), d_box.as<float>(), (uint32_t)T, sign ? d_delta.as<int32_t>() : nullptr, bx,
                               by, (uint32_t)groups, d_out.as<float>(), tests);
            ok = launched();
        }
    } else if (ok) {
        hipLaunchKernelGGL(k_sdf_occupancy, blocks_for(samples, TB), dim3(TB), 0, st, g, d_delta.as<int32_t>(), samples, d_out.as<float>());
        ok = launched();
    }
    ok = ok && hip_ok(hipMemcpyAsync(out_values, d_out.as<void>(), samples * 4, hipMemcpyDeviceToHost, st), "hipMemcpy(voxelisation download)");
#ifdef PT_SDF_COUNT
    ok = ok && hip_ok(hipMemcpyAsync(&pt_sdf_tests_counted, tests, 8, hipMemcpyDeviceToHost, st), "hipMemcpy(voxelisation count)");
#endif
    // (the caller's arrays are pageable and the device buffers go out of scope: nothing may still read or write them)
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(voxelisation)") || !ok) return -1;
    return 0;
}
