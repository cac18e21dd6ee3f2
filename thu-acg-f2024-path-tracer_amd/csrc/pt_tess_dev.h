// The kernels and launch helpers that mesh tessellation (pt_tess.hip) and Loop subdivision (pt_subdiv.hip, §28) share:
// the edge keys of a level, the heads of their sorted runs, the four children of a face, and smooth normals by sorted (vertex, corner)
// pairs. Included by those two units only; everything has internal linkage, so each unit carries its own copy of a kernel it launches.
// No floating-point atomics anywhere: which vertex gets which index, and the order of every sum, follow from integer sorts.
// Indices are 32-bit, byte offsets are not: every address is formed in size_t.
#pragma once
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "pt_scene_gpu.h"
#include "pt_tess.h"

// The including unit names its stage: the word the error labels below carry ("hipMalloc(tessellation)", "hipMalloc(subdivision)")
#ifndef PT_MESH_STAGE
#error "define PT_MESH_STAGE (the stage's name in error labels) before including pt_tess_dev.h"
#endif

namespace pt {
namespace {

constexpr int TB = 256;   // four waves a block; every kernel here is a stream of independent elements

__global__ __launch_bounds__(TB) void k_tess_emit(const uint32_t* __restrict__ idx, uint32_t F, uint64_t* __restrict__ keys, uint32_t* __restrict__ slots) {
    const size_t f = (size_t)blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    const uint32_t a = idx[3 * f], b = idx[3 * f + 1], c = idx[3 * f + 2];
    keys[3 * f] = tess_edge_key(a, b);
    keys[3 * f + 1] = tess_edge_key(b, c);
    keys[3 * f + 2] = tess_edge_key(c, a);
    slots[3 * f] = (uint32_t)(3 * f);
    slots[3 * f + 1] = (uint32_t)(3 * f + 1);
    slots[3 * f + 2] = (uint32_t)(3 * f + 2);
}

__global__ __launch_bounds__(TB) void k_tess_heads(const uint64_t* __restrict__ keys, uint32_t M, uint32_t* __restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(TB) void k_tess_children(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ mid, uint32_t F, uint32_t* __restrict__ out) {
    const size_t f = (size_t)blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    const uint32_t a = idx[3 * f], b = idx[3 * f + 1], c = idx[3 * f + 2], ab = mid[3 * f], bc = mid[3 * f + 1], ca = mid[3 * f + 2];
    uint32_t* o = out + 12 * f;
    o[0] = a; o[1] = ab; o[2] = ca;
    o[3] = ab; o[4] = b; o[5] = bc;
    o[6] = ca; o[7] = bc; o[8] = c;
    o[9] = ab; o[10] = bc; o[11] = ca;
}

__global__ __launch_bounds__(TB) void k_tess_corners(const uint32_t* __restrict__ idx, uint32_t M, uint32_t* __restrict__ verts, uint32_t* __restrict__ corners) {
    const size_t c = (size_t)blockIdx.x * TB + threadIdx.x;
    if (c >= M) return;
    verts[c] = idx[c];
    corners[c] = (uint32_t)c;
}

// start[v] = the first sorted pair of vertex v; 0xFFFFFFFF (the memset before the launch) where no corner refers to v
__global__ __launch_bounds__(TB) void k_tess_starts(const uint32_t* __restrict__ verts, uint32_t M, uint32_t* __restrict__ start) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    const uint32_t v = verts[i];
    if (i == 0 || verts[i - 1] != v) start[v] = (uint32_t)i;
}

__global__ __launch_bounds__(TB) void k_tess_smooth(const float* __restrict__ pos, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ verts,
                                                    const uint32_t* __restrict__ corners, uint32_t M, const uint32_t* __restrict__ start, uint32_t n,
                                                    const float* __restrict__ prev, float* __restrict__ out) {
    const size_t v = (size_t)blockIdx.x * TB + threadIdx.x;
    if (v >= n) return;
    size_t first = start[v], len = 0;
    if (first == 0xFFFFFFFFu) first = 0;
    else
        while (first + len < M && verts[first + len] == v) ++len;
    tess_smooth_normal(pos, idx, corners + first, len, prev ? prev + 3 * v : nullptr, out + 3 * v);
}

dim3 grid_for(size_t n) { return dim3((unsigned)((n + TB - 1) / TB)); }

struct DevMesh {
    DevMem pos, nrm, uv, idx;
    size_t n = 0, F = 0;
};

bool get(DevMem& m, size_t bytes) { return m.alloc(bytes, "hipMalloc(" PT_MESH_STAGE ")"); }
bool launched() { return hip_ok(hipGetLastError(), "kernel launch (" PT_MESH_STAGE ")"); }

// Smooth normals of m's positions into `out` (n x 3 floats); prev: the normals the vertices had (device) or NULL
bool smooth(hipStream_t st, const DevMesh& m, const float* prev, DevMem& out) {
    const size_t M = 3 * m.F, n = m.n;
    if (!get(out, n * 12)) return false;
    if (n == 0) return true;
    DevMem verts, corners, verts_s, corners_s, start, tmp;
    if (!get(start, n * 4) || !hip_ok(hipMemsetAsync(start.as<void>(), 0xFF, n * 4, st), "hipMemset(" PT_MESH_STAGE ")")) return false;
    if (!get(verts_s, M * 4) || !get(corners_s, M * 4)) return false;
    if (M) {
        if (!get(verts, M * 4) || !get(corners, M * 4)) return false;
        hipLaunchKernelGGL(k_tess_corners, grid_for(M), dim3(TB), 0, st, m.idx.as<uint32_t>(), (uint32_t)M, verts.as<uint32_t>(), corners.as<uint32_t>());
        if (!launched()) return false;
        size_t sort_bytes = 0;
        if (!hip_ok(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, verts.as<uint32_t>(), verts_s.as<uint32_t>(), corners.as<uint32_t>(), corners_s.as<uint32_t>(), (int)M,
                                                       0, 32, st), "hipcub sort (" PT_MESH_STAGE ")") ||
            !get(tmp, sort_bytes) ||
            !hip_ok(hipcub::DeviceRadixSort::SortPairs(tmp.as<void>(), sort_bytes, verts.as<uint32_t>(), verts_s.as<uint32_t>(), corners.as<uint32_t>(), corners_s.as<uint32_t>(),
                                                       (int)M, 0, 32, st), "hipcub sort (" PT_MESH_STAGE ")"))
            return false;
        hipLaunchKernelGGL(k_tess_starts, grid_for(M), dim3(TB), 0, st, verts_s.as<uint32_t>(), (uint32_t)M, start.as<uint32_t>());
        if (!launched()) return false;
    }
    hipLaunchKernelGGL(k_tess_smooth, grid_for(n), dim3(TB), 0, st, m.pos.as<float>(), m.idx.as<uint32_t>(), verts_s.as<uint32_t>(), corners_s.as<uint32_t>(), (uint32_t)M,
                       start.as<uint32_t>(), (uint32_t)n, prev, out.as<float>());
    if (!launched()) return false;
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(" PT_MESH_STAGE " normals)");
}

}  // namespace
}  // namespace pt
