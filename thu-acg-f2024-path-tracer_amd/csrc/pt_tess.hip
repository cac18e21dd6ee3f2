// Mesh tessellation and displacement on the GPU (include/pt_amd.h has the rule, pt_tess.h its arithmetic, pt_tess_host.cpp
// the host twin this stage matches byte for byte). One upload, `levels` subdivisions, the displacement and the normal pass on the
// context's stream, one download; between levels only the scalar E (the number of distinct edges) comes back, to size the next mesh.
// A level of F faces and n vertices:
//   k_tess_emit     : one lane per face: its three (edge key, slot 3f + k) pairs
//   hipcub radix sort of the pairs by key
//   k_tess_heads    : one lane per sorted pair: 1 where a run of equal keys begins; hipcub exclusive sum of the flags = the key's rank
//   k_tess_mid      : one lane per sorted pair: vertex n + rank goes to the pair's slot; a run's head writes the midpoint's attributes
//   k_tess_children : one lane per face: its four children
// Smooth normals:
//   k_tess_corners  : (vertex, corner) pairs; hipcub radix sort by vertex (stable: corners stay ascending within a vertex)
//   k_tess_starts   : where each vertex's run begins
//   k_tess_smooth   : one lane per vertex walks its run in order (a sum in a fixed order has no parallel form that keeps the bits)
//   k_tess_displace : one lane per vertex
// No floating-point atomics anywhere: which vertex gets which index, and the order of every sum, follow from integer sorts.
// Indices are 32-bit, byte offsets are not: every address is formed in size_t.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_scene_gpu.h"
#include "pt_tess.h"
#define PT_MESH_STAGE "tessellation"
#include "pt_tess_dev.h"

using namespace pt;

namespace pt {
namespace {

// (k_tess_emit, k_tess_heads, k_tess_children, the normal pass and the launch helpers: pt_tess_dev.h, shared with pt_subdiv.hip)
// pos / nrm / uv hold the n old vertices already (copied before the launch) and have room for n + E
__global__ __launch_bounds__(TB) void k_tess_mid(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ flags,
                                                 const uint32_t* __restrict__ ranks, uint32_t M, uint32_t n, float* pos, float* nrm, float* uv,
                                                 uint32_t* __restrict__ mid) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    const uint32_t head = flags[i];
    const size_t m = (size_t)n + (ranks[i] + head - 1u);   // ranks is exclusive: a head's own flag is not in it yet
    mid[slots[i]] = (uint32_t)m;
    if (!head) return;
    const uint64_t key = keys[i];
    const size_t a = (size_t)(key >> 32), b = (size_t)(key & 0xFFFFFFFFu);   // a <= b < n: old vertices, never written by this kernel
    tess_mid_lin(pos + 3 * a, pos + 3 * b, 3, pos + 3 * m);
    if (nrm) tess_mid_normal(nrm + 3 * a, nrm + 3 * b, nrm + 3 * m);
    if (uv) tess_mid_lin(uv + 2 * a, uv + 2 * b, 2, uv + 2 * m);
}

__global__ __launch_bounds__(TB) void k_tess_displace(float* __restrict__ pos, const float* __restrict__ nrm, const float* __restrict__ uv, uint32_t n, TessDisp D,
                                                      const float* __restrict__ img) {
    const size_t v = (size_t)blockIdx.x * TB + threadIdx.x;
    if (v >= n) return;
    tess_displace(pos + 3 * v, nrm + 3 * v, tess_height(D, img, (double)uv[2 * v], (double)uv[2 * v + 1]));
}

// One subdivision level: `a` in, `b` out. Everything but the mesh `b` is freed on return.
bool subdivide(hipStream_t st, const TessPlan& plan, const DevMesh& a, DevMesh& b) {
    const size_t F = a.F, M = 3 * F, n = a.n;
    size_t E = 0;
    DevMem keys, slots, keys_s, slots_s, flags, ranks, mid, tmp;
    if (M) {
        if (!get(keys, M * 8) || !get(slots, M * 4) || !get(keys_s, M * 8) || !get(slots_s, M * 4) || !get(flags, M * 4) || !get(ranks, M * 4) || !get(mid, M * 4))
            return false;
        hipLaunchKernelGGL(k_tess_emit, grid_for(F), dim3(TB), 0, st, a.idx.as<uint32_t>(), (uint32_t)F, keys.as<uint64_t>(), slots.as<uint32_t>());
        if (!launched()) return false;
        size_t sort_bytes = 0, scan_bytes = 0;
        if (!hip_ok(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys.as<uint64_t>(), keys_s.as<uint64_t>(), slots.as<uint32_t>(), slots_s.as<uint32_t>(), (int)M,
                                                       0, 64, st), "hipcub sort (tessellation)") ||
            !hip_ok(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, flags.as<uint32_t>(), ranks.as<uint32_t>(), (int)M, st), "hipcub scan (tessellation)"))
            return false;
        if (!get(tmp, std::max(sort_bytes, scan_bytes))) return false;
        if (!hip_ok(hipcub::DeviceRadixSort::SortPairs(tmp.as<void>(), sort_bytes, keys.as<uint64_t>(), keys_s.as<uint64_t>(), slots.as<uint32_t>(), slots_s.as<uint32_t>(), (int)M,
                                                       0, 64, st), "hipcub sort (tessellation)"))
            return false;
        hipLaunchKernelGGL(k_tess_heads, grid_for(M), dim3(TB), 0, st, keys_s.as<uint64_t>(), (uint32_t)M, flags.as<uint32_t>());
        if (!launched()) return false;
        if (!hip_ok(hipcub::DeviceScan::ExclusiveSum(tmp.as<void>(), scan_bytes, flags.as<uint32_t>(), ranks.as<uint32_t>(), (int)M, st), "hipcub scan (tessellation)"))
            return false;
        uint32_t last[2] = {0, 0};   // E = the last pair's rank + its flag
        const bool ok = hip_ok(hipMemcpyAsync(&last[0], ranks.as<uint32_t>() + (M - 1), 4, hipMemcpyDeviceToHost, st), "hipMemcpy(edge count)") &&
                        hip_ok(hipMemcpyAsync(&last[1], flags.as<uint32_t>() + (M - 1), 4, hipMemcpyDeviceToHost, st), "hipMemcpy(edge count)");
        if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(tessellation level)") || !ok) return false;
        E = (size_t)last[0] + last[1];
    }
    if (n + E > 0xFFFFFFFFull) {   // (tess_check's bound rules it out)
        set_error("pt_mesh_tessellate: the vertex count passes 32 bits");
        return false;
    }
    b.n = n + E;
    b.F = 4 * F;
    if (!get(b.pos, b.n * 12) || (plan.has_nrm && !get(b.nrm, b.n * 12)) || (plan.has_uv && !get(b.uv, b.n * 8)) || !get(b.idx, b.F * 12)) return false;
    if (n) {
        if (!hip_ok(hipMemcpyAsync(b.pos.as<void>(), a.pos.as<void>(), n * 12, hipMemcpyDeviceToDevice, st), "hipMemcpy(tessellation)")) return false;
        if (plan.has_nrm && !hip_ok(hipMemcpyAsync(b.nrm.as<void>(), a.nrm.as<void>(), n * 12, hipMemcpyDeviceToDevice, st), "hipMemcpy(tessellation)")) return false;
        if (plan.has_uv && !hip_ok(hipMemcpyAsync(b.uv.as<void>(), a.uv.as<void>(), n * 8, hipMemcpyDeviceToDevice, st), "hipMemcpy(tessellation)")) return false;
    }
    if (M) {
        hipLaunchKernelGGL(k_tess_mid, grid_for(M), dim3(TB), 0, st, keys_s.as<uint64_t>(), slots_s.as<uint32_t>(), flags.as<uint32_t>(), ranks.as<uint32_t>(), (uint32_t)M,
                           (uint32_t)n, b.pos.as<float>(), plan.has_nrm ? b.nrm.as<float>() : nullptr, plan.has_uv ? b.uv.as<float>() : nullptr, mid.as<uint32_t>());
        if (!launched()) return false;
        hipLaunchKernelGGL(k_tess_children, grid_for(F), dim3(TB), 0, st, a.idx.as<uint32_t>(), mid.as<uint32_t>(), (uint32_t)F, b.idx.as<uint32_t>());
        if (!launched()) return false;
    }
    // the scratch buffers go out of scope here: the kernels that read them must be done first
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(tessellation level)");
}

}  // namespace
}  // namespace pt

extern "C" int pt_mesh_tessellate(pt_ctx* ctx, const pt_tess_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t n_nrm,
                                  const float* nrm, uint32_t n_uv, const float* uv, float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx,
                                  float** out_nrm, float** out_uv) {
    const char* who = "pt_mesh_tessellate";
    if (!ctx) return set_error("pt_mesh_tessellate: null context");
    const TessIn in{n_pos, pos, n_idx, idx, n_nrm, nrm, n_uv, uv};
    const TessOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm, out_uv};
    TessPlan plan;
    if (tess_check(who, opts, in, out, plan) != 0) return -1;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = ctx->stream;
    auto up = [&](void* d, const void* h, size_t bytes) { return bytes == 0 || hip_ok(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st), "hipMemcpy(tessellation upload)"); };

    // the upload: the mesh (attribute arrays brought to n entries) and the height image
    std::unique_ptr<DevMesh> cur(new DevMesh);
    cur->n = plan.n;
    cur->F = plan.F;
    const size_t n0 = plan.n;
    DevMem img;
    if (!get(cur->pos, n0 * 12) || !get(cur->idx, (size_t)plan.F * 12) || (plan.has_nrm && !get(cur->nrm, n0 * 12)) || (plan.has_uv && !get(cur->uv, n0 * 8))) return -1;
    if (plan.displace && !get(img, (size_t)plan.disp.w * plan.disp.h * 4)) return -1;
    bool ok = up(cur->pos.as<void>(), pos, n0 * 12) && up(cur->idx.as<void>(), idx, (size_t)plan.F * 12);
    if (ok && plan.has_nrm)
        ok = hip_ok(hipMemsetAsync(cur->nrm.as<void>(), 0, n0 ? n0 * 12 : 8, st), "hipMemset(tessellation)") && up(cur->nrm.as<void>(), nrm, std::min<size_t>(n0, n_nrm) * 12);
    if (ok && plan.has_uv)
        ok = hip_ok(hipMemsetAsync(cur->uv.as<void>(), 0, n0 ? n0 * 8 : 8, st), "hipMemset(tessellation)") && up(cur->uv.as<void>(), uv, std::min<size_t>(n0, n_uv) * 8);
    if (ok && plan.displace) ok = up(img.as<void>(), opts->height, (size_t)plan.disp.w * plan.disp.h * 4);
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(tessellation upload)") || !ok) return -1;   // (the caller's arrays are pageable: done with them here)

    for (uint32_t level = 0; level < plan.levels; ++level) {
        std::unique_ptr<DevMesh> next(new DevMesh);
        if (!subdivide(st, plan, *cur, *next)) return -1;
        cur = std::move(next);
    }
    const size_t n = cur->n, F = cur->F;
    DevMem smooth0, smooth1;
    const float* carried = plan.has_nrm ? cur->nrm.as<float>() : nullptr;
    if (plan.displace) {
        if (!carried) {
            if (!smooth(st, *cur, nullptr, smooth0)) return -1;
            carried = smooth0.as<float>();
        }
        if (n) {
            hipLaunchKernelGGL(k_tess_displace, grid_for(n), dim3(TB), 0, st, cur->pos.as<float>(), carried, cur->uv.as<float>(), (uint32_t)n, plan.disp, img.as<float>());
            if (!launched()) return -1;
        }
    }
    const float* d_nrm = plan.out_normals == 1 ? carried : nullptr;
    if (plan.out_normals == 2) {
        if (!smooth(st, *cur, carried, smooth1)) return -1;
        d_nrm = smooth1.as<float>();
    }

    // the download, straight into the arrays the caller gets (malloc'd: pt_free)
    struct HostOut {
        void* p = nullptr;
        ~HostOut() { free(p); }
        bool get(size_t bytes) { return (p = malloc(bytes + 8)) != nullptr; }
        void* give() { void* q = p; p = nullptr; return q; }
    } P, I, N, T;
    if (!P.get(n * 12) || !I.get(F * 12) || (d_nrm && !N.get(n * 12)) || (plan.has_uv && !T.get(n * 8))) return set_error(std::string(who) + ": out of host memory");
    auto down = [&](void* h, const void* d, size_t bytes) { return bytes == 0 || hip_ok(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st), "hipMemcpy(tessellation download)"); };
    ok = down(P.p, cur->pos.as<void>(), n * 12) && down(I.p, cur->idx.as<void>(), F * 12) && (!d_nrm || down(N.p, d_nrm, n * 12)) &&
         (!plan.has_uv || down(T.p, cur->uv.as<void>(), n * 8));
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(tessellation download)") || !ok) return -1;
    *out_pos = (float*)P.give(); *out_n_pos = (uint32_t)n;
    *out_idx = (uint32_t*)I.give(); *out_n_idx = (uint32_t)(3 * F);
    *out_nrm = (float*)N.give(); *out_uv = (float*)T.give();
    return 0;
}
