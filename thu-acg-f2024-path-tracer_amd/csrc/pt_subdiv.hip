// Loop subdivision with creases, corners and limit projection on the GPU (include/pt_amd.h has the rule, pt_subdiv.h its
// arithmetic, pt_subdiv_host.cpp the host twin this stage matches byte for byte). One upload, `levels` levels, the limit projection and
// the normal pass on the context's stream, one download; between levels only the scalar E comes back, to size the next mesh.
// The edges of a mesh of F faces (k_tess_emit, radix sort, k_tess_heads, exclusive sum: pt_tess_dev.h, as §27), then
//   k_sub_angle    : once, on the input mesh: one lane per sorted pair; the head of a two-slot run tests the fold and flags its slots
//   k_sub_edge     : one lane per sorted pair: vertex n + rank goes to the pair's slot; a run's head walks the run (its length, its
//                    flags, the two opposite vertices), writes the edge's class and its odd vertex, and emits the edge's two
//                    (v, w) -> rank pairs
//   hipcub radix sort of the 2E pairs by (v, w); k_sub_starts: where each vertex's run begins
//   k_sub_even     : one lane per old vertex walks its run in order (a sum in a fixed order has no parallel form that keeps the bits)
//   k_tess_children, k_sub_child_flags : one lane per face
// The limit projection builds the same structure once more on the final mesh and runs k_sub_even with the limit weights.
// The odd and even kernels read the old level's buffers and write the new one's. No floating-point atomics anywhere; every address is
// formed in size_t.
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
#include "pt_subdiv.h"
#define PT_MESH_STAGE "subdivision"
#include "pt_tess_dev.h"

using namespace pt;

namespace pt {
namespace {

constexpr uint64_t NO_RAY = ~0ull;   // the pair of a self-edge: sorts last, belongs to no vertex (v <= 2^32 - 2)

__global__ __launch_bounds__(TB) void k_sub_angle(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ flags, uint32_t M,
                                                  const float* __restrict__ pos, const uint32_t* __restrict__ idx, double crease_cos, uint8_t* __restrict__ crease) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M || !flags[i]) return;
    const uint64_t key = keys[i];
    if (i + 1 >= M || keys[i + 1] != key || (i + 2 < M && keys[i + 2] == key)) return;   // a run of exactly two slots
    if ((uint32_t)(key >> 32) == (uint32_t)key) return;
    const uint32_t s0 = slots[i], s1 = slots[i + 1];
    if (!subdiv_fold(pos, idx, s0 / 3u, s1 / 3u, crease_cos)) return;
    crease[s0] = 1;   // (no other lane touches this run's slots, and nothing in this kernel reads a flag)
    crease[s1] = 1;
}

// pos1 NULL: classification only (the limit projection): no odd vertices, no midpoint indices
__global__ __launch_bounds__(TB) void k_sub_edge(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ flags,
                                                 const uint32_t* __restrict__ ranks, uint32_t M, uint32_t n, const uint32_t* __restrict__ idx,
                                                 const uint8_t* __restrict__ crease, const float* __restrict__ pos0, const float* __restrict__ uv0,
                                                 float* __restrict__ pos1, float* __restrict__ uv1, uint32_t* __restrict__ mid, uint8_t* __restrict__ sharp,
                                                 uint8_t* __restrict__ eflag, uint64_t* __restrict__ rays, uint32_t* __restrict__ ray_rank) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    const uint32_t head = flags[i];
    const size_t r = (size_t)ranks[i] + head - 1u;   // ranks is exclusive: a head's own flag is not in it yet
    if (pos1) mid[slots[i]] = (uint32_t)((size_t)n + r);
    if (!head) return;
    const uint64_t key = keys[i];
    size_t len = 1;
    while (i + len < M && keys[i + len] == key) ++len;
    const uint32_t A = (uint32_t)(key >> 32), B = (uint32_t)key;   // A <= B < n
    const SubdivEdge e = subdiv_edge(A, B, slots + i, len, idx, crease);
    sharp[r] = e.sharp ? 1 : 0;
    eflag[r] = e.flagged ? 1 : 0;
    rays[2 * r] = A != B ? ((uint64_t)A << 32) | B : NO_RAY;
    rays[2 * r + 1] = A != B ? ((uint64_t)B << 32) | A : NO_RAY;
    ray_rank[2 * r] = (uint32_t)r;
    ray_rank[2 * r + 1] = (uint32_t)r;
    if (!pos1) return;
    const size_t m = (size_t)n + r;
    subdiv_odd(pos0 + 3 * (size_t)A, pos0 + 3 * (size_t)B, pos0 + 3 * (size_t)e.C, pos0 + 3 * (size_t)e.D, 3, e.sharp, pos1 + 3 * m);
    if (uv0) subdiv_odd(uv0 + 2 * (size_t)A, uv0 + 2 * (size_t)B, uv0 + 2 * (size_t)e.C, uv0 + 2 * (size_t)e.D, 2, e.sharp, uv1 + 2 * m);
}

// start[v] = the first sorted ray of vertex v; 0xFFFFFFFF (the memset before the launch) where v has no neighbour
__global__ __launch_bounds__(TB) void k_sub_starts(const uint64_t* __restrict__ rays, uint32_t R, uint32_t n, uint32_t* __restrict__ start) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= R) return;
    const uint32_t v = (uint32_t)(rays[i] >> 32);
    if (v >= n) return;   // NO_RAY
    if (i == 0 || (uint32_t)(rays[i - 1] >> 32) != v) start[v] = (uint32_t)i;
}

__global__ __launch_bounds__(TB) void k_sub_even(const float* __restrict__ pos0, const float* __restrict__ uv0, uint32_t n, const uint64_t* __restrict__ rays,
                                                 const uint32_t* __restrict__ ray_rank, uint32_t R, const uint32_t* __restrict__ start,
                                                 const uint8_t* __restrict__ sharp, double corner_cos, int limit, float* __restrict__ pos1, float* __restrict__ uv1) {
    const size_t v = (size_t)blockIdx.x * TB + threadIdx.x;
    if (v >= n) return;
    size_t first = start[v], k = 0;
    if (first == 0xFFFFFFFFu) first = 0;
    else
        while (first + k < R && (size_t)(rays[first + k] >> 32) == v) ++k;
    subdiv_even(pos0, uv0, v, rays + first, ray_rank + first, k, sharp, corner_cos, limit != 0, pos1 + 3 * v, uv0 ? uv1 + 2 * v : nullptr);
}

// The twelve flag bytes of face f's children as three words: (e0, 0, e2, e0) (e1, 0, 0, e1) (e2, 0, 0, 0)
__global__ __launch_bounds__(TB) void k_sub_child_flags(const uint32_t* __restrict__ mid, const uint8_t* __restrict__ eflag, uint32_t n, uint32_t F,
                                                        uint32_t* __restrict__ out) {
    const size_t f = (size_t)blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    const uint32_t e0 = eflag[(size_t)(mid[3 * f] - n)], e1 = eflag[(size_t)(mid[3 * f + 1] - n)], e2 = eflag[(size_t)(mid[3 * f + 2] - n)];
    out[3 * f] = e0 | (e2 << 16) | (e0 << 24);
    out[3 * f + 1] = e1 | (e1 << 24);
    out[3 * f + 2] = e2;
}

struct SubMesh {
    DevMesh m;       // pos, uv, idx (nrm unused)
    DevMem crease;   // one byte per slot
};

// The sorted edges of a mesh: what §27's level makes before k_tess_mid
struct DevEdges {
    DevMem keys, slots, flags, ranks;
    size_t M = 0, E = 0;
};

bool sort_pairs(hipStream_t st, const uint64_t* k_in, uint64_t* k_out, const uint32_t* v_in, uint32_t* v_out, size_t count, int end_bit, DevMem& tmp) {
    size_t bytes = 0;
    return hip_ok(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k_in, k_out, v_in, v_out, (int)count, 0, end_bit, st), "hipcub sort (subdivision)") && get(tmp, bytes) &&
           hip_ok(hipcub::DeviceRadixSort::SortPairs(tmp.as<void>(), bytes, k_in, k_out, v_in, v_out, (int)count, 0, end_bit, st), "hipcub sort (subdivision)");
}

bool build_edges(hipStream_t st, const SubMesh& a, DevEdges& e) {
    const size_t F = a.m.F, M = 3 * F;
    e.M = M;
    e.E = 0;
    if (!M) return true;
    DevMem keys, slots, tmp, tmp2;
    if (!get(keys, M * 8) || !get(slots, M * 4) || !get(e.keys, M * 8) || !get(e.slots, M * 4) || !get(e.flags, M * 4) || !get(e.ranks, M * 4)) return false;
    hipLaunchKernelGGL(k_tess_emit, grid_for(F), dim3(TB), 0, st, a.m.idx.as<uint32_t>(), (uint32_t)F, keys.as<uint64_t>(), slots.as<uint32_t>());
    if (!launched()) return false;
    if (!sort_pairs(st, keys.as<uint64_t>(), e.keys.as<uint64_t>(), slots.as<uint32_t>(), e.slots.as<uint32_t>(), M, 64, tmp)) return false;
    hipLaunchKernelGGL(k_tess_heads, grid_for(M), dim3(TB), 0, st, e.keys.as<uint64_t>(), (uint32_t)M, e.flags.as<uint32_t>());
    if (!launched()) return false;
    size_t scan_bytes = 0;
    if (!hip_ok(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, e.flags.as<uint32_t>(), e.ranks.as<uint32_t>(), (int)M, st), "hipcub scan (subdivision)") ||
        !get(tmp2, scan_bytes) ||
        !hip_ok(hipcub::DeviceScan::ExclusiveSum(tmp2.as<void>(), scan_bytes, e.flags.as<uint32_t>(), e.ranks.as<uint32_t>(), (int)M, st), "hipcub scan (subdivision)"))
        return false;
    uint32_t last[2] = {0, 0};   // E = the last pair's rank + its flag
    const bool ok = hip_ok(hipMemcpyAsync(&last[0], e.ranks.as<uint32_t>() + (M - 1), 4, hipMemcpyDeviceToHost, st), "hipMemcpy(edge count)") &&
                    hip_ok(hipMemcpyAsync(&last[1], e.flags.as<uint32_t>() + (M - 1), 4, hipMemcpyDeviceToHost, st), "hipMemcpy(edge count)");
    // (the scratch buffers go out of scope here: the work that reads them must be done first)
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(subdivision edges)") || !ok) return false;
    e.E = (size_t)last[0] + last[1];
    return true;
}

// The classes of a's edges and the sorted neighbour runs of its vertices, then every even vertex (or limit position) into pos1 / uv1.
// odd: the new mesh to write odd vertices and midpoint indices for (NULL: the limit projection). eflag / mid come back for the children.
bool rings_and_even(hipStream_t st, const SubdivPlan& plan, const SubMesh& a, const DevEdges& e, bool limit, float* pos1, float* uv1, bool odd, DevMem& mid, DevMem& eflag) {
    const size_t n = a.m.n, M = e.M, E = e.E, R = 2 * E;
    DevMem sharp, rays, ray_rank, rays_s, rank_s, start, tmp;
    if (!get(sharp, E) || !get(eflag, E) || !get(rays, R * 8) || !get(ray_rank, R * 4) || !get(rays_s, R * 8) || !get(rank_s, R * 4) || !get(start, n * 4) ||
        (odd && !get(mid, M * 4)))
        return false;
    const float* uv0 = plan.has_uv ? a.m.uv.as<float>() : nullptr;
    if (M) {
        hipLaunchKernelGGL(k_sub_edge, grid_for(M), dim3(TB), 0, st, e.keys.as<uint64_t>(), e.slots.as<uint32_t>(), e.flags.as<uint32_t>(), e.ranks.as<uint32_t>(), (uint32_t)M,
                           (uint32_t)n, a.m.idx.as<uint32_t>(), a.crease.as<uint8_t>(), a.m.pos.as<float>(), uv0, odd ? pos1 : nullptr, odd ? uv1 : nullptr,
                           mid.as<uint32_t>(), sharp.as<uint8_t>(), eflag.as<uint8_t>(), rays.as<uint64_t>(), ray_rank.as<uint32_t>());
        if (!launched()) return false;
        if (!sort_pairs(st, rays.as<uint64_t>(), rays_s.as<uint64_t>(), ray_rank.as<uint32_t>(), rank_s.as<uint32_t>(), R, 64, tmp)) return false;
    }
    if (n) {
        if (!hip_ok(hipMemsetAsync(start.as<void>(), 0xFF, n * 4, st), "hipMemset(subdivision)")) return false;
        if (R) {
            hipLaunchKernelGGL(k_sub_starts, grid_for(R), dim3(TB), 0, st, rays_s.as<uint64_t>(), (uint32_t)R, (uint32_t)n, start.as<uint32_t>());
            if (!launched()) return false;
        }
        hipLaunchKernelGGL(k_sub_even, grid_for(n), dim3(TB), 0, st, a.m.pos.as<float>(), uv0, (uint32_t)n, rays_s.as<uint64_t>(), rank_s.as<uint32_t>(), (uint32_t)R,
                           start.as<uint32_t>(), sharp.as<uint8_t>(), plan.corner_cos, limit ? 1 : 0, pos1, uv1);
        if (!launched()) return false;
    }
    // the scratch buffers go out of scope here: the kernels that read them must be done first
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(subdivision level)");
}

// One level: `a` in, `b` out
bool level(hipStream_t st, const SubdivPlan& plan, const SubMesh& a, const DevEdges& e, SubMesh& b) {
    const size_t F = a.m.F, n = a.m.n;
    if (n + e.E > 0xFFFFFFFFull) {   // (subdiv_check's bound rules it out)
        set_error("pt_mesh_subdivide: the vertex count passes 32 bits");
        return false;
    }
    b.m.n = n + e.E;
    b.m.F = 4 * F;
    if (!get(b.m.pos, b.m.n * 12) || (plan.has_uv && !get(b.m.uv, b.m.n * 8)) || !get(b.m.idx, b.m.F * 12) || !get(b.crease, b.m.F * 3)) return false;
    DevMem mid, eflag;
    if (!rings_and_even(st, plan, a, e, false, b.m.pos.as<float>(), plan.has_uv ? b.m.uv.as<float>() : nullptr, true, mid, eflag)) return false;
    if (F) {
        hipLaunchKernelGGL(k_tess_children, grid_for(F), dim3(TB), 0, st, a.m.idx.as<uint32_t>(), mid.as<uint32_t>(), (uint32_t)F, b.m.idx.as<uint32_t>());
        if (!launched()) return false;
        hipLaunchKernelGGL(k_sub_child_flags, grid_for(F), dim3(TB), 0, st, mid.as<uint32_t>(), eflag.as<uint8_t>(), (uint32_t)n, (uint32_t)F, b.crease.as<uint32_t>());
        if (!launched()) return false;
    }
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(subdivision level)");
}

}  // namespace
}  // namespace pt

extern "C" int pt_mesh_subdivide(pt_ctx* ctx, const pt_subdiv_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t n_uv,
                                 const float* uv, const uint8_t* crease, float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm,
                                 float** out_uv, uint8_t** out_crease) {
    const char* who = "pt_mesh_subdivide";
    if (!ctx) return set_error("pt_mesh_subdivide: null context");
    const SubdivIn in{n_pos, pos, n_idx, idx, n_uv, uv, crease};
    const SubdivOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm, out_uv, out_crease};
    SubdivPlan plan;
    if (subdiv_check(who, opts, in, out, plan) != 0) return -1;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = ctx->stream;
    auto up = [&](void* d, const void* h, size_t bytes) { return bytes == 0 || hip_ok(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st), "hipMemcpy(subdivision upload)"); };

    // the upload: the mesh (texcoords brought to n entries, flags read as 0 or 1)
    std::unique_ptr<SubMesh> cur(new SubMesh);
    cur->m.n = plan.n;
    cur->m.F = plan.F;
    const size_t n0 = plan.n, M0 = 3 * (size_t)plan.F;
    std::vector<uint8_t> flags01(M0 + 1, 0);
    if (crease)
        for (size_t i = 0; i < M0; ++i) flags01[i] = crease[i] != 0 ? 1 : 0;
    if (!get(cur->m.pos, n0 * 12) || !get(cur->m.idx, M0 * 4) || (plan.has_uv && !get(cur->m.uv, n0 * 8)) || !get(cur->crease, M0)) return -1;
    bool ok = up(cur->m.pos.as<void>(), pos, n0 * 12) && up(cur->m.idx.as<void>(), idx, M0 * 4) && up(cur->crease.as<void>(), flags01.data(), M0);
    if (ok && plan.has_uv)
        ok = hip_ok(hipMemsetAsync(cur->m.uv.as<void>(), 0, n0 ? n0 * 8 : 8, st), "hipMemset(subdivision)") && up(cur->m.uv.as<void>(), uv, std::min<size_t>(n0, n_uv) * 8);
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(subdivision upload)") || !ok) return -1;   // (the caller's arrays are pageable: done with them here)

    DevEdges e;
    if (!build_edges(st, *cur, e)) return -1;
    if (e.M) {
        hipLaunchKernelGGL(k_sub_angle, grid_for(e.M), dim3(TB), 0, st, e.keys.as<uint64_t>(), e.slots.as<uint32_t>(), e.flags.as<uint32_t>(), (uint32_t)e.M,
                           cur->m.pos.as<float>(), cur->m.idx.as<uint32_t>(), plan.crease_cos, cur->crease.as<uint8_t>());
        if (!launched()) return -1;
    }
    for (uint32_t l = 0; l < plan.levels; ++l) {
        std::unique_ptr<SubMesh> next(new SubMesh);
        if (!level(st, plan, *cur, e, *next)) return -1;
        cur = std::move(next);
        if ((l + 1 < plan.levels || plan.limit) && !build_edges(st, *cur, e)) return -1;
    }
    const size_t n = cur->m.n, F = cur->m.F;
    if (plan.limit) {
        DevMesh lim;
        DevMem none0, none1;
        if (!get(lim.pos, n * 12) || (plan.has_uv && !get(lim.uv, n * 8))) return -1;
        if (!rings_and_even(st, plan, *cur, e, true, lim.pos.as<float>(), plan.has_uv ? lim.uv.as<float>() : nullptr, false, none0, none1)) return -1;
        // the projected values take the place of the ones they were computed from (every lane of the pass is done: it synchronised)
        if (n && !hip_ok(hipMemcpyAsync(cur->m.pos.as<void>(), lim.pos.as<void>(), n * 12, hipMemcpyDeviceToDevice, st), "hipMemcpy(subdivision)")) return -1;
        if (n && plan.has_uv && !hip_ok(hipMemcpyAsync(cur->m.uv.as<void>(), lim.uv.as<void>(), n * 8, hipMemcpyDeviceToDevice, st), "hipMemcpy(subdivision)")) return -1;
        if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(subdivision limit)")) return -1;   // (lim goes out of scope)
    }
    DevMem nrm;
    if (plan.normals && !smooth(st, cur->m, nullptr, nrm)) return -1;

    // the download, straight into the arrays the caller gets (malloc'd: pt_free)
    struct HostOut {
        void* p = nullptr;
        ~HostOut() { free(p); }
        bool get(size_t bytes) { return (p = malloc(bytes + 8)) != nullptr; }
        void* give() { void* q = p; p = nullptr; return q; }
    } P, I, N, T, Cr;
    if (!P.get(n * 12) || !I.get(F * 12) || (plan.normals && !N.get(n * 12)) || (plan.has_uv && !T.get(n * 8)) || (plan.want_crease && !Cr.get(F * 3)))
        return set_error(std::string(who) + ": out of host memory");
    auto down = [&](void* h, const void* d, size_t bytes) { return bytes == 0 || hip_ok(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st), "hipMemcpy(subdivision download)"); };
    ok = down(P.p, cur->m.pos.as<void>(), n * 12) && down(I.p, cur->m.idx.as<void>(), F * 12) && (!plan.normals || down(N.p, nrm.as<void>(), n * 12)) &&
         (!plan.has_uv || down(T.p, cur->m.uv.as<void>(), n * 8)) && (!plan.want_crease || down(Cr.p, cur->crease.as<void>(), F * 3));
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(subdivision download)") || !ok) return -1;
    *out_pos = (float*)P.give(); *out_n_pos = (uint32_t)n;
    *out_idx = (uint32_t*)I.give(); *out_n_idx = (uint32_t)(3 * F);
    *out_nrm = (float*)N.give(); *out_uv = (float*)T.give();
    if (out_crease) *out_crease = (uint8_t*)Cr.give();
    return 0;
}
