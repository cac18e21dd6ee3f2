// Mesh welding and simplification by quadric vertex clustering on the GPU (include/pt_amd.h has the rule, pt_simplify.h
// its arithmetic, pt_simplify_host.cpp the host twin this stage matches byte for byte). One upload, the passes below on the context's
// stream, one download; between them only three counts come back (clusters; surviving faces and vertices), to size what follows.
//   k_simp_ref        : a flag per vertex some index names
//   k_simp_keys_*     : a vertex's key (mode 1: its cell, 63 bits; mode 0: its 96 position bits, -0 canonicalised, in two parts); the
//                       key of an unreferenced vertex sorts last. hipcub stable radix sorts of (key, vertex): one in mode 1, two in mode 0
//   k_simp_heads      : one lane per sorted vertex: the heads of the runs of equal keys, by sorted position and by vertex
//   two exclusive sums: a run's rank in key order; a head's rank in vertex order, which is its cluster's id
//   k_simp_runs, k_simp_assign : where each run starts and which run a cluster is; every member's cluster
//   k_simp_corner_keys, a sort by cluster, k_simp_corner_starts : quadric placement only: the (cluster, corner) pairs
//   k_simp_place      : sixteen lanes a cluster, clusters by stride: the members' mean, the nine sums of the quadric (TSUM: a tile of
//                       sixteen terms is four xor-butterfly steps across the lanes, tiles are added in order), the 3 x 3 solve
//   k_simp_faces      : a face's cluster triple; degenerate faces go; with dedup the sorted triple and the parity, two sorts by
//                       vertex set, and k_simp_groups: the head of a group walks it (twice: the counts, then the survivors)
//   exclusive sums of the kept faces and (k_simp_used) the clusters they name; k_simp_emit_*: the mesh and the vertex map
// then section 27's smooth normals by the kernels of pt_tess_dev.h. Every kernel here walks its work by stride from a grid of at most
// 4096 blocks (k_simp_place: 2048). No floating-point atomic, no integer atomic either: the flag kernels store the same 1 from every lane. Every address is
// formed in size_t.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_scene_gpu.h"
#include "pt_simplify.h"
#define PT_MESH_STAGE "simplification"
#include "pt_tess_dev.h"

using namespace pt;

namespace pt {
namespace {

constexpr uint32_t MAX_BLOCKS = 4096;
constexpr uint32_t GROUPS = TB / SIMP_TILE;   // sixteen-lane groups a block
constexpr uint32_t PLACE_BLOCKS = 2048;       // k_simp_place: eight blocks a CU, 32 768 clusters a pass; its lanes wait on gathers, not on a launch

dim3 capped(size_t n) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((n + TB - 1) / TB, MAX_BLOCKS))); }

#define SIMP_STRIDE(i, n) for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < (n); i += (size_t)gridDim.x * TB)

__global__ __launch_bounds__(TB) void k_simp_ref(const uint32_t* __restrict__ idx, size_t M, uint32_t* __restrict__ ref) {
    SIMP_STRIDE(s, M) ref[idx[s]] = 1u;   // (every lane that meets a vertex stores the same word)
}

__global__ __launch_bounds__(TB) void k_simp_keys_cell(const float* __restrict__ pos, const uint32_t* __restrict__ ref, size_t n, const SimpGrid g,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ verts) {
    SIMP_STRIDE(v, n) {
        keys[v] = ref[v] ? simp_cell_key(g, pos + 3 * v) : SIMP_NO_KEY;
        verts[v] = (uint32_t)v;
    }
}

// Mode 0, the minor part: z. A finite float never has the bits 0xFFFFFFFF, so that key sorts an unreferenced vertex last.
__global__ __launch_bounds__(TB) void k_simp_keys_weld_z(const float* __restrict__ pos, const uint32_t* __restrict__ ref, size_t n, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ verts) {
    SIMP_STRIDE(v, n) {
        keys[v] = ref[v] ? simp_weld_bits(pos[3 * v + 2]) : 0xFFFFFFFFu;
        verts[v] = (uint32_t)v;
    }
}

// Mode 0, the major part, of the vertices as the first sort left them: (x << 32) | y
__global__ __launch_bounds__(TB) void k_simp_keys_weld_xy(const float* __restrict__ pos, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ verts, size_t n,
                                                          uint64_t* __restrict__ keys) {
    SIMP_STRIDE(i, n) {
        const size_t v = verts[i];
        keys[i] = ref[v] ? ((uint64_t)simp_weld_bits(pos[3 * v]) << 32) | simp_weld_bits(pos[3 * v + 1]) : SIMP_NO_KEY;
    }
}

// run_flag[i]: the sorted vertex i starts a run of referenced vertices of one key; is_head[v]: vertex v does. keys: mode 1's sorted
// keys, or NULL: mode 0, where the 96 bits are compared in the positions themselves. run_flag[n] = 0 closes the sum that follows.
__global__ __launch_bounds__(TB) void k_simp_heads(const uint64_t* __restrict__ keys, const float* __restrict__ pos, const uint32_t* __restrict__ ref,
                                                   const uint32_t* __restrict__ sv, size_t n, uint32_t* __restrict__ run_flag, uint32_t* __restrict__ is_head) {
    SIMP_STRIDE(i, n) {
        const size_t v = sv[i];
        uint32_t head = 0;
        if (ref[v]) {
            if (i == 0) head = 1;
            else if (keys) head = keys[i] != keys[i - 1] ? 1u : 0u;
            else {
                const size_t w = sv[i - 1];   // (referenced: the unreferenced vertices sort last)
                head = (simp_weld_bits(pos[3 * v]) != simp_weld_bits(pos[3 * w]) || simp_weld_bits(pos[3 * v + 1]) != simp_weld_bits(pos[3 * w + 1]) ||
                        simp_weld_bits(pos[3 * v + 2]) != simp_weld_bits(pos[3 * w + 2])) ? 1u : 0u;
            }
        }
        run_flag[i] = head;
        is_head[v] = head;
        if (i == 0) run_flag[n] = 0;
    }
}

// run_start[r]: the sorted position where the run of rank r begins; run_start[C]: the number of referenced vertices, where the last
// run ends; crun[c]: the run of cluster c
__global__ __launch_bounds__(TB) void k_simp_runs(const uint32_t* __restrict__ run_flag, const uint32_t* __restrict__ run_rank, const uint32_t* __restrict__ head_rank,
                                                  const uint32_t* __restrict__ ref, const uint32_t* __restrict__ sv, size_t n, uint32_t C,
                                                  uint32_t* __restrict__ run_start, uint32_t* __restrict__ crun) {
    SIMP_STRIDE(i, n) {
        const bool mine = ref[sv[i]] != 0;
        if (run_flag[i]) {
            const uint32_t r = run_rank[i];
            run_start[r] = (uint32_t)i;
            crun[head_rank[sv[i]]] = r;
        }
        if (mine && i + 1 == n) run_start[C] = (uint32_t)n;
        if (!mine && (i == 0 || ref[sv[i - 1]] != 0)) run_start[C] = (uint32_t)i;   // (exactly one lane meets one of the two)
    }
}

__global__ __launch_bounds__(TB) void k_simp_assign(const uint32_t* __restrict__ run_flag, const uint32_t* __restrict__ run_rank, const uint32_t* __restrict__ head_rank,
                                                    const uint32_t* __restrict__ ref, const uint32_t* __restrict__ sv, const uint32_t* __restrict__ run_start, size_t n,
                                                    uint32_t* __restrict__ vcl) {
    SIMP_STRIDE(i, n) {
        const size_t v = sv[i];
        if (!ref[v]) {
            vcl[v] = SIMP_NONE;
            continue;
        }
        const uint32_t r = run_rank[i] + run_flag[i] - 1u;   // run_rank is exclusive: a head's own flag is not in it yet
        vcl[v] = head_rank[sv[run_start[r]]];
    }
}

__global__ __launch_bounds__(TB) void k_simp_corner_keys(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ vcl, size_t M, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ slots) {
    SIMP_STRIDE(s, M) {
        keys[s] = vcl[idx[s]];
        slots[s] = (uint32_t)s;
    }
}

// start[c]: the first sorted corner of cluster c (every cluster has one: its members are referenced); start[C] = M
__global__ __launch_bounds__(TB) void k_simp_corner_starts(const uint32_t* __restrict__ keys, size_t M, uint32_t C, uint32_t* __restrict__ start) {
    SIMP_STRIDE(i, M) {
        if (i == 0 || keys[i] != keys[i - 1]) start[keys[i]] = (uint32_t)i;
        if (i + 1 == M) start[C] = (uint32_t)M;
    }
}

// A tile's value in every lane of its sixteen: pt_simplify.h's tree, level l adding the lanes that differ in bit l
__device__ inline double tile_sum(double x) {
    x = x + __shfl_xor(x, 1, SIMP_TILE);
    x = x + __shfl_xor(x, 2, SIMP_TILE);
    x = x + __shfl_xor(x, 4, SIMP_TILE);
    x = x + __shfl_xor(x, 8, SIMP_TILE);
    return x;
}

// Mode 1. Sixteen lanes a cluster; every lane of a group runs the same trip counts, so the shuffles of tile_sum read live lanes.
__global__ __launch_bounds__(TB) void k_simp_place(const float* __restrict__ pos, const float* __restrict__ uv, const uint32_t* __restrict__ idx,
                                                   const uint32_t* __restrict__ sv, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ run_start,
                                                   const uint32_t* __restrict__ crun, const uint32_t* __restrict__ corners, const uint32_t* __restrict__ corner_start,
                                                   uint32_t C, const SimpGrid g, double reg, int quadric, float* __restrict__ cpos, float* __restrict__ cuv) {
    const uint32_t lane = threadIdx.x % SIMP_TILE;
    for (size_t c = (size_t)blockIdx.x * GROUPS + threadIdx.x / SIMP_TILE; c < C; c += (size_t)gridDim.x * GROUPS) {
        const uint32_t r = crun[c];
        const size_t first = run_start[r], count = run_start[r + 1] - first;
        double o[3], m[3] = {0.0, 0.0, 0.0}, t[2] = {0.0, 0.0};
        simp_cell_origin(g, keys[first], o);
        for (size_t j = 0; j < count; j += SIMP_TILE) {
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (j + lane < count) {
                const size_t w = sv[first + j + lane];
                for (int a = 0; a < 3; ++a) v[a] = ((double)pos[3 * w + a] - o[a]) / (double)count;
                if (uv) {
                    v[3] = (double)uv[2 * w];
                    v[4] = (double)uv[2 * w + 1];
                }
            }
            for (int a = 0; a < 5; ++a) v[a] = tile_sum(v[a]);
            for (int a = 0; a < 3; ++a) m[a] = j == 0 ? v[a] : m[a] + v[a];
            for (int a = 0; a < 2; ++a) t[a] = j == 0 ? v[3 + a] : t[a] + v[3 + a];
        }
        double x[3] = {m[0], m[1], m[2]};
        if (quadric) {
            const size_t cf = corner_start[c], len = corner_start[c + 1] - cf;
            double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (size_t j = 0; j < len; j += SIMP_TILE) {
                double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (j + lane < len) simp_corner_terms(pos, idx + 3 * (size_t)(corners[cf + j + lane] / 3u), o, v);
                for (int k = 0; k < 9; ++k) v[k] = tile_sum(v[k]);
                for (int k = 0; k < 9; ++k) q[k] = j == 0 ? v[k] : q[k] + v[k];
            }
            simp_solve(q, m, reg, g.cell, x);
        }
        if (lane == 0) {
            for (int a = 0; a < 3; ++a) cpos[3 * c + a] = (float)(o[a] + x[a]);
            if (uv)
                for (int a = 0; a < 2; ++a) cuv[2 * c + a] = (float)(t[a] / (double)count);
        }
    }
}

// Mode 0: the head's position bits and texcoord
__global__ __launch_bounds__(TB) void k_simp_place_weld(const float* __restrict__ pos, const float* __restrict__ uv, const uint32_t* __restrict__ sv,
                                                        const uint32_t* __restrict__ run_start, const uint32_t* __restrict__ crun, size_t C, float* __restrict__ cpos,
                                                        float* __restrict__ cuv) {
    SIMP_STRIDE(c, C) {
        const size_t h = sv[run_start[crun[c]]];
        for (int a = 0; a < 3; ++a) cpos[3 * c + a] = pos[3 * h + a];
        if (uv)
            for (int a = 0; a < 2; ++a) cuv[2 * c + a] = uv[2 * h + a];
    }
}

// keep[f] without dedup: the face is not degenerate. With dedup keep[f] = 0 for now, and the face's group key: hi alone (C for a
// degenerate face: one group past every real one), (lo << bits) | mid, and the parity. keep[F] = 0 closes the sum that follows.
__global__ __launch_bounds__(TB) void k_simp_faces(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ vcl, size_t F, uint32_t C, int dedup, int bits,
                                                   uint32_t* __restrict__ keep, uint32_t* __restrict__ fhi, uint64_t* __restrict__ flm, uint8_t* __restrict__ fodd,
                                                   uint32_t* __restrict__ faces) {
    SIMP_STRIDE(f, F) {
        const uint32_t A = vcl[idx[3 * f]], B = vcl[idx[3 * f + 1]], Cc = vcl[idx[3 * f + 2]];
        const bool live = A != B && B != Cc && Cc != A;
        if (f == 0) keep[F] = 0;
        if (!dedup) {
            keep[f] = live ? 1u : 0u;
            continue;
        }
        keep[f] = 0;
        faces[f] = (uint32_t)f;
        uint32_t lo = 0, mid = 0, hi = C;
        const bool odd = live && simp_sorted_triple(A, B, Cc, lo, mid, hi);
        fhi[f] = hi;
        flm[f] = ((uint64_t)lo << bits) | mid;
        fodd[f] = odd ? 1 : 0;
    }
}

__global__ __launch_bounds__(TB) void k_simp_face_key2(const uint32_t* __restrict__ faces, const uint64_t* __restrict__ flm, size_t F, uint64_t* __restrict__ keys) {
    SIMP_STRIDE(i, F) keys[i] = flm[faces[i]];
}

// faces: sorted by vertex set, ascending face index within a set. The head of a group counts its even and odd members, then keeps the
// first |e - o| of the majority: one lane a group, linear in the total.
__global__ __launch_bounds__(TB) void k_simp_groups(const uint32_t* __restrict__ faces, const uint32_t* __restrict__ fhi, const uint64_t* __restrict__ flm,
                                                    const uint8_t* __restrict__ fodd, size_t F, uint32_t C, uint32_t* __restrict__ keep) {
    SIMP_STRIDE(i, F) {
        const size_t f0 = faces[i];
        const uint32_t hi = fhi[f0];
        const uint64_t lm = flm[f0];
        if (hi == C) continue;   // degenerate
        if (i > 0 && fhi[faces[i - 1]] == hi && flm[faces[i - 1]] == lm) continue;
        size_t len = 0, e = 0, od = 0;
        for (; i + len < F; ++len) {
            const size_t f = faces[i + len];
            if (fhi[f] != hi || flm[f] != lm) break;
            if (fodd[f]) ++od;
            else ++e;
        }
        const uint8_t want = od > e ? 1 : 0;
        size_t left = od > e ? od - e : e - od;
        for (size_t k = 0; k < len && left; ++k) {
            const size_t f = faces[i + k];
            if (fodd[f] == want) {
                keep[f] = 1u;
                --left;
            }
        }
    }
}

__global__ __launch_bounds__(TB) void k_simp_used(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ vcl, const uint32_t* __restrict__ keep, size_t F,
                                                  uint32_t* __restrict__ used) {
    SIMP_STRIDE(f, F) {
        if (!keep[f]) continue;
        for (int k = 0; k < 3; ++k) used[vcl[idx[3 * f + k]]] = 1u;   // (the same word from every lane)
    }
}

__global__ __launch_bounds__(TB) void k_simp_emit_vertices(const uint32_t* __restrict__ used, const uint32_t* __restrict__ cout, const float* __restrict__ cpos,
                                                           const float* __restrict__ cuv, size_t C, float* __restrict__ pos, float* __restrict__ uv) {
    SIMP_STRIDE(c, C) {
        if (!used[c]) continue;
        const size_t w = cout[c];
        for (int a = 0; a < 3; ++a) pos[3 * w + a] = cpos[3 * c + a];
        if (cuv)
            for (int a = 0; a < 2; ++a) uv[2 * w + a] = cuv[2 * c + a];
    }
}

__global__ __launch_bounds__(TB) void k_simp_emit_faces(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ vcl, const uint32_t* __restrict__ keep,
                                                        const uint32_t* __restrict__ fout, const uint32_t* __restrict__ cout, size_t F, uint32_t* __restrict__ out) {
    SIMP_STRIDE(f, F) {
        if (!keep[f]) continue;
        const size_t w = fout[f];
        for (int k = 0; k < 3; ++k) out[3 * w + k] = cout[vcl[idx[3 * f + k]]];
    }
}

__global__ __launch_bounds__(TB) void k_simp_map(const uint32_t* __restrict__ vcl, const uint32_t* __restrict__ used, const uint32_t* __restrict__ cout, size_t n,
                                                 uint32_t* __restrict__ map) {
    SIMP_STRIDE(v, n) {
        const uint32_t c = vcl[v];
        map[v] = c != SIMP_NONE && used[c] ? cout[c] : SIMP_NONE;
    }
}

template <class K>
bool sort_pairs(hipStream_t st, const K* k_in, K* k_out, const uint32_t* v_in, uint32_t* v_out, size_t count, int end_bit, DevMem& tmp) {
    size_t bytes = 0;
    return hip_ok(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k_in, k_out, v_in, v_out, (int)count, 0, end_bit, st), "hipcub sort (simplification)") && get(tmp, bytes) &&
           hip_ok(hipcub::DeviceRadixSort::SortPairs(tmp.as<void>(), bytes, k_in, k_out, v_in, v_out, (int)count, 0, end_bit, st), "hipcub sort (simplification)");
}

bool scan(hipStream_t st, const uint32_t* in, uint32_t* out, size_t count, DevMem& tmp) {
    size_t bytes = 0;
    return hip_ok(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)count, st), "hipcub scan (simplification)") && get(tmp, bytes) &&
           hip_ok(hipcub::DeviceScan::ExclusiveSum(tmp.as<void>(), bytes, in, out, (int)count, st), "hipcub scan (simplification)");
}

int bits_for(uint32_t x) {   // the bits that hold every value up to x
    int b = 1;
    while (b < 32 && (x >> b) != 0) ++b;
    return b;
}

}  // namespace
}  // namespace pt

extern "C" int pt_mesh_simplify(pt_ctx* ctx, const pt_simplify_opts* opts, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx, uint32_t n_uv, const float* uv,
                                float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm, float** out_uv, uint32_t** out_map) {
    const char* who = "pt_mesh_simplify";
    if (!ctx) return set_error("pt_mesh_simplify: null context");
    const SimpIn in{n_pos, pos, n_idx, idx, n_uv, uv};
    const SimpOut out{out_pos, out_n_pos, out_idx, out_n_idx, out_nrm, out_uv, out_map};
    SimpPlan plan;
    if (simplify_check(who, opts, in, out, plan) != 0) return -1;
    const size_t n = plan.n, F = plan.F, M = 3 * F;
    if (n > 0x7FFFFFFEull) return set_error(std::string(who) + ": too many vertices for the device sorts: at most 2^31 - 2");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = ctx->stream;
    auto up = [&](void* d, const void* h, size_t bytes) { return bytes == 0 || hip_ok(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st), "hipMemcpy(simplification upload)"); };
    auto zero = [&](DevMem& m, size_t bytes) { return hip_ok(hipMemsetAsync(m.as<void>(), 0, bytes ? bytes : 8, st), "hipMemset(simplification)"); };

    // the upload: the mesh, texcoords brought to n entries
    DevMem d_pos, d_idx, d_uv;
    if (!get(d_pos, n * 12) || !get(d_idx, M * 4) || (plan.has_uv && !get(d_uv, n * 8))) return -1;
    bool ok = up(d_pos.as<void>(), pos, n * 12) && up(d_idx.as<void>(), idx, M * 4);
    if (ok && plan.has_uv) ok = zero(d_uv, n * 8) && up(d_uv.as<void>(), uv, std::min<size_t>(n, n_uv) * 8);
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(simplification upload)") || !ok) return -1;   // (the caller's arrays are pageable: done with them here)
    const float* P = d_pos.as<float>();
    const float* T = plan.has_uv ? d_uv.as<float>() : nullptr;
    const uint32_t* I = d_idx.as<uint32_t>();

    // keys, the sorted vertices, the runs
    DevMem ref, keys, keys_s, verts, sv, run_flag, is_head, run_rank, head_rank, tmp0, tmp1, tmp2, tmp3;
    if (!get(ref, n * 4) || !zero(ref, n * 4) || !get(keys, n * 8) || !get(keys_s, n * 8) || !get(verts, n * 4) || !get(sv, n * 4) || !get(run_flag, (n + 1) * 4) ||
        !get(is_head, n * 4) || !get(run_rank, (n + 1) * 4) || !get(head_rank, n * 4))
        return -1;
    hipLaunchKernelGGL(k_simp_ref, capped(M), dim3(TB), 0, st, I, M, ref.as<uint32_t>());
    if (!launched()) return -1;
    if (plan.mode == 1) {
        hipLaunchKernelGGL(k_simp_keys_cell, capped(n), dim3(TB), 0, st, P, ref.as<uint32_t>(), n, plan.grid, keys.as<uint64_t>(), verts.as<uint32_t>());
        if (!launched() || !sort_pairs(st, keys.as<uint64_t>(), keys_s.as<uint64_t>(), verts.as<uint32_t>(), sv.as<uint32_t>(), n, 64, tmp0)) return -1;
    } else {
        DevMem z, z_s, v1;
        if (!get(z, n * 4) || !get(z_s, n * 4) || !get(v1, n * 4)) return -1;
        hipLaunchKernelGGL(k_simp_keys_weld_z, capped(n), dim3(TB), 0, st, P, ref.as<uint32_t>(), n, z.as<uint32_t>(), verts.as<uint32_t>());
        if (!launched() || !sort_pairs(st, z.as<uint32_t>(), z_s.as<uint32_t>(), verts.as<uint32_t>(), v1.as<uint32_t>(), n, 32, tmp0)) return -1;
        hipLaunchKernelGGL(k_simp_keys_weld_xy, capped(n), dim3(TB), 0, st, P, ref.as<uint32_t>(), v1.as<uint32_t>(), n, keys.as<uint64_t>());
        if (!launched() || !sort_pairs(st, keys.as<uint64_t>(), keys_s.as<uint64_t>(), v1.as<uint32_t>(), sv.as<uint32_t>(), n, 64, tmp1)) return -1;
        if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(simplification keys)")) return -1;   // (z, z_s and v1 go out of scope)
    }
    hipLaunchKernelGGL(k_simp_heads, capped(n), dim3(TB), 0, st, plan.mode == 1 ? keys_s.as<uint64_t>() : nullptr, P, ref.as<uint32_t>(), sv.as<uint32_t>(), n,
                       run_flag.as<uint32_t>(), is_head.as<uint32_t>());
    if (!launched() || !scan(st, run_flag.as<uint32_t>(), run_rank.as<uint32_t>(), n + 1, tmp2) || !scan(st, is_head.as<uint32_t>(), head_rank.as<uint32_t>(), n, tmp3)) return -1;
    uint32_t C32 = 0;
    ok = hip_ok(hipMemcpyAsync(&C32, run_rank.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st), "hipMemcpy(simplification counts)");
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(simplification counts)") || !ok) return -1;
    const size_t C = C32;   // >= 1: some vertex is referenced
    const int bits = bits_for(C32);

    DevMem run_start, crun, vcl, cpos, cuv;
    if (!get(run_start, (C + 1) * 4) || !get(crun, C * 4) || !get(vcl, n * 4) || !get(cpos, C * 12) || (plan.has_uv && !get(cuv, C * 8))) return -1;
    hipLaunchKernelGGL(k_simp_runs, capped(n), dim3(TB), 0, st, run_flag.as<uint32_t>(), run_rank.as<uint32_t>(), head_rank.as<uint32_t>(), ref.as<uint32_t>(), sv.as<uint32_t>(), n,
                       C32, run_start.as<uint32_t>(), crun.as<uint32_t>());
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_simp_assign, capped(n), dim3(TB), 0, st, run_flag.as<uint32_t>(), run_rank.as<uint32_t>(), head_rank.as<uint32_t>(), ref.as<uint32_t>(), sv.as<uint32_t>(),
                       run_start.as<uint32_t>(), n, vcl.as<uint32_t>());
    if (!launched()) return -1;

    // placement
    DevMem ck, cs, ck_s, cs_s, corner_start, tmp4;
    if (plan.mode == 0) {
        hipLaunchKernelGGL(k_simp_place_weld, capped(C), dim3(TB), 0, st, P, T, sv.as<uint32_t>(), run_start.as<uint32_t>(), crun.as<uint32_t>(), C, cpos.as<float>(),
                           plan.has_uv ? cuv.as<float>() : nullptr);
        if (!launched()) return -1;
    } else {
        if (plan.quadric) {
            if (!get(ck, M * 4) || !get(cs, M * 4) || !get(ck_s, M * 4) || !get(cs_s, M * 4) || !get(corner_start, (C + 1) * 4)) return -1;
            hipLaunchKernelGGL(k_simp_corner_keys, capped(M), dim3(TB), 0, st, I, vcl.as<uint32_t>(), M, ck.as<uint32_t>(), cs.as<uint32_t>());
            if (!launched() || !sort_pairs(st, ck.as<uint32_t>(), ck_s.as<uint32_t>(), cs.as<uint32_t>(), cs_s.as<uint32_t>(), M, bits, tmp4)) return -1;
            hipLaunchKernelGGL(k_simp_corner_starts, capped(M), dim3(TB), 0, st, ck_s.as<uint32_t>(), M, C32, corner_start.as<uint32_t>());
            if (!launched()) return -1;
        }
        const size_t blocks = std::max<size_t>(1, std::min<size_t>((C + GROUPS - 1) / GROUPS, PLACE_BLOCKS));
        hipLaunchKernelGGL(k_simp_place, dim3((unsigned)blocks), dim3(TB), 0, st, P, T, I, sv.as<uint32_t>(), keys_s.as<uint64_t>(), run_start.as<uint32_t>(), crun.as<uint32_t>(),
                           plan.quadric ? cs_s.as<uint32_t>() : nullptr, plan.quadric ? corner_start.as<uint32_t>() : nullptr, C32, plan.grid, plan.reg, plan.quadric ? 1 : 0,
                           cpos.as<float>(), plan.has_uv ? cuv.as<float>() : nullptr);
        if (!launched()) return -1;
    }

    // the faces that survive, the clusters they name
    DevMem keep, fout, used, cout, fhi, flm, fodd, faces, faces1, faces2, fhi_s, k2, k2_s, tmp5, tmp6, tmp7, tmp8;
    if (!get(keep, (F + 1) * 4) || !get(fout, (F + 1) * 4) || !get(used, (C + 1) * 4) || !zero(used, (C + 1) * 4) || !get(cout, (C + 1) * 4)) return -1;
    if (plan.dedup && (!get(fhi, F * 4) || !get(flm, F * 8) || !get(fodd, F) || !get(faces, F * 4) || !get(faces1, F * 4) || !get(faces2, F * 4) || !get(fhi_s, F * 4) ||
                       !get(k2, F * 8) || !get(k2_s, F * 8)))
        return -1;
    hipLaunchKernelGGL(k_simp_faces, capped(F), dim3(TB), 0, st, I, vcl.as<uint32_t>(), F, C32, plan.dedup ? 1 : 0, bits, keep.as<uint32_t>(), fhi.as<uint32_t>(),
                       flm.as<uint64_t>(), fodd.as<uint8_t>(), faces.as<uint32_t>());
    if (!launched()) return -1;
    if (plan.dedup) {
        if (!sort_pairs(st, fhi.as<uint32_t>(), fhi_s.as<uint32_t>(), faces.as<uint32_t>(), faces1.as<uint32_t>(), F, bits, tmp5)) return -1;
        hipLaunchKernelGGL(k_simp_face_key2, capped(F), dim3(TB), 0, st, faces1.as<uint32_t>(), flm.as<uint64_t>(), F, k2.as<uint64_t>());
        if (!launched() || !sort_pairs(st, k2.as<uint64_t>(), k2_s.as<uint64_t>(), faces1.as<uint32_t>(), faces2.as<uint32_t>(), F, 2 * bits, tmp6)) return -1;
        hipLaunchKernelGGL(k_simp_groups, capped(F), dim3(TB), 0, st, faces2.as<uint32_t>(), fhi.as<uint32_t>(), flm.as<uint64_t>(), fodd.as<uint8_t>(), F, C32,
                           keep.as<uint32_t>());
        if (!launched()) return -1;
    }
    hipLaunchKernelGGL(k_simp_used, capped(F), dim3(TB), 0, st, I, vcl.as<uint32_t>(), keep.as<uint32_t>(), F, used.as<uint32_t>());
    if (!launched() || !scan(st, keep.as<uint32_t>(), fout.as<uint32_t>(), F + 1, tmp7) || !scan(st, used.as<uint32_t>(), cout.as<uint32_t>(), C + 1, tmp8)) return -1;
    uint32_t Fo32 = 0, no32 = 0;
    ok = hip_ok(hipMemcpyAsync(&Fo32, fout.as<uint32_t>() + F, 4, hipMemcpyDeviceToHost, st), "hipMemcpy(simplification counts)") &&
         hip_ok(hipMemcpyAsync(&no32, cout.as<uint32_t>() + C, 4, hipMemcpyDeviceToHost, st), "hipMemcpy(simplification counts)");
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(simplification counts)") || !ok) return -1;
    const size_t Fo = Fo32, no = no32;

    // the mesh
    DevMesh m;
    m.n = no;
    m.F = Fo;
    DevMem nrm, map;
    if (!get(m.pos, no * 12) || !get(m.idx, Fo * 12) || (plan.has_uv && !get(m.uv, no * 8)) || (plan.want_map && !get(map, n * 4))) return -1;
    hipLaunchKernelGGL(k_simp_emit_vertices, capped(C), dim3(TB), 0, st, used.as<uint32_t>(), cout.as<uint32_t>(), cpos.as<float>(), plan.has_uv ? cuv.as<float>() : nullptr, C,
                       m.pos.as<float>(), plan.has_uv ? m.uv.as<float>() : nullptr);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_simp_emit_faces, capped(F), dim3(TB), 0, st, I, vcl.as<uint32_t>(), keep.as<uint32_t>(), fout.as<uint32_t>(), cout.as<uint32_t>(), F, m.idx.as<uint32_t>());
    if (!launched()) return -1;
    if (plan.want_map) {
        hipLaunchKernelGGL(k_simp_map, capped(n), dim3(TB), 0, st, vcl.as<uint32_t>(), used.as<uint32_t>(), cout.as<uint32_t>(), n, map.as<uint32_t>());
        if (!launched()) return -1;
    }
    if (plan.normals && !smooth(st, m, nullptr, nrm)) return -1;

    // the download, straight into the arrays the caller gets (malloc'd: pt_free)
    struct HostOut {
        void* p = nullptr;
        ~HostOut() { free(p); }
        bool get(size_t bytes) { return (p = malloc(bytes + 8)) != nullptr; }
        void* give() { void* q = p; p = nullptr; return q; }
    } hP, hI, hN, hT, hM;
    if (!hP.get(no * 12) || !hI.get(Fo * 12) || (plan.normals && !hN.get(no * 12)) || (plan.has_uv && !hT.get(no * 8)) || (plan.want_map && !hM.get(n * 4))) {
        (void)hipStreamSynchronize(st);   // (the device buffers go out of scope: the kernels that write them must be done first)
        return set_error(std::string(who) + ": out of host memory");
    }
    auto down = [&](void* h, const void* d, size_t bytes) { return bytes == 0 || hip_ok(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st), "hipMemcpy(simplification download)"); };
    ok = down(hP.p, m.pos.as<void>(), no * 12) && down(hI.p, m.idx.as<void>(), Fo * 12) && (!plan.normals || down(hN.p, nrm.as<void>(), no * 12)) &&
         (!plan.has_uv || down(hT.p, m.uv.as<void>(), no * 8)) && (!plan.want_map || down(hM.p, map.as<void>(), n * 4));
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(simplification download)") || !ok) return -1;
    *out_pos = (float*)hP.give(); *out_n_pos = (uint32_t)no;
    *out_idx = (uint32_t*)hI.give(); *out_n_idx = (uint32_t)(3 * Fo);
    *out_nrm = (float*)hN.give(); *out_uv = (float*)hT.give();
    if (out_map) *out_map = (uint32_t*)hM.give();
    return 0;
}
