// Environment importance sampling: the tables' builder and the probe. The tables are read from the texture where it
// already lives, the device atlas. Deterministic: one thread scans one row in column order, then one thread scans the row totals —
// no atomics, the same bits on every run (the exact summation order is written down in include/pt_amd.h).
#include <hip/hip_runtime.h>

#include "pt_envmap.h"
#include "pt_kernels.h"

namespace pt {
namespace {

constexpr int EBLOCK = 256;

// row j: col[j*(W+1) + i + 1] = col[j*(W+1) + i] + w_ij, w_ij = (lum_ij * (c_j - c_{j+1})) * (2 pi / W)
__global__ __launch_bounds__(EBLOCK) void k_env_rows(SceneD sc, TexD T, double* col) {
    const uint32_t j = blockIdx.x * EBLOCK + threadIdx.x;
    if (j >= T.h) return;
    const double dphi = (2.0 * D_PI) / (double)T.w;
    const double dc = env_row_cos(j, T.h) - env_row_cos(j + 1, T.h);
    double* p = col + (size_t)j * (T.w + 1);
    double acc = 0.0;
    p[0] = acc;
    for (uint32_t i = 0; i < T.w; ++i) {
        acc = acc + env_texel_lum(sc, T, i, j) * dc * dphi;
        p[i + 1] = acc;
    }
}
// row[j + 1] = row[j] + R_j, R_j = col[j*(W+1) + W]; row[H] = Z
__global__ void k_env_total(const double* col, uint32_t w, uint32_t h, double* row) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double acc = 0.0;
    row[0] = acc;
    for (uint32_t j = 0; j < h; ++j) {
        acc = acc + col[(size_t)j * (w + 1) + w];
        row[j + 1] = acc;
    }
}
// which 0: in = n pairs (u1, u2), out = n x {dir.xyz, pdf}; which 1: in = n directions xyz, out = n env_pdf values
__global__ __launch_bounds__(EBLOCK) void k_env_probe(SceneD sc, TexD T, EnvTabD e, int which, const double* in, uint32_t n, double* out) {
    for (uint32_t k = blockIdx.x * EBLOCK + threadIdx.x; k < n; k += gridDim.x * EBLOCK) {
        if (which == 0) {
            double pdf;
            const V3 d = env_sample(sc, T, e, in[2 * (size_t)k], in[2 * (size_t)k + 1], pdf);
            double* o = out + 4 * (size_t)k;
            o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = pdf;
        } else {
            const double* q = in + 3 * (size_t)k;
            out[k] = env_pdf(sc, T, e, V3{q[0], q[1], q[2]});
        }
    }
}

}  // namespace

void launch_env_tables(const SceneD& sc, const TexD& tex, double* col, double* row, hipStream_t st) {
    hipLaunchKernelGGL(k_env_rows, dim3((tex.h + EBLOCK - 1) / EBLOCK), dim3(EBLOCK), 0, st, sc, tex, col);
    hipLaunchKernelGGL(k_env_total, dim3(1), dim3(64), 0, st, (const double*)col, tex.w, tex.h, row);
}
void launch_env_probe(const SceneD& sc, const TexD& tex, const EnvTabD& e, int which, const double* in, uint32_t n, double* out, hipStream_t st) {
    uint32_t blocks = (n + EBLOCK - 1) / EBLOCK;
    if (blocks > 2048u) blocks = 2048u;
    if (blocks == 0u) blocks = 1u;
    hipLaunchKernelGGL(k_env_probe, dim3(blocks), dim3(EBLOCK), 0, st, sc, tex, e, which, in, n, out);
}

}  // namespace pt
