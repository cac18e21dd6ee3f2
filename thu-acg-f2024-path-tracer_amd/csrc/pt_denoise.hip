// The a-trous denoiser behind pt_denoise (pt_post.cpp; no counterpart in the reference). The rule is written out in
// include/pt_amd.h; in short:
//   k_dn_prepare  per pixel: demodulated colour c = mu / max(albedo, 1e-3) and its variance v from the two disjoint sample sets
//                 (A, B) the frame was rendered as; the guides N (unit shading normal) and z (mean first-hit depth). Background
//                 pixels (no first hit) carry v = -1 and take no part in any filter.
//   k_dn_level    one a-trous level with step s = 2^k: a 3x3 binomial prefilter of v, then the 5x5 B3-spline taps at distance s
//                 weighted by luminance (in standard deviations of the prefiltered v), relative depth and normal agreement; c and
//                 v are filtered together (v with the squared weights). One launch per level, ping-ponging two buffers.
//   k_dn_final    foreground: c * max(albedo, 1e-3); background: mu.
// f64 throughout, one thread per pixel, deterministic (no atomics). The 25 taps of a level are read straight from global memory:
// neighbouring lanes read neighbouring pixels, so each tap row is one or two cache lines per wave, and the working set of a
// 16x16 block at step s (a (16+4s)^2 window) stays in L2 (DESIGN.md §9 has the measured time).
#include <hip/hip_runtime.h>

#include "pt_dev_math.h"
#include "pt_kernels.h"

namespace pt {
namespace {
constexpr int DN_X = 16, DN_Y = 16;   // 2-D blocks of 256 threads: a wave covers 16 x 4 pixels

typedef double d4v __attribute__((ext_vector_type(4)));

PT_DEV double lum(double r, double g, double b) { return luminance(V3{r, g, b}); }

__global__ __launch_bounds__(DN_X * DN_Y) void k_dn_prepare(uint32_t width, uint32_t height, const double* sum_a, double n_a, const double* sum_b,
                                                           double n_b, const double* aov, double n_aov, d4v* col, d4v* guide) {
    const uint32_t x = blockIdx.x * DN_X + threadIdx.x, y = blockIdx.y * DN_Y + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const double* f = aov + 8 * p;
    const double hits = f[7];
    if (hits == 0.0) {
        col[p] = d4v{0.0, 0.0, 0.0, -1.0};
        guide[p] = d4v{0.0, 0.0, 0.0, 0.0};
        return;
    }
    const double* sa = sum_a + 3 * p;
    const double* sb = sum_b + 3 * p;
    double c[3], ca[3], cb[3];
    for (int k = 0; k < 3; ++k) {
        const double a = fmax(f[k] / n_aov, 1e-3);
        c[k] = ((sa[k] + sb[k]) / (n_a + n_b)) / a;
        ca[k] = (sa[k] / n_a) / a;
        cb[k] = (sb[k] / n_b) / a;
    }
    const double d = lum(ca[0], ca[1], ca[2]) - lum(cb[0], cb[1], cb[2]);
    const double v = d * d * (n_a * n_b / ((n_a + n_b) * (n_a + n_b)));
    col[p] = d4v{c[0], c[1], c[2], v};
    const double len = sqrt(f[3] * f[3] + f[4] * f[4] + f[5] * f[5]);
    const d4v nz = len > 0.0 ? d4v{f[3] / len, f[4] / len, f[5] / len, f[6] / hits} : d4v{0.0, 0.0, 0.0, f[6] / hits};
    guide[p] = nz;
}

__global__ __launch_bounds__(DN_X * DN_Y) void k_dn_level(uint32_t width, uint32_t height, int step, double sigma_l, double sigma_z, const d4v* col,
                                                         const d4v* guide, d4v* out) {
    const int x = (int)(blockIdx.x * DN_X + threadIdx.x), y = (int)(blockIdx.y * DN_Y + threadIdx.y);
    const int w = (int)width, h = (int)height;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * width + x;
    const d4v cp = col[p];
    if (cp.w < 0.0) {   // background
        out[p] = cp;
        return;
    }
    // variance prefilter: (1/4, 1/2, 1/4)^2 over the in-image foreground 3x3 neighbours, normalised by the weight present
    const double k3[3] = {0.25, 0.5, 0.25};
    double gs = 0.0, gw = 0.0;
    for (int j = -1; j <= 1; ++j) {
        const int yy = y + j;
        if (yy < 0 || yy >= h) continue;
        for (int i = -1; i <= 1; ++i) {
            const int xx = x + i;
            if (xx < 0 || xx >= w) continue;
            const double vq = col[(size_t)yy * width + xx].w;
            if (vq < 0.0) continue;
            const double kk = k3[j + 1] * k3[i + 1];
            gw += kk;
            gs += kk * vq;
        }
    }
    const double g = gs / gw;
    const d4v gp = guide[p];
    const double lp = lum(cp.x, cp.y, cp.z);
    const double dl = sigma_l * sqrt(g) + 1e-10, dz = sigma_z * gp.w + 1e-10;
    const double h5[5] = {1.0 / 16.0, 0.25, 0.375, 0.25, 1.0 / 16.0};
    double sw = 0.0, sv = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
    for (int j = -2; j <= 2; ++j) {
        const int yy = y + step * j;
        if (yy < 0 || yy >= h) continue;
        for (int i = -2; i <= 2; ++i) {
            const int xx = x + step * i;
            if (xx < 0 || xx >= w) continue;
            const size_t q = (size_t)yy * width + xx;
            const d4v cq = col[q];
            if (cq.w < 0.0) continue;
            const d4v gq = guide[q];
            const double e = detmath::exp(-(fabs(lp - lum(cq.x, cq.y, cq.z)) / dl) - fabs(gp.w - gq.w) / dz);
            double n = fmax(0.0, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
#pragma unroll
            for (int s = 0; s < 7; ++s) n = n * n;   // ^128
            const double wq = h5[i + 2] * h5[j + 2] * e * n;
            sw += wq;
            sr += wq * cq.x;
            sg += wq * cq.y;
            sb += wq * cq.z;
            sv += wq * wq * cq.w;
        }
    }
    out[p] = sw > 0.0 ? d4v{sr / sw, sg / sw, sb / sw, sv / (sw * sw)} : cp;   // (sw == 0 only with a zero normal: nothing to average)
}

__global__ __launch_bounds__(DN_X * DN_Y) void k_dn_final(uint32_t width, uint32_t height, const double* sum_a, const double* sum_b, double n_ab,
                                                         const double* aov, double n_aov, const d4v* col, double* out) {
    const uint32_t x = blockIdx.x * DN_X + threadIdx.x, y = blockIdx.y * DN_Y + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const double* f = aov + 8 * p;
    const bool fg = f[7] != 0.0;
    const d4v c = col[p];
    const double cc[3] = {c.x, c.y, c.z};
    for (int k = 0; k < 3; ++k)
        out[3 * p + k] = fg ? cc[k] * fmax(f[k] / n_aov, 1e-3) : (sum_a[3 * p + k] + sum_b[3 * p + k]) / n_ab;
}
}  // namespace

void launch_denoise(uint32_t width, uint32_t height, const double* sum_a, double n_a, const double* sum_b, double n_b, const double* aov, double n_aov,
                    uint32_t iterations, double sigma_l, double sigma_z, double* tmp, double* out, hipStream_t st) {
    const size_t n = (size_t)width * height;
    d4v* col[2] = {reinterpret_cast<d4v*>(tmp), reinterpret_cast<d4v*>(tmp) + n};
    d4v* guide = reinterpret_cast<d4v*>(tmp) + 2 * n;
    const dim3 block(DN_X, DN_Y), grid((width + DN_X - 1) / DN_X, (height + DN_Y - 1) / DN_Y);
    hipLaunchKernelGGL(k_dn_prepare, grid, block, 0, st, width, height, sum_a, n_a, sum_b, n_b, aov, n_aov, col[0], guide);
    for (uint32_t k = 0; k < iterations; ++k)
        hipLaunchKernelGGL(k_dn_level, grid, block, 0, st, width, height, 1 << k, sigma_l, sigma_z, col[k & 1], guide, col[(k + 1) & 1]);
    hipLaunchKernelGGL(k_dn_final, grid, block, 0, st, width, height, sum_a, sum_b, n_a + n_b, aov, n_aov, col[iterations & 1], out);
}

}  // namespace pt
