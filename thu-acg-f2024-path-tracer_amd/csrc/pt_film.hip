// The film stage behind pt_film_develop (pt_post.cpp; no counterpart in the reference, whose camera.rs:109-130 is the default
// options' special case). The rule is written out in include/pt_amd.h; in short:
//   k_film_prepare  per pixel: x = max(mean * 2^ev, 0) and the bright part B = x * (Y - T) / Y for Y = lum(x) > T, as three planes.
//   k_film_conv     one separable pass of one glare level: out[c][x][y] (+)= scale * sum_i k[i] in[c][y][x + i], i = -r .. r, zero
//                   outside the image. The result is written TRANSPOSED, so the vertical pass is this kernel again on the transposed
//                   planes, and its output lands back in image order; it adds (1/L) V_l into G (the first level stores).
//   k_film_develop  per pixel: x and B again (the same operations, so the same bits), o = (x - s B) + s G, hdr_out = o, the tone
//                   curve and the quantiser of k_quantise.
// f64 throughout, deterministic (no atomics). The convolution is the hot path: a block of 256 threads takes a tile of
// CONV_TY rows x CONV_TX columns. It stages the rows with both halos in LDS once, split into four PHASE PLANES (element e of a row
// lives in plane e & 3 at index e >> 2), so that a lane which owns four neighbouring outputs reads consecutive 8-byte words with its
// neighbours: conflict-free ds_read_b64. Each lane slides a four-element register window over the row: one LDS read feeds four
// multiply-adds. The results go through a second LDS tile so that the transposed store writes runs of CONV_TY doubles. Both tiles are
// padded so that their stores are conflict-free as well (conv_plane_words, CONV_TPL).
#include <hip/hip_runtime.h>

#include "pt_dev_math.h"
#include "pt_kernels.h"

namespace pt {
namespace {
constexpr int FBLOCK = 256;
constexpr int CONV_TX = 256, CONV_TY = 8;   // tile: columns (4 per lane, one wave per row) x rows (2 per wave); tests/test_film_gpu.py states CONV_TX
constexpr int CONV_TP = CONV_TY + 1;        // transpose tile: a column's CONV_TY results, padded to an odd number of 8-byte words
// The transpose tile keeps the lanes' four columns in four planes too (column xl in plane xl & 3 at index xl >> 2): a lane's stride is
// CONV_TP = 9 words, odd, so the 16 lanes of a ds_write_b64 group hit 16 different bank pairs; the planes start 8 words (mod 32)
// apart, so the 32 lanes of a ds_read_b64 group of the store loop (4 columns x 8 rows) read 32 different words.
constexpr int CONV_TPL = (CONV_TX / 4) * CONV_TP + 8;   // words per plane: 584 = 8 (mod 32)

PT_DEV double lum3(double r, double g, double b) { return luminance(V3{r, g, b}); }

// steps 1-2 of the rule for one pixel: x (exposed, clamped mean) and the weight w of its bright part
template <bool COUNTS> PT_DEV void film_pixel(const double* sums, size_t p, double scale, const uint32_t* counts, double k, double thr, double x[3], double& w) {
    const double sc = COUNTS ? 1.0 / (double)counts[p] : scale;
    for (int c = 0; c < 3; ++c) {
        const double m = sums[3 * p + c] * sc;
        x[c] = fmax(m * k, 0.0);
    }
    const double y = lum3(x[0], x[1], x[2]);
    w = (y > thr && y < D_INF) ? (y - thr) / y : 0.0;
}

template <bool COUNTS>
__global__ __launch_bounds__(FBLOCK) void k_film_prepare(const double* sums, uint32_t n_pixels, double scale, const uint32_t* counts, double k, double thr,
                                                         double* bright) {
    for (uint32_t p = blockIdx.x * FBLOCK + threadIdx.x; p < n_pixels; p += gridDim.x * FBLOCK) {
        double x[3], w;
        film_pixel<COUNTS>(sums, p, scale, counts, k, thr, x, w);
        for (int c = 0; c < 3; ++c) bright[(size_t)c * n_pixels + p] = x[c] * w;
    }
}

PT_DEV double oetf(double t) { return t <= 0.0031308 ? 12.92 * t : 1.055 * detmath::pow(t, 1.0 / 2.4) - 0.055; }

template <bool COUNTS>
__global__ __launch_bounds__(FBLOCK) void k_film_develop(const double* sums, uint32_t n_pixels, double scale, const uint32_t* counts, double k, double thr,
                                                         double s, const double* glare, uint32_t tonemap, double white, double* hdr, uint8_t* rgb8) {
    for (uint32_t p = blockIdx.x * FBLOCK + threadIdx.x; p < n_pixels; p += gridDim.x * FBLOCK) {
        double o[3], w;
        film_pixel<COUNTS>(sums, p, scale, counts, k, thr, o, w);
        if (glare)
            for (int c = 0; c < 3; ++c) o[c] = (o[c] - s * (o[c] * w)) + s * glare[(size_t)c * n_pixels + p];
        if (hdr)
            for (int c = 0; c < 3; ++c) hdr[3 * (size_t)p + c] = o[c];
        if (!rgb8) continue;
        double v[3];
        if (tonemap == 0u) {
            for (int c = 0; c < 3; ++c) v[c] = sqrt(o[c]);
        } else {
            for (int c = 0; c < 3; ++c) o[c] = fmin(o[c], 1e150);
            if (tonemap == 1u) {
                for (int c = 0; c < 3; ++c) v[c] = oetf(fmin(o[c], 1.0));
            } else if (tonemap == 2u) {
                const double y = lum3(o[0], o[1], o[2]);
                const double sc = (1.0 + y / (white * white)) / (1.0 + y);
                for (int c = 0; c < 3; ++c) v[c] = oetf(fmin(o[c] * sc, 1.0));
            } else {
                for (int c = 0; c < 3; ++c) {
                    const double t = (o[c] * (2.51 * o[c] + 0.03)) / (o[c] * (2.43 * o[c] + 0.59) + 0.14);
                    v[c] = oetf(clampd(t, 0.0, 1.0));
                }
            }
        }
        for (int c = 0; c < 3; ++c) {
            const double q = clampd(v[c], 0.0, 0.999) * 256.0;
            rgb8[3 * (size_t)p + c] = (q != q) ? (uint8_t)0 : (uint8_t)q;
        }
    }
}

// One separable pass. in: 3 planes of `rows` x `cols`; out: 3 planes of `cols` x `rows`; taps: the 2 r + 1 weights.
// LDS: CONV_TY staged rows of 4 * pl doubles (pl = words per phase plane), then the 4 x CONV_TPL transpose tile.
template <bool ACC>
__global__ __launch_bounds__(FBLOCK) void k_film_conv(const double* __restrict__ in, double* __restrict__ out, int rows, int cols, int r, int pl, const double* __restrict__ taps, double scale) {
    extern __shared__ double lds[];
    const int S = 4 * pl;
    double* tile = lds + (size_t)CONV_TY * S;
    const int x0 = (int)blockIdx.x * CONV_TX, y0 = (int)blockIdx.y * CONV_TY;
    const size_t plane = (size_t)rows * cols;
    const double* src = in + blockIdx.z * plane;
    double* dst = out + blockIdx.z * plane;
    const int tid = (int)threadIdx.x;
    // stage: element e of staged row yy is input column x0 - r + e (0 outside the image or below the last row)
    // (the rows in the inner, unrolled loop: CONV_TY independent loads in flight per lane)
    for (int e = tid; e < S; e += FBLOCK) {
        const int x = x0 - r + e;
        const bool in_x = x >= 0 && x < cols;
        double v[CONV_TY];
#pragma unroll
        for (int yy = 0; yy < CONV_TY; ++yy) v[yy] = (in_x && y0 + yy < rows) ? src[(size_t)(y0 + yy) * cols + x] : 0.0;
        double* at = lds + (e & 3) * pl + (e >> 2);
#pragma unroll
        for (int yy = 0; yy < CONV_TY; ++yy) at[(size_t)yy * S] = v[yy];
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int n = 2 * r + 1;
    for (int yy = wave; yy < CONV_TY; yy += FBLOCK / 64) {
        const double* p0 = lds + (size_t)yy * S + lane;   // plane j at p0 + j * pl; this lane's outputs are columns x0 + 4 lane + (0 .. 3)
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        double w0 = p0[0], w1 = p0[pl], w2 = p0[2 * pl], w3 = p0[3 * pl];   // elements 4 lane + ii + (0 .. 3)
        int ii = 0;
        for (; ii + 4 <= n; ii += 4) {
            const double* q = p0 + (ii >> 2) + 1;
            const double k0 = taps[ii], k1 = taps[ii + 1], k2 = taps[ii + 2], k3 = taps[ii + 3];
            const double n0 = q[0], n1 = q[pl], n2 = q[2 * pl], n3 = q[3 * pl];
            a0 += k0 * w0; a1 += k0 * w1; a2 += k0 * w2; a3 += k0 * w3;
            a0 += k1 * w1; a1 += k1 * w2; a2 += k1 * w3; a3 += k1 * n0;
            a0 += k2 * w2; a1 += k2 * w3; a2 += k2 * n0; a3 += k2 * n1;
            a0 += k3 * w3; a1 += k3 * n0; a2 += k3 * n1; a3 += k3 * n2;
            w0 = n0; w1 = n1; w2 = n2; w3 = n3;
        }
        {   // n is odd: one or three taps are left
            const double* q = p0 + (ii >> 2) + 1;
            const double k0 = taps[ii];
            a0 += k0 * w0; a1 += k0 * w1; a2 += k0 * w2; a3 += k0 * w3;
            if (ii + 3 == n) {
                const double k1 = taps[ii + 1], k2 = taps[ii + 2];
                const double n0 = q[0], n1 = q[pl];
                a0 += k1 * w1; a1 += k1 * w2; a2 += k1 * w3; a3 += k1 * n0;
                a0 += k2 * w2; a1 += k2 * w3; a2 += k2 * n0; a3 += k2 * n1;
            }
        }
        double* t = tile + lane * CONV_TP + yy;
        t[0] = a0; t[CONV_TPL] = a1; t[2 * CONV_TPL] = a2; t[3 * CONV_TPL] = a3;
    }
    __syncthreads();
    // transposed store: out[x][y], y fastest
    for (int i = tid; i < CONV_TX * CONV_TY; i += FBLOCK) {
        const int yl = i % CONV_TY, xl = i / CONV_TY;
        const int x = x0 + xl, y = y0 + yl;
        if (x < cols && y < rows) {
            const double v = scale * tile[(xl & 3) * CONV_TPL + (xl >> 2) * CONV_TP + yl];
            double* o = dst + (size_t)x * rows + y;
            *o = ACC ? *o + v : v;
        }
    }
}

dim3 grid_px(uint32_t n) {
    uint32_t b = (n + FBLOCK - 1) / FBLOCK;
    if (b > 4096u) b = 4096u;
    return dim3(b ? b : 1u);
}
// words per phase plane of a staged row: the lanes' 64, the taps' share and one more for the window's look-ahead, rounded up to 4 (mod 16):
// the four planes then start 4 words apart (mod 16), and the 16 lanes of a staging ds_write_b64 group (4 planes x 4 consecutive words)
// hit 16 different bank pairs
int conv_plane_words(int r) {
    const int need = CONV_TX / 4 + (2 * r + 1 + 3) / 4 + 1;
    return (need + 11) / 16 * 16 + 4;
}
size_t conv_lds_bytes(int r) { return ((size_t)CONV_TY * 4 * conv_plane_words(r) + (size_t)4 * CONV_TPL) * sizeof(double); }
}  // namespace

void launch_film_prepare(const double* sums, uint32_t n_pixels, double scale, const uint32_t* counts, double k, double thr, double* bright, hipStream_t st) {
    if (counts) hipLaunchKernelGGL(k_film_prepare<true>, grid_px(n_pixels), dim3(FBLOCK), 0, st, sums, n_pixels, scale, counts, k, thr, bright);
    else hipLaunchKernelGGL(k_film_prepare<false>, grid_px(n_pixels), dim3(FBLOCK), 0, st, sums, n_pixels, scale, counts, k, thr, bright);
}

bool launch_film_conv(const double* in, double* out, uint32_t rows, uint32_t cols, uint32_t r, const double* taps, double scale, bool accumulate, hipStream_t st) {
    const size_t lds = conv_lds_bytes((int)r);
    auto kern = accumulate ? k_film_conv<true> : k_film_conv<false>;
    if (lds > 160u * 1024u || (rows + CONV_TY - 1) / CONV_TY > 65535u) return false;   // (pt_film_develop refuses such frames up front)
    if (lds > 64u * 1024u && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
    const dim3 grid((cols + CONV_TX - 1) / CONV_TX, (rows + CONV_TY - 1) / CONV_TY, 3);
    hipLaunchKernelGGL(kern, grid, dim3(FBLOCK), lds, st, in, out, (int)rows, (int)cols, (int)r, conv_plane_words((int)r), taps, scale);
    return true;
}

void launch_film_develop(const double* sums, uint32_t n_pixels, double scale, const uint32_t* counts, double k, double thr, double s, const double* glare,
                         uint32_t tonemap, double white, double* hdr, uint8_t* rgb8, hipStream_t st) {
    if (counts)
        hipLaunchKernelGGL(k_film_develop<true>, grid_px(n_pixels), dim3(FBLOCK), 0, st, sums, n_pixels, scale, counts, k, thr, s, glare, tonemap, white, hdr, rgb8);
    else
        hipLaunchKernelGGL(k_film_develop<false>, grid_px(n_pixels), dim3(FBLOCK), 0, st, sums, n_pixels, scale, counts, k, thr, s, glare, tonemap, white, hdr, rgb8);
}

}  // namespace pt
