// Adaptive sampling (pt_render_adaptive, pt_render.cpp; its resolve pt_resolve_u8_counts, pt_post.cpp): the kernels that run between the render passes of a round schedule.
//
// Every round renders the sample range [b_i, b_{i+1}) of the ACTIVE pixels (one pixel-list pass of the render core) into one of
// two device accumulators: E takes the even rounds, O the odd ones. Two independent sample sets of one pixel estimate its noise
// without any per-sample state in K3: A = E / n_E and B = O / n_O are two means of the same pixel, and their difference is the
// error. After round i >= 1 (if b_{i+1} < max_spp):
//   k_adapt_error   err[p] = (|A_r-B_r| + |A_g-B_g| + |A_b-B_b|) / (1e-4 + sqrt(M)),  M = (E_r+O_r + E_g+O_g + E_b+O_b) / (n_E+n_O)
//                   for active pixels (left to right, one IEEE rounding per operation), 0 for stopped ones;
//   k_adapt_count / k_adapt_scan / k_adapt_scatter
//                   a pixel stays active if !(err < threshold) holds for itself or for any of its 8 neighbours (3x3 dilation; a
//                   stopped neighbour's 0 never counts for threshold > 0, NaN never converges); the survivors are compacted into the
//                   next list IN ORDER (per-block counts, one scan, scatter), walking the frame in tiled order (8x8 tiles, as the
//                   dynamic mode hands out work), so the list stays sorted by tiled index; a pixel that stops records its count;
//   k_adapt_final   E += O and each pixel's sample count at the end.
// Everything here is deterministic: no atomics decide an order.
#include <hip/hip_runtime.h>

#include "pt_dev_math.h"
#include "pt_kernels.h"

namespace pt {
namespace {
constexpr int ABLOCK = 256;   // threads per block; one block per 256 tiled indices in the select kernels
constexpr int SCAN_BLOCK = 1024;

__global__ __launch_bounds__(ABLOCK) void k_adapt_error(const double* E, const double* O, const uint32_t* stop, uint32_t n_pixels, double n_e,
                                                        double n_o, double* err) {
    for (uint32_t p = blockIdx.x * ABLOCK + threadIdx.x; p < n_pixels; p += gridDim.x * ABLOCK) {
        if (stop[p] != 0u) {
            err[p] = 0.0;
            continue;
        }
        const double* e = E + 3 * (size_t)p;
        const double* o = O + 3 * (size_t)p;
        const double d = fabs(e[0] / n_e - o[0] / n_o) + fabs(e[1] / n_e - o[1] / n_o) + fabs(e[2] / n_e - o[2] / n_o);
        const double m = (e[0] + o[0] + e[1] + o[1] + e[2] + o[2]) / (n_e + n_o);
        err[p] = d / (1e-4 + sqrt(m));
    }
}

// tiled index t -> row-major pixel; false outside the frame (ragged tiles)
PT_DEV bool tiled_pixel(uint32_t t, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t& x, uint32_t& y) {
    const uint32_t tile = t >> 6, in_tile = t & 63u;
    x = (tile % tiles_x) * 8u + (in_tile & 7u);
    y = (tile / tiles_x) * 8u + (in_tile >> 3);
    return x < width && y < height;
}
// does the pixel at tiled index t stay active? (reads err only for the neighbours: a stopped pixel's entry is 0)
PT_DEV bool adapt_keep(uint32_t t, const double* err, const uint32_t* stop, uint32_t width, uint32_t height, uint32_t tiles_x, double threshold,
                       uint32_t& p) {
    uint32_t x, y;
    if (!tiled_pixel(t, width, height, tiles_x, x, y)) return false;
    p = y * width + x;
    if (stop[p] != 0u) return false;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = (int)y + dy;
        if (yy < 0 || yy >= (int)height) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = (int)x + dx;
            if (xx < 0 || xx >= (int)width) continue;
            if (!(err[(size_t)yy * width + (uint32_t)xx] < threshold)) return true;
        }
    }
    return false;
}

__global__ __launch_bounds__(ABLOCK) void k_adapt_count(const double* err, const uint32_t* stop, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                        uint32_t n_tiled, double threshold, uint32_t* block_counts) {
    const uint32_t t = blockIdx.x * ABLOCK + threadIdx.x;
    uint32_t p = 0;
    const bool keep = t < n_tiled && adapt_keep(t, err, stop, width, height, tiles_x, threshold, p);
    const int n = __syncthreads_count(keep);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)n;
}

// exclusive scan of the block counts in place (one block); the total goes to *n_out
__global__ __launch_bounds__(SCAN_BLOCK) void k_adapt_scan(uint32_t* block_counts, uint32_t n_blocks, uint32_t* n_out) {
    __shared__ uint32_t s_sum[SCAN_BLOCK];
    const uint32_t per = (n_blocks + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const uint32_t lo = threadIdx.x * per, hi = min(lo + per, n_blocks);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += block_counts[i];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < SCAN_BLOCK; off *= 2) {   // inclusive Hillis-Steele scan of the per-thread sums
        const uint32_t v = threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = s_sum[threadIdx.x] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = block_counts[i];
        block_counts[i] = run;
        run += c;
    }
    if (threadIdx.x == SCAN_BLOCK - 1) *n_out = s_sum[SCAN_BLOCK - 1];
}

__global__ __launch_bounds__(ABLOCK) void k_adapt_scatter(const double* err, uint32_t* stop, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                          uint32_t n_tiled, double threshold, uint32_t stop_value, const uint32_t* block_offsets,
                                                          uint32_t* list_out) {
    __shared__ uint32_t s_wave[ABLOCK / 64];
    const uint32_t t = blockIdx.x * ABLOCK + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    uint32_t p = 0;
    bool keep = false, active = false;
    if (t < n_tiled) {
        keep = adapt_keep(t, err, stop, width, height, tiles_x, threshold, p);
        uint32_t x, y;
        active = !keep && tiled_pixel(t, width, height, tiles_x, x, y) && stop[y * width + x] == 0u;
        if (active) p = y * width + x;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = block_offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    if (keep) list_out[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = p;
    if (active) stop[p] = stop_value;   // an active pixel that does not stay: it stops with stop_value samples
}

__global__ __launch_bounds__(ABLOCK) void k_adapt_final(double* E, const double* O, const uint32_t* stop, uint32_t n_pixels, uint32_t max_spp,
                                                        uint32_t* counts) {
    for (uint32_t p = blockIdx.x * ABLOCK + threadIdx.x; p < n_pixels; p += gridDim.x * ABLOCK) {
        for (int c = 0; c < 3; ++c) E[3 * (size_t)p + c] += O[3 * (size_t)p + c];
        counts[p] = stop[p] != 0u ? stop[p] : max_spp;
    }
}

// pt_resolve_u8 (k_quantise) with each pixel's own count: mean = sum * (1.0 / n_p)
__global__ __launch_bounds__(ABLOCK) void k_quantise_counts(const double* accum, uint32_t n_pixels, const uint32_t* counts, uint8_t* rgb8) {
    for (uint32_t p = blockIdx.x * ABLOCK + threadIdx.x; p < n_pixels; p += gridDim.x * ABLOCK) {
        const double scale = 1.0 / (double)counts[p];
        for (int ch = 0; ch < 3; ++ch) {
            const size_t i = 3 * (size_t)p + ch;
            double c = accum[i] * scale;
            double g = sqrt(fmax(c, 0.0));
            double q = clampd(g, 0.0, 0.999) * 256.0;
            rgb8[i] = (q != q) ? (uint8_t)0 : (uint8_t)q;
        }
    }
}

dim3 grid_over(uint32_t n, uint32_t max_blocks = 8192) {
    uint32_t b = (n + ABLOCK - 1) / ABLOCK;
    if (b > max_blocks) b = max_blocks;
    return dim3(b ? b : 1u);
}
uint32_t tiles_x_of(uint32_t width) { return (width + 7) / 8; }
uint32_t n_tiled_of(uint32_t width, uint32_t height) { return tiles_x_of(width) * ((height + 7) / 8) * 64u; }
}  // namespace

uint32_t adapt_select_blocks(uint32_t width, uint32_t height) { return (n_tiled_of(width, height) + ABLOCK - 1) / ABLOCK; }

void launch_adapt_error(const double* E, const double* O, const uint32_t* stop, uint32_t n_pixels, double n_e, double n_o, double* err, hipStream_t st) {
    hipLaunchKernelGGL(k_adapt_error, grid_over(n_pixels), dim3(ABLOCK), 0, st, E, O, stop, n_pixels, n_e, n_o, err);
}
void launch_adapt_select(const double* err, uint32_t* stop, uint32_t width, uint32_t height, double threshold, uint32_t stop_value, uint32_t* block_counts,
                         uint32_t* list_out, uint32_t* n_out, hipStream_t st) {
    const uint32_t tx = tiles_x_of(width), n_tiled = n_tiled_of(width, height), nb = adapt_select_blocks(width, height);
    hipLaunchKernelGGL(k_adapt_count, dim3(nb), dim3(ABLOCK), 0, st, err, stop, width, height, tx, n_tiled, threshold, block_counts);
    hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(SCAN_BLOCK), 0, st, block_counts, nb, n_out);
    hipLaunchKernelGGL(k_adapt_scatter, dim3(nb), dim3(ABLOCK), 0, st, err, stop, width, height, tx, n_tiled, threshold, stop_value, block_counts, list_out);
}
void launch_adapt_final(double* E, const double* O, const uint32_t* stop, uint32_t n_pixels, uint32_t max_spp, uint32_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(k_adapt_final, grid_over(n_pixels), dim3(ABLOCK), 0, st, E, O, stop, n_pixels, max_spp, counts);
}
void launch_quantise_counts(const double* accum, uint32_t n_pixels, const uint32_t* counts, uint8_t* rgb8, hipStream_t st) {
    hipLaunchKernelGGL(k_quantise_counts, grid_over(n_pixels, 4096), dim3(ABLOCK), 0, st, accum, n_pixels, counts, rgb8);
}
}  // namespace pt
