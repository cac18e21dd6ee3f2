// The post stage, after the samples are summed: the u8 resolves (pixel_sample_scale + quantisation), the a-trous denoiser
// (pt_denoise.hip) and the film stage (pt_film.hip). Host arrays in, host arrays out, unless the film options say otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_kernels.h"
#include "pt_scene_gpu.h"

using namespace pt;

extern "C" int pt_resolve_u8(pt_ctx* ctx, const double* accum, uint32_t n_pixels, uint32_t total_spp, uint8_t* rgb8) {
    if (!ctx) return set_error("pt_resolve_u8: null context");
    const uint32_t n = n_pixels * 3;
    return run_probe(ctx, {{accum, (size_t)n * sizeof(double)}}, rgb8, n, [&](void* const* d_in, void* d_out) {
        launch_quantise((const double*)d_in[0], n, 1.0 / (double)total_spp, (uint8_t*)d_out, ctx->stream);   // pixel_sample_scale camera.rs:53
    });
}

extern "C" int pt_resolve_u8_counts(pt_ctx* ctx, const double* accum, uint32_t n_pixels, const uint32_t* spp_per_pixel, uint8_t* rgb8) {
    if (!ctx) return set_error("pt_resolve_u8_counts: null context");
    if (!accum || !spp_per_pixel || !rgb8) return set_error("pt_resolve_u8_counts: null buffer");
    for (uint32_t p = 0; p < n_pixels; ++p)
        if (spp_per_pixel[p] == 0) return set_error("pt_resolve_u8_counts: a pixel has no samples");
    const size_t n = (size_t)n_pixels * 3;
    return run_probe(ctx, {{accum, n * sizeof(double)}, {spp_per_pixel, (size_t)n_pixels * sizeof(uint32_t)}}, rgb8, n, [&](void* const* d_in, void* d_out) {
        launch_quantise_counts((const double*)d_in[0], n_pixels, (const uint32_t*)d_in[1], (uint8_t*)d_out, ctx->stream);
    });
}

extern "C" int pt_denoise(pt_ctx* ctx, uint32_t width, uint32_t height, const double* sum_a, uint32_t n_a, const double* sum_b, uint32_t n_b,
                          const double* aov, uint32_t n_aov, const pt_denoise_opts* opts_in, double* out) {
    if (!ctx) return set_error("pt_denoise: null context");
    if (!sum_a || !sum_b || !aov || !out) return set_error("pt_denoise: null buffer");
    if (width == 0 || height == 0) return set_error("pt_denoise: width and height must be positive");
    if ((uint64_t)width * height > 0x7FFFFFFFull) return set_error("pt_denoise: image too large");
    if (n_a == 0 || n_b == 0 || n_aov == 0) return set_error("pt_denoise: n_a, n_b and n_aov must be positive");
    pt_denoise_opts o{5u, 4.0, 0.1};
    if (opts_in) o = *opts_in;
    if (o.iterations > 10) return set_error("pt_denoise: at most 10 iterations");
    if (!(o.sigma_l > 0.0) || !(o.sigma_z > 0.0)) return set_error("pt_denoise: sigma_l and sigma_z must be positive");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    const size_t n = (size_t)width * height;
    // scratch (12 per pixel: two colour + variance buffers and the guides, 32-B records: first), sum_a, sum_b, out (3 each), aov (8)
    DevMem mem;
    if (!mem.alloc(n * 29 * sizeof(double), "hipMalloc(denoise)")) return -1;
    double* d_tmp = mem.as<double>();
    double* d_a = d_tmp + 12 * n;
    double* d_b = d_a + 3 * n;
    double* d_out = d_b + 3 * n;
    double* d_aov = d_out + 3 * n;
    hipStream_t st = ctx->stream;
    if (!hip_ok(hipMemcpyAsync(d_a, sum_a, 3 * n * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(sum_a)") ||
        !hip_ok(hipMemcpyAsync(d_b, sum_b, 3 * n * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(sum_b)") ||
        !hip_ok(hipMemcpyAsync(d_aov, aov, 8 * n * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(aov)"))
        return -1;
    launch_denoise(width, height, d_a, (double)n_a, d_b, (double)n_b, d_aov, (double)n_aov, o.iterations, o.sigma_l, o.sigma_z, d_tmp, d_out, st);
    if (!hip_ok(hipGetLastError(), "kernel launch") ||
        !hip_ok(hipMemcpyAsync(out, d_out, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(out)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(denoise)"))
        return -1;
    return 0;
}

// The film stage (include/pt_amd.h has the rule; the kernels: pt_film.hip). Everything that can refuse the call is checked before the
// first device call, so a refused call writes nothing.
static pt_film_opts film_defaults() {
    pt_film_opts o;
    memset(&o, 0, sizeof o);
    o.white = 4.0; o.bloom_threshold = 1.0; o.bloom_sigma = 2.0; o.bloom_levels = 5u;
    return o;
}
extern "C" int pt_film_opts_check(const pt_film_opts* opts) {
    const pt_film_opts o = opts ? *opts : film_defaults();
    if (!std::isfinite(o.exposure_ev) || std::fabs(o.exposure_ev) > 100.0) return set_error("pt_film_develop: exposure_ev must be finite and within +-100");
    if (o.tonemap > 3u) return set_error("pt_film_develop: tonemap must be 0 (reference), 1 (srgb), 2 (reinhard) or 3 (aces)");
    if (!std::isfinite(o.white) || !(o.white >= 1e-3)) return set_error("pt_film_develop: white must be finite and >= 1e-3");
    if (!(o.bloom_strength >= 0.0 && o.bloom_strength <= 1.0)) return set_error("pt_film_develop: bloom_strength must be in [0, 1]");
    if (!std::isfinite(o.bloom_threshold) || !(o.bloom_threshold >= 0.0)) return set_error("pt_film_develop: bloom_threshold must be finite and >= 0");
    if (!(o.bloom_sigma >= 0.5 && o.bloom_sigma <= 64.0)) return set_error("pt_film_develop: bloom_sigma must be in [0.5, 64]");
    if (o.bloom_levels < 1u || o.bloom_levels > 6u || !(o.bloom_sigma * (double)(1u << (o.bloom_levels - 1u)) <= 128.0))
        return set_error("pt_film_develop: bloom_levels must be in 1..6 with bloom_sigma * 2^(levels - 1) <= 128");
    return 0;
}
extern "C" int pt_film_develop(pt_ctx* ctx, uint32_t width, uint32_t height, const double* sums, uint32_t total_spp, const uint32_t* counts,
                               const pt_film_opts* opts_in, double* hdr_out, uint8_t* rgb8_out) {
    if (!ctx) return set_error("pt_film_develop: null context");
    if (!sums) return set_error("pt_film_develop: null sums");
    if (!hdr_out && !rgb8_out) return set_error("pt_film_develop: both outputs are null");
    if (width == 0 || height == 0) return set_error("pt_film_develop: width and height must be positive");
    if ((uint64_t)width * height > 0x7FFFFFFFull) return set_error("pt_film_develop: image too large");
    if (!counts && total_spp == 0) return set_error("pt_film_develop: total_spp must be positive without per-pixel counts");
    pt_film_opts o = film_defaults();
    if (opts_in) o = *opts_in;
    if (pt_film_opts_check(&o) != 0) return -1;
    const bool glare = o.bloom_strength > 0.0;
    // (the convolution's grid has one row of blocks per 8 rows of its input, which is the frame and then its transpose)
    if (glare && std::max(width, height) > 524280u) return set_error("pt_film_develop: with glare, width and height must be at most 524280");
    const uint32_t n = width * height;
    if (!o.on_device && counts)
        for (uint32_t p = 0; p < n; ++p)
            if (counts[p] == 0) return set_error("pt_film_develop: a pixel has no samples");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = o.stream ? (hipStream_t)o.stream : ctx->stream;
    const uint32_t L = o.bloom_levels;
    // the levels' weights, one after the other: k_l[i] = exp(-(i * i) / (2 sigma_l^2)) / their sum
    std::vector<double> taps;
    std::vector<uint32_t> radius(L), first(L);
    if (glare)
        for (uint32_t l = 0; l < L; ++l) {
            const double sigma = o.bloom_sigma * (double)(1u << l);
            const int r = (int)std::ceil(3.0 * sigma);
            radius[l] = (uint32_t)r;
            first[l] = (uint32_t)taps.size();
            double sum = 0.0;
            for (int i = -r; i <= r; ++i) {
                const double k = std::exp(-((double)i * (double)i) / (2.0 * sigma * sigma));
                taps.push_back(k);
                sum += k;
            }
            for (size_t i = first[l]; i < taps.size(); ++i) taps[i] /= sum;
        }
    // device memory, doubles first: glare scratch (bright, transposed pass, G: 3 planes each) and the weights; then, for host
    // buffers, the sums and hdr_out; then the counts and rgb8_out
    const size_t n3 = (size_t)n * 3;
    const size_t f64s = (glare ? 3 * n3 + taps.size() : 0) + (o.on_device ? 0 : 2 * n3);
    const size_t tail = o.on_device ? 0 : (size_t)n * sizeof(uint32_t) + n3;
    DevMem mem;
    if (f64s + tail > 0 && !mem.alloc(f64s * sizeof(double) + tail, "hipMalloc(film)")) return -1;
    double* at = mem.as<double>();
    double *d_bright = nullptr, *d_pass = nullptr, *d_glare = nullptr, *d_taps = nullptr;
    if (glare) {
        d_bright = at; d_pass = at + n3; d_glare = at + 2 * n3; d_taps = at + 3 * n3;
        at += 3 * n3 + taps.size();
    }
    const double* d_sums = sums;
    const uint32_t* d_counts = counts;
    double* d_hdr = hdr_out;
    uint8_t* d_rgb = rgb8_out;
    if (!o.on_device) {
        double* in = at;
        d_hdr = hdr_out ? at + n3 : nullptr;
        uint32_t* cnt = (uint32_t*)(at + 2 * n3);
        d_rgb = rgb8_out ? (uint8_t*)(cnt + n) : nullptr;
        if (!hip_ok(hipMemcpyAsync(in, sums, n3 * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(film sums)")) return -1;
        if (counts && !hip_ok(hipMemcpyAsync(cnt, counts, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st), "hipMemcpy(film counts)")) return -1;
        d_sums = in;
        d_counts = counts ? cnt : nullptr;
    }
    const double scale = counts ? 0.0 : 1.0 / (double)total_spp;   // pixel_sample_scale camera.rs:53
    const double k = std::exp2(o.exposure_ev);
    if (glare) {
        if (!hip_ok(hipMemcpyAsync(d_taps, taps.data(), taps.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(film weights)")) return -1;
        launch_film_prepare(d_sums, n, scale, d_counts, k, o.bloom_threshold, d_bright, st);
        if (!hip_ok(hipGetLastError(), "k_film_prepare launch")) return -1;
        for (uint32_t l = 0; l < L; ++l) {   // rows, written transposed; then the columns as rows, transposed back and added into G
            if (!launch_film_conv(d_bright, d_pass, height, width, radius[l], d_taps + first[l], 1.0, false, st) ||
                !launch_film_conv(d_pass, d_glare, width, height, radius[l], d_taps + first[l], 1.0 / (double)L, l > 0, st)) {
                (void)hipStreamSynchronize(st);
                return set_error("pt_film_develop: no convolution kernel for this radius");
            }
            if (!hip_ok(hipGetLastError(), "k_film_conv launch")) {
                (void)hipStreamSynchronize(st);
                return -1;
            }
        }
    }
    launch_film_develop(d_sums, n, scale, d_counts, k, o.bloom_threshold, o.bloom_strength, glare ? d_glare : nullptr, o.tonemap, o.white, d_hdr, d_rgb, st);
    bool ok = hip_ok(hipGetLastError(), "k_film_develop launch");
    if (ok && !o.on_device) {
        if (hdr_out) ok = hip_ok(hipMemcpyAsync(hdr_out, d_hdr, n3 * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(film hdr)");
        if (ok && rgb8_out) ok = hip_ok(hipMemcpyAsync(rgb8_out, d_rgb, n3, hipMemcpyDeviceToHost, st), "hipMemcpy(film rgb8)");
    }
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(film)") && ok ? 0 : -1;
}
