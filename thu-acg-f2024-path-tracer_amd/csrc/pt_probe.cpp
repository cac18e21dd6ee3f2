// The device probes: entry points that run single device functions of the kernels (intersection, environment / medium / light /
// dispersion sampling, the camera, the samplers, the deterministic math) on host arrays, for the tests and tools that compare them with
// the oracle. They share one path, run_probe (declared in pt_scene.h; the u8 resolves of pt_post.cpp take it too). Every function checks
// its own arguments before the first device call: a refused call writes nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_kernels.h"
#include "pt_scene_gpu.h"

using namespace pt;

int pt::run_probe(pt_ctx* ctx, std::initializer_list<ProbeIn> in, void* out, size_t out_bytes,
                  const std::function<void(void* const* d_in, void* d_out)>& launch) {
    if (out_bytes == 0) return 0;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    std::vector<DevMem> d_in(in.size());
    std::vector<void*> p_in(in.size());
    DevMem d_out;
    size_t k = 0;
    for (const ProbeIn& i : in) {
        if (!d_in[k].alloc(i.bytes, "hipMalloc")) return -1;
        p_in[k] = d_in[k].as<void>();
        ++k;
    }
    if (!d_out.alloc(out_bytes, "hipMalloc")) return -1;
    k = 0;
    for (const ProbeIn& i : in)
        if (!hip_ok(hipMemcpyAsync(p_in[k++], i.host, i.bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy")) return -1;
    launch(p_in.data(), d_out.as<void>());
    // (a failure from here on still waits for the stream: the buffers are freed when this returns)
    const bool ok = hip_ok(hipGetLastError(), "kernel launch") &&
                    hip_ok(hipMemcpyAsync(out, d_out.as<void>(), out_bytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy");
    return hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize") && ok ? 0 : -1;
}

extern "C" int pt_intersect(pt_scene* s, const double* rays, uint32_t n, double* out) {
    if (!s || !s->built) return set_error("pt_intersect: world not built");
    return run_probe(s->ctx, {{rays, (size_t)n * 7 * sizeof(double)}}, out, (size_t)n * 15 * sizeof(double), [&](void* const* d_in, void* d_out) {
        launch_probe(s->gpu->dev.view, (const double*)d_in[0], n, (double*)d_out, s->ctx->stream);
    });
}

extern "C" int pt_env_probe(pt_scene* s, const pt_camera* cam, int which, const double* in, uint32_t n, double* out) {
    if (!s || !s->built) return set_error("pt_env_probe: world not built");
    if (!cam || (which != 0 && which != 1)) return set_error("pt_env_probe: which must be 0 or 1");
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    CamD dc;
    if (make_camd(s, cam, dc) != 0) return -1;
    if (!dc.env_is_map) return set_error("pt_env_probe: the camera's environment is not a map");
    EnvTabD e;
    if (env_tables(s, dc, ctx->stream, e) != 0) return -1;
    if (!(e.z > 0.0)) return set_error("pt_env_probe: the environment map has no weight (Z = 0)");
    TexD T;
    if (!hip_ok(hipMemcpyAsync(&T, s->gpu->dev.view.tex + dc.env_tex, sizeof T, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") ||
        !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))
        return -1;
    const size_t n_in = (size_t)n * (which == 0 ? 2 : 3), n_out = (size_t)n * (which == 0 ? 4 : 1);
    return run_probe(ctx, {{in, n_in * sizeof(double)}}, out, n_out * sizeof(double), [&](void* const* d_in, void* d_out) {
        launch_env_probe(s->gpu->dev.view, T, e, which, (const double*)d_in[0], n, (double*)d_out, ctx->stream);
    });
}

extern "C" int pt_medium_probe(pt_scene* s, int mat, int which, const double* in, uint32_t n, double* out) {
    if (!s || !s->ctx) return set_error("pt_medium_probe: null scene");
    if (mat < 0 || (size_t)mat >= s->mats.size() || s->mats[mat].kind != MAT_MEDIUM) return set_error("pt_medium_probe: not a medium material");
    if (which < 0 || which > 4) return set_error("pt_medium_probe: which must be 0, 1, 2, 3 or 4");
    const bool grid = which == 2 || which == 3;
    if (grid && s->mats[mat].p[6] == 0.0) return set_error("pt_medium_probe: which 2 and 3 need a grid-density medium (pt_mat_medium_grid)");
    if (n == 0) return 0;
    if (!in || !out) return set_error("pt_medium_probe: null buffer");
    static const size_t IN_COLS[5] = {5, 1, 3, 7, 1}, OUT_COLS[5] = {4, 1, 1, 3, 3};
    const size_t n_in = (size_t)n * IN_COLS[which], n_out = (size_t)n * OUT_COLS[which];
    if (which == 3)   // the loop's expected trip count is bounded for unit directions (pt_mat_medium_grid): longer ones are refused
        for (uint32_t i = 0; i < n; ++i) {
            const double* d = in + 7 * (size_t)i + 3;
            if (!(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= 1.0 + 1e-9)) return set_error("pt_medium_probe: which 3 takes directions of length <= 1");
        }
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    DevMem d_g, d_v;
    if (grid) {   // the medium's own grid, uploaded for the call (the world need not be built)
        const HostGrid& hg = s->grids[(size_t)s->mats[mat].p[6] - 1];
        if (!d_g.alloc(sizeof(GridD), "hipMalloc") || !d_v.alloc(hg.vals.size() * sizeof(float), "hipMalloc") ||
            !hip_ok(hipMemcpyAsync(d_g.as<GridD>(), &hg.d, sizeof(GridD), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy") ||
            !hip_ok(hipMemcpyAsync(d_v.as<float>(), hg.vals.data(), hg.vals.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy"))
            return -1;
    }
    return run_probe(ctx, {{in, n_in * sizeof(double)}}, out, n_out * sizeof(double), [&](void* const* d_in, void* d_out) {
        const double* d_i = (const double*)d_in[0];
        double* d_o = (double*)d_out;
        if (grid) launch_grid_probe(which, d_g.as<GridD>(), d_v.as<float>(), d_i, n, d_o, ctx->stream);
        else if (which == 4) launch_absorb_probe(s->mats[mat].p + 7, d_i, n, d_o, ctx->stream);
        else launch_medium_probe(which, s->mats[mat].p[0], s->mats[mat].p[1], d_i, n, d_o, ctx->stream);
    });
}

extern "C" int pt_light_probe(pt_scene* s, int which, const double* in, uint32_t n, double* out) {
    if (!s || !s->built) return set_error("pt_light_probe: world not built");
    if (which != 0 && which != 1) return set_error("pt_light_probe: which must be 0 or 1");
    if (s->gpu->dev.view.n_lights == 0u) return set_error("pt_light_probe: the world has no lights list");
    const bool exact = s->light_sampling == 1;
    // (pt_render's refusal: the exact functions' chain walks read the stored poses, so they would answer for the scene at time 0)
    if (exact && s->has_moving_instance) return set_error("pt_light_probe: motion together with exact light sampling is not supported (set light sampling to 0, or take the moving instances out)");
    if (exact && s->light_mesh_bad_area) return set_error("pt_light_probe: exact light sampling needs light meshes of finite, positive area");
    if (exact && s->light_blas_depth > (uint32_t)LIGHT_STACK) return set_error("pt_light_probe: exact light sampling: a light mesh's BVH is deeper than the 24 levels its pdf walk's stack holds");
    if (n == 0) return 0;
    if (!in || !out) return set_error("pt_light_probe: null buffer");
    const size_t n_in = (size_t)n * (which == 0 ? 4 : 7), n_out = (size_t)n * (which == 0 ? 6 : 1);
    return run_probe(s->ctx, {{in, n_in * sizeof(double)}}, out, n_out * sizeof(double), [&](void* const* d_in, void* d_out) {
        launch_light_probe(s->gpu->dev.view, exact, which, (const double*)d_in[0], n, (double*)d_out, s->ctx->stream);
    });
}

extern "C" int pt_punctual_probe(pt_scene* s, int which, const double* in, uint32_t n, double* out) {
    if (!s || !s->built) return set_error("pt_punctual_probe: world not built");
    if (which < 0 || which > 3) return set_error("pt_punctual_probe: which must be 0, 1, 2 or 3");
    const uint32_t n_lights = s->gpu->dev.view.n_punctual;
    if (n_lights == 0u) return set_error("pt_punctual_probe: the world was built without punctual lights");
    if (which >= 2 && !s->gpu->dev.view.punctual_cdf) return set_error("pt_punctual_probe: which 2 and 3 need the light grid in effect (pt_scene_set_punctual_selection, then pt_world_build)");
    if (n == 0) return 0;
    if (!in || !out) return set_error("pt_punctual_probe: null buffer");
    if (which == 1)
        for (uint32_t i = 0; i < n; ++i) {
            const double k = in[4 * (size_t)i];
            if (!(k >= 0.0 && k < (double)n_lights) || k != std::floor(k)) return set_error("pt_punctual_probe: which 1 takes (k, point.xyz) rows with k a light of the built list");
        }
    if (which == 3)
        for (uint32_t i = 0; i < n; ++i) {
            const double c = in[2 * (size_t)i], k = in[2 * (size_t)i + 1];
            if (!(c >= 0.0 && c < (double)s->grid_built.cells) || c != std::floor(c) || !(k >= 0.0 && k < (double)n_lights) || k != std::floor(k))
                return set_error("pt_punctual_probe: which 3 takes (cell, k) rows with a cell of the built grid and k a light of the built list");
        }
    static const size_t IN_COLS[4] = {3, 4, 3, 2}, OUT_COLS[4] = {9, 7, 11, 1};
    const size_t n_in = (size_t)n * IN_COLS[which], n_out = (size_t)n * OUT_COLS[which];
    return run_probe(s->ctx, {{in, n_in * sizeof(double)}}, out, n_out * sizeof(double), [&](void* const* d_in, void* d_out) {
        launch_punctual_probe(s->gpu->dev.view, which, (const double*)d_in[0], n, (double*)d_out, s->ctx->stream);
    });
}

extern "C" int pt_dispersion_probe(pt_scene* s, int glass_mat, int which, uint64_t seed, const double* in, uint32_t n, double* out) {
    if (!s || !s->ctx) return set_error("pt_dispersion_probe: null scene");
    if (glass_mat < 0 || (size_t)glass_mat >= s->mats.size() || s->mats[glass_mat].kind != MAT_GLASS || s->mats[glass_mat].p[3] == 0.0)
        return set_error("pt_dispersion_probe: not a dispersive glass material (pt_mat_glass_set_dispersion)");
    if (which != 0 && which != 1) return set_error("pt_dispersion_probe: which must be 0 or 1");
    if (n == 0) return 0;
    if (!in || !out) return set_error("pt_dispersion_probe: null buffer");
    if (which == 0)
        for (size_t i = 0; i < 2 * (size_t)n; ++i)
            if (!(in[i] >= 0.0 && in[i] <= 4294967295.0) || in[i] != std::floor(in[i])) return set_error("pt_dispersion_probe: which 0 takes (pixel, sample) pairs of 32-bit unsigned integers");
    const size_t n_in = (size_t)n * (which == 0 ? 2 : 1), n_out = (size_t)n * (which == 0 ? 7 : 1);
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    const double* d_w = dispersion_table(s, ctx->stream);
    if (!d_w) return -1;
    const MatD& m = s->mats[glass_mat];
    return run_probe(ctx, {{in, n_in * sizeof(double)}}, out, n_out * sizeof(double), [&](void* const* d_in, void* d_out) {
        launch_dispersion_probe(s->sampler, which, seed, m.ior, m.p[1], m.p[2], d_w, (const double*)d_in[0], n, (double*)d_out, ctx->stream);
    });
}

extern "C" int pt_camera_probe(pt_scene* s, const pt_camera* cam, uint64_t seed, const double* in, uint32_t n, double* out) {
    if (!s || !s->ctx) return set_error("pt_camera_probe: null scene");
    if (!cam) return set_error("pt_camera_probe: null camera");
    CamD dc;
    if (make_camd(s, cam, dc) != 0) return -1;
    const uint64_t n_pixels = (uint64_t)dc.width * dc.height;
    if (n_pixels > 0x7FFFFFFFull) return set_error("pt_camera_probe: bad image size");
    if (n == 0) return 0;
    if (!in || !out) return set_error("pt_camera_probe: null buffer");
    for (uint32_t i = 0; i < n; ++i) {
        const double p = in[2 * (size_t)i], sm = in[2 * (size_t)i + 1];
        if (!(p >= 0.0 && p < (double)n_pixels) || p != std::floor(p) || !(sm >= 0.0 && sm <= 4294967295.0) || sm != std::floor(sm))
            return set_error("pt_camera_probe: takes (pixel, sample) pairs: pixel < width * height, sample a 32-bit unsigned integer");
    }
    return run_probe(s->ctx, {{in, (size_t)n * 2 * sizeof(double)}}, out, (size_t)n * 8 * sizeof(double), [&](void* const* d_in, void* d_out) {
        launch_camera_probe(dc, s->sampler, seed, (const double*)d_in[0], n, (double*)d_out, s->ctx->stream, s->built && s->motion_on());
    });
}

extern "C" int pt_sampler_probe(pt_ctx* ctx, int kind, uint64_t seed, uint32_t pixel, uint32_t sample_begin, uint32_t n_samples, uint32_t draw_begin,
                                uint32_t n_draws, uint64_t* out) {
    if (!ctx) return set_error("pt_sampler_probe: null context");
    if (kind != 0 && kind != 1) return set_error("pt_sampler_probe: kind must be 0 (independent) or 1 (Sobol)");
    const uint64_t n = (uint64_t)n_samples * n_draws;
    if (n == 0) return 0;
    if (!out || n > (1ull << 28)) return set_error("pt_sampler_probe: null output or more than 2^28 values");
    return run_probe(ctx, {}, out, n * sizeof(uint64_t), [&](void* const*, void* d_out) {
        launch_sampler_probe(kind, seed, pixel, sample_begin, n_samples, draw_begin, n_draws, (uint64_t*)d_out, ctx->stream);
    });
}

extern "C" int pt_math_probe(pt_ctx* ctx, int which, const double* in, uint32_t n, double* out) {
    if (!ctx) return set_error("pt_math_probe: null context");
    return run_probe(ctx, {{in, (size_t)n * 2 * sizeof(double)}}, out, (size_t)n * sizeof(double), [&](void* const* d_in, void* d_out) {
        launch_math_probe(which, (const double*)d_in[0], n, (double*)d_out, ctx->stream);
    });
}
