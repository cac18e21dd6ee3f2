// The physical sky (include/pt_amd.h has the rule): a stage of its own that produces a float lat-long map. The render
// kernels never see it: pt_tex_sky hands the baked map to pt_tex_image_rgbf32, and from there it is an environment texture like any other.
//   k_sky_count : the disc's 8 x 8 sub-direction counts n_ij, only for the texels of the disc's window (a rectangle of rows and columns
//                 that wraps in phi and spans whole rows when the disc reaches a pole); the counts go to a window-sized byte table and are
//                 added into one uint32 counter per row — integer atomics, so the sums do not depend on the order of arrival.
//   k_sky_bake  : one lane per texel: sky_radiance (pt_sky.h) at the texel's centre plus the disc's radiance times n_ij / 64.
//   k_sky_probe : sky_radiance on given directions.
// Between the two launches of a bake the host forms the disc's solid angle from the row counters, in row order. No floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_scene_gpu.h"
#include "pt_sky.h"

using namespace pt;

namespace pt {
namespace {

constexpr int SBLOCK = 256;

// The disc's window: rows [j0, j0 + nr), columns i0, i0 + 1, ... (nc of them, modulo W). fb: no sub-direction of any texel fell inside
// the disc, so texel (fb_i, fb_j) — the one sample_environment reads for the sun's direction — carries all of it (n = 64).
struct SkyWin {
    uint32_t w, h;
    uint32_t j0, nr, i0, nc;
    uint32_t fb, fb_i, fb_j;
};

__global__ __launch_bounds__(SBLOCK) void k_sky_count(SkyParams P, SkyWin Wn, uint8_t* cnt, uint32_t* rows) {
    const uint32_t k = blockIdx.x * SBLOCK + threadIdx.x;
    if (k >= Wn.nr * Wn.nc) return;
    const uint32_t r = k / Wn.nc, ci = k - r * Wn.nc;
    const uint32_t j = Wn.j0 + r;
    uint32_t i = Wn.i0 + ci;
    if (i >= Wn.w) i -= Wn.w;
    double cp[8], sp[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const double phi = -SKY_PI + ((2.0 * SKY_PI) * ((double)i + ((double)b + 0.5) / 8.0)) / (double)Wn.w;
        detmath::sincos(phi, sp[b], cp[b]);
    }
    uint32_t n = 0;
    for (int a = 0; a < 8; ++a) {
        const double theta = (((double)j + ((double)a + 0.5) / 8.0) * SKY_PI) / (double)Wn.h;
        double st, ct;
        detmath::sincos(theta, st, ct);
#pragma unroll
        for (int b = 0; b < 8; ++b) n += sky_dot(P.s, st * cp[b], ct, st * sp[b]) >= P.cos_alpha ? 1u : 0u;
    }
    cnt[k] = (uint8_t)n;
    if (n) atomicAdd(rows + j, n);
}

__global__ __launch_bounds__(SBLOCK) void k_sky_bake(SkyParams P, SkyWin Wn, const uint8_t* cnt, float* out) {
    const uint32_t k = blockIdx.x * SBLOCK + threadIdx.x;
    if (k >= Wn.w * Wn.h) return;
    const uint32_t j = k / Wn.w, i = k - j * Wn.w;
    const double theta = (((double)j + 0.5) * SKY_PI) / (double)Wn.h;
    const double phi = -SKY_PI + ((2.0 * SKY_PI) * ((double)i + 0.5)) / (double)Wn.w;
    double st, ct, sp, cp;
    detmath::sincos(theta, st, ct);
    detmath::sincos(phi, sp, cp);
    double c[3];
    sky_radiance(P, st * cp, ct, st * sp, c);
    uint32_t n = 0;
    if (j - Wn.j0 < Wn.nr) {   // (unsigned: rows above j0 wrap to huge values)
        const uint32_t ci = i >= Wn.i0 ? i - Wn.i0 : i + Wn.w - Wn.i0;
        if (ci < Wn.nc) n = cnt[(size_t)(j - Wn.j0) * Wn.nc + ci];
    }
    if (Wn.fb && i == Wn.fb_i && j == Wn.fb_j) n = 64u;
    if (n) {
        const double f = (double)n / 64.0;
        c[0] = c[0] + P.l_sun[0] * f;
        c[1] = c[1] + P.l_sun[1] * f;
        c[2] = c[2] + P.l_sun[2] * f;
    }
    float* o = out + (size_t)k * 3;
    o[0] = (float)c[0]; o[1] = (float)c[1]; o[2] = (float)c[2];
}

__global__ __launch_bounds__(SBLOCK) void k_sky_probe(SkyParams P, const double* dirs, uint32_t n, double* out) {
    for (uint32_t k = blockIdx.x * SBLOCK + threadIdx.x; k < n; k += gridDim.x * SBLOCK) {
        const double* d = dirs + 3 * (size_t)k;
        double c[3];
        sky_radiance(P, d[0], d[1], d[2], c);
        double* o = out + 3 * (size_t)k;
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    }
}

pt_sky_opts sky_defaults() {
    pt_sky_opts o;
    memset(&o, 0, sizeof o);
    o.sun_dir[1] = 1.0;
    o.turbidity = 3.0;
    o.ground_albedo[0] = o.ground_albedo[1] = o.ground_albedo[2] = 0.3;
    o.sun_radius_deg = 0.2665;
    o.sun_scale = 1.0;
    o.scale = 0.04;
    return o;
}

// Everything of the rule that does not depend on the direction. e_sun: the sun's irradiance E_sun (klx, before sun_scale and scale).
struct SkySetup {
    SkyParams P;
    double e_sun[3];
    double irr[3];   // scale * sun_scale * E_sun: pt_sky_sun_irradiance's answer
};

void sky_setup(const pt_sky_opts& o, SkySetup& S) {
    SkyParams& P = S.P;
    const double T = o.turbidity;
    // s = v' / |v'| with v' = sun_dir / its largest |component| (no overflow for any finite length)
    double m = std::fmax(std::fabs(o.sun_dir[0]), std::fmax(std::fabs(o.sun_dir[1]), std::fabs(o.sun_dir[2])));
    const double v[3] = {o.sun_dir[0] / m, o.sun_dir[1] / m, o.sun_dir[2] / m};
    const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int c = 0; c < 3; ++c) P.s[c] = v[c] / len;
    const double sy = P.s[1];
    const double cs = sy < 0.0 ? 0.0 : (sy > 1.0 ? 1.0 : sy);
    const double ts = detmath::acos(cs);
    static const double K[3][5][2] = {
        {{0.1787, -1.4630}, {-0.3554, 0.4275}, {-0.0227, 5.3251}, {0.1206, -2.5771}, {-0.0670, 0.3703}},
        {{-0.0193, -0.2592}, {-0.0665, 0.0008}, {-0.0004, 0.2125}, {-0.0641, -0.8989}, {-0.0033, 0.0452}},
        {{-0.0167, -0.2608}, {-0.0950, 0.0092}, {-0.0079, 0.2102}, {-0.0441, -1.6537}, {-0.0109, 0.0529}}};
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < 5; ++k) P.coef[q][k] = K[q][k][0] * T + K[q][k][1];
    // zenith values
    const double chi = (4.0 / 9.0 - T / 120.0) * (SKY_PI - 2.0 * ts);
    double sc, cc;
    detmath::sincos(chi, sc, cc);
    P.zen[0] = ((4.0453 * T - 4.9710) * (sc / cc) - 0.2155 * T) + 2.4192;
    static const double M[2][3][4] = {{{0.00166, -0.00375, 0.00209, 0.0}, {-0.02903, 0.06377, -0.03202, 0.00394}, {0.11693, -0.21196, 0.06052, 0.25886}},
                                      {{0.00275, -0.00610, 0.00317, 0.0}, {-0.04214, 0.08970, -0.04153, 0.00516}, {0.15346, -0.26756, 0.06670, 0.26688}}};
    const double t2 = ts * ts, t3 = t2 * ts;
    for (int q = 0; q < 2; ++q) {
        double p[3];
        for (int r = 0; r < 3; ++r) p[r] = ((M[q][r][0] * t3 + M[q][r][1] * t2) + M[q][r][2] * ts) + M[q][r][3];
        P.zen[1 + q] = ((T * T) * p[0] + T * p[1]) + p[2];
    }
    for (int q = 0; q < 3; ++q) P.den[q] = sky_perez(P.coef[q], 1.0, ts, cs);
    P.scale = o.scale;
    const double alpha = (o.sun_radius_deg * SKY_PI) / 180.0;
    P.cos_alpha = detmath::cos(alpha);
    // the sun's irradiance: Rayleigh and Angstrom extinction only
    for (int c = 0; c < 3; ++c) S.e_sun[c] = 0.0;
    if (sy > 0.0) {
        const double mass = 1.0 / (sy + 0.15 * detmath::pow(93.885 - (ts * 180.0) / SKY_PI, -1.253));
        const double beta = 0.04608 * T - 0.04586;
        static const double LAMBDA[3] = {0.610, 0.550, 0.465};
        for (int c = 0; c < 3; ++c) {
            const double tau = 0.008735 * detmath::pow(LAMBDA[c], -4.08) + beta * detmath::pow(LAMBDA[c], -1.3);
            S.e_sun[c] = 127.5 * detmath::exp(-(tau * mass));
        }
    }
    for (int c = 0; c < 3; ++c) S.irr[c] = (o.scale * o.sun_scale) * S.e_sun[c];
    // the ground: a Lambertian plane under this sky. E_sky by a fixed 16 x 64 midpoint quadrature of the unscaled sky.
    for (int c = 0; c < 3; ++c) P.ground[c] = P.l_sun[c] = 0.0;
    P.scale = 1.0;
    double e_sky[3] = {0.0, 0.0, 0.0};
    const double dphi = (2.0 * SKY_PI) / 64.0;
    for (int a = 0; a < 16; ++a) {
        double st, ct, s0, c0, s1, c1;
        detmath::sincos((((double)a + 0.5) * (SKY_PI / 2.0)) / 16.0, st, ct);
        detmath::sincos(((double)a * (SKY_PI / 2.0)) / 16.0, s0, c0);
        detmath::sincos(((double)(a + 1) * (SKY_PI / 2.0)) / 16.0, s1, c1);
        const double wgt = (ct * (c0 - c1)) * dphi;
        for (int b = 0; b < 64; ++b) {
            double sp, cp, L[3];
            detmath::sincos(-SKY_PI + ((2.0 * SKY_PI) * ((double)b + 0.5)) / 64.0, sp, cp);
            sky_radiance(P, st * cp, ct, st * sp, L);
            for (int c = 0; c < 3; ++c) e_sky[c] = e_sky[c] + L[c] * wgt;
        }
    }
    P.scale = o.scale;
    const double up = sy > 0.0 ? sy : 0.0;
    for (int c = 0; c < 3; ++c) P.ground[c] = ((o.scale * o.ground_albedo[c]) * (e_sky[c] + (o.sun_scale * S.e_sun[c]) * up)) / SKY_PI;
}

// c_j = cos((j pi) / H), as pt_envmap.h forms it
double row_cos(uint32_t j, uint32_t h) {
    double s, c;
    detmath::sincos(((double)j * SKY_PI) / (double)h, s, c);
    return c;
}

// The texel sample_environment reads for direction d (pt_envmap.h env_texel_of, on the host)
void texel_of(uint32_t w, uint32_t h, const double* d, uint32_t& i, uint32_t& j) {
    auto clamp01 = [](double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); };
    auto as_u32 = [](double x) { return (x != x || x <= 0.0) ? 0u : (x >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)x); };
    const double theta = detmath::acos(d[1]);
    const double phi = detmath::atan2(d[2], d[0]);
    const double u = clamp01((phi + SKY_PI) / (2.0 * SKY_PI));
    const double v = 1.0 - clamp01(1.0 - theta / SKY_PI);
    i = as_u32(u * (double)w);
    j = as_u32(v * (double)h);
    if (i > w - 1) i = w - 1;
    if (j > h - 1) j = h - 1;
}

// A window that contains every texel with a sub-direction inside the disc, padded by a row and a column on each side (libm is good
// enough here: the counts do not depend on the window as long as it covers the disc).
void disc_window(const SkyParams& P, double alpha, SkyWin& Wn) {
    const uint32_t W = Wn.w, H = Wn.h;
    const double tc = std::acos(std::fmin(1.0, std::fmax(-1.0, P.s[1])));
    const double tlo = tc - alpha - SKY_PI / (double)H, thi = tc + alpha + SKY_PI / (double)H;
    const uint32_t j0 = tlo <= 0.0 ? 0u : std::min(H - 1, (uint32_t)std::floor(tlo / SKY_PI * (double)H));
    const uint32_t j1 = thi >= SKY_PI ? H - 1 : std::min(H - 1, (uint32_t)std::floor(thi / SKY_PI * (double)H));
    Wn.j0 = j0;
    Wn.nr = j1 - j0 + 1;
    Wn.i0 = 0;
    Wn.nc = W;   // whole rows unless the cap stays clear of both poles and is narrower than the map
    const double margin = 1e-6;
    if (tc - alpha > margin && tc + alpha < SKY_PI - margin) {
        const double sd = std::sin(alpha) / std::sin(tc);
        if (sd < 1.0 - margin) {
            const double dphi = std::asin(sd) + (2.0 * SKY_PI) / (double)W + margin;
            const double pc = std::atan2(P.s[2], P.s[0]);
            const double lo = std::floor((pc - dphi + SKY_PI) / (2.0 * SKY_PI) * (double)W);
            const double hi = std::floor((pc + dphi + SKY_PI) / (2.0 * SKY_PI) * (double)W);
            const double nc = hi - lo + 1.0;
            if (nc < (double)W) {
                const double i0 = lo - std::floor(lo / (double)W) * (double)W;   // lo mod W, in [0, W)
                Wn.i0 = std::min(W - 1, (uint32_t)i0);
                Wn.nc = (uint32_t)nc;
            }
        }
    }
}

int check_opts(const pt_sky_opts& o, const char* who) {
    const std::string p = std::string(who) + ": ";
    double l2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(o.sun_dir[c])) return set_error(p + "sun_dir must be finite");
        l2 = std::fmax(l2, std::fabs(o.sun_dir[c]));
    }
    if (!(l2 > 0.0)) return set_error(p + "sun_dir must have a length above 0");
    if (!(o.turbidity >= 1.7 && o.turbidity <= 10.0)) return set_error(p + "turbidity must be in [1.7, 10]");
    for (int c = 0; c < 3; ++c)
        if (!(o.ground_albedo[c] >= 0.0 && o.ground_albedo[c] <= 1.0)) return set_error(p + "each ground_albedo channel must be in [0, 1]");
    if (!(o.sun_radius_deg > 0.0 && o.sun_radius_deg <= 10.0)) return set_error(p + "sun_radius_deg must be above 0 and at most 10");
    if (!(o.sun_scale >= 0.0) || !std::isfinite(o.sun_scale)) return set_error(p + "sun_scale must be finite and >= 0");
    if (!(o.scale > 0.0) || !std::isfinite(o.scale)) return set_error(p + "scale must be finite and > 0");
    return 0;
}

uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + SBLOCK - 1) / SBLOCK); }

}  // namespace
}  // namespace pt

extern "C" int pt_sky_opts_default(pt_sky_opts* o) {
    if (!o) return set_error("pt_sky_opts_default: null options");
    *o = sky_defaults();
    return 0;
}
extern "C" int pt_sky_opts_check(const pt_sky_opts* opts) { return check_opts(opts ? *opts : sky_defaults(), "pt_sky_opts_check"); }

extern "C" int pt_sky_eval(const pt_sky_opts* opts, const double* dirs, uint32_t n, double* out_rgb) {
    const pt_sky_opts o = opts ? *opts : sky_defaults();
    if (check_opts(o, "pt_sky_eval") != 0) return -1;
    if (n == 0) return 0;
    if (!dirs || !out_rgb) return set_error("pt_sky_eval: null buffer");
    SkySetup S;
    sky_setup(o, S);
    for (uint32_t k = 0; k < n; ++k) sky_radiance(S.P, dirs[3 * (size_t)k], dirs[3 * (size_t)k + 1], dirs[3 * (size_t)k + 2], out_rgb + 3 * (size_t)k);
    return 0;
}

extern "C" int pt_sky_sun_irradiance(const pt_sky_opts* opts, double out[3]) {
    const pt_sky_opts o = opts ? *opts : sky_defaults();
    if (check_opts(o, "pt_sky_sun_irradiance") != 0) return -1;
    if (!out) return set_error("pt_sky_sun_irradiance: null buffer");
    SkySetup S;
    sky_setup(o, S);
    for (int c = 0; c < 3; ++c) out[c] = S.irr[c];
    return 0;
}

extern "C" int pt_sky_probe(pt_ctx* ctx, const pt_sky_opts* opts, const double* dirs, uint32_t n, double* out_rgb) {
    if (!ctx) return set_error("pt_sky_probe: null context");
    const pt_sky_opts o = opts ? *opts : sky_defaults();
    if (check_opts(o, "pt_sky_probe") != 0) return -1;
    if (n == 0) return 0;
    if (!dirs || !out_rgb) return set_error("pt_sky_probe: null buffer");
    SkySetup S;
    sky_setup(o, S);
    return run_probe(ctx, {{dirs, (size_t)n * 3 * sizeof(double)}}, out_rgb, (size_t)n * 3 * sizeof(double), [&](void* const* d_in, void* d_out) {
        uint32_t blocks = blocks_for(n);
        if (blocks > 2048u) blocks = 2048u;
        hipLaunchKernelGGL(k_sky_probe, dim3(blocks), dim3(SBLOCK), 0, ctx->stream, S.P, (const double*)d_in[0], n, (double*)d_out);
    });
}

extern "C" int pt_sky_bake(pt_ctx* ctx, const pt_sky_opts* opts, uint32_t w, uint32_t h, float* rgb, int rgb_on_device) {
    if (!ctx) return set_error("pt_sky_bake: null context");
    const pt_sky_opts o = opts ? *opts : sky_defaults();
    if (check_opts(o, "pt_sky_bake") != 0) return -1;
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 26)) return set_error("pt_sky_bake: width and height must be positive with width * height <= 2^26");
    if (!rgb) return set_error("pt_sky_bake: null buffer");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = ctx->stream;
    SkySetup S;
    sky_setup(o, S);
    SkyWin Wn;
    memset(&Wn, 0, sizeof Wn);
    Wn.w = w;
    Wn.h = h;
    const bool disc = o.sun_scale > 0.0 && (S.e_sun[0] > 0.0 || S.e_sun[1] > 0.0 || S.e_sun[2] > 0.0);
    DevMem d_cnt, d_rows, d_out;
    if (disc) {
        disc_window(S.P, (o.sun_radius_deg * SKY_PI) / 180.0, Wn);
        const size_t n_win = (size_t)Wn.nr * Wn.nc;
        std::vector<uint32_t> rows(h);
        if (!d_cnt.alloc(n_win, "hipMalloc(sky counts)") || !d_rows.alloc((size_t)h * sizeof(uint32_t), "hipMalloc(sky rows)")) return -1;
        if (!hip_ok(hipMemsetAsync(d_rows.as<void>(), 0, (size_t)h * sizeof(uint32_t), st), "hipMemset(sky rows)")) return -1;
        hipLaunchKernelGGL(k_sky_count, dim3(blocks_for(n_win)), dim3(SBLOCK), 0, st, S.P, Wn, d_cnt.as<uint8_t>(), d_rows.as<uint32_t>());
        const bool ok = hip_ok(hipGetLastError(), "kernel launch") &&
                        hip_ok(hipMemcpyAsync(rows.data(), d_rows.as<void>(), (size_t)h * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "hipMemcpy(sky rows)");
        if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(sky count)") || !ok) return -1;
        uint64_t total = 0;
        for (uint32_t j = 0; j < h; ++j) total += rows[j];
        if (total == 0) {   // the disc slipped between the sub-directions: its texel carries all of it
            texel_of(w, h, S.P.s, Wn.fb_i, Wn.fb_j);
            Wn.fb = 1u;
            Wn.nr = Wn.nc = 0u;
            rows[Wn.fb_j] = 64u;
        }
        // Omega = sum_j ((sum_i n_ij) / 64) * (c_j - c_{j+1}) * ((2 pi) / W), rows in order
        const double dphi = (2.0 * SKY_PI) / (double)w;
        double omega = 0.0;
        for (uint32_t j = 0; j < h; ++j)
            if (rows[j]) omega = omega + (((double)rows[j] / 64.0) * (row_cos(j, h) - row_cos(j + 1, h))) * dphi;
        if (!(omega > 0.0)) return set_error("pt_sky_bake: the disc has no solid angle in this map");
        for (int c = 0; c < 3; ++c) S.P.l_sun[c] = S.irr[c] / omega;
    }
    const size_t n_out = (size_t)w * h * 3;
    float* d_rgb = rgb;
    if (!rgb_on_device) {
        if (!d_out.alloc(n_out * sizeof(float), "hipMalloc(sky map)")) return -1;
        d_rgb = d_out.as<float>();
    }
    hipLaunchKernelGGL(k_sky_bake, dim3(blocks_for((uint64_t)w * h)), dim3(SBLOCK), 0, st, S.P, Wn, (const uint8_t*)d_cnt.as<uint8_t>(), d_rgb);
    bool ok = hip_ok(hipGetLastError(), "kernel launch");
    if (ok && !rgb_on_device) ok = hip_ok(hipMemcpyAsync(rgb, d_rgb, n_out * sizeof(float), hipMemcpyDeviceToHost, st), "hipMemcpy(sky map)");
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(sky bake)") && ok ? 0 : -1;
}

extern "C" int pt_tex_sky(pt_scene* s, const pt_sky_opts* opts, uint32_t w, uint32_t h) {
    if (!s || !s->ctx) return set_error("pt_tex_sky: null scene");
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 26)) return set_error("pt_tex_sky: width and height must be positive with width * height <= 2^26");
    std::vector<float> map((size_t)w * h * 3);
    if (pt_sky_bake(s->ctx, opts, w, h, map.data(), 0) != 0) return -1;
    return pt_tex_image_rgbf32(s, w, h, map.data());
}
