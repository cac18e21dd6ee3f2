// Environment importance sampling (the rule in include/pt_amd.h): the device functions that k_shade's ENV forms,
// the table builder and the probe of pt_envmap.hip share. The distribution is over the W x H texels of the camera's environment
// texture, texel (i, j) weighted by its luminance times its solid angle; within a texel, directions are uniform in (cos theta, phi),
// i.e. uniform in solid angle, so the density is lum_ij / Z per steradian. Texel (i, j) is the one sample_environment reads:
// row j covers theta in [j pi / H, (j + 1) pi / H), column i covers phi in [-pi + 2 pi i / W, -pi + 2 pi (i + 1) / W).
#pragma once
#include "pt_dev_bsdf.h"

namespace pt {

// lum_ij: the luminance of the texel value exactly as tex_image returns it (RGB8 times 1/255, or f32 widened), negative or NaN -> 0
PT_DEV double env_texel_lum(const SceneD& sc, const TexD& T, uint32_t i, uint32_t j) {
    V3 c;
    if (T.kind == TEX_IMAGE_F32) {
        const float* q = sc.atlas_f + T.ofs + ((size_t)j * T.w + i) * 3;
        c = V3{(double)q[0], (double)q[1], (double)q[2]};
    } else {
        const uint8_t* p = sc.atlas + T.ofs + ((size_t)j * T.w + i) * 3;
        const double s = 1.0 / 255.0;
        c = V3{s * (double)p[0], s * (double)p[1], s * (double)p[2]};
    }
    return fmax(luminance(c), 0.0);
}
// c_j = cos(j pi / H)
PT_DEV double env_row_cos(uint32_t j, uint32_t h) { return dev_sincos((double)j * D_PI / (double)h).c; }

// The texel sample_environment (pt_dev_geom.h) reads for direction d: its acos / atan2 and tex_image's clamp and Q6 rule.
PT_DEV void env_texel_of(const TexD& T, V3 d, uint32_t& i, uint32_t& j) {
    double theta = dev_acos(d.y);
    double phi = dev_atan2(d.z, d.x);
    double u = (phi + D_PI) / (2.0 * D_PI);
    double v = 1.0 - theta / D_PI;
    u = clampd(u, 0.0, 1.0);
    v = 1.0 - clampd(v, 0.0, 1.0);
    i = f64_as_u32(u * (double)T.w);
    j = f64_as_u32(v * (double)T.h);
    if (i > T.w - 1) i = T.w - 1;
    if (j > T.h - 1) j = T.h - 1;
}
// env_pdf(d) = lum(texel(d)) / Z, per steradian
PT_DEV double env_pdf(const SceneD& sc, const TexD& T, const EnvTabD& e, V3 d) {
    uint32_t i, j;
    env_texel_of(T, d, i, j);
    return env_texel_lum(sc, T, i, j) / e.z;
}
// smallest k in [0, n) with x < p[k + 1], for x < p[n] (p: n + 1 non-decreasing prefix sums, p[0] = 0 <= x)
PT_DEV uint32_t env_search(const double* p, uint32_t n, double x) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (x < p[mid + 1]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// Two draws u1, u2 in [0, 1) -> direction d and its density (the chosen texel's lum / Z). A draw that rounds onto the total
// (u * total == total) is taken as the largest double below it. The texel found has a non-zero weight.
PT_DEV V3 env_sample(const SceneD& sc, const TexD& T, const EnvTabD& e, double u1, double u2, double& pdf) {
    const uint32_t W = e.w, H = e.h;
    double x = u1 * e.z;
    if (!(x < e.z)) x = nextafter(e.z, 0.0);
    const uint32_t j = env_search(e.row, H, x);
    const double t1 = (x - e.row[j]) / (e.row[j + 1] - e.row[j]);
    const double c0 = env_row_cos(j, H), c1 = env_row_cos(j + 1, H);
    const double cos_t = c0 - t1 * (c0 - c1);
    const double* p = e.col + (size_t)j * (W + 1);
    const double r = p[W];
    double y = u2 * r;
    if (!(y < r)) y = nextafter(r, 0.0);
    const uint32_t i = env_search(p, W, y);
    const double t2 = (y - p[i]) / (p[i + 1] - p[i]);
    const double phi = -D_PI + (2.0 * D_PI) * ((double)i + t2) / (double)W;
    const double sin_t = sqrt(fmax(0.0, 1.0 - cos_t * cos_t));
    const SinCos sp = dev_sincos(phi);
    pdf = env_texel_lum(sc, T, i, j) / e.z;
    return V3{sin_t * sp.c, cos_t, sin_t * sp.s};
}

// The density of mat_sample's MAT_METAL direction l (local frame, view v): ggx_sample_microfacet_normal draws visible normals of
// GGX with alpha_s = roughness^2 (Q2: the pdf/eval of metal.rs use alpha = roughness), reflected: G1_s(v) D_s(h) / (4 v.z) for
// l.z > 0 (below, the sampler returns None). Used by the ENV mixture for metal (pt_amd.h): metal's pdf is not its sampler's density.
PT_DEV double metal_sample_density(V3 v, V3 l, double rough) {
    if (!(v.z > 0.0) || !(l.z > 0.0)) return 0.0;
    const V3 h = normalize(v + l);
    if (!(dot(v, h) > 0.0)) return 0.0;
    const double a = rough * rough, a2 = a * a;
    const double den = (a2 - 1.0) * (h.z * h.z) + 1.0;
    const double d = a2 / (D_PI * den * den);
    const double g1 = 2.0 * v.z / (v.z + sqrt(v.z * v.z * (1.0 - a2) + a2));
    return g1 * d / (4.0 * v.z);
}
constexpr double ENV_METAL_MIN_ROUGHNESS = 0.05;   // pt_amd.h: metal below this roughness stays out of the env set E
// The env set E (pt_amd.h): diffuse, and metal with roughness >= ENV_METAL_MIN_ROUGHNESS seen from the front of its shading frame
PT_DEV bool env_in_set(const MatD& m, const TexVals& tv, const LocalFrame& lf) {
    return m.kind == MAT_DIFFUSE || (m.kind == MAT_METAL && tv.rough >= ENV_METAL_MIN_ROUGHNESS && lf.v.z > 0.0);
}

}  // namespace pt
