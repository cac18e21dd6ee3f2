// Scene builder + flattener + BVH builder (host). See pt_scene.h.
#include "pt_scene.h"
#include "pt_bvh_device.h"
#include "pt_detmath.h"
#include "pt_dev_punctual.h"
#include "pt_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "../../include/pt_amd.h"

using namespace pt;
using namespace pt::host;

namespace pt {
static thread_local std::string g_error;
int set_error(const std::string& msg) {
    g_error = msg;
    return -1;
}
const char* last_error() { return g_error.c_str(); }
bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
const char* exp_env(const char* name) {
    const char* on = getenv("PT_EXPERIMENT");
    return (on && on[0] == '1') ? getenv(name) : nullptr;
}
void DeviceBuffers::release() {
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    view = SceneD{};
}
}  // namespace pt

pt_scene::~pt_scene() {
    dev.release();   // (the cached buffers free themselves: pt_devmem.h GrowBuf)
    if (disp_w) (void)hipFree(disp_w);
    if (d_counters) (void)hipFree(d_counters);
    if (h_counters) (void)hipHostFree(h_counters);
}

#define TEX_RGB_OK(s, t) ((t) >= 0 && (size_t)(t) < (s)->tex.size() && (s)->tex[t].is_rgb)
#define TEX_F_OK(s, t) ((t) >= 0 && (size_t)(t) < (s)->tex.size() && !(s)->tex[t].is_rgb)
#define MAT_OK(s, m) ((m) >= 0 && (size_t)(m) < (s)->mats.size())
#define OBJ_OK(s, o) ((o) >= 0 && (size_t)(o) < (s)->objs.size())

static int push_tex(pt_scene* s, HostTex&& t) {
    s->tex.push_back(std::move(t));
    s->built = false;
    return (int)s->tex.size() - 1;
}
extern "C" int pt_tex_solid_rgb(pt_scene* s, double r, double g, double b) {
    HostTex t;
    t.d.kind = TEX_SOLID_RGB;
    t.d.v[0] = r; t.d.v[1] = g; t.d.v[2] = b;
    t.is_rgb = true;
    return push_tex(s, std::move(t));
}
extern "C" int pt_tex_solid_f(pt_scene* s, double v) {
    HostTex t;
    t.d.kind = TEX_SOLID_F;
    t.d.v[0] = v;
    return push_tex(s, std::move(t));
}
extern "C" int pt_tex_checker(pt_scene* s, double scale, int t1, int t2) {
    if (!((TEX_RGB_OK(s, t1) && TEX_RGB_OK(s, t2)) || (TEX_F_OK(s, t1) && TEX_F_OK(s, t2))))
        return set_error("pt_tex_checker: both child textures must exist and have the same value type");
    HostTex t;
    t.d.kind = TEX_CHECKER;
    t.d.t1 = (uint32_t)t1; t.d.t2 = (uint32_t)t2;
    t.d.inv_scale = 1.0 / scale;   // scale.recip() texture.rs:36
    t.is_rgb = s->tex[t1].is_rgb;
    return push_tex(s, std::move(t));
}
extern "C" int pt_tex_image_rgb8(pt_scene* s, uint32_t w, uint32_t h, const uint8_t* rgb) {
    if (!rgb && w != 0 && h != 0) return set_error("pt_tex_image_rgb8: null pixels");
    HostTex t;
    t.d.kind = TEX_IMAGE;
    t.d.w = w; t.d.h = h;
    t.image.assign(rgb, rgb + (size_t)w * h * 3);
    t.is_rgb = true;
    return push_tex(s, std::move(t));
}
extern "C" int pt_tex_image_rgbf32(pt_scene* s, uint32_t w, uint32_t h, const float* rgb) {
    if (!rgb && w != 0 && h != 0) return set_error("pt_tex_image_rgbf32: null pixels");
    HostTex t;
    t.d.kind = TEX_IMAGE_F32;
    t.d.w = w; t.d.h = h;
    t.image_f.assign(rgb, rgb + (size_t)w * h * 3);
    t.is_rgb = true;
    return push_tex(s, std::move(t));
}
extern "C" int pt_scene_set_float_hdr(pt_scene* s, int on) {
    if (!s) return set_error("pt_scene_set_float_hdr: null scene");
    s->float_hdr = on != 0;
    return 0;
}
extern "C" int pt_scene_float_hdr(pt_scene* s) { return s && s->float_hdr ? 1 : 0; }
extern "C" int pt_scene_set_env_sampling(pt_scene* s, double f) {
    if (!s) return set_error("pt_scene_set_env_sampling: null scene");
    if (!(f >= 0.0 && f < 1.0)) return set_error("pt_scene_set_env_sampling: f must be finite and in [0, 1)");
    s->env_f = f;
    return 0;
}
extern "C" double pt_scene_env_sampling(pt_scene* s) { return s ? s->env_f : 0.0; }
extern "C" int pt_scene_set_sampler(pt_scene* s, int kind) {
    if (!s) return set_error("pt_scene_set_sampler: null scene");
    if (kind != 0 && kind != 1) return set_error("pt_scene_set_sampler: kind must be 0 (independent) or 1 (Sobol)");
    s->sampler = kind;
    return 0;
}
extern "C" int pt_scene_sampler(pt_scene* s) { return s ? s->sampler : 0; }
extern "C" int pt_scene_set_light_sampling(pt_scene* s, int kind) {
    if (!s) return set_error("pt_scene_set_light_sampling: null scene");
    if (kind != 0 && kind != 1) return set_error("pt_scene_set_light_sampling: kind must be 0 (reference) or 1 (exact)");
    s->light_sampling = kind;
    return 0;
}
extern "C" int pt_scene_light_sampling(pt_scene* s) { return s ? s->light_sampling : 0; }
extern "C" int pt_scene_set_projection(pt_scene* s, int kind) {
    if (!s) return set_error("pt_scene_set_projection: null scene");
    if (kind < 0 || kind > 3) return set_error("pt_scene_set_projection: kind must be 0 (perspective), 1 (orthographic), 2 (fisheye) or 3 (panorama)");
    s->projection = kind;
    return 0;
}
extern "C" int pt_scene_projection(pt_scene* s) { return s ? s->projection : 0; }
extern "C" int pt_register_image(pt_scene* s, const char* name, uint32_t w, uint32_t h, const uint8_t* rgb) {
    int t = pt_tex_image_rgb8(s, w, h, rgb);
    if (t < 0) return -1;
    s->images[name] = t;
    return 0;
}

static int push_mat(pt_scene* s, const MatD& m) {
    s->mats.push_back(m);
    s->built = false;
    return (int)s->mats.size() - 1;
}
static MatD blank_mat(uint32_t kind) {
    MatD m;
    memset(&m, 0, sizeof m);
    m.kind = kind;
    m.color_tex = m.rough_tex = m.nmap_tex = -1;
    return m;
}
extern "C" int pt_mat_diffuse(pt_scene* s, int color_tex, int nmap) {
    if (!TEX_RGB_OK(s, color_tex)) return set_error("pt_mat_diffuse: bad colour texture");
    MatD m = blank_mat(MAT_DIFFUSE);
    m.color_tex = color_tex;
    if (nmap >= 0) {
        if (!TEX_RGB_OK(s, nmap) || (s->tex[nmap].d.kind != TEX_IMAGE && s->tex[nmap].d.kind != TEX_IMAGE_F32)) return set_error("pt_mat_diffuse: normal map must be an image texture");
        m.nmap_tex = nmap;
    }
    return push_mat(s, m);
}
extern "C" int pt_mat_metal(pt_scene* s, int color_tex, int rough_tex) {
    if (!TEX_RGB_OK(s, color_tex) || !TEX_F_OK(s, rough_tex)) return set_error("pt_mat_metal: bad texture handle");
    MatD m = blank_mat(MAT_METAL);
    m.color_tex = color_tex;
    m.rough_tex = rough_tex;
    return push_mat(s, m);
}
extern "C" int pt_mat_glass(pt_scene* s, int color_tex, int rough_tex, double, double ior) {
    if (!TEX_RGB_OK(s, color_tex) || !TEX_F_OK(s, rough_tex)) return set_error("pt_mat_glass: bad texture handle");
    MatD m = blank_mat(MAT_GLASS);
    m.color_tex = color_tex;
    m.rough_tex = rough_tex;
    m.ior = ior;
    return push_mat(s, m);
}
extern "C" int pt_mat_principled(pt_scene* s, int color_tex, const double p[11]) {
    if (!TEX_RGB_OK(s, color_tex)) return set_error("pt_mat_principled: bad colour texture");
    MatD m = blank_mat(MAT_PRINCIPLED);
    m.color_tex = color_tex;
    for (int i = 0; i < 11; ++i) m.p[i] = p[i];
    m.ior = p[5];
    const double metallic = p[0], spec_trans = p[6], clearcoat = p[9], gloss = p[10];
    m.lobe_w[0] = (1.0 - metallic) * (1.0 - spec_trans);   // principled.rs:79-85
    m.lobe_w[1] = 1.0 - spec_trans * (1.0 - metallic);
    m.lobe_w[2] = spec_trans * (1.0 - metallic);
    m.lobe_w[3] = 0.25 * clearcoat;
    double inv_total = 1.0 / (m.lobe_w[0] + m.lobe_w[1] + m.lobe_w[2] + m.lobe_w[3]);   // :87-100
    for (int i = 0; i < 4; ++i) m.lobe_p[i] = m.lobe_w[i] * inv_total;
    m.alpha_g = (1.0 - gloss) * 0.1 + gloss * 0.001;       // :75-77
    return push_mat(s, m);
}
extern "C" int pt_mat_mix(pt_scene* s, double t, int m1, int m2) {   // MixBxDf::new mix.rs:14-20
    if (!MAT_OK(s, m1) || !MAT_OK(s, m2)) return set_error("pt_mat_mix: bad material handle");
    if (s->mats[m1].kind == MAT_MEDIUM || s->mats[m2].kind == MAT_MEDIUM) return set_error("pt_mat_mix: a medium cannot be mixed (it is a volume, not a BxDF)");
    for (int c : {m1, m2})   // (a mix child is never a glass with an interior, so neither is a child's child)
        if (s->mats[c].kind == MAT_GLASS && s->mats[c].p[0] != 0.0) return set_error("pt_mat_mix: a glass with an interior medium cannot be mixed");
    for (int c : {m1, m2})
        if (s->mats[c].kind == MAT_GLASS && s->mats[c].p[3] != 0.0) return set_error("pt_mat_mix: a dispersive glass cannot be mixed");
    // a child may be a mix (MixBxDf::new takes any Arc<dyn BxDFMaterial>, mix.rs:14-20) — of leaves: the kernels evaluate two levels
    for (int c : {m1, m2})
        if (s->mats[c].kind == MAT_MIX && (s->mats[s->mats[c].color_tex].kind == MAT_MIX || s->mats[s->mats[c].rough_tex].kind == MAT_MIX))
            return set_error("pt_mat_mix: MixBxDf nested deeper than two levels is not supported");
    MatD m = blank_mat(MAT_MIX);
    m.p[0] = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);   // t.clamp(0, 1)
    m.color_tex = m1;
    m.rough_tex = m2;
    return push_mat(s, m);
}
extern "C" int pt_mat_sheen(pt_scene* s, double r, double g, double b, double sheen_tint) {   // SheenBRDF::new sheen.rs:17-22
    MatD m = blank_mat(MAT_SHEEN);
    m.p[0] = r; m.p[1] = g; m.p[2] = b; m.p[3] = sheen_tint;
    return push_mat(s, m);
}
extern "C" int pt_mat_clearcoat(pt_scene* s, double clearcoat_gloss) {   // ClearcoatBRDF::new clearcoat.rs:14-18
    MatD m = blank_mat(MAT_CLEARCOAT);
    m.alpha_g = (1.0 - clearcoat_gloss) * 0.1 + clearcoat_gloss * 0.001;
    return push_mat(s, m);
}
// HomogeneousVolume of the reference's commented-out volume.rs, as a material: the object that carries it is the medium's boundary
extern "C" int pt_mat_medium(pt_scene* s, double density, double r, double g, double b, double hg_g) {
    if (!s) return set_error("pt_mat_medium: null scene");
    if (!(density > 0.0) || !std::isfinite(density)) return set_error("pt_mat_medium: density must be finite and > 0");
    for (double a : {r, g, b})
        if (!(a >= 0.0 && a <= 1.0)) return set_error("pt_mat_medium: each albedo channel must be in [0, 1]");
    if (!(std::fabs(hg_g) < 1.0)) return set_error("pt_mat_medium: |hg_g| must be below 1");
    if (s->mats.size() >= MEDIUM_MAX_MATS) return set_error("pt_mat_medium: a medium's material handle must be below 4094 (create media before other materials)");
    MatD m = blank_mat(MAT_MEDIUM);
    m.p[0] = density;
    m.p[1] = hg_g;
    m.p[2] = r; m.p[3] = g; m.p[4] = b;
    return push_mat(s, m);
}
// A homogeneous medium with an absorption coefficient per channel on top of its scattering (the rule is in pt_amd.h): the same material
// kind, with the coefficients in p[7..9] and p[10] = 1 (what makes a medium "tinted", whatever its coefficients)
extern "C" int pt_mat_medium_tinted(pt_scene* s, double density, double r, double g, double b, double hg_g, const double absorption[3]) {
    if (!s) return set_error("pt_mat_medium_tinted: null scene");
    if (!absorption) return set_error("pt_mat_medium_tinted: null argument");
    if (!(density >= 0.0) || !std::isfinite(density)) return set_error("pt_mat_medium_tinted: density must be finite and >= 0");
    for (double a : {r, g, b})
        if (!(a >= 0.0 && a <= 1.0)) return set_error("pt_mat_medium_tinted: each albedo channel must be in [0, 1]");
    if (!(std::fabs(hg_g) < 1.0)) return set_error("pt_mat_medium_tinted: |hg_g| must be below 1");
    double amax = 0.0;
    for (int c = 0; c < 3; ++c) {
        if (!(absorption[c] >= 0.0) || !std::isfinite(absorption[c])) return set_error("pt_mat_medium_tinted: each absorption coefficient must be finite and >= 0");
        amax = std::max(amax, absorption[c]);
    }
    if (!(density + amax > 0.0)) return set_error("pt_mat_medium_tinted: density and absorption are all 0 (no medium)");
    if (s->mats.size() >= MEDIUM_MAX_MATS) return set_error("pt_mat_medium_tinted: a medium's material handle must be below 4094 (create media before other materials)");
    MatD m = blank_mat(MAT_MEDIUM);
    m.p[0] = density;
    m.p[1] = hg_g;
    m.p[2] = r; m.p[3] = g; m.p[4] = b;
    for (int c = 0; c < 3; ++c) m.p[7 + c] = absorption[c];
    m.p[10] = 1.0;
    return push_mat(s, m);
}
// The medium that fills a glass object (the rule is in pt_amd.h): its handle + 1 in the glass's p[0], which glass does not use otherwise
extern "C" int pt_mat_glass_set_interior(pt_scene* s, int glass_mat, int medium_mat) {
    if (!s) return set_error("pt_mat_glass_set_interior: null scene");
    if (!MAT_OK(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return set_error("pt_mat_glass_set_interior: not a glass material");
    if (medium_mat != -1 && (!MAT_OK(s, medium_mat) || s->mats[medium_mat].kind != MAT_MEDIUM)) return set_error("pt_mat_glass_set_interior: not a medium material (-1 = detach)");
    for (const MatD& m : s->mats)
        if (m.kind == MAT_MIX && (m.color_tex == glass_mat || m.rough_tex == glass_mat)) return set_error("pt_mat_glass_set_interior: the glass is a child of a mix");
    s->mats[glass_mat].p[0] = (double)(medium_mat + 1);
    s->built = false;
    return 0;
}
extern "C" int pt_mat_glass_interior(pt_scene* s, int glass_mat) {
    if (!s || !MAT_OK(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return -1;
    return (int)s->mats[glass_mat].p[0] - 1;
}
// Spectral dispersion of a glass (the rule is in pt_amd.h): the two-term Cauchy law through (n_d, V_d). b in the glass's p[1], inv2(0.58756) in
// p[2], the Abbe number in p[3] — slots glass does not use otherwise (p[0] is the interior).
namespace pt {
static double inv2(double l) { return 1.0 / (l * l); }
double dispersion_ior(const MatD& m, double lambda_nm) { return m.ior + m.p[1] * (inv2(lambda_nm * 1e-3) - m.p[2]); }
void dispersion_weights(double w[DSP_BINS][3]) {
    auto g = [](double l, double mu, double s1, double s2) {
        const double t = (l - mu) / (l < mu ? s1 : s2);
        return std::exp(-0.5 * (t * t));
    };
    double sum[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < DSP_BINS; ++j) {
        const double l = 380.0 + ((double)j + 0.5) * (350.0 / (double)DSP_BINS);
        const double x = 1.056 * g(l, 599.8, 37.9, 31.0) + 0.362 * g(l, 442.0, 16.0, 26.7) - 0.065 * g(l, 501.1, 20.4, 26.2);
        const double y = 0.821 * g(l, 568.8, 46.9, 40.5) + 0.286 * g(l, 530.9, 16.3, 31.1);
        const double z = 1.217 * g(l, 437.0, 11.8, 36.0) + 0.681 * g(l, 459.0, 26.0, 13.8);
        const double rgb[3] = {3.2404542 * x - 1.5371385 * y - 0.4985314 * z, -0.9692660 * x + 1.8760108 * y + 0.0415560 * z,
                               0.0556434 * x - 0.2040259 * y + 1.0572252 * z};
        for (int c = 0; c < 3; ++c) {
            w[j][c] = std::max(0.0, rgb[c]);
            sum[c] += w[j][c];
        }
    }
    for (int j = 0; j < DSP_BINS; ++j)
        for (int c = 0; c < 3; ++c) w[j][c] = w[j][c] * (double)DSP_BINS / sum[c];
}
double* dispersion_table(pt_scene* s, hipStream_t st) {
    if (s->disp_w) return s->disp_w;
    double w[DSP_BINS][3];
    dispersion_weights(w);
    double* d = nullptr;
    if (!hip_ok(hipMalloc((void**)&d, sizeof w), "hipMalloc(dispersion weights)")) return nullptr;
    if (!hip_ok(hipMemcpyAsync(d, w, sizeof w, hipMemcpyHostToDevice, st), "hipMemcpy(dispersion weights)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(dispersion weights)")) {   // (`w` is on this stack)
        (void)hipFree(d);
        return nullptr;
    }
    return s->disp_w = d;
}
}  // namespace pt
extern "C" int pt_mat_glass_set_dispersion(pt_scene* s, int glass_mat, double abbe) {
    if (!s) return set_error("pt_mat_glass_set_dispersion: null scene");
    if (!MAT_OK(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return set_error("pt_mat_glass_set_dispersion: not a glass material");
    if (!(abbe >= 0.0) || !std::isfinite(abbe)) return set_error("pt_mat_glass_set_dispersion: the Abbe number must be finite and >= 0 (0 = off)");
    for (const MatD& m : s->mats)
        if (m.kind == MAT_MIX && (m.color_tex == glass_mat || m.rough_tex == glass_mat)) return set_error("pt_mat_glass_set_dispersion: the glass is a child of a mix");
    MatD m = s->mats[glass_mat];
    m.p[1] = m.p[2] = m.p[3] = 0.0;
    if (abbe > 0.0) {
        m.p[1] = (m.ior - 1.0) / (abbe * (inv2(0.48613) - inv2(0.65627)));
        m.p[2] = inv2(0.58756);
        m.p[3] = abbe;
        for (double l : {380.0, 730.0}) {
            const double n = dispersion_ior(m, l);
            if (!std::isfinite(n) || !(n > 1.0)) return set_error("pt_mat_glass_set_dispersion: the index of refraction must be finite and above 1 over 380..730 nm");
        }
    }
    s->mats[glass_mat] = m;
    s->built = false;
    return 0;
}
extern "C" double pt_mat_glass_dispersion(pt_scene* s, int glass_mat) {
    if (!s || !MAT_OK(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return -1.0;
    return s->mats[glass_mat].p[3];
}
// A medium whose extinction is scale * V(x), V trilinear in a grid of f32 samples (the rule is in pt_amd.h): the same material kind,
// with its row of the grid table in p[6] and its majorant in p[0]
extern "C" int pt_mat_medium_grid(pt_scene* s, double scale, double r, double g, double b, double hg_g, uint32_t nx, uint32_t ny, uint32_t nz, const float* values,
                                  const double box_lo[3], const double box_hi[3]) {
    if (!s) return set_error("pt_mat_medium_grid: null scene");
    if (!values || !box_lo || !box_hi) return set_error("pt_mat_medium_grid: null argument");
    if (!(scale > 0.0) || !std::isfinite(scale)) return set_error("pt_mat_medium_grid: scale must be finite and > 0");
    for (double a : {r, g, b})
        if (!(a >= 0.0 && a <= 1.0)) return set_error("pt_mat_medium_grid: each albedo channel must be in [0, 1]");
    if (!(std::fabs(hg_g) < 1.0)) return set_error("pt_mat_medium_grid: |hg_g| must be below 1");
    if (nx < 2 || ny < 2 || nz < 2) return set_error("pt_mat_medium_grid: every grid dimension must be at least 2");
    if ((uint64_t)nx * ny > (1ull << 28) || (uint64_t)nx * ny * nz > (1ull << 28)) return set_error("pt_mat_medium_grid: more than 2^28 grid values");
    double diag2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(box_lo[a]) || !std::isfinite(box_hi[a]) || !(box_lo[a] < box_hi[a])) return set_error("pt_mat_medium_grid: the box must be finite with box_lo < box_hi on every axis");
        diag2 += (box_hi[a] - box_lo[a]) * (box_hi[a] - box_lo[a]);
    }
    const size_t n = (size_t)nx * ny * nz;
    float vmax = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        if (!(values[i] >= 0.0f) || !std::isfinite(values[i])) return set_error("pt_mat_medium_grid: every value must be finite and >= 0");
        vmax = std::max(vmax, values[i]);
    }
    if (!(vmax > 0.0f)) return set_error("pt_mat_medium_grid: all values are 0 (no medium)");
    const double mu = scale * (double)vmax;
    // a design limit: the expected trip count of the longest tracking loop a lane can run (the box's diagonal at the majorant)
    if (!(mu * std::sqrt(diag2) <= 4096.0)) return set_error("pt_mat_medium_grid: the majorant optical diagonal scale * max(values) * |box_hi - box_lo| exceeds 4096 (model a medium that thick as a surface)");
    if (s->mats.size() >= MEDIUM_MAX_MATS) return set_error("pt_mat_medium_grid: a medium's material handle must be below 4094 (create media before other materials)");
    HostGrid hg;
    hg.d.nx = nx; hg.d.ny = ny; hg.d.nz = nz;
    const uint32_t dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        hg.d.lo[a] = box_lo[a];
        hg.d.hi[a] = box_hi[a];
        hg.d.cells[a] = (double)dims[a] / (box_hi[a] - box_lo[a]);
    }
    hg.d.scale = scale;
    hg.d.mu = mu;
    hg.vals.assign(values, values + n);
    s->grids.push_back(std::move(hg));
    MatD m = blank_mat(MAT_MEDIUM);
    m.p[0] = mu;
    m.p[1] = hg_g;
    m.p[2] = r; m.p[3] = g; m.p[4] = b;
    m.p[6] = (double)s->grids.size();
    return push_mat(s, m);
}
extern "C" int pt_scene_set_camera_medium(pt_scene* s, int mat) {
    if (!s) return set_error("pt_scene_set_camera_medium: null scene");
    if (mat != -1 && (!MAT_OK(s, mat) || s->mats[mat].kind != MAT_MEDIUM)) return set_error("pt_scene_set_camera_medium: not a medium material (-1 = none)");
    s->camera_medium = mat;
    return 0;
}
extern "C" int pt_scene_camera_medium(pt_scene* s) { return s ? s->camera_medium : -1; }
extern "C" int pt_mat_light(pt_scene* s, int tex) {
    if (!TEX_RGB_OK(s, tex)) return set_error("pt_mat_light: bad emission texture");
    MatD m = blank_mat(MAT_LIGHT);
    m.color_tex = tex;
    return push_mat(s, m);
}

static int push_obj(pt_scene* s, HostObj&& o) {
    s->objs.push_back(std::move(o));
    s->built = false;
    return (int)s->objs.size() - 1;
}
static QuadD make_quad(D3 q, D3 u, D3 v) {   // Quad::new quad.rs:17-36
    QuadD r;
    D3 n = cross(u, v);
    D3 normal = normalize(n);
    st3(r.q, q); st3(r.u, u); st3(r.v, v);
    st3(r.n, normal);
    r.d = dot(normal, q);
    st3(r.w, n / dot(n, n));
    return r;
}
extern "C" int pt_sphere(pt_scene* s, double radius, const double p1[3], const double p2[3], int mat) {
    if (!MAT_OK(s, mat)) return set_error("pt_sphere: bad material");
    HostObj o;
    o.kind = OBJ_SPHERE;
    o.mat = mat;
    o.sphere.r = std::fmax(radius, 0.0);   // sphere.rs:26
    for (int i = 0; i < 3; ++i) { o.sphere.p1[i] = p1[i]; o.sphere.p2[i] = p2[i]; }
    return push_obj(s, std::move(o));
}
extern "C" int pt_quad(pt_scene* s, const double q[3], const double u[3], const double v[3], int mat) {
    if (!MAT_OK(s, mat)) return set_error("pt_quad: bad material");
    HostObj o;
    o.kind = OBJ_QUAD;
    o.mat = mat;
    o.quads.push_back(make_quad(d3(q), d3(u), d3(v)));
    return push_obj(s, std::move(o));
}
extern "C" int pt_cuboid(pt_scene* s, const double a[3], const double b[3], int mat) {   // cuboid.rs:11-58
    if (!MAT_OK(s, mat)) return set_error("pt_cuboid: bad material");
    HostObj o;
    o.kind = OBJ_CUBOID;
    o.mat = mat;
    D3 mn = vmin(d3(a), d3(b)), mx = vmax(d3(a), d3(b));
    D3 dx{mx.x - mn.x, 0.0, 0.0}, dy{0.0, mx.y - mn.y, 0.0}, dz{0.0, 0.0, mx.z - mn.z};
    o.quads.push_back(make_quad(D3{mn.x, mn.y, mx.z}, dx, dy));    // front
    o.quads.push_back(make_quad(D3{mx.x, mn.y, mx.z}, -dz, dy));   // right
    o.quads.push_back(make_quad(D3{mx.x, mn.y, mn.z}, -dx, dy));   // back
    o.quads.push_back(make_quad(D3{mn.x, mn.y, mn.z}, dz, dy));    // left
    o.quads.push_back(make_quad(D3{mn.x, mx.y, mx.z}, dx, -dz));   // top
    o.quads.push_back(make_quad(D3{mn.x, mn.y, mn.z}, dx, dz));    // bottom
    return push_obj(s, std::move(o));
}
extern "C" int pt_mesh(pt_scene* s, double scale, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                       uint32_t n_nrm, const float* nrm, uint32_t n_uv, const float* uv, int mat) {   // mesh.rs:149-197
    if (!MAT_OK(s, mat)) return set_error("pt_mesh: bad material");
    if (n_idx % 3 != 0) return set_error("pt_mesh: index count must be a multiple of 3");
    if (n_idx / 3 > 0x07FFFFFFu) return set_error("pt_mesh: too many triangles");
    for (uint32_t i = 0; i < n_idx; ++i) {
        if (idx[i] >= n_pos) return set_error("pt_mesh: position index out of range");
        if (n_nrm && idx[i] >= n_nrm) return set_error("pt_mesh: normal index out of range");
        if (n_uv && idx[i] >= n_uv) return set_error("pt_mesh: texcoord index out of range");
    }
    HostObj o;
    o.kind = OBJ_MESH;
    o.mat = mat;
    o.has_normals = n_nrm != 0;
    o.has_uvs = n_uv != 0;
    auto vertex = [&](uint32_t i) { return D3{(double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2]} * scale; };
    o.tris.resize(n_idx / 3);
    if (o.has_normals || o.has_uvs) o.tri_attr.resize(n_idx / 3);
    for (uint32_t f = 0; f < n_idx / 3; ++f) {
        const uint32_t ii[3] = {idx[3 * f], idx[3 * f + 1], idx[3 * f + 2]};
        st3(o.tris[f].v0, vertex(ii[0]));
        st3(o.tris[f].v1, vertex(ii[1]));
        st3(o.tris[f].v2, vertex(ii[2]));
        if (!o.tri_attr.empty()) {
            TriAttr& a = o.tri_attr[f];
            memset(&a, 0, sizeof a);
            for (int k = 0; k < 3; ++k) {
                if (o.has_normals) for (int c = 0; c < 3; ++c) a.n[k][c] = (double)nrm[3 * ii[k] + c];
                if (o.has_uvs) for (int c = 0; c < 2; ++c) a.uv[k][c] = (double)uv[2 * ii[k] + c];
            }
        }
    }
    return push_obj(s, std::move(o));
}
static void make_pose(D3 axis, double angle, D3 tr, InstD& xf);
extern "C" int pt_instance(pt_scene* s, int obj, const double axis[3], double angle, const double tr[3]) {   // instance.rs:20-30
    if (!OBJ_OK(s, obj)) return set_error("pt_instance: bad object handle");
    // the wrapped object may be wrapped again (shared geometry), may itself be an instance (nesting) and may also be placed directly
    HostObj o;
    o.kind = OBJ_INSTANCE;
    o.child = obj;
    make_pose(d3(axis), angle, d3(tr), o.xf);
    return push_obj(s, std::move(o));
}
// The forward transform and its analytic inverse of Instance::new(axis, angle, tr). THE operation sequence of an instance's pose: pt_instance,
// the keys of pt_instance_moving, pt_motion_pose and — operation by operation — the device's pose_at (pt_dev_geom.h) all form it this way.
static void make_pose(D3 axis, double angle, D3 tr, InstD& xf) {
    // DQuat::from_axis_angle, DMat4::from_rotation_translation (glam 0.29 quat_to_axes)
    // detmath, not libm: g++ turns a sin/cos pair into one sincos() call, clang keeps two calls, and glibc's sincos can
    // differ from its sin and cos in the last bit on some CPUs — found by fuzzing (one instance angle in 40 scenes gave
    // a rotation matrix one ulp off the oracle's). The shared implementation makes the transform machine-independent.
    double sn, cs;
    detmath::sincos(angle * 0.5, sn, cs);
    D3 v = axis * sn;
    double qx = v.x, qy = v.y, qz = v.z, qw = cs;
    double x2 = qx + qx, y2 = qy + qy, z2 = qz + qz;
    double xx = qx * x2, xy = qx * y2, xz = qx * z2;
    double yy = qy * y2, yz = qy * z2, zz = qz * z2;
    double wx = qw * x2, wy = qw * y2, wz = qw * z2;
    D3 c0{1.0 - (yy + zz), xy + wz, xz - wy};
    D3 c1{xy - wz, 1.0 - (xx + zz), yz + wx};
    D3 c2{xz + wy, yz - wx, 1.0 - (xx + yy)};
    D3 t = tr;
    // analytic rigid inverse: R^T and -(R^T t)  
    D3 i0{c0.x, c1.x, c2.x}, i1{c0.y, c1.y, c2.y}, i2{c0.z, c1.z, c2.z};
    D3 it = -xform_vector(i0, i1, i2, t);
    st3(xf.c0, c0); st3(xf.c1, c1); st3(xf.c2, c2); st3(xf.t, t);
    st3(xf.i0, i0); st3(xf.i1, i1); st3(xf.i2, i2); st3(xf.it, it);
    xf.inner = xf.outer = -1;
}
// ---- motion (pt_instance_moving, pt_scene_set_shutter; the rule: pt_amd.h) ----
static bool finite3(const double* v) { return v && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
static bool keys_ok(const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3]) {
    return finite3(axis) && finite3(tr0) && finite3(tr1) && std::isfinite(angle0) && std::isfinite(angle1);
}
static InstMotionD make_keys(const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3]) {
    InstMotionD k{};
    for (int i = 0; i < 3; ++i) { k.axis[i] = axis[i]; k.tr0[i] = tr0[i]; k.dtr[i] = tr1[i] - tr0[i]; }
    k.angle0 = angle0;
    k.dangle = angle1 - angle0;
    k.moves = 1u;
    k.spins = angle0 != angle1 ? 1u : 0u;
    return k;
}
// the pose of keys `k` at `time`: the rule's two lerps, then pt_instance's sequence (a key pair that does not spin builds the same columns
// at every time — the ones the record stores)
static void pose_of_keys(const InstMotionD& k, double time, InstD& xf) {
    const double angle = k.angle0 + k.dangle * time;
    const D3 tr = d3(k.tr0) + d3(k.dtr) * time;
    make_pose(d3(k.axis), k.spins ? angle : k.angle0 + k.dangle * 0.0, tr, xf);
}
extern "C" int pt_instance_moving(pt_scene* s, int obj, const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3]) {
    if (!s) return set_error("pt_instance_moving: null scene");
    if (!OBJ_OK(s, obj)) return set_error("pt_instance_moving: bad object handle");
    if (!keys_ok(axis, angle0, angle1, tr0, tr1)) return set_error("pt_instance_moving: axis, angles and translations must be finite");
    HostObj o;
    o.kind = OBJ_INSTANCE;
    o.child = obj;
    o.motion = make_keys(axis, angle0, angle1, tr0, tr1);
    pose_of_keys(o.motion, 0.0, o.xf);   // InstD holds the pose at time 0
    return push_obj(s, std::move(o));
}
extern "C" int pt_scene_set_shutter(pt_scene* s, double open, double close) {
    if (!s) return set_error("pt_scene_set_shutter: null scene");
    if (!std::isfinite(open) || !std::isfinite(close) || !(0.0 <= open && open <= close && close <= 1.0))
        return set_error("pt_scene_set_shutter: the shutter needs finite times with 0 <= open <= close <= 1");
    s->shutter_open = open;
    s->shutter_close = close;
    return 0;
}
extern "C" int pt_scene_shutter(pt_scene* s, double out[2]) {
    if (!s || !out) return set_error("pt_scene_shutter: null scene or buffer");
    out[0] = s->shutter_open;
    out[1] = s->shutter_close;
    return 0;
}
extern "C" int pt_scene_motion(pt_scene* s) {
    if (!s || !s->built) return set_error("pt_scene_motion: world not built");
    return s->motion_on() ? 1 : 0;
}
extern "C" int pt_motion_pose(const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3], double time, double out24[24]) {
    if (!out24) return set_error("pt_motion_pose: null buffer");
    if (!keys_ok(axis, angle0, angle1, tr0, tr1) || !std::isfinite(time)) return set_error("pt_motion_pose: axis, angles, translations and time must be finite");
    InstD xf;
    pose_of_keys(make_keys(axis, angle0, angle1, tr0, tr1), time, xf);
    memcpy(out24, xf.c0, 24 * sizeof(double));   // c0, c1, c2, t, i0, i1, i2, it: InstD's order
    return 0;
}
// ---- punctual lights (pt_light_point, pt_light_spot, pt_light_directional; the rule: pt_amd.h) ----
static bool colour_ok(const double* c) { return finite3(c) && c[0] >= 0.0 && c[1] >= 0.0 && c[2] >= 0.0; }
static int push_punctual(pt_scene* s, const PunctualD& L, const char* who) {
    if (s->punctual.size() >= PLT_MAX_LIGHTS) return set_error(std::string(who) + ": the list of punctual lights is full (2048)");
    s->punctual.push_back(L);
    return (int)s->punctual.size() - 1;
}
// axis = normalize(v), or false for a zero-length or non-finite one
static bool unit_axis(D3 v, double out[3]) {
    const double len = length(v);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    const D3 a = normalize(v);
    if (!std::isfinite(a.x) || !std::isfinite(a.y) || !std::isfinite(a.z)) return false;
    st3(out, a);
    return true;
}
extern "C" int pt_light_point(pt_scene* s, const double position[3], const double power[3]) {
    if (!s) return set_error("pt_light_point: null scene");
    if (!finite3(position)) return set_error("pt_light_point: the position must be finite");
    if (!colour_ok(power)) return set_error("pt_light_point: the power must be finite and not negative");
    PunctualD L{};
    L.kind = 0u;
    for (int i = 0; i < 3; ++i) { L.pos[i] = position[i]; L.I[i] = power[i] / (4.0 * PI); }
    return push_punctual(s, L, "pt_light_point");
}
extern "C" int pt_light_spot(pt_scene* s, const double position[3], const double target[3], double inner_deg, double outer_deg, const double intensity[3]) {
    if (!s) return set_error("pt_light_spot: null scene");
    if (!finite3(position) || !finite3(target)) return set_error("pt_light_spot: position and target must be finite");
    if (!colour_ok(intensity)) return set_error("pt_light_spot: the intensity must be finite and not negative");
    if (!std::isfinite(inner_deg) || !std::isfinite(outer_deg) || !(0.0 <= inner_deg && inner_deg <= outer_deg && outer_deg < 180.0))
        return set_error("pt_light_spot: the cone angles need 0 <= inner_deg <= outer_deg < 180");
    PunctualD L{};
    L.kind = 1u;
    if (!unit_axis(d3(target) - d3(position), L.axis)) return set_error("pt_light_spot: target and position must differ (zero-length axis)");
    double sn;
    detmath::sincos(inner_deg * (PI / 180.0), sn, L.cos_i);   // the deterministic cosine of pt_instance's angles
    detmath::sincos(outer_deg * (PI / 180.0), sn, L.cos_o);
    for (int i = 0; i < 3; ++i) { L.pos[i] = position[i]; L.I[i] = intensity[i]; }
    return push_punctual(s, L, "pt_light_spot");
}
extern "C" int pt_light_directional(pt_scene* s, const double direction[3], const double irradiance[3]) {
    if (!s) return set_error("pt_light_directional: null scene");
    if (!finite3(direction)) return set_error("pt_light_directional: the direction must be finite");
    if (!colour_ok(irradiance)) return set_error("pt_light_directional: the irradiance must be finite and not negative");
    PunctualD L{};
    L.kind = 2u;
    if (!unit_axis(d3(direction), L.axis)) return set_error("pt_light_directional: the direction must not be zero");
    for (int i = 0; i < 3; ++i) L.I[i] = irradiance[i];
    return push_punctual(s, L, "pt_light_directional");
}
extern "C" int pt_scene_clear_punctual_lights(pt_scene* s) {
    if (!s) return set_error("pt_scene_clear_punctual_lights: null scene");
    s->punctual.clear();
    return 0;
}
extern "C" int pt_scene_punctual_count(pt_scene* s) {
    if (!s) return set_error("pt_scene_punctual_count: null scene");
    return (int)s->punctual.size();
}
static void punctual_to16(const PunctualD& L, double out[16]) {   // kind, pos, axis, I, cos_i, cos_o, then zeros
    out[0] = (double)L.kind;
    for (int i = 0; i < 3; ++i) { out[1 + i] = L.pos[i]; out[4 + i] = L.axis[i]; out[7 + i] = L.I[i]; }
    out[10] = L.cos_i; out[11] = L.cos_o;
    for (int i = 12; i < 16; ++i) out[i] = 0.0;
}
extern "C" int pt_scene_punctual_light(pt_scene* s, int k, double out[16]) {
    if (!s || !out) return set_error("pt_scene_punctual_light: null scene or buffer");
    if (k < 0 || (size_t)k >= s->punctual.size()) return set_error("pt_scene_punctual_light: no such light");
    punctual_to16(s->punctual[k], out);
    return 0;
}
extern "C" int pt_scene_set_punctual_fraction(pt_scene* s, double f) {
    if (!s) return set_error("pt_scene_set_punctual_fraction: null scene");
    if (!std::isfinite(f) || !(0.0 < f && f < 1.0)) return set_error("pt_scene_set_punctual_fraction: the fraction must be finite with 0 < f < 1");
    s->punctual_f = f;
    s->dev.view.punctual_f = f;   // (read by the PLT forms only: a scene without punctual lights renders the same bits whatever f is)
    return 0;
}
extern "C" int pt_scene_set_punctual_media(pt_scene* s, int on) {
    if (!s) return set_error("pt_scene_set_punctual_media: null scene");
    if (on != 0 && on != 1) return set_error("pt_scene_set_punctual_media: the setting is 0 or 1");
    s->punctual_media = on;   // (read by pt_render's choice of the kernels only: nothing to rebuild)
    return 0;
}
extern "C" int pt_scene_punctual_media(pt_scene* s) {
    if (!s) return set_error("pt_scene_punctual_media: null scene");
    return s->punctual_media;
}
extern "C" double pt_scene_punctual_fraction(pt_scene* s) {
    if (!s) { set_error("pt_scene_punctual_fraction: null scene"); return -1.0; }
    return s->punctual_f;
}
extern "C" int pt_punctual_eval(const double rec16[16], const double point[3], double out7[7]) {
    if (!rec16 || !point || !out7) return set_error("pt_punctual_eval: null buffer");
    if (!(rec16[0] == 0.0 || rec16[0] == 1.0 || rec16[0] == 2.0)) return set_error("pt_punctual_eval: the record's kind must be 0, 1 or 2");
    PunctualD L{};
    L.kind = (uint32_t)rec16[0];
    for (int i = 0; i < 3; ++i) { L.pos[i] = rec16[1 + i]; L.axis[i] = rec16[4 + i]; L.I[i] = rec16[7 + i]; }
    L.cos_i = rec16[10]; L.cos_o = rec16[11];
    const PunctualEval e = punctual_eval(L, point);   // the device's function, compiled for the host
    out7[0] = e.w[0]; out7[1] = e.w[1]; out7[2] = e.w[2]; out7[3] = e.D; out7[4] = e.E[0]; out7[5] = e.E[1]; out7[6] = e.E[2];
    return 0;
}
// ---- the light grid (pt_scene_set_punctual_selection, pt_scene_set_punctual_grid; the rule: pt_amd.h) ----
static PunctualD punctual_from16(const double* r) {
    PunctualD L{};
    L.kind = (uint32_t)r[0];
    for (int i = 0; i < 3; ++i) { L.pos[i] = r[1 + i]; L.axis[i] = r[4 + i]; L.I[i] = r[7 + i]; }
    L.cos_i = r[10]; L.cos_o = r[11];
    return L;
}
static bool grid_dims_ok(const uint32_t d[3]) { return d[0] >= 1u && d[0] <= PLT_GRID_MAX_DIM && d[1] >= 1u && d[1] <= PLT_GRID_MAX_DIM && d[2] >= 1u && d[2] <= PLT_GRID_MAX_DIM; }
static bool grid_box_ok(const double b[6]) {
    for (int i = 0; i < 6; ++i) if (!std::isfinite(b[i])) return false;
    return b[3] >= b[0] && b[4] >= b[1] && b[5] >= b[2];
}
static PunctualGridD grid_descriptor(const double box[6], const uint32_t dims[3], uint32_t n) {
    PunctualGridD g{};
    for (int ax = 0; ax < 3; ++ax) {
        g.lo[ax] = box[ax];
        g.inv[ax] = box[3 + ax] > box[ax] ? (double)dims[ax] / (box[3 + ax] - box[ax]) : 0.0;
        g.n[ax] = dims[ax];
    }
    g.stride = n;
    return g;
}
extern "C" int pt_scene_set_punctual_selection(pt_scene* s, int kind) {
    if (!s) return set_error("pt_scene_set_punctual_selection: null scene");
    if (kind != 0 && kind != 1) return set_error("pt_scene_set_punctual_selection: the kind is 0 (uniform) or 1 (the light grid)");
    s->punctual_selection = kind;   // (takes effect at the next pt_world_build, like the list)
    return 0;
}
extern "C" int pt_scene_punctual_selection(pt_scene* s) {
    if (!s) return set_error("pt_scene_punctual_selection: null scene");
    return s->punctual_selection;
}
extern "C" int pt_scene_set_punctual_grid(pt_scene* s, uint32_t nx, uint32_t ny, uint32_t nz, const double* box6) {
    if (!s) return set_error("pt_scene_set_punctual_grid: null scene");
    const uint32_t d[3] = {nx, ny, nz};
    if (!((nx == 0u && ny == 0u && nz == 0u) || grid_dims_ok(d))) return set_error("pt_scene_set_punctual_grid: the dims are 0, 0, 0 (automatic) or each in 1..64");
    if (box6 && !grid_box_ok(box6)) return set_error("pt_scene_set_punctual_grid: the box must be finite with hi >= lo on every axis");
    for (int i = 0; i < 3; ++i) s->grid_dims_set[i] = d[i];
    s->grid_box_given = box6 != nullptr;
    if (box6) memcpy(s->grid_box_set, box6, sizeof s->grid_box_set);
    return 0;
}
extern "C" int pt_scene_punctual_grid(pt_scene* s, uint32_t dims3[3], double box6[6]) {
    if (!s) return set_error("pt_scene_punctual_grid: null scene");
    if (!s->built || s->grid_built.cells == 0u) return set_error("pt_scene_punctual_grid: the light grid is not in effect");
    if (dims3) memcpy(dims3, s->grid_built.dims, 3 * sizeof(uint32_t));
    if (box6) memcpy(box6, s->grid_built.box, 6 * sizeof(double));
    return 0;
}
static int grid_twin_args(const char* who, uint32_t n, const double* box6, const uint32_t* dims3) {
    if (!box6 || !dims3) return set_error(std::string(who) + ": null buffer");
    if (n == 0u || n > PLT_MAX_LIGHTS) return set_error(std::string(who) + ": the list holds 1..2048 lights");
    if (!grid_dims_ok(dims3)) return set_error(std::string(who) + ": each dim is in 1..64");
    if (!grid_box_ok(box6)) return set_error(std::string(who) + ": the box must be finite with hi >= lo on every axis");
    return 0;
}
extern "C" int pt_punctual_grid_row(const double* recs16, uint32_t n, const double box6[6], const uint32_t dims3[3], uint32_t cell, double* out_cdf) {
    if (grid_twin_args("pt_punctual_grid_row", n, box6, dims3) != 0) return -1;
    if (!recs16 || !out_cdf) return set_error("pt_punctual_grid_row: null buffer");
    if (cell >= dims3[0] * dims3[1] * dims3[2]) return set_error("pt_punctual_grid_row: no such cell");
    for (uint32_t k = 0; k < n; ++k) {
        const double kind = recs16[16 * (size_t)k];
        if (!(kind == 0.0 || kind == 1.0 || kind == 2.0)) return set_error("pt_punctual_grid_row: a record's kind must be 0, 1 or 2");
    }
    const PunctualCell c = punctual_grid_geometry(box6, dims3, cell);   // the device's functions, compiled for the host
    punctual_grid_row([&](uint32_t k) { return punctual_from16(recs16 + 16 * (size_t)k); }, n, c, [&](uint32_t k, double C) { out_cdf[k] = C; });
    return 0;
}
extern "C" int pt_punctual_grid_select(const double box6[6], const uint32_t dims3[3], const double* table, uint32_t n, const double* points, const double* u, uint32_t m, double* out3) {
    if (grid_twin_args("pt_punctual_grid_select", n, box6, dims3) != 0) return -1;
    if (m == 0u) return 0;
    if (!table || !points || !u || !out3) return set_error("pt_punctual_grid_select: null buffer");
    const PunctualGridD g = grid_descriptor(box6, dims3, n);
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t cell = punctual_grid_cell(g, points + 3 * (size_t)i);
        double p;
        const uint32_t k = punctual_select(table + (size_t)cell * n, n, u[i], p);
        out3[3 * (size_t)i] = (double)cell; out3[3 * (size_t)i + 1] = (double)k; out3[3 * (size_t)i + 2] = p;
    }
    return 0;
}
static Box xform_box(const Box& b, const InstD& m) {   // box of the box (aabb.rs:50-76)
    Box r;
    for (int i = 0; i < 8; ++i) {
        D3 p{(i & 1) ? b.hi.x : b.lo.x, (i & 2) ? b.hi.y : b.lo.y, (i & 4) ? b.hi.z : b.lo.z};
        r.grow(xform_point(d3(m.c0), d3(m.c1), d3(m.c2), d3(m.t), p));
    }
    return r;
}
// One level of the box rule: the box of `b` under a moving instance over every time in [0, 1].
// Translates only: the union of the transformed boxes at times 0 and 1 — exact, since every corner is R p + tr(t) with R fixed and tr(t)
// monotone in t component by component (in floating point too: rounding is monotone). Spins: a corner p lands at R(t) p + tr(t) with
// |R(t) p| = |p| <= rho, the largest corner norm, so the union of tr(0) +- rho and tr(1) +- rho holds it; rho is widened by 1e-14 relative and
// the box by four ulps of its largest coordinate for the rounding of R(t) p and of the sum.
static Box swept_box(const Box& b, const InstMotionD& k) {
    InstD m0, m1;
    pose_of_keys(k, 0.0, m0);
    pose_of_keys(k, 1.0, m1);
    Box r;
    if (!k.spins) {
        r = xform_box(b, m0);
        r.grow(xform_box(b, m1));
        return r;
    }
    double rho = 0.0;
    for (int i = 0; i < 8; ++i) {
        D3 p{(i & 1) ? b.hi.x : b.lo.x, (i & 2) ? b.hi.y : b.lo.y, (i & 4) ? b.hi.z : b.lo.z};
        rho = std::fmax(rho, std::sqrt(dot(p, p)));
    }
    rho = rho * (1.0 + 1e-14);
    const D3 e{rho, rho, rho};
    r.grow(d3(m0.t) - e); r.grow(d3(m0.t) + e);
    r.grow(d3(m1.t) - e); r.grow(d3(m1.t) + e);
    double mx = 0.0;
    for (double x : {r.lo.x, r.lo.y, r.lo.z, r.hi.x, r.hi.y, r.hi.z}) mx = std::fmax(mx, std::fabs(x));
    const D3 pad{mx * (4.0 * DBL_EPSILON), mx * (4.0 * DBL_EPSILON), mx * (4.0 * DBL_EPSILON)};
    r.lo = r.lo - pad;
    r.hi = r.hi + pad;
    return r;
}
extern "C" int pt_motion_swept_box(const double box[6], const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3], double out[6]) {
    if (!box || !out) return set_error("pt_motion_swept_box: null buffer");
    if (!finite3(box) || !finite3(box + 3) || !keys_ok(axis, angle0, angle1, tr0, tr1)) return set_error("pt_motion_swept_box: box, axis, angles and translations must be finite");
    if (!(box[0] <= box[3] && box[1] <= box[4] && box[2] <= box[5])) return set_error("pt_motion_swept_box: the box needs lo <= hi on every axis");
    Box b;
    b.lo = d3(box);
    b.hi = d3(box + 3);
    const Box r = swept_box(b, make_keys(axis, angle0, angle1, tr0, tr1));
    st3(out, r.lo);
    st3(out + 3, r.hi);
    return 0;
}
extern "C" int pt_world_entry_box(pt_scene* s, uint32_t entry, double out[6]) {
    if (!s || !s->built) return set_error("pt_world_entry_box: world not built");
    if (!out) return set_error("pt_world_entry_box: null buffer");
    if ((size_t)entry * 6 >= s->entry_boxes.size()) return set_error("pt_world_entry_box: entry out of range");
    memcpy(out, &s->entry_boxes[(size_t)entry * 6], 6 * sizeof(double));
    return 0;
}
static int place(pt_scene* s, int obj, std::vector<int>& list, const char* who) {
    if (!OBJ_OK(s, obj)) return set_error(std::string(who) + ": bad object handle");
    // World::add_object / add_light take any Arc<dyn Hittable> (world.rs:18-24): the same object any number of times, under instances
    // as well. Every entry of the two lists is one PLACEMENT with its own primitive ids (scene_build).
    list.push_back(obj);
    s->built = false;
    return 0;
}
extern "C" int pt_world_add_object(pt_scene* s, int obj) { return place(s, obj, s->world_objects, "pt_world_add_object"); }
extern "C" int pt_world_add_light(pt_scene* s, int obj) {
    if (OBJ_OK(s, obj)) {   // a medium's boundary is invisible: it cannot be a light (the object an instance chain finally wraps decides)
        int oi = obj;
        for (int guard = 0; s->objs[oi].kind == OBJ_INSTANCE && guard <= 64; ++guard) oi = s->objs[oi].child;
        if (MAT_OK(s, s->objs[oi].mat) && s->mats[s->objs[oi].mat].kind == MAT_MEDIUM)
            return set_error("pt_world_add_light: an object with a medium material cannot be in the lights list");
    }
    return place(s, obj, s->world_lights, "pt_world_add_light");
}
extern "C" uint32_t pt_world_prim_count(pt_scene* s) { return s->n_prims; }
extern "C" int pt_world_set_device_bvh_threshold(pt_scene* s, uint32_t min_triangles) {
    if (!s) return set_error("pt_world_set_device_bvh_threshold: null scene");
    s->device_bvh_min_tris = min_triangles;
    s->built = false;
    return 0;
}
extern "C" int pt_world_device_bvh_info(pt_scene* s, uint32_t* n_meshes, uint32_t* deepest) {
    if (!s || !s->built) return set_error("pt_world_device_bvh_info: world not built");
    if (n_meshes) *n_meshes = s->n_device_blas;
    if (deepest) *deepest = s->device_blas_depth;
    return 0;
}
extern "C" int pt_world_build(pt_scene* s) { return scene_build(s); }

// ----------------------------------------------------------------------------------------
// BVH builder: top-down binned SAH (16 bins) over item boxes, depth-limited (falls back to
// object-median splits when the remaining depth budget is tight) so that the traversal
// kernel's LDS stack (TRAVERSAL_STACK levels) can never overflow. The reference's O(n^2)
// full-sweep SAH (bvh.rs:54-120) is NOT reproduced: closest-hit results do not depend on the
// tree, only on the canonical tie rule both sides share.
// ----------------------------------------------------------------------------------------
namespace {
struct BuildItem {
    Box box;
    D3 c;
    uint32_t ref_payload;   // original index
};
struct Builder {
    std::vector<BvhNode>& nodes;
    std::vector<BuildItem>& items;
    int leaf_max, max_depth;
    bool tri_leaves;                       // leaf = REF_TRIS range, else REF_ENTRY single
    std::vector<uint32_t>* order;          // BLAS: output permutation (leaf order)
    uint32_t leaf_base = 0;                // BLAS: index of this mesh's first triangle in the global array
    int depth_reached = 0;
    int n_bins = 16;                       // SAH bins per axis (<= MAX_BINS)
    size_t sweep_below = 0;                // ranges of at most this many items are split by the exact SAH sweep (every split position of every axis)
    static constexpr int MAX_BINS = 64;

    static float down(double v) {
        float f = (float)v;
        if ((double)f > v) f = std::nextafterf(f, -INFINITY);
        return f;
    }
    static float up(double v) {
        float f = (float)v;
        if ((double)f < v) f = std::nextafterf(f, INFINITY);
        return f;
    }
    static void store_box(const Box& b, float* lo, float* hi) {
        // pad, then round outward to f32: strictly conservative for the f64 slab test
        double m = 1e-3;
        const double v[6] = {b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z};
        for (double x : v) m = std::fmax(m, std::fabs(x));
        double pad = 1e-7 * m;
        lo[0] = down(b.lo.x - pad); lo[1] = down(b.lo.y - pad); lo[2] = down(b.lo.z - pad);
        hi[0] = up(b.hi.x + pad); hi[1] = up(b.hi.y + pad); hi[2] = up(b.hi.z + pad);
    }
    static double axis_of(D3 v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; }

    uint32_t make_leaf(size_t begin, size_t end) {
        if (tri_leaves) {
            uint32_t first = leaf_base + (uint32_t)order->size();
            for (size_t i = begin; i < end; ++i) order->push_back(items[i].ref_payload);
            return REF_TRIS | ((uint32_t)(end - begin - 1) << 27) | first;
        }
        return REF_ENTRY | items[begin].ref_payload;
    }
    // returns child reference; `out_box` = bounds of the subtree
    uint32_t build(size_t begin, size_t end, int depth, Box& out_box) {
        depth_reached = std::max(depth_reached, depth);
        Box box, cbox;
        for (size_t i = begin; i < end; ++i) { box.grow(items[i].box); cbox.grow(items[i].c); }
        out_box = box;
        const size_t n = end - begin;
        if (n <= (size_t)leaf_max) return make_leaf(begin, end);
        // depth budget: levels still needed with perfect median splits
        int needed = 0;
        for (size_t cap = (size_t)leaf_max; cap < n; cap *= 2) ++needed;
        const bool force_median = needed >= max_depth - depth;
        D3 ext = cbox.hi - cbox.lo;
        int axis = ext.x >= ext.y && ext.x >= ext.z ? 0 : (ext.y >= ext.z ? 1 : 2);
        size_t mid = begin + n / 2;
        bool done = false;
        if (!force_median && n <= sweep_below) {
            // exact sweep: the items sorted along each axis, every position between two neighbours a candidate
            double best_cost = INFINITY;
            int best_axis = -1;
            size_t best_pos = 0;
            std::vector<BuildItem> tmp(items.begin() + begin, items.begin() + end);
            std::vector<double> right_area(n);
            for (int a = 0; a < 3; ++a) {
                std::stable_sort(tmp.begin(), tmp.end(), [&](const BuildItem& x, const BuildItem& y) { return axis_of(x.c, a) < axis_of(y.c, a); });
                Box acc;
                for (size_t i = n; i-- > 1;) { acc.grow(tmp[i].box); right_area[i] = acc.half_area(); }
                acc = Box();
                for (size_t i = 0; i + 1 < n; ++i) {
                    acc.grow(tmp[i].box);
                    const double cost = acc.half_area() * (double)(i + 1) + right_area[i + 1] * (double)(n - i - 1);
                    if (cost < best_cost) { best_cost = cost; best_axis = a; best_pos = i + 1; }
                }
            }
            if (best_axis >= 0) {
                std::stable_sort(items.begin() + begin, items.begin() + end,
                                 [&](const BuildItem& x, const BuildItem& y) { return axis_of(x.c, best_axis) < axis_of(y.c, best_axis); });
                mid = begin + best_pos;
                done = true;
            }
        }
        if (!force_median && !done) {
            const int NB = n_bins;
            double best_cost = INFINITY;
            int best_axis = -1, best_bin = -1;
            for (int a = 0; a < 3; ++a) {
                double lo = axis_of(cbox.lo, a), hi = axis_of(cbox.hi, a);
                if (!(hi > lo)) continue;
                Box bb[MAX_BINS];
                size_t bc[MAX_BINS] = {0};
                double k = (double)NB / (hi - lo);
                for (size_t i = begin; i < end; ++i) {
                    int b = (int)((axis_of(items[i].c, a) - lo) * k);
                    b = std::min(std::max(b, 0), NB - 1);
                    bb[b].grow(items[i].box);
                    ++bc[b];
                }
                Box right_acc[MAX_BINS];
                size_t right_cnt[MAX_BINS];
                Box acc;
                size_t cnt = 0;
                for (int b = NB - 1; b > 0; --b) {
                    acc.grow(bb[b]);
                    cnt += bc[b];
                    right_acc[b] = acc;
                    right_cnt[b] = cnt;
                }
                acc = Box();
                cnt = 0;
                for (int b = 0; b < NB - 1; ++b) {
                    acc.grow(bb[b]);
                    cnt += bc[b];
                    if (cnt == 0 || right_cnt[b + 1] == 0) continue;
                    double cost = acc.half_area() * (double)cnt + right_acc[b + 1].half_area() * (double)right_cnt[b + 1];
                    if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = b; }
                }
            }
            if (best_axis >= 0) {
                double lo = axis_of(cbox.lo, best_axis), hi = axis_of(cbox.hi, best_axis);
                double k = (double)NB / (hi - lo);
                auto it = std::stable_partition(items.begin() + begin, items.begin() + end, [&](const BuildItem& it_) {
                    int b = (int)((axis_of(it_.c, best_axis) - lo) * k);
                    b = std::min(std::max(b, 0), NB - 1);
                    return b <= best_bin;
                });
                mid = (size_t)(it - items.begin());
                done = mid > begin && mid < end;
            }
        }
        if (!done) {
            mid = begin + n / 2;
            std::stable_sort(items.begin() + begin, items.begin() + end,
                             [&](const BuildItem& a, const BuildItem& b) { return axis_of(a.c, axis) < axis_of(b.c, axis); });
        }
        uint32_t me = (uint32_t)nodes.size();
        nodes.emplace_back();
        Box lb, rb;
        uint32_t l = build(begin, mid, depth + 1, lb);
        uint32_t r = build(mid, end, depth + 1, rb);
        BvhNode& nd = nodes[me];
        store_box(lb, nd.lo0, nd.hi0);
        store_box(rb, nd.lo1, nd.hi1);
        nd.child0 = l;
        nd.child1 = r;
        nd.pad0 = nd.pad1 = 0;
        return REF_NODE | me;
    }
};

template <class T>
bool upload(DeviceBuffers& dev, const std::vector<T>& v, const T*& out) {
    out = nullptr;
    size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
    void* p = nullptr;
    if (!hip_ok(hipMalloc(&p, bytes), "hipMalloc(scene)")) return false;
    dev.allocs.push_back(p);
    if (!v.empty() && !hip_ok(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy(scene)")) return false;
    out = (const T*)p;
    return true;
}
// max |coordinate| of a subtree's bounds, as the f32 slab test's error margin needs it: padded like
// the stored boxes and rounded up
float box_extent(const Box& b) {
    double m = 1e-3;
    const double v[6] = {b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z};
    for (double x : v) m = std::fmax(m, std::fabs(x));
    return std::nextafterf((float)(m * 1.000001), INFINITY);
}
Box sphere_box(const SphereD& s) {
    Box b;
    D3 r{s.r, s.r, s.r};
    b.grow(d3(s.p1) - r); b.grow(d3(s.p1) + r);
    b.grow(d3(s.p2) - r); b.grow(d3(s.p2) + r);
    return b;
}
Box quad_box(const QuadD& q) {
    Box b;
    D3 o = d3(q.q), u = d3(q.u), v = d3(q.v);
    b.grow(o); b.grow(o + u); b.grow(o + v); b.grow(o + u + v);
    return b;
}
}  // namespace

int pt::scene_build(pt_scene* s) {
    if (!s->ctx) return set_error("scene has no context");
    if (!hip_ok(hipSetDevice(s->ctx->device), "hipSetDevice")) return -1;
    s->dev.release();
    s->built = false;

    std::vector<BvhNode> nodes;
    std::vector<Entry> entries;
    std::vector<PrimRef> prims;
    std::vector<SphereD> spheres;
    std::vector<QuadD> quads;
    std::vector<TriD> tris;
    std::vector<TriAttr> tri_attr;
    std::vector<uint32_t> tri_gid;
    std::vector<InstD> insts;
    std::vector<InstMotionD> inst_motion;   // parallel to insts (SceneD::inst_motion); uploaded when an instance moves
    bool any_moving = false;
    std::vector<uint32_t> lights;
    std::vector<double> light_cdf;   // the light meshes' running area sums (SceneD::light_cdf), one table per mesh object
    s->lights_have_mesh_or_sphere = s->light_mesh_bad_area = false;
    s->light_blas_depth = 0;
    std::vector<BuildItem> tlas_items;
    bool any_attr = false;
    for (auto& o : s->objs) any_attr = any_attr || !o.tri_attr.empty();

    // canonical global primitive ids: lights list first, then objects, insertion order
    std::vector<int> order = s->world_lights;
    order.insert(order.end(), s->world_objects.begin(), s->world_objects.end());
    if (order.empty()) return set_error("pt_world_build: the world is empty");
    int max_blas_depth = 0;
    s->n_device_blas = s->device_blas_depth = 0;
    struct SharedBlas {   // one tree and one triangle range per MESH OBJECT, however many placements it has
        uint32_t root, tri_base;
        float extent;
        Box local;
        std::vector<uint32_t> face_pos;   // face -> position in BLAS (leaf) order
        int depth = 0;                    // of the tree
        uint32_t cdf_ofs = 0xFFFFFFFFu;   // its area table in light_cdf, once a placement of it is a light
    };
    std::map<int, SharedBlas> blas_of;
    for (size_t wi = 0; wi < order.size(); ++wi) {
        // the placement's instance chain, outermost first, down to the object it finally wraps
        int oi = order[wi];
        int inst = -1;
        std::vector<int> chain;
        for (int guard = 0; s->objs[oi].kind == OBJ_INSTANCE; ++guard) {
            if (guard > 64) return set_error("pt_world_build: instance chain too deep");
            chain.push_back((int)insts.size());
            insts.push_back(s->objs[oi].xf);
            inst_motion.push_back(s->objs[oi].motion);
            any_moving = any_moving || s->objs[oi].motion.moves != 0u;
            oi = s->objs[oi].child;
        }
        for (size_t k = 0; k < chain.size(); ++k) {
            insts[chain[k]].outer = k == 0 ? -1 : chain[k - 1];
            insts[chain[k]].inner = k + 1 < chain.size() ? chain[k + 1] : -1;
        }
        if (!chain.empty()) inst = chain.front();
        const HostObj* o = &s->objs[oi];
        auto to_world = [&](D3 p) {   // object space -> world: innermost instance first
            for (size_t k = chain.size(); k-- > 0;) {
                const InstD& m = insts[chain[k]];
                p = xform_point(d3(m.c0), d3(m.c1), d3(m.c2), d3(m.t), p);
            }
            return p;
        };
        const bool is_light = wi < s->world_lights.size();
        if (is_light) lights.push_back((uint32_t)entries.size());   // any hittable may be a light (world.rs:18-20)
        if (is_light && (o->kind == OBJ_MESH || o->kind == OBJ_SPHERE)) s->lights_have_mesh_or_sphere = true;
        Entry e{};
        memset(&e, 0, sizeof e);
        e.first_prim = (uint32_t)prims.size();
        e.inst = inst;
        e.blas_root = REF_EMPTY;
        Box local;
        switch (o->kind) {
        case OBJ_SPHERE:
            e.kind = ENTRY_SPHERE;
            prims.push_back(PrimRef{PRIM_SPHERE, (uint32_t)spheres.size(), (uint32_t)o->mat, inst});
            spheres.push_back(o->sphere);
            local = sphere_box(o->sphere);
            break;
        case OBJ_QUAD:
        case OBJ_CUBOID:
            e.kind = o->kind == OBJ_QUAD ? ENTRY_QUAD : ENTRY_CUBOID;
            for (const QuadD& q : o->quads) {
                prims.push_back(PrimRef{PRIM_QUAD, (uint32_t)quads.size(), (uint32_t)o->mat, inst});
                quads.push_back(q);
                local.grow(quad_box(q));
            }
            break;
        case OBJ_MESH: {
            e.kind = ENTRY_MESH;
            if (o->tris.empty()) return set_error("pt_world_build: empty mesh");
            auto it = blas_of.find(oi);
            if (it == blas_of.end()) {
                std::vector<BuildItem> items(o->tris.size());
                SharedBlas sb;
                for (size_t i = 0; i < o->tris.size(); ++i) {
                    Box b;
                    b.grow(d3(o->tris[i].v0)); b.grow(d3(o->tris[i].v1)); b.grow(d3(o->tris[i].v2));
                    items[i] = BuildItem{b, b.centroid(), (uint32_t)i};
                    sb.local.grow(b);
                }
                std::vector<uint32_t> perm;
                sb.tri_base = (uint32_t)tris.size();
                if ((size_t)sb.tri_base + o->tris.size() > 0x07FFFFFFu) return set_error("pt_world_build: too many triangles");
                int leaf_max = 4;   // PT_LEAF_MAX: experiments only (smaller leaves were slower on scene 6)
                if (const char* ev = exp_env("PT_LEAF_MAX")) leaf_max = std::min(8, std::max(1, atoi(ev)));
                Box bb = sb.local;
                bool on_device = false;
                if (s->device_bvh_min_tris != 0 && o->tris.size() >= s->device_bvh_min_tris) {
                    // large mesh: depth-bounded LBVH on the GPU (pt_bvh_device.hip); only a HIP failure falls back to the host builder
                    DeviceBlas db;
                    const double lo[3] = {sb.local.lo.x, sb.local.lo.y, sb.local.lo.z}, hi[3] = {sb.local.hi.x, sb.local.hi.y, sb.local.hi.z};
                    // depth budget: eight levels above a perfectly balanced tree — the radix tree of 1.3 M triangles comes out 27 deep, and
                    // every level the bound takes away bends Morton splits (measured on that mesh, K2 per launch: 27 levels 1.78 ms,
                    // 23: 1.83, 21: 2.19, 20: 2.50; the host's SAH tree 1.50) — within what the traversal stacks cover (k_extend2's
                    // largest LDS stack holds 32 entries; TRAVERSAL_STACK bounds top level + mesh tree)
                    int bal = 0;
                    for (size_t cap = (size_t)leaf_max; cap < o->tris.size(); cap *= 2) ++bal;
                    int dev_depth = std::min(29, std::max((int)MAX_BLAS_DEPTH, bal + 8));
                    if (const char* ev = exp_env("PT_LBVH_DEPTH")) dev_depth = std::min(29, std::max(bal, atoi(ev)));
                    uint32_t median_below = 0;
                    if (const char* ev = exp_env("PT_LBVH_MEDIAN")) median_below = (uint32_t)atoi(ev);
                    if (build_blas_device(o->tris.data(), (uint32_t)o->tris.size(), lo, hi, (uint32_t)leaf_max, (uint32_t)dev_depth, median_below, db, s->ctx->stream)) {
                        const uint32_t node_base = (uint32_t)nodes.size();
                        auto fix = [&](uint32_t ref) {
                            if ((ref & REF_TYPE_MASK) == REF_NODE) return REF_NODE | (node_base + ref);
                            return (ref & ~0x07FFFFFFu) | (sb.tri_base + (ref & 0x07FFFFFFu));     // REF_TRIS: count bits kept
                        };
                        for (BvhNode nd : db.nodes) {
                            nd.child0 = fix(nd.child0);
                            nd.child1 = fix(nd.child1);
                            nodes.push_back(nd);
                        }
                        sb.root = REF_NODE | node_base;
                        perm = db.order;
                        max_blas_depth = std::max(max_blas_depth, db.depth);
                        sb.depth = db.depth;
                        ++s->n_device_blas;
                        s->device_blas_depth = std::max<uint32_t>(s->device_blas_depth, (uint32_t)db.depth);
                        on_device = true;
                    }
                }
                if (!on_device) {
                    Builder bl{nodes, items, leaf_max, MAX_BLAS_DEPTH, true, &perm, sb.tri_base};
                    if (const char* ev = exp_env("PT_SAH_BINS")) bl.n_bins = std::min((int)Builder::MAX_BINS, std::max(2, atoi(ev)));
                    if (const char* ev = exp_env("PT_SAH_SWEEP")) bl.sweep_below = (size_t)std::max(0, atoi(ev));
                    sb.root = bl.build(0, items.size(), 0, bb);
                    max_blas_depth = std::max(max_blas_depth, bl.depth_reached);
                    sb.depth = bl.depth_reached;
                }
                sb.extent = box_extent(bb);
                sb.face_pos.resize(perm.size());
                for (size_t k = 0; k < perm.size(); ++k) {
                    const uint32_t face = perm[k];
                    sb.face_pos[face] = (uint32_t)k;
                    tris.push_back(o->tris[face]);
                    tri_gid.push_back(face);                 // face index inside the mesh; the kernels add Entry::first_prim
                    if (any_attr) tri_attr.push_back(o->tri_attr.empty() ? TriAttr{} : o->tri_attr[face]);
                }
                it = blas_of.emplace(oi, std::move(sb)).first;
            }
            SharedBlas& sb = it->second;
            if (is_light) {
                // exact light sampling's table (the rule in pt_amd.h), built whatever the kind: C[0] = 0, C[i + 1] = C[i] + A_i in face order,
                // A_i = 0.5 |cross(v1 - v0, v2 - v0)| of the local-space vertices — instance chains are rigid, so every placement shares it
                if (sb.cdf_ofs == 0xFFFFFFFFu) {
                    if (light_cdf.size() + o->tris.size() + 1 > 0xFFFFFFF0ull) return set_error("pt_world_build: too many light triangles");
                    sb.cdf_ofs = (uint32_t)light_cdf.size();
                    double c = 0.0;
                    light_cdf.push_back(c);
                    for (const TriD& t : o->tris) {
                        const D3 v0 = d3(t.v0);
                        c = c + 0.5 * length(cross(d3(t.v1) - v0, d3(t.v2) - v0));
                        light_cdf.push_back(c);
                    }
                }
                const double A = light_cdf[sb.cdf_ofs + o->tris.size()];
                s->light_mesh_bad_area = s->light_mesh_bad_area || !(A > 0.0 && std::isfinite(A));
                s->light_blas_depth = std::max<uint32_t>(s->light_blas_depth, (uint32_t)sb.depth);
                e.pad[0] = sb.cdf_ofs;
            }
            e.blas_root = sb.root;
            e.extent = sb.extent;
            local = sb.local;
            const uint32_t flags = PRIM_TRI | (o->has_normals ? PRIM_HAS_NORMALS : 0u) | (o->has_uvs ? PRIM_HAS_UVS : 0u);
            for (size_t face = 0; face < o->tris.size(); ++face)   // one PrimRef per PLACED triangle: ids are per placement
                prims.push_back(PrimRef{flags, sb.tri_base + sb.face_pos[face], (uint32_t)o->mat, inst});
            break;
        }
        default:
            return set_error("pt_world_build: unsupported object kind");
        }
        e.n_prims = (uint32_t)prims.size() - e.first_prim;
        Box world = local;
        bool chain_moves = false;
        for (size_t k = chain.size(); k-- > 0;) {   // box of the box, per instance (aabb.rs:50-76); a moving level: the box rule over [0, 1] (swept_box)
            const InstMotionD& mk = inst_motion[chain[k]];
            chain_moves = chain_moves || mk.moves != 0u;
            world = mk.moves ? swept_box(world, mk) : xform_box(world, insts[chain[k]]);
        }
        if (chain.size() == 1 && chain_moves && !inst_motion[chain[0]].spins && o->kind == OBJ_MESH) {
            // a mesh under ONE instance that translates only: the bounds of its transformed vertices at times 0 and 1, as below — every
            // vertex is R p + tr(t) with tr(t) monotone in t component by component, so the two ends hold every time in between
            InstD m0, m1;
            pose_of_keys(inst_motion[chain[0]], 0.0, m0);
            pose_of_keys(inst_motion[chain[0]], 1.0, m1);
            Box tight;
            for (const TriD& t : o->tris)
                for (const double* v : {t.v0, t.v1, t.v2}) {
                    tight.grow(xform_point(d3(m0.c0), d3(m0.c1), d3(m0.c2), d3(m0.t), d3(v)));
                    tight.grow(xform_point(d3(m1.c0), d3(m1.c1), d3(m1.c2), d3(m1.t), d3(v)));
                }
            world = tight;
        }
        if (!chain.empty() && o->kind == OBJ_MESH && !chain_moves) {
            // an instanced mesh gets the bounds of its TRANSFORMED VERTICES, not the box of its transformed box
            // (aabb.rs:50-76 does the latter): a mesh turned by ~50 degrees has a third less box to enter, and
            // every ray that enters costs a trip through the mesh pass. Any conservative box gives the same
            // closest hit; store_box pads by 1e-7 relative, far above the rounding of the transform.
            Box tight;
            for (const TriD& t : o->tris)
                for (const double* v : {t.v0, t.v1, t.v2}) tight.grow(to_world(d3(v)));
            world = tight;
        }
        tlas_items.push_back(BuildItem{world, world.centroid(), (uint32_t)entries.size()});
        entries.push_back(e);
    }
    if (prims.size() >= (size_t)HIT_ID_MASK - 4) return set_error("pt_world_build: too many primitives (28-bit ids)");
    // (a medium's boundary sorts with glass — the other kind that sends the ray on — so that K2's result word keeps its classes: pt_types.h)
    s->world_has_medium = s->world_has_grid_medium = s->world_has_interior = s->world_has_dispersion = false;
    // PRIM_NEEDS_UV (pt_types.h): can this material read HitD::u / v? A normal map, an image texture in the colour texture's tree
    // (through checker children), or a mix with such a child, at both nesting levels. An index out of range counts as "can".
    std::function<bool(int32_t, int)> tex_reads_uv = [&](int32_t t, int depth) -> bool {
        if (t < 0) return false;
        if ((size_t)t >= s->tex.size() || depth > 16) return true;
        const TexD& T = s->tex[t].d;
        if (T.kind == TEX_IMAGE || T.kind == TEX_IMAGE_F32) return true;
        return T.kind == TEX_CHECKER && (tex_reads_uv((int32_t)T.t1, depth + 1) || tex_reads_uv((int32_t)T.t2, depth + 1));
    };
    std::function<bool(int32_t, int)> mat_reads_uv = [&](int32_t mi, int depth) -> bool {
        if (mi < 0 || (size_t)mi >= s->mats.size() || depth > 2) return true;   // (pt_mat_mix admits two levels)
        const MatD& m = s->mats[mi];
        if (m.nmap_tex >= 0) return true;
        if (m.kind == MAT_MIX) return mat_reads_uv(m.color_tex, depth + 1) || mat_reads_uv(m.rough_tex, depth + 1);   // (a mix keeps its children there)
        return tex_reads_uv(m.color_tex, 0);
    };
    for (PrimRef& pr : prims) {
        const uint32_t kind = s->mats[pr.mat].kind;
        if ((pr.kind & 0xFFu) == PRIM_SPHERE && mat_reads_uv((int32_t)pr.mat, 0)) pr.kind |= PRIM_NEEDS_UV;
        s->world_has_medium = s->world_has_medium || kind == MAT_MEDIUM;
        s->world_has_grid_medium = s->world_has_grid_medium || (kind == MAT_MEDIUM && s->mats[pr.mat].p[6] != 0.0);
        // a glass with an interior, or a tinted medium's boundary
        s->world_has_interior = s->world_has_interior || (kind == MAT_GLASS && s->mats[pr.mat].p[0] != 0.0) || (kind == MAT_MEDIUM && s->mats[pr.mat].p[10] != 0.0);
        s->world_has_dispersion = s->world_has_dispersion || (kind == MAT_GLASS && s->mats[pr.mat].p[3] != 0.0);   // a dispersive glass
        pr.kind |= (kind == MAT_MEDIUM ? MEDIUM_SORT_KIND : kind) << PRIM_MAT_KIND_SHIFT;
    }
    // the short-path pass's shadeable entries (pt_k_short.hip shades them itself): a world-level sphere or quad, no instance
    // chain, still, a diffuse material without a normal map (fetch_tex looks up whatever colour texture it has)
    s->entry_shadeable.assign(entries.size(), 0);
    s->shade_prims.clear();
    s->shade_self_ok.clear();
    s->shade_entry.clear();
    for (size_t i = 0; i < entries.size(); ++i) {
        const Entry& e = entries[i];
        if ((e.kind != ENTRY_SPHERE && e.kind != ENTRY_QUAD) || e.inst >= 0 || e.n_prims != 1u) continue;
        const PrimRef& pr = prims[e.first_prim];
        const MatD& m = s->mats[pr.mat];
        if (pr.inst >= 0 || m.kind != MAT_DIFFUSE || m.nmap_tex >= 0) continue;
        if ((pr.kind & 0xFFu) == PRIM_SPHERE) {
            const SphereD& sp = spheres[pr.index];
            if (!(sp.p1[0] == sp.p2[0] && sp.p1[1] == sp.p2[1] && sp.p1[2] == sp.p2[2])) continue;
        } else if ((pr.kind & 0xFFu) != PRIM_QUAD) continue;
        s->entry_shadeable[i] = 1;
        s->shade_prims.push_back(e.first_prim);
        s->shade_entry.push_back((uint32_t)i);
        //  a quad whose numbers keep the proof's bound: finite, |coordinates| <= 1e6, the stored normal of unit length
        bool self_ok = (pr.kind & 0xFFu) == PRIM_QUAD;
        if (self_ok) {
            const QuadD& q = quads[pr.index];
            for (int a = 0; a < 3; ++a)
                for (double x : {q.q[a], q.q[a] + q.u[a], q.q[a] + q.v[a], q.q[a] + q.u[a] + q.v[a], q.n[a]}) self_ok = self_ok && std::fabs(x) <= 1e6;
            const double n2 = (q.n[0] * q.n[0] + q.n[1] * q.n[1]) + q.n[2] * q.n[2];
            self_ok = self_ok && std::fabs(q.d) <= 2e6 && std::fabs(n2 - 1.0) <= 1e-9;   // (a NaN fails every comparison)
        }
        s->shade_self_ok.push_back(self_ok ? 1 : 0);
    }
    // the place of every entry in SceneD::entry_box, the order the flat top level's loop runs in (below: non-mesh entries first, each kind in entry order)
    s->entry_at.assign(entries.size(), 0);
    {
        uint32_t at = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (size_t i = 0; i < entries.size(); ++i)
                if ((entries[i].kind == ENTRY_MESH) == (pass == 1)) s->entry_at[i] = at++;
    }
    std::vector<Box> entry_boxes(tlas_items.size());
    for (const BuildItem& it : tlas_items) entry_boxes[it.ref_payload] = it.box;
    s->entry_boxes.clear();   // pt_world_entry_box: the f64 boxes, before the f32 rounding
    for (const Box& b : entry_boxes)
        for (double x : {b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z}) s->entry_boxes.push_back(x);
    // the light grid: its box and dims are settled, and their refusals made, before the top level is built and anything is uploaded
    PunctualGridBuild gb{};
    s->grid_built = gb;
    if (s->punctual_selection == 1 && !s->punctual.empty()) {
        const uint64_t n = s->punctual.size();
        if (s->grid_box_given) memcpy(gb.box, s->grid_box_set, sizeof gb.box);
        else {
            Box u;
            for (const Box& b : entry_boxes) { u.grow(b.lo); u.grow(b.hi); }
            const double ub[6] = {u.lo.x, u.lo.y, u.lo.z, u.hi.x, u.hi.y, u.hi.z};
            if (entry_boxes.empty() || !grid_box_ok(ub)) return set_error("pt_world_build: the light grid needs a finite box and the world's bounds are not finite: give one (pt_scene_set_punctual_grid)");
            memcpy(gb.box, ub, sizeof gb.box);
        }
        if (s->grid_dims_set[0] != 0u) {
            memcpy(gb.dims, s->grid_dims_set, sizeof gb.dims);
            if ((uint64_t)gb.dims[0] * gb.dims[1] * gb.dims[2] * n > PLT_GRID_MAX_ENTRIES)
                return set_error("pt_world_build: the light grid's table would hold more than 2^25 entries (cells x lights): take fewer cells (pt_scene_set_punctual_grid)");
        } else {
            const double ext[3] = {gb.box[3] - gb.box[0], gb.box[4] - gb.box[1], gb.box[5] - gb.box[2]};
            const double ext_max = std::max(ext[0], std::max(ext[1], ext[2]));
            for (uint32_t R = PLT_GRID_AUTO_RES;; R /= 2u) {
                for (int ax = 0; ax < 3; ++ax) {
                    const double c = ext[ax] > 0.0 ? std::ceil((double)R * ext[ax] / ext_max) : 1.0;   // (the longest axis: exactly R)
                    gb.dims[ax] = (uint32_t)(c < 1.0 ? 1.0 : (c > (double)R ? (double)R : c));
                }
                if ((uint64_t)gb.dims[0] * gb.dims[1] * gb.dims[2] * n <= PLT_GRID_MAX_ENTRIES || R == 1u) break;
            }
        }
        gb.cells = gb.dims[0] * gb.dims[1] * gb.dims[2];
    }
    // Build the TLAS over world entries (one entry per leaf).
    Builder tl{nodes, tlas_items, 1, MAX_TLAS_DEPTH, false, nullptr};
    Box wb;
    uint32_t tlas_root = tl.build(0, tlas_items.size(), 0, wb);
    if (tl.depth_reached + 1 + max_blas_depth + 1 > TRAVERSAL_STACK) return set_error("pt_world_build: BVH too deep for the traversal stack");
    s->stack_need = (uint32_t)(tl.depth_reached + 1 + max_blas_depth + 1);
    if (exp_env("PT_VERBOSE")) fprintf(stderr, "[pt] BVH: top-level depth %d, deepest mesh tree %d, %zu nodes, %zu triangles\n", tl.depth_reached, max_blas_depth, nodes.size(), tris.size());

    // texture atlas
    std::vector<TexD> tex(s->tex.size());
    std::vector<uint8_t> atlas;
    std::vector<float> atlas_f;
    for (size_t i = 0; i < s->tex.size(); ++i) {
        tex[i] = s->tex[i].d;
        if (tex[i].kind == TEX_IMAGE) {
            tex[i].ofs = atlas.size();
            atlas.insert(atlas.end(), s->tex[i].image.begin(), s->tex[i].image.end());
        } else if (tex[i].kind == TEX_IMAGE_F32) {
            tex[i].ofs = atlas_f.size();
            atlas_f.insert(atlas_f.end(), s->tex[i].image_f.begin(), s->tex[i].image_f.end());
        }
    }
    for (TexD& t : tex)   // checkers of two solid children carry the children's values
        if (t.kind == TEX_CHECKER) {
            const TexD &a = tex[t.t1], &b = tex[t.t2];
            const bool solid = (a.kind == TEX_SOLID_RGB || a.kind == TEX_SOLID_F) && (b.kind == TEX_SOLID_RGB || b.kind == TEX_SOLID_F);
            t.flat = solid ? 1u : 0u;
            for (int c = 0; c < 3; ++c) { t.c1[c] = solid ? a.v[c] : 0.0; t.c2[c] = solid ? b.v[c] : 0.0; }
        }
    std::vector<MatD> mats = s->mats;   // solid textures' values into the material records (MatD::color_solid)
    for (const PrimRef& pr : prims)   // a medium that bounds something in the world (MatD::p[5], pt_dev_medium.h)
        if (mats[pr.mat].kind == MAT_MEDIUM) mats[pr.mat].p[5] = 1.0;
        else if (mats[pr.mat].kind == MAT_GLASS && mats[pr.mat].p[0] != 0.0) mats[(size_t)mats[pr.mat].p[0] - 1].p[5] = 1.0;   // ... or fills a glass object
    for (MatD& m : mats) {
        m.color_solid = m.rough_solid = 0u;
        const bool has_color = m.kind == MAT_DIFFUSE || m.kind == MAT_METAL || m.kind == MAT_PRINCIPLED || m.kind == MAT_LIGHT;
        const bool has_rough = m.kind == MAT_METAL || m.kind == MAT_GLASS;
        if (has_color && m.color_tex >= 0 && (size_t)m.color_tex < tex.size() && tex[m.color_tex].kind == TEX_SOLID_RGB && !exp_env("PT_NO_SOLID_IN_MAT")) {
            m.color_solid = 1u;
            for (int c = 0; c < 3; ++c) m.color_v[c] = tex[m.color_tex].v[c];
        }
        if (has_rough && m.rough_tex >= 0 && (size_t)m.rough_tex < tex.size() && tex[m.rough_tex].kind == TEX_SOLID_F && !exp_env("PT_NO_SOLID_IN_MAT")) {
            m.rough_solid = 1u;
            m.rough_v = tex[m.rough_tex].v[0];
        }
    }
    std::vector<CuboidBox> cuboid_box;
    std::vector<EntryBox> entry_box;   // tlas_items[i] is entry i (built in entry order, before the builder permutes them)
    for (int pass = 0; pass < 2; ++pass)   // spheres / quads / cuboids first: their hits trim the mesh boxes
        for (size_t i = 0; i < entry_boxes.size(); ++i) {
            if ((entries[i].kind == ENTRY_MESH) != (pass == 1)) continue;
            EntryBox eb{};
            const Entry& e = entries[i];
            Builder::store_box(entry_boxes[i], eb.lo, eb.hi);
            eb.entry = (uint32_t)i;
            eb.kind = e.kind;
            eb.first_prim = e.first_prim;
            eb.inst = e.inst;
            eb.blas_root = e.blas_root;
            eb.extent = e.extent;
            eb.n_prims = e.n_prims;
            eb.prim_kind = ENTRYBOX_VIA_PRIMREF;
            if (e.kind != ENTRY_MESH) {   // one kind, consecutive records: the walk addresses them without prims[]
                const PrimRef& p0 = prims[e.first_prim];
                bool direct = true;
                for (uint32_t k = 0; k < e.n_prims; ++k) {
                    const PrimRef& pk = prims[e.first_prim + k];
                    direct = direct && (pk.kind & 0xFFu) == (p0.kind & 0xFFu) && pk.index == p0.index + k && pk.inst == e.inst;
                }
                if (direct && !exp_env("PT_ENTRYBOX_VIA_PRIMREF")) {
                    eb.prim_kind = p0.kind & 0xFFu;
                    eb.prim_index = p0.index;
                }
            }
            CuboidBox cb{};
            if (e.kind == ENTRY_CUBOID && eb.prim_kind == PRIM_QUAD) {   // object-space box of the six faces (they are consecutive QuadD records)
                Box local;
                for (uint32_t k = 0; k < 6; ++k) local.grow(quad_box(quads[eb.prim_index + k]));
                Builder::store_box(local, cb.lo, cb.hi);
                eb.extent = box_extent(local);
            }
            cuboid_box.push_back(cb);
            entry_box.push_back(eb);
        }
    std::vector<GridD> grids;          // the grid-density media's table and their samples, one array
    std::vector<float> grid_vals;
    for (const HostGrid& hg : s->grids) {
        grids.push_back(hg.d);
        grids.back().ofs = grid_vals.size();
        grid_vals.insert(grid_vals.end(), hg.vals.begin(), hg.vals.end());
    }
    SceneD v{};
    DeviceBuffers& dev = s->dev;
    bool ok = upload(dev, nodes, v.nodes) && upload(dev, entries, v.entries) && upload(dev, prims, v.prims) &&
              upload(dev, spheres, v.spheres) && upload(dev, quads, v.quads) && upload(dev, tris, v.tris) &&
              upload(dev, tri_gid, v.tri_gid) && upload(dev, insts, v.insts) && upload(dev, tex, v.tex) &&
              upload(dev, mats, v.mats) && upload(dev, atlas, v.atlas) && upload(dev, atlas_f, v.atlas_f) && upload(dev, lights, v.lights) && upload(dev, entry_box, v.entry_box) && upload(dev, cuboid_box, v.cuboid_box) &&
              upload(dev, light_cdf, v.light_cdf);
    if (ok && any_attr) ok = upload(dev, tri_attr, v.tri_attr);
    if (ok && any_moving) ok = upload(dev, inst_motion, v.inst_motion);
    if (ok && !grids.empty()) ok = upload(dev, grids, v.grids) && upload(dev, grid_vals, v.grid_vals);
    if (ok && !s->punctual.empty()) ok = upload(dev, s->punctual, v.punctual);
    if (ok && gb.cells != 0u) {   // the table: one row of n doubles per cell, formed on the GPU from the list just uploaded
        void* table = nullptr;
        const uint32_t n = (uint32_t)s->punctual.size();
        ok = hip_ok(hipMalloc(&table, (size_t)gb.cells * n * sizeof(double)), "hipMalloc(light grid)");
        if (ok) {
            dev.allocs.push_back(table);
            hipEvent_t e0 = nullptr, e1 = nullptr;
            const bool timed = exp_env("PT_VERBOSE") && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
            if (timed) (void)hipEventRecord(e0, s->ctx->stream);
            launch_punctual_grid(v.punctual, n, gb, (double*)table, !exp_env("PT_GRID_DIRECT"), s->ctx->stream);
            if (timed) (void)hipEventRecord(e1, s->ctx->stream);
            ok = hip_ok(hipGetLastError(), "kernel launch") && hip_ok(hipStreamSynchronize(s->ctx->stream), "hipStreamSynchronize");
            float ms = 0.0f;
            if (ok && timed && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
                s->grid_build_ms = ms;
                fprintf(stderr, "[pt] light grid: %u x %u x %u cells x %u lights, %zu bytes, built in %.3f ms (%s)\n", gb.dims[0], gb.dims[1], gb.dims[2], n,
                        (size_t)gb.cells * n * sizeof(double), ms, exp_env("PT_GRID_DIRECT") ? "direct stores" : "staged through LDS");
            }
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            v.punctual_cdf = (const double*)table;
            v.punctual_grid = grid_descriptor(gb.box, gb.dims, n);
        }
    }
    if (!ok) {
        dev.release();
        return -1;
    }
    s->grid_built = gb;
    v.tlas_root = tlas_root;
    v.tlas_extent = box_extent(wb);
    v.n_entries = (uint32_t)entries.size();
    v.n_prims = (uint32_t)prims.size();
    v.n_lights = (uint32_t)lights.size();
    v.n_punctual = (uint32_t)s->punctual.size();
    v.punctual_f = s->punctual_f;
    uint32_t flat_max = TLAS_FLAT_MAX;
    if (const char* ev = exp_env("PT_FLAT_MAX")) flat_max = (uint32_t)atoi(ev);
    bool pair_ids_fit = true;   // the flat walk packs (primitive id, lane) into one word: ids of spheres / quads / cuboid faces below 2^26
    for (const Entry& e : entries) pair_ids_fit = pair_ids_fit && (e.kind == ENTRY_MESH || (uint64_t)e.first_prim + e.n_prims <= (1ull << 26));
    v.tlas_flat = entries.size() <= flat_max && pair_ids_fit && !exp_env("PT_NO_FLAT_TLAS") ? 1u : 0u;
    v.flat_pairs = 0;
    for (const Entry& e : entries) v.flat_pairs |= (v.tlas_flat && e.kind == ENTRY_CUBOID && !exp_env("PT_NO_FLAT_PAIRS")) ? 1u : 0u;
    s->stack_need_extend2 = v.tlas_flat ? (uint32_t)(max_blas_depth + 1) : s->stack_need;
    dev.view = v;
    s->n_prims = v.n_prims;
    s->n_mesh_entries = 0;
    s->n_punctual_built = v.n_punctual;
    s->has_moving_instance = any_moving;
    s->motionless = !any_moving;   // (a moving instance: a ray's time reaches its pose)
    for (const SphereD& sp : spheres)
        for (int i = 0; i < 3; ++i) s->motionless = s->motionless && sp.p1[i] == sp.p2[i];
    for (const Entry& e : entries) s->n_mesh_entries += e.kind == ENTRY_MESH ? 1u : 0u;
    s->built = true;
    return 0;
}
