// The scene graph (host-only): every entry point of the C ABI that edits or reads the host fields of a pt_scene, the record constructors
// they share with the flattener (pt_flatten.cpp), and the pure host twins of the motion and punctual-light rules. See pt_scene.h.
#include "pt_scene.h"
#include "pt_detmath.h"
#include "pt_dev_punctual.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "../../include/pt_amd.h"

using namespace pt;
using namespace pt::host;

static bool tex_rgb_ok(const pt_scene* s, int t) { return t >= 0 && (size_t)t < s->tex.size() && s->tex[t].is_rgb; }
static bool tex_f_ok(const pt_scene* s, int t) { return t >= 0 && (size_t)t < s->tex.size() && !s->tex[t].is_rgb; }
static bool mat_ok(const pt_scene* s, int m) { return m >= 0 && (size_t)m < s->mats.size(); }
static bool obj_ok(const pt_scene* s, int o) { return o >= 0 && (size_t)o < s->objs.size(); }

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
    if (!((tex_rgb_ok(s, t1) && tex_rgb_ok(s, t2)) || (tex_f_ok(s, t1) && tex_f_ok(s, t2))))
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
extern "C" int pt_find_registered_image(pt_scene* s, const char* name) {
    auto it = s->images.find(name);
    return it == s->images.end() ? -1 : it->second;
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
    if (!tex_rgb_ok(s, color_tex)) return set_error("pt_mat_diffuse: bad colour texture");
    MatD m = blank_mat(MAT_DIFFUSE);
    m.color_tex = color_tex;
    if (nmap >= 0) {
        if (!tex_rgb_ok(s, nmap) || (s->tex[nmap].d.kind != TEX_IMAGE && s->tex[nmap].d.kind != TEX_IMAGE_F32)) return set_error("pt_mat_diffuse: normal map must be an image texture");
        m.nmap_tex = nmap;
    }
    return push_mat(s, m);
}
extern "C" int pt_mat_metal(pt_scene* s, int color_tex, int rough_tex) {
    if (!tex_rgb_ok(s, color_tex) || !tex_f_ok(s, rough_tex)) return set_error("pt_mat_metal: bad texture handle");
    MatD m = blank_mat(MAT_METAL);
    m.color_tex = color_tex;
    m.rough_tex = rough_tex;
    return push_mat(s, m);
}
extern "C" int pt_mat_glass(pt_scene* s, int color_tex, int rough_tex, double, double ior) {
    if (!tex_rgb_ok(s, color_tex) || !tex_f_ok(s, rough_tex)) return set_error("pt_mat_glass: bad texture handle");
    MatD m = blank_mat(MAT_GLASS);
    m.color_tex = color_tex;
    m.rough_tex = rough_tex;
    m.ior = ior;
    return push_mat(s, m);
}
extern "C" int pt_mat_principled(pt_scene* s, int color_tex, const double p[11]) {
    if (!tex_rgb_ok(s, color_tex)) return set_error("pt_mat_principled: bad colour texture");
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
    if (!mat_ok(s, m1) || !mat_ok(s, m2)) return set_error("pt_mat_mix: bad material handle");
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
    if (!mat_ok(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return set_error("pt_mat_glass_set_interior: not a glass material");
    if (medium_mat != -1 && (!mat_ok(s, medium_mat) || s->mats[medium_mat].kind != MAT_MEDIUM)) return set_error("pt_mat_glass_set_interior: not a medium material (-1 = detach)");
    for (const MatD& m : s->mats)
        if (m.kind == MAT_MIX && (m.color_tex == glass_mat || m.rough_tex == glass_mat)) return set_error("pt_mat_glass_set_interior: the glass is a child of a mix");
    s->mats[glass_mat].p[0] = (double)(medium_mat + 1);
    s->built = false;
    return 0;
}
extern "C" int pt_mat_glass_interior(pt_scene* s, int glass_mat) {
    if (!s || !mat_ok(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return -1;
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
}  // namespace pt
extern "C" int pt_mat_glass_set_dispersion(pt_scene* s, int glass_mat, double abbe) {
    if (!s) return set_error("pt_mat_glass_set_dispersion: null scene");
    if (!mat_ok(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return set_error("pt_mat_glass_set_dispersion: not a glass material");
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
    if (!s || !mat_ok(s, glass_mat) || s->mats[glass_mat].kind != MAT_GLASS) return -1.0;
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
    if (mat != -1 && (!mat_ok(s, mat) || s->mats[mat].kind != MAT_MEDIUM)) return set_error("pt_scene_set_camera_medium: not a medium material (-1 = none)");
    s->camera_medium = mat;
    return 0;
}
extern "C" int pt_scene_camera_medium(pt_scene* s) { return s ? s->camera_medium : -1; }
extern "C" int pt_mat_light(pt_scene* s, int tex) {
    if (!tex_rgb_ok(s, tex)) return set_error("pt_mat_light: bad emission texture");
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
    if (!mat_ok(s, mat)) return set_error("pt_sphere: bad material");
    HostObj o;
    o.kind = OBJ_SPHERE;
    o.mat = mat;
    o.sphere.r = std::fmax(radius, 0.0);   // sphere.rs:26
    for (int i = 0; i < 3; ++i) { o.sphere.p1[i] = p1[i]; o.sphere.p2[i] = p2[i]; }
    return push_obj(s, std::move(o));
}
extern "C" int pt_quad(pt_scene* s, const double q[3], const double u[3], const double v[3], int mat) {
    if (!mat_ok(s, mat)) return set_error("pt_quad: bad material");
    HostObj o;
    o.kind = OBJ_QUAD;
    o.mat = mat;
    o.quads.push_back(make_quad(d3(q), d3(u), d3(v)));
    return push_obj(s, std::move(o));
}
extern "C" int pt_cuboid(pt_scene* s, const double a[3], const double b[3], int mat) {   // cuboid.rs:11-58
    if (!mat_ok(s, mat)) return set_error("pt_cuboid: bad material");
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
    if (!mat_ok(s, mat)) return set_error("pt_mesh: bad material");
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
    if (!obj_ok(s, obj)) return set_error("pt_instance: bad object handle");
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
void pt::pose_of_keys(const InstMotionD& k, double time, InstD& xf) {
    const double angle = k.angle0 + k.dangle * time;
    const D3 tr = d3(k.tr0) + d3(k.dtr) * time;
    make_pose(d3(k.axis), k.spins ? angle : k.angle0 + k.dangle * 0.0, tr, xf);
}
extern "C" int pt_instance_moving(pt_scene* s, int obj, const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3]) {
    if (!s) return set_error("pt_instance_moving: null scene");
    if (!obj_ok(s, obj)) return set_error("pt_instance_moving: bad object handle");
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
// (pt_scene_set_punctual_fraction also edits the device view: pt_scene_upload.cpp)
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
bool pt::grid_box_ok(const double b[6]) {
    for (int i = 0; i < 6; ++i) if (!std::isfinite(b[i])) return false;
    return b[3] >= b[0] && b[4] >= b[1] && b[5] >= b[2];
}
PunctualGridD pt::grid_descriptor(const double box[6], const uint32_t dims[3], uint32_t n) {
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
Box pt::xform_box(const Box& b, const InstD& m) {   // box of the box (aabb.rs:50-76)
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
Box pt::swept_box(const Box& b, const InstMotionD& k) {
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
    if (!obj_ok(s, obj)) return set_error(std::string(who) + ": bad object handle");
    // World::add_object / add_light take any Arc<dyn Hittable> (world.rs:18-24): the same object any number of times, under instances
    // as well. Every entry of the two lists is one PLACEMENT with its own primitive ids (pt_flatten.cpp).
    list.push_back(obj);
    s->built = false;
    return 0;
}
extern "C" int pt_world_add_object(pt_scene* s, int obj) { return place(s, obj, s->world_objects, "pt_world_add_object"); }
extern "C" int pt_world_add_light(pt_scene* s, int obj) {
    if (obj_ok(s, obj)) {   // a medium's boundary is invisible: it cannot be a light (the object an instance chain finally wraps decides)
        int oi = obj;
        for (int guard = 0; s->objs[oi].kind == OBJ_INSTANCE && guard <= 64; ++guard) oi = s->objs[oi].child;
        if (mat_ok(s, s->objs[oi].mat) && s->mats[s->objs[oi].mat].kind == MAT_MEDIUM)
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
