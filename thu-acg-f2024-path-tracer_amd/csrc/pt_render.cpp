// Context management and the wavefront render loop (host side of Camera::render,
// camera.rs:79-126): size the path pool, launch init -> {extend, shade}* -> resolve on one HIP
// stream, poll the live-slot counter every few iterations, report per-kernel HIP-event times.
// The render core is a short list of steps (render_core, below); the pixel-list, adaptive and AOV drivers follow it. The probes are
// in pt_probe.cpp, the post stage (resolve, denoise, film) in pt_post.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_kernels.h"
#include "pt_scene_gpu.h"
#include "pt_sky_tiles.h"

using namespace pt;
using namespace pt::host;

extern "C" int pt_ctx_create(int device, pt_ctx** out) {
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_error("pt_ctx_create: no HIP device available — this library has no CPU fallback");
    if (device < 0 || device >= n) return set_error("pt_ctx_create: device index out of range");
    if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return -1;
    hipDeviceProp_t prop;
    if (!hip_ok(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) return -1;
    pt_ctx* c = new pt_ctx();
    c->device = device;
    c->n_cus = prop.multiProcessorCount;
    c->name = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    if (!hip_ok(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate")) {
        delete c;
        return -1;
    }
    *out = c;
    return 0;
}
extern "C" void pt_ctx_destroy(pt_ctx* c) {
    if (!c) return;
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}
extern "C" int pt_device_name(pt_ctx* c, char* buf, uint32_t n) {
    if (!c || !buf || n == 0) return set_error("pt_device_name: bad arguments");
    strncpy(buf, c->name.c_str(), n - 1);
    buf[n - 1] = 0;
    return 0;
}
extern "C" pt_scene* pt_scene_create(pt_ctx* c) {
    if (!c) {
        set_error("pt_scene_create: null context");
        return nullptr;
    }
    pt_scene* s = new pt_scene();
    s->ctx = c;
    s->gpu = new SceneGpu();
    return s;
}
extern "C" void pt_scene_destroy(pt_scene* s) {
    if (s) delete s->gpu;   // (its members free what they hold: pt_scene_gpu.h)
    delete s;
}
extern "C" pt_ctx* pt_scene_ctx(pt_scene* s) { return s ? s->ctx : nullptr; }

// Camera::init camera.rs:51-77 (host, once per render)
namespace {
struct CamDerived {
    D3 forward, right, up, center, pixel00, pixel_du, pixel_dv;
    uint32_t height;
};
int derive_camera(const pt_camera* c, CamDerived& d) {
    if (c->image_width == 0 || !(c->aspect_ratio > 0.0)) return set_error("camera: image_width and aspect_ratio must be positive");
    d.height = (uint32_t)((double)c->image_width / c->aspect_ratio);
    if (d.height == 0) return set_error("camera: image height is zero");
    d.center = d3(c->look_from);
    double theta = c->vfov * (PI / 180.0);   // f64::to_radians
    double h = std::tan(theta / 2.0);
    double viewport_height = 2.0 * h * c->focal_length;
    double viewport_width = viewport_height * ((double)c->image_width / (double)d.height);
    d.forward = normalize(d3(c->look_from) - d3(c->look_at));
    d.right = normalize(cross(d3(c->vup), d.forward));
    d.up = cross(d.forward, d.right);
    D3 viewport_u = d.right * viewport_width;
    D3 viewport_v = d.up * -viewport_height;
    d.pixel_du = viewport_u / (double)c->image_width;
    d.pixel_dv = viewport_v / (double)d.height;
    D3 upperleft = d.center - (d.forward * c->focal_length) - (viewport_u / 2.0) - (viewport_v / 2.0);
    d.pixel00 = upperleft + (d.pixel_du + d.pixel_dv) * 0.5;
    return 0;
}
}  // namespace
extern "C" int pt_camera_init(const pt_camera* c, double out[18], uint32_t* image_height) {
    CamDerived d;
    if (derive_camera(c, d) != 0) return -1;
    const D3 v[6] = {d.forward, d.right, d.up, d.pixel00, d.pixel_du, d.pixel_dv};
    for (int i = 0; i < 6; ++i) st3(out + 3 * i, v[i]);
    *image_height = d.height;
    return 0;
}

// The sky pass's tile test (pt_sky_tiles.h) for a camera and a list of boxes: the camera as the render's kernels see it (make_camd's
// center, pixel vectors and lens vectors), and the boxes the test walks — the caller's, or their union when there are more than SKY_MAX_BOXES.
namespace {
SkyCam sky_camera(const double center[3], const double forward[3], const double pixel00[3], const double pixel_du[3], const double pixel_dv[3],
                  const double dof_right[3], const double dof_up[3], double blur_strength, uint32_t width, uint32_t height) {
    SkyCam c;
    memset(&c, 0, sizeof c);
    for (int i = 0; i < 3; ++i) {
        c.center[i] = center[i]; c.forward[i] = forward[i]; c.pixel00[i] = pixel00[i]; c.pixel_du[i] = pixel_du[i]; c.pixel_dv[i] = pixel_dv[i];
        c.dof_right[i] = dof_right[i]; c.dof_up[i] = dof_up[i];
    }
    c.blur_strength = blur_strength;
    c.width = width;
    c.height = height;
    return c;
}
std::vector<double> sky_boxes(uint32_t n_boxes, const double* boxes6) {
    std::vector<double> b(boxes6, boxes6 + 6 * (size_t)n_boxes);
    if (n_boxes <= SKY_MAX_BOXES) return b;
    std::vector<double> u(b.begin(), b.begin() + 6);
    for (uint32_t i = 1; i < n_boxes; ++i)
        for (int a = 0; a < 3; ++a) {
            if (!(b[6 * (size_t)i + a] >= u[a])) u[a] = b[6 * (size_t)i + a];           // (a NaN stays: the test then clears nothing)
            if (!(b[6 * (size_t)i + 3 + a] <= u[3 + a])) u[3 + a] = b[6 * (size_t)i + 3 + a];
        }
    return u;
}
}  // namespace
static int tiles_of(const char* who, const pt_camera* cam, uint32_t n_boxes, const double* boxes6, const uint8_t* shadeable, bool classes, uint8_t* out_tiles,
                    uint64_t* out_reach = nullptr);
extern "C" int pt_tile_reach(const pt_camera* cam, uint32_t n_boxes, const double* boxes6, uint64_t* out_masks) {
    return tiles_of("pt_tile_reach", cam, n_boxes, boxes6, nullptr, false, nullptr, out_masks);
}
extern "C" int pt_sky_tiles(const pt_camera* cam, uint32_t n_boxes, const double* boxes6, uint8_t* out_tiles) {
    return tiles_of("pt_sky_tiles", cam, n_boxes, boxes6, nullptr, false, out_tiles);
}
extern "C" int pt_short_tiles(const pt_camera* cam, uint32_t n_boxes, const double* boxes6, const uint8_t* shadeable, uint8_t* out_tiles) {
    return tiles_of("pt_short_tiles", cam, n_boxes, boxes6, shadeable, true, out_tiles);
}
// classes: the three kinds of tile (sky_tile_class), with the shadeable boxes flagged; else 1 = sure sky, 0 = not (sky_tile_is_clear).
// out_reach: the tiles' reach masks instead (sky_tile_reach, bit b = box b; more boxes than the cap: all ones unless their union is cleared)
static int tiles_of(const char* who, const pt_camera* cam, uint32_t n_boxes, const double* boxes6, const uint8_t* shadeable, bool classes, uint8_t* out_tiles,
                    uint64_t* out_reach) {
    if (!cam || (!out_tiles && !out_reach) || (n_boxes && !boxes6)) return set_error(std::string(who) + ": bad arguments");
    CamDerived d;
    if (derive_camera(cam, d) != 0) return -1;
    const double lens_radius = std::tan((cam->defocus_angle / 2.0) * (PI / 180.0)) * cam->focal_length;   // (make_camd's)
    double v[7][3];
    const D3 vec[7] = {d.center, d.forward, d.pixel00, d.pixel_du, d.pixel_dv, d.right * lens_radius, d.up * lens_radius};
    for (int i = 0; i < 7; ++i) st3(v[i], vec[i]);
    SkyCam c = sky_camera(v[0], v[1], v[2], v[3], v[4], v[5], v[6], cam->blur_strength, cam->image_width, d.height);
    const std::vector<double> boxes = sky_boxes(n_boxes, boxes6);
    const uint32_t nb = (uint32_t)(boxes.size() / 6);
    c.extent = sky_extent(c, nb, boxes.data());
    unsigned long long mask = 0ull;   // (more boxes than the cap are their union: nothing is shadeable)
    for (uint32_t b = 0; shadeable && nb == n_boxes && b < nb; ++b)
        if (shadeable[b]) mask |= 1ull << b;
    const uint32_t tiles_x = (c.width + 7) / 8, tiles_y = (c.height + 7) / 8;
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx)
            if (out_reach) {
                const unsigned long long m = sky_tile_reach(c, ty, tx, nb, boxes.data());
                out_reach[(size_t)ty * tiles_x + tx] = nb != n_boxes && m != 0ull ? ~0ull : m;
            } else
                out_tiles[(size_t)ty * tiles_x + tx] = classes ? sky_tile_class(c, ty, tx, nb, boxes.data(), mask) : sky_tile_is_clear(c, ty, tx, nb, boxes.data()) ? 1 : 0;
    return 0;
}

namespace {
struct EventTimer {   // per-launch HIP-event timing, drained at the polling syncs
    struct Pending {
        hipEvent_t a, b;
        int kind;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_list;
    double ms[6] = {0, 0, 0, 0, 0, 0};   // K2, K3, the small kernels, k_sky, k_short, k_short's pilot
    uint64_t launches[6] = {0, 0, 0, 0, 0, 0};
    bool enabled = false;
    hipEvent_t get() {
        if (!free_list.empty()) {
            hipEvent_t e = free_list.back();
            free_list.pop_back();
            return e;
        }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
    void begin(int kind, hipStream_t st) {
        ++launches[kind];
        if (!enabled) return;
        Pending p{get(), get(), kind};
        (void)hipEventRecord(p.a, st);
        pending.push_back(p);
    }
    void end(hipStream_t st) {
        if (!enabled) return;
        (void)hipEventRecord(pending.back().b, st);
    }
    void drain() {   // call after a stream sync
        for (auto& p : pending) {
            float t = 0;
            if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) ms[p.kind] += t;
            free_list.push_back(p.a);
            free_list.push_back(p.b);
        }
        pending.clear();
    }
    ~EventTimer() {
        drain();
        for (auto e : free_list) (void)hipEventDestroy(e);
    }
};
}  // namespace

// The device camera of a render (CamD) from the public one: Camera::init's derived vectors plus what K1 and K3 read per sample.
// pt_render's core and pt_render_aovs both start here, so an AOV sample traces the same camera ray as the render sample.
int pt::make_camd(pt_scene* s, const pt_camera* cam, CamD& dc) {
    CamDerived cd;
    if (derive_camera(cam, cd) != 0) return -1;
    memset(&dc, 0, sizeof dc);
    st3(dc.center, cd.center); st3(dc.pixel00, cd.pixel00); st3(dc.pixel_du, cd.pixel_du); st3(dc.pixel_dv, cd.pixel_dv);
    double lens_radius = std::tan((cam->defocus_angle / 2.0) * (PI / 180.0)) * cam->focal_length;   // camera.rs:159
    st3(dc.dof_right, cd.right * lens_radius);
    st3(dc.dof_up, cd.up * lens_radius);
    dc.blur_strength = cam->blur_strength;
    for (int i = 0; i < 3; ++i) dc.env_color[i] = cam->env_color[i];
    {   // rand 0.8.5 UniformFloat::new_inclusive(0, 2pi): scale = (high-low)/(1-eps), nudged down if needed
        const double hi = 2.0 * PI, max_rand = 1.0 - 1.0 / 4503599627370496.0;
        double scale = hi / max_rand;
        while (!(scale * max_rand <= hi)) scale = std::nextafter(scale, 0.0);
        dc.two_pi_scale = scale;
    }
    dc.width = cam->image_width;
    dc.height = cd.height;
    dc.max_depth = cam->max_depth;
    dc.env_is_map = cam->env_is_map ? 1u : 0u;
    dc.env_tex = cam->env_tex;
    dc.n_lights = s->gpu->dev.view.n_lights;
    dc.medium = s->camera_medium >= 0 ? (uint32_t)s->camera_medium + 1u : 0u;
    {   // camera.rs:159-163 with radius 0: origin = center + 0 * px + 0 * py = center bit for bit (px, py are finite), unless a
        // component of center is -0.0 (then -0 + +0 = +0): only then must the products be formed
        bool zero = true;
        for (int i = 0; i < 3; ++i)
            zero = zero && dc.dof_right[i] == 0.0 && dc.dof_up[i] == 0.0 && !(dc.center[i] == 0.0 && std::signbit(dc.center[i]));
        dc.lens_zero = zero ? 1u : 0u;
        // sphere.rs:64-66: center = p1 + (p2 - p1) * time; with p1 == p2 that is p1 + (+0) * time = p1 for every time in [0, 1)
        dc.motionless = s->motionless && !exp_env("PT_DRAW_TIME") ? 1u : 0u;
    }
    if (dc.env_is_map) {
        if (cam->env_tex < 0 || (size_t)cam->env_tex >= s->tex.size() || (s->tex[cam->env_tex].d.kind != TEX_IMAGE && s->tex[cam->env_tex].d.kind != TEX_IMAGE_F32))
            return set_error("pt_render: env_tex must be an image texture of this scene");
    }
    // the projection (pt_scene_set_projection's rule): what kinds 1-3 read on top of the above, and their refusals
    dc.projection = (uint32_t)s->projection;
    dc.th = (cam->vfov * (PI / 180.0)) / 2.0;
    dc.focal_length = cam->focal_length;
    dc.fw = (double)dc.width;
    dc.fh = (double)dc.height;
    st3(dc.forward, cd.forward); st3(dc.right, cd.right); st3(dc.up, cd.up);
    dc.shutter_open = s->shutter_open;   // (pt_scene_set_shutter; read where motion is in effect)
    dc.shutter_span = s->shutter_close - s->shutter_open;
    if ((dc.projection == PROJ_FISHEYE || dc.projection == PROJ_PANORAMA) && cam->defocus_angle != 0.0)
        return set_error("camera: the fisheye and panorama projections have no lens (defocus_angle must be 0)");
    if (dc.projection == PROJ_FISHEYE) {
        if (!std::isfinite(cam->vfov) || !(cam->vfov > 0.0)) return set_error("camera: the fisheye projection needs a finite vfov > 0");
        const double a = (double)dc.width / (double)dc.height;
        if (std::sqrt(a * a + 1.0) * dc.th > PI)
            return set_error("camera: the fisheye image circle must cover the frame: sqrt((W/H)^2 + 1) * vfov / 2 may not exceed 180 degrees (lower vfov)");
    }
    return 0;
}

// Environment importance sampling: the tables of the camera's environment map, built once per (scene, texture) at the
// first call that needs them — from the device atlas, by pt_envmap.hip — and kept until pt_scene_destroy (one texture's at a time).
// `e` gets the tables and Z; e.z > 0 (finite) is the map's half of the in-effect rule. The caller has checked dc.env_is_map.
int pt::env_tables(pt_scene* s, const CamD& dc, hipStream_t st, EnvTabD& e) {
    memset(&e, 0, sizeof e);
    if (s->env_tab_tex != dc.env_tex) {
        TexD T;
        if (!hip_ok(hipMemcpyAsync(&T, s->gpu->dev.view.tex + dc.env_tex, sizeof T, hipMemcpyDeviceToHost, st), "hipMemcpy(env texture)") ||
            !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(env texture)"))
            return -1;
        s->gpu->env_tab.release();   // the tables are forgotten before they are rebuilt: a failed rebuild leaves none
        s->env_tab_tex = -1;
        s->env_tab_w = T.w;
        s->env_tab_h = T.h;
        s->env_tab_z = 0.0;
        if (T.w != 0 && T.h != 0) {
            const size_t n_col = (size_t)T.h * (T.w + 1), bytes = (n_col + T.h + 1) * sizeof(double);
            if (!s->gpu->env_tab.reserve(bytes, "hipMalloc(env tables)")) return -1;
            double* tab = s->gpu->env_tab.as<double>();
            launch_env_tables(s->gpu->dev.view, T, tab, tab + n_col, st);
            if (!hip_ok(hipGetLastError(), "env tables") ||
                !hip_ok(hipMemcpyAsync(&s->env_tab_z, tab + n_col + T.h, sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(env Z)") ||
                !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(env tables)"))
                return -1;
        }
        s->env_tab_tex = dc.env_tex;
    }
    e.w = s->env_tab_w;
    e.h = s->env_tab_h;
    e.f = s->env_f;
    if (s->gpu->env_tab && std::isfinite(s->env_tab_z) && s->env_tab_z > 0.0) {
        e.col = s->gpu->env_tab.as<double>();
        e.row = e.col + (size_t)e.h * (e.w + 1);
        e.z = s->env_tab_z;
    }
    return 0;
}

// The shading mode of a render (pt_types.h ShadeMode), or an error: which of the exclusive features is in effect (the rules: pt_amd.h),
// the refusal of two of them at once and of what a mode's path records or kernels cannot hold. env: the table argument of a mode that
// has one (pt_types.h mode_has_table), zeroed by the caller.
static int render_mode(pt_scene* s, const CamD& dc, hipStream_t st, ShadeMode& mode, EnvTabD& env) {
    // environment sampling is in effect: f > 0, the environment is a map and its weight Z > 0 (pt_amd.h); otherwise no new code runs
    if (s->env_f > 0.0 && dc.env_is_map && env_tables(s, dc, st, env) != 0) return -1;
    const bool env_on = env.z > 0.0;   // (env arrives zeroed: only env_tables sets a weight)

    // participating media are in effect (pt_amd.h): a world object carries a medium material or a glass with an interior, or the camera medium is set
    const bool med = s->media_on();
    if (med && env_on) return set_error("pt_render: environment importance sampling together with participating media is not supported (set one of them off)");
    if (med && dc.max_depth > MEDIUM_BOUNCE_MASK) return set_error("pt_render: max_depth must be below 2^20 when participating media are in effect");

    // exact light sampling is in effect (pt_amd.h): kind 1 and a mesh or sphere entry in the lights list; otherwise no new code runs
    const bool lse = s->light_sampling_on();
    if (lse && env_on) return set_error("pt_render: exact light sampling together with environment importance sampling is not supported (set one of them off)");
    if (lse && med) return set_error("pt_render: exact light sampling together with participating media is not supported (set light sampling to 0 or take the media out)");
    if (lse && s->light_mesh_bad_area) return set_error("pt_render: exact light sampling needs light meshes of finite, positive area (a mesh in the lights list has area 0 or a non-finite one)");
    if (lse && s->light_blas_depth > (uint32_t)LIGHT_STACK) return set_error("pt_render: exact light sampling: a light mesh's BVH is deeper than the 24 levels its pdf walk's stack holds");

    // spectral dispersion is in effect (pt_amd.h): some world object's material is a glass with an Abbe number; otherwise no new code runs
    const bool dsp = s->dispersion_on();
    if (dsp && env_on) return set_error("pt_render: spectral dispersion together with environment importance sampling is not supported (set one of them off)");
    if (dsp && med) return set_error("pt_render: spectral dispersion together with participating media or a glass interior is not supported (clear the dispersion or take the media out)");
    if (dsp && lse) return set_error("pt_render: spectral dispersion together with exact light sampling is not supported (set one of them off)");
    if (dsp && dc.max_depth > DSP_BOUNCE_MASK) return set_error("pt_render: max_depth must be below 2^31 when spectral dispersion is in effect");
    if (dsp && !(env.col = dispersion_table(s, st))) return -1;   // the DSP forms read the weight table where the ENV forms read their tables (pt_types.h)
    // motion is in effect (pt_amd.h): a placed instance was made by pt_instance_moving, or the shutter is not (0, 1) and something moves. Its
    // kernels are plain-mode forms (pt_forms.h), so it excludes every other mode; otherwise no new code runs
    const bool mot = s->motion_on();
    if (mot && env_on) return set_error("pt_render: motion together with environment importance sampling is not supported (set the sampling off, or take the moving instances out and reset the shutter)");
    if (mot && med) return set_error("pt_render: motion together with participating media or a glass interior is not supported (take the media out, or take the moving instances out and reset the shutter)");
    if (mot && lse) return set_error("pt_render: motion together with exact light sampling is not supported (set light sampling to 0, or take the moving instances out and reset the shutter)");
    if (mot && dsp) return set_error("pt_render: motion together with spectral dispersion is not supported (clear the dispersion, or take the moving instances out and reset the shutter)");
    // punctual lights are in effect (pt_amd.h): the list held a light at the last build. Their kernels are plain-mode forms without motion
    // (pt_forms.h), and a path's SHADOW flag and light index ride in bits 20..31 of its bounce word; otherwise no new code runs.
    // Light shafts (pt_scene_set_punctual_media): with the option set, punctual lights and media in the modes MED and HET are
    // in effect together — forms of their own, whose bounce word holds the medium, the flag, the index and an 8-bit bounce number (pt_types.h SHF_*).
    const bool plt = s->punctual_on();
    const bool shf = plt && med && s->punctual_media != 0;
    if (shf && s->interior_on()) return set_error("pt_render: punctual lights together with a glass interior or a tinted medium are not supported, also with pt_scene_set_punctual_media (take the interiors / tinted media out, or clear the punctual lights and rebuild)");
    if (shf && dc.max_depth > SHF_BOUNCE_MASK) return set_error("pt_render: max_depth must be at most 255 when punctual lights light participating media (pt_scene_set_punctual_media)");
    if (plt && env_on) return set_error("pt_render: punctual lights together with environment importance sampling are not supported (set the sampling off, or clear the punctual lights and rebuild)");
    if (plt && med && !shf) return set_error("pt_render: punctual lights together with participating media or a glass interior are not supported (take the media out, or clear the punctual lights and rebuild)");
    if (plt && lse) return set_error("pt_render: punctual lights together with exact light sampling are not supported (set light sampling to 0, or clear the punctual lights and rebuild)");
    if (plt && dsp) return set_error("pt_render: punctual lights together with spectral dispersion are not supported (clear the dispersion, or clear the punctual lights and rebuild)");
    if (plt && mot) return set_error("pt_render: punctual lights together with motion are not supported (take the moving instances out and reset the shutter, or clear the punctual lights and rebuild)");
    if (plt && dc.max_depth > PLT_BOUNCE_MASK) return set_error("pt_render: max_depth must be below 2^20 when punctual lights are in effect");
    mode = dsp ? MODE_DSP : lse ? MODE_LSE : !med ? (env_on ? MODE_ENV : MODE_PLAIN) : s->interior_on() ? MODE_INT : s->grid_media_on() ? MODE_HET : MODE_MED;
    return 0;
}


// ---- the render core, step by step (render_core, at the end, calls them in this order) ------------------------------------------------
namespace {

// What one call renders: the caller's arguments and what the camera and the scene make of them.
struct Job {
    pt_render_opts opts;
    hipStream_t st;
    uint64_t seed;
    uint32_t spp_begin, spp_end, spp;
    const uint32_t *d_list, *h_list;   // a pixel-list render (PoolD::list): the device list, sorted by tiled index, and the same pixels on the host
    uint32_t n_list;
    bool list;
    uint32_t n_pixels, n_items;   // of the frame; rendered (the list's, or all)
    CamD dc;
    ShadeMode mode;
    EnvTabD env;   // the table argument of a mode that has one
    // the sky pass (classify_sky): on, and then the tiles of the frame the wavefront still renders, the sure-sky tiles k_sky
    // renders, their list on the device, the pixels of theirs inside the image and the samples one k_sky wave takes
    bool sky = false;
    uint32_t n_active_tiles = 0, n_sky_tiles = 0, n_sky_pixels = 0, sky_chunk = 0;
    const uint32_t* sky_list = nullptr;
    const uint32_t* tile_map = nullptr;   // where classify_sky wrote the map: tiled_accum checks that the kernels will look there
    // the short-path pass (classify_sky, run_short): the short tiles taken, their pixels inside the image, their list on the
    // device, the hard samples the pass left to the wavefront, the samples it finished and their segments
    uint32_t n_short_tiles = 0, n_short_pixels = 0;
    const uint32_t* short_list = nullptr;
    uint64_t n_hard = 0, short_samples = 0, short_segments = 0;
    uint32_t short_chunk = 0, short_sample_bits = 0;
    bool short_wide = false;
    const uint32_t* shade_prims = nullptr;
    // the tiles' reach masks, the shadeable primitives' places in the top level's loop (ShortArgsD), the direct hit is on
    const uint32_t *reach = nullptr, *shade_at = nullptr;
    bool short_direct = false;
    unsigned long long* short_words = nullptr;   // k_short's device words (ShortArgsD::n_hard, SHORT_WORDS of them; pt_types.h says which is which)
    ShortHdrD short_hdr;   // the record behind the tile map (run_short)
    // the yield pilot (DESIGN.md §23 "Taking tiles by yield"; classify_sky, select_by_yield): it ran; the tiles it added to the short list and
    // their pixels inside the image; the entries the hard list holds (the proven tiles' worst case + the taken tiles' projection with its
    // margin); the pass overflowed that list and ran again with the proven tiles alone; the miss proof's stack budget; the classification's
    // device buffers, which the fallback selects from once more
    bool pilot_ran = false, short_fallback = false;
    uint32_t n_pilot_tiles = 0, n_pilot_pixels = 0, walk_cap = SHORT_WALK_STACK, n_tiles = 0;
    // the bounces' miss proofs run in dense passes; the records they walked and the passes; the short pass's waves per tile x this
    bool short_defer = true, prof = false;   // (prof: PT_PROF, for the diagnostic build's print)
    uint64_t short_walks = 0, short_walk_passes = 0, short_direct_tiles = 0, short_self_prims = 0;
    uint32_t short_chunk_mult = 4;
    uint64_t short_cap_entries = 0;
    uint8_t* d_flags = nullptr;
    uint32_t *d_counts = nullptr, *d_pilot = nullptr, *d_hist = nullptr, *d_tile_map = nullptr, *d_sky_list = nullptr, *d_short_list = nullptr;
    ShadeForm form;   // the form of K1 / K3 this render launches (render_core; classify_sky and choose_kernels both read this one)
};

// Every experiment switch of a render (exp_env: read under PT_EXPERIMENT=1 only), read once. An explicit option wins over its switch.
constexpr size_t SKY_HDR_BYTES = 32 + SHORT_WORDS * sizeof(unsigned long long);   // classify_sky's eight counts, then k_short's words
constexpr uint32_t PILOT_SAMPLES = 8, PILOT_MIN = 256;   // the yield pilot's samples per pixel; the shortest sample range it runs on
constexpr double PILOT_THETA = 0.5;                      // the pilot yield from which a tile is taken
struct Switches {
    uint32_t slots_per_pixel = 0;   // opts.slots_per_pixel, else PT_SLOTS_PER_PIXEL
    bool pool_slots_set = false;    // PT_POOL_SLOTS: the dynamic pool's size (plan_pool refuses 0)
    uint64_t pool_slots = 0;
    int shade_variant = 42;   // k_shade<sort, min waves/SIMD>: sort*10 + waves (12 = windowed material sort with 256 threads / 2048-slot windows, 2 = plain;
                              // [r3] 22 = the same with 512 threads / 4096-slot windows: K3 -2 % on scenes 6, 3 and 5; 32 = 8192-slot windows: another
                              // -1.6 % on scene 6's 33.6 M-slot pool, +2.5 % on scene 5's 16.8 M; 42 = per launch, 32 while the pool holds >= 16 such
                              // windows per block launched, else 22)
    bool pool_in_place = false, no_defer_regen = false, no_compact_records = false, init_shuffle = false, accum_linear = false, no_compact_pool = false,
         prof = false, no_sky_pass = false, no_short_pass = false;   // no_sky_pass: PT_SKY_PASS=0; no_short_pass: PT_SHORT_PASS=0
    uint64_t short_cap_bytes = 0;   // PT_SHORT_CAP_BYTES: the hard list's byte cap in place of the pool's bytes (0: not set)
    // the yield pilot of the short-path pass: PT_SHORT_PILOT=0 turns it off (the A/B switch inside one library);
    // PT_PILOT_ANY_RANGE=1 lets it run on a sample range shorter than PILOT_MIN; PT_PILOT_THETA=x: tiles are taken from a pilot yield of x
    // (read in sixteenths, rounded up); PT_PILOT_MARGIN=x: the taken tiles' part of the hard list is x times the projection and nothing
    // more (default: 1.5 times and 64 entries per tile); PT_PILOT_STACK=n: the miss proof's stack budget, 0 .. SHORT_WALK_STACK entries;
    // PT_PILOT_NARROW=1: no more tiles than 4-byte list entries address
    bool no_pilot = false, pilot_any_range = false, pilot_margin_set = false, pilot_narrow = false;
    double pilot_theta = PILOT_THETA, pilot_margin = 1.5;
    uint32_t walk_cap = SHORT_WALK_STACK;
    // PT_SHORT_DEFER=0: k_short walks for a bounce where it enters a mesh's box (the A/B switch of DESIGN.md §23.2 inside one library);
    // PT_SHORT_CHUNK_MULT=n: the short pass cuts its tiles' samples into n times as many waves as k_sky's rule would (k_sky's chunks stay).
    // Default 4: k_short's waves differ a lot in cost and the kernel's end ran underfilled — headline ms_short 327.8 / 316.5 / 310.8 / 308.2
    // at 1 / 2 / 4 / 8, spreads under 1 ms (profiles/r25_short_defer.md); 8 was not taken: its last 2.6 ms put chunks at the 32-sample floor from 500 spp down
    bool no_short_defer = false;
    uint32_t short_chunk_mult = 4;
    // DESIGN.md §23.3, each the A/B switch of its step inside one library: PT_SHORT_REACH=0: k_short's camera rays test every entry (the masks
    // are all ones); PT_SHORT_DIRECT=0: a tile whose mask names one shadeable entry walks the top level like any other; PT_SHORT_SELF=0: a bounce
    // tests the quad it left
    bool no_short_reach = false, no_short_direct = false, no_short_self = false;
    int grid_mult = 1;   // persistent grids: resident blocks per CU x CUs x this
    uint32_t wide_window_min = 16;
    int ext2 = 0;        // PT_EXT2 = stack*10 + blocks per CU picks the two-phase K2's instantiation (0: not set)
    // k_extend2's mid-window rounds (pt_k2_extend.h "rounds of a window"): PT_K2_SPLIT=0: none (the A/B switch inside one library), 1: a full
    // window whose first half fills more than half of the candidate list runs phase B there, 2: the drain form. PT_K2_BLOCKS=n: K2's
    // persistent grid is n blocks — with the product grid every window of a pool under 2 M slots is a tail window, so a test of a full
    // window's code has to ask for fewer.
    uint32_t k2_split = 1;
    int k2_blocks = 0;
    enum { K2_AUTO, K2_BATCH, K2_TWOPHASE } k2 = K2_AUTO;   // PT_K2=batch forces the batch kernel, twophase the two-phase one where it can run
    uint64_t compact_num = 1, compact_den = 2;   // compact when live <= num/den of the slots still covered (25 % .. 85 % measured level: within 0.5 %)
    uint32_t poll_cap = 8;
};
Switches read_switches(const pt_render_opts& opts) {
    Switches sw;
    sw.slots_per_pixel = opts.slots_per_pixel;
    if (sw.slots_per_pixel == 0)
        if (const char* e = exp_env("PT_SLOTS_PER_PIXEL")) sw.slots_per_pixel = (uint32_t)atoi(e);
    if (const char* e = exp_env("PT_POOL_SLOTS")) {
        sw.pool_slots_set = true;
        sw.pool_slots = strtoull(e, nullptr, 10);
    }
    if (const char* e = exp_env("PT_SHADE_VARIANT")) sw.shade_variant = atoi(e);
    sw.pool_in_place = exp_env("PT_POOL_IN_PLACE") != nullptr;
    sw.no_defer_regen = exp_env("PT_NO_DEFER_REGEN") != nullptr;
    sw.no_compact_records = exp_env("PT_NO_COMPACT_RECORDS") != nullptr;
    sw.init_shuffle = exp_env("PT_INIT_SHUFFLE") != nullptr;
    if (const char* e = exp_env("PT_GRID_MULT")) sw.grid_mult = std::max(1, atoi(e));
    if (const char* e = exp_env("PT_WIDE_WINDOW_MIN")) sw.wide_window_min = (uint32_t)std::max(1, atoi(e));
    if (const char* e = exp_env("PT_EXT2")) sw.ext2 = atoi(e);
    if (const char* e = exp_env("PT_K2_SPLIT")) sw.k2_split = (uint32_t)std::min(2, std::max(0, atoi(e)));
    if (const char* e = exp_env("PT_K2_BLOCKS")) sw.k2_blocks = std::max(0, atoi(e));
    if (const char* e = exp_env("PT_K2")) sw.k2 = !strcmp(e, "batch") ? Switches::K2_BATCH : !strcmp(e, "twophase") ? Switches::K2_TWOPHASE : Switches::K2_AUTO;
    sw.accum_linear = exp_env("PT_ACCUM_LINEAR") != nullptr;
    sw.no_compact_pool = exp_env("PT_NO_COMPACT_POOL") != nullptr;
    if (const char* e = exp_env("PT_COMPACT_AT")) { sw.compact_num = (uint64_t)std::max(1, atoi(e)); sw.compact_den = 100; }   // per cent
    if (const char* e = exp_env("PT_POLL_CAP")) sw.poll_cap = (uint32_t)std::max(1, atoi(e));
    sw.prof = exp_env("PT_PROF") != nullptr;
    if (const char* e = exp_env("PT_SKY_PASS")) sw.no_sky_pass = atoi(e) == 0;
    if (const char* e = exp_env("PT_SHORT_PASS")) sw.no_short_pass = atoi(e) == 0;
    if (const char* e = exp_env("PT_SHORT_CAP_BYTES")) sw.short_cap_bytes = strtoull(e, nullptr, 10);
    if (const char* e = exp_env("PT_SHORT_PILOT")) sw.no_pilot = atoi(e) == 0;
    if (const char* e = exp_env("PT_PILOT_ANY_RANGE")) sw.pilot_any_range = atoi(e) != 0;
    if (const char* e = exp_env("PT_PILOT_THETA")) sw.pilot_theta = atof(e);
    if (const char* e = exp_env("PT_PILOT_MARGIN")) { sw.pilot_margin_set = true; sw.pilot_margin = std::max(0.0, atof(e)); }
    if (const char* e = exp_env("PT_PILOT_STACK")) sw.walk_cap = (uint32_t)std::min<int>(SHORT_WALK_STACK, std::max(0, atoi(e)));
    if (const char* e = exp_env("PT_PILOT_NARROW")) sw.pilot_narrow = atoi(e) != 0;
    if (const char* e = exp_env("PT_SHORT_DEFER")) sw.no_short_defer = atoi(e) == 0;
    if (const char* e = exp_env("PT_SHORT_REACH")) sw.no_short_reach = atoi(e) == 0;
    if (const char* e = exp_env("PT_SHORT_DIRECT")) sw.no_short_direct = atoi(e) == 0;
    if (const char* e = exp_env("PT_SHORT_SELF")) sw.no_short_self = atoi(e) == 0;
    if (const char* e = exp_env("PT_SHORT_CHUNK_MULT")) sw.short_chunk_mult = (uint32_t)std::min(64, std::max(1, atoi(e)));
    return sw;
}

// The bytes of the tiled frame accumulator (tiled_accum, below): three channel planes, and behind them the sky pass's tile map, one word per
// tile (pt_k_common.h pool_tile_map).
// tile_map_behind: where that map lies for an accumulator at `accum` — the one host statement of what pool_tile_map computes on the device.
// ... and behind the map, at the next 8-byte boundary, the short-path pass's record of its hard list (ShortHdrD; pt_k_common.h pool_short_hdr)
size_t tiled_accum_bytes(size_t n_tile_pixels) { return n_tile_pixels * 3 * sizeof(double) + ((n_tile_pixels / 64 + 1) & ~(size_t)1) * sizeof(uint32_t) + sizeof(ShortHdrD); }
uint32_t* tile_map_behind(double* accum, size_t n_tile_pixels) { return reinterpret_cast<uint32_t*>(accum + 3 * n_tile_pixels); }
ShortHdrD* short_hdr_behind(double* accum, size_t n_tile_pixels) { return reinterpret_cast<ShortHdrD*>(tile_map_behind(accum, n_tile_pixels) + ((n_tile_pixels / 64 + 1) & ~(size_t)1)); }

// The short-path pass's helpers. short_entries_wide: a hard-list entry of a list of n_listed tiles needs 8 bytes.
// short_pool / short_args: what k_short and its pilot read of the pool — the frame, its tiling, the sample range, the tiled planes — and
// the arguments the two launches share. adopt_tile_counts: the job's view of k_sky_scan's counts, and the samples one wave takes.
bool short_entries_wide(const Job& job, uint64_t n_listed) {
    uint32_t ord_bits = 1u;
    while ((1ull << ord_bits) < n_listed) ++ord_bits;
    return ord_bits + 6u + job.short_sample_bits > 32u;
}
PoolD short_pool(pt_scene* s, const Job& job) {
    PoolD pool;
    memset(&pool, 0, sizeof pool);
    pool.accum = s->gpu->tile_accum.as<double>();
    pool.accum_tiled = 1u;
    pool.width = job.dc.width;
    pool.height = job.dc.height;
    pool.tiles_x = (job.dc.width + 7) / 8;
    pool.n_tile_pixels = (uint32_t)((size_t)pool.tiles_x * ((job.dc.height + 7) / 8) * 64);
    pool.spp_begin = job.spp_begin;
    pool.spp_end = job.spp_end;
    return pool;
}
ShortArgsD short_args(const pt_scene* s, const Job& job) {
    ShortArgsD a;
    memset(&a, 0, sizeof a);
    a.shade_prims = job.shade_prims;
    a.n_shade = (uint32_t)s->shade_prims.size();
    a.n_hard = job.short_words;
    a.sample_bits = job.short_sample_bits;
    a.walk_cap = job.walk_cap;
    a.defer = job.short_defer ? 1u : 0u;
    a.reach = job.reach;
    a.shade_at = job.shade_at;
    a.direct = job.short_direct ? 1u : 0u;
    return a;
}
void adopt_tile_counts(const pt_scene* s, Job& job, const uint32_t counts[8]) {
    job.n_active_tiles = counts[0];
    job.n_sky_tiles = counts[1];
    job.n_sky_pixels = counts[2];
    job.n_short_tiles = counts[3];
    job.n_short_pixels = counts[4];
    job.n_pilot_tiles = counts[6];
    job.n_pilot_pixels = counts[7];
    job.short_wide = short_entries_wide(job, (uint64_t)counts[5] + counts[6]);
    // one wave renders `chunk` samples of a tile: enough waves to fill the machine four times over, at least 32 samples each
    const uint64_t target = (uint64_t)std::max(1, s->ctx->n_cus) * 4 * 8 * 4;
    auto chunk_for = [&](uint32_t n_tiles_of, uint32_t mult) {
        const uint64_t per_tile = std::max<uint64_t>(1, target * mult / std::max(1u, n_tiles_of));
        uint32_t chunk = (uint32_t)std::max<uint64_t>(32, (job.spp + per_tile - 1) / per_tile);
        while ((uint64_t)n_tiles_of * ((job.spp + chunk - 1) / chunk) > 0x7FFFFFFFull) chunk *= 2;   // (the kernels' wave index)
        return chunk;
    };
    job.sky_chunk = chunk_for(counts[1], 1u);
    job.short_chunk = chunk_for(counts[3], job.short_chunk_mult);
}
// The pilot's selection: k_short_select flags the piloted tiles whose yield bin is at least min_bin, k_sky_scan lists them with the proven
// short tiles and takes them out of the wavefront's map; the counts and the histogram of the yields come back (one small synchronisation).
int select_by_yield(pt_scene* s, Job& job, EventTimer& timer, uint32_t min_bin, uint32_t counts[8], uint32_t* hist) {
    (void)s;
    timer.begin(2, job.st);
    launch_short_select(job.d_flags, job.n_tiles, job.d_pilot, min_bin, job.d_hist, job.st);
    launch_sky_scan(job.dc.width, job.dc.height, 0xFFFFFFFFu, job.n_tiles, job.d_flags, job.d_tile_map, job.d_sky_list, job.d_short_list, job.d_counts, job.st);
    timer.end(job.st);
    if (!hip_ok(hipGetLastError(), "yield selection") ||
        !hip_ok(hipMemcpyAsync(counts, job.d_counts, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, job.st), "hipMemcpy(sky counts)") ||
        !hip_ok(hipMemcpyAsync(hist, job.d_hist, 3 * SHORT_YIELD_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, job.st), "hipMemcpy(pilot histogram)") ||
        !hip_ok(hipStreamSynchronize(job.st), "hipStreamSynchronize(yield selection)"))
        return -1;
    timer.drain();
    if ((uint64_t)counts[0] + counts[1] + counts[3] != job.n_tiles) return set_error("pt_render: the sky pass's tile counts do not add up (internal error)");
    return 0;
}

// The sky pass, per render: the tiles whose camera rays provably enter no box of the world are classified on the device
// (pt_sky_tiles.h; one thread per tile, then a one-block scan), the host reads the three counts back — the one small synchronisation — and
// the wavefront's work items then cover the other tiles only (PoolD::n_work_pixels, the tile map behind the tiled accumulator) while k_sky
// renders the sure-sky ones (run_wavefront). The pass is ON only for what k_sky's one form reproduces: the dynamic mode's whole-frame
// render in the plain mode with the independent sampler under the perspective projection, nothing moving, no camera medium. Everywhere
// else this step does nothing, and every kernel argument is what it was without it.
uint64_t pool_bytes_for_cap(const Switches& sw, const Job& job, int n_cus);   // (below, after plan_pool)
int classify_sky(pt_scene* s, const Switches& sw, Job& job, EventTimer& timer) {
    const CamD& dc = job.dc;
    const uint64_t n_tiles64 = (uint64_t)((dc.width + 7) / 8) * ((dc.height + 7) / 8);
    // A black constant environment: a sure-sky sample adds an exact zero, which nobody adds — there is no radiance for the pass to move,
    // and the wavefront's miss is at its cheapest (no lookup, no atomic). Measured on scene 3 at 1920x1920 (8.2 % sure-sky tiles beside the
    // open box): -1.3 % with the pass. Such a render keeps the wavefront alone and does not pay for the classification either.
    const bool black = !dc.env_is_map && dc.env_color[0] == 0.0 && dc.env_color[1] == 0.0 && dc.env_color[2] == 0.0;
    const bool on = !black && sw.slots_per_pixel == 0 && !job.list && job.mode == MODE_PLAIN && s->sampler == 0 && dc.projection == PROJ_PERSPECTIVE && !s->motion_on() && !s->punctual_on() &&
                    shade_form_maps_tiles(job.form) && s->camera_medium < 0 && !sw.no_sky_pass && !sw.accum_linear /* k_sky adds into the tiled planes */ && job.spp != 0 && dc.max_depth != 0 &&
                    n_tiles64 * 64 <= 0x7FFFFFFFull /* (plan_pool refuses the rest) */;
    if (!on) return 0;
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    const std::vector<double> boxes = sky_boxes((uint32_t)(s->entry_boxes.size() / 6), s->entry_boxes.data());
    const uint32_t n_boxes = (uint32_t)(boxes.size() / 6);
    SkyCam cam = sky_camera(dc.center, dc.forward, dc.pixel00, dc.pixel_du, dc.pixel_dv, dc.dof_right, dc.dof_up, dc.blur_strength, dc.width, dc.height);
    cam.extent = sky_extent(cam, n_boxes, boxes.data());
    // The short-path pass is on where the sky pass is, and only when K2 walks the top level flat (k_short calls that walk), the
    // scene has no lights list (the selector draw then only moves the counter), some entry is shadeable (pt_flatten.cpp; every entry has its own
    // box here: more than SKY_MAX_BOXES would be walked as their union) and a path may have two segments.
    unsigned long long shadeable = 0ull;
    const bool short_on = !sw.no_short_pass && s->gpu->dev.view.tlas_flat != 0u && s->gpu->dev.view.n_lights == 0u && !s->shade_prims.empty() && dc.max_depth >= 2u && job.spp <= (1u << 26) /* k_short packs pixel << sample_bits | sample in 32 bits */ &&
                          s->entry_shadeable.size() == (size_t)n_boxes && s->entry_boxes.size() / 6 == (size_t)n_boxes &&
                          n_boxes <= 32u /* k_short walks the top level by a 32-bit mask of entries; a flat top level of more (PT_FLAT_MAX) keeps the wavefront */;
    if (short_on)
        for (uint32_t i = 0; i < n_boxes; ++i)
            if (s->entry_shadeable[i]) shadeable |= 1ull << i;
    // sky_mem: the counts and k_short's words (SKY_HDR_BYTES), the boxes, the sure-sky tile list, the short tile list, the shadeable primitives'
    // ids, the tiles' flags; the tile map lies behind the tiled accumulator's planes
    const size_t box_bytes = (size_t)SKY_MAX_BOXES * 6 * sizeof(double), prim_bytes = (size_t)SKY_MAX_BOXES * sizeof(uint32_t);
    // ... and behind the flags, at the next 8-byte boundary, the yield pilot's two words per tile and its histogram
    const size_t pilot_at = (SKY_HDR_BYTES + box_bytes + prim_bytes + (size_t)n_tiles * (2 * sizeof(uint32_t) + 1) + 7) & ~(size_t)7;
    // ... and behind those the tiles' reach masks, one word per tile
    const size_t reach_at = pilot_at + ((size_t)n_tiles * 2 + 3 * SHORT_YIELD_BINS) * sizeof(uint32_t);
    if (!s->gpu->sky_mem.reserve(reach_at + (size_t)n_tiles * sizeof(uint32_t), "hipMalloc(sky pass)")) return -1;
    if (!s->gpu->tile_accum.reserve(tiled_accum_bytes((size_t)n_tiles * 64), "hipMalloc(tiled accumulator)")) return -1;
    char* m = s->gpu->sky_mem.as<char>();
    uint32_t* d_counts = (uint32_t*)m;
    double* d_boxes = (double*)(m + SKY_HDR_BYTES);
    uint32_t* d_prims = (uint32_t*)(m + SKY_HDR_BYTES + box_bytes);
    uint32_t* d_sky_list = (uint32_t*)(m + SKY_HDR_BYTES + box_bytes + prim_bytes);
    uint32_t* d_short_list = d_sky_list + n_tiles;
    uint8_t* d_flags = (uint8_t*)(d_short_list + n_tiles);
    uint32_t* d_tile_map = tile_map_behind(s->gpu->tile_accum.as<double>(), (size_t)n_tiles * 64);
    uint32_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    job.n_tiles = n_tiles;
    job.d_flags = d_flags;
    job.d_counts = d_counts;
    job.d_pilot = (uint32_t*)(m + pilot_at);
    job.d_hist = job.d_pilot + (size_t)n_tiles * 2;
    job.d_tile_map = d_tile_map;
    job.d_sky_list = d_sky_list;
    job.d_short_list = d_short_list;
    job.shade_prims = d_prims;
    // (the shadeable ids take at most TLAS_FLAT_MAX of the SKY_MAX_BOXES words: their places in the loop lie in the second half)
    uint32_t* d_shade_at = d_prims + SKY_MAX_BOXES / 2;
    uint32_t* d_reach = (uint32_t*)(m + reach_at);
    ReachOrder order;
    memset(&order, 0, sizeof order);
    std::vector<uint32_t> shade_at;
    const bool reach_on = short_on && s->entry_at.size() == (size_t)n_boxes && n_boxes <= TLAS_FLAT_MAX && s->shade_prims.size() <= SKY_MAX_BOXES / 2 &&
                          s->shade_entry.size() == s->shade_prims.size() && s->shade_self_ok.size() == s->shade_prims.size();
    if (reach_on) {
        for (uint32_t i = 0; i < n_boxes; ++i) order.at[i] = (uint8_t)s->entry_at[i];
        // step 3's bound on the camera rays' origins (the proof): the lens within 1e6 of the origin
        bool cam_ok = true;
        for (int i = 0; i < 3; ++i) cam_ok = cam_ok && std::fabs(dc.center[i]) + std::fabs(dc.dof_right[i]) + std::fabs(dc.dof_up[i]) <= 1e6;
        for (size_t j = 0; j < s->shade_prims.size(); ++j)
            shade_at.push_back(s->entry_at[s->shade_entry[j]] | (s->shade_self_ok[j] && cam_ok && !sw.no_short_self ? SHADE_AT_SELF_OK : 0u));
        job.shade_at = d_shade_at;
        for (uint32_t v : shade_at) job.short_self_prims += (v & SHADE_AT_SELF_OK) ? 1u : 0u;
        job.reach = sw.no_short_reach ? nullptr : d_reach;
        job.short_direct = !sw.no_short_reach && !sw.no_short_direct;
    }
    job.short_words = (unsigned long long*)(m + 32);
    job.walk_cap = sw.walk_cap;
    job.short_defer = !sw.no_short_defer;
    job.prof = sw.prof;
    job.short_chunk_mult = sw.short_chunk_mult;
    // (`boxes` and `counts` are this function's: both copies are done at its synchronise, below)
    if (n_boxes && !hip_ok(hipMemcpyAsync(d_boxes, boxes.data(), boxes.size() * sizeof(double), hipMemcpyHostToDevice, job.st), "hipMemcpy(sky boxes)")) return -1;
    if (short_on && !hip_ok(hipMemcpyAsync(d_prims, s->shade_prims.data(), s->shade_prims.size() * sizeof(uint32_t), hipMemcpyHostToDevice, job.st), "hipMemcpy(shadeable ids)")) return -1;
    if (reach_on && !hip_ok(hipMemcpyAsync(d_shade_at, shade_at.data(), shade_at.size() * sizeof(uint32_t), hipMemcpyHostToDevice, job.st), "hipMemcpy(shadeable places)")) return -1;
    auto classify = [&](uint32_t max_short) -> int {
        timer.begin(2, job.st);
        launch_sky_classify(cam, n_boxes, d_boxes, shadeable, max_short, n_tiles, d_flags, d_tile_map, d_sky_list, d_short_list, d_counts, job.reach ? d_reach : nullptr, order, job.st);
        timer.end(job.st);
        if (!hip_ok(hipGetLastError(), "sky classification") ||
            !hip_ok(hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, job.st), "hipMemcpy(sky counts)") ||
            !hip_ok(hipStreamSynchronize(job.st), "hipStreamSynchronize(sky classification)"))
            return -1;
        timer.drain();
        if ((uint64_t)counts[0] + counts[1] + counts[3] != n_tiles) return set_error("pt_render: the sky pass's tile counts do not add up (internal error)");
        return 0;
    };
    if (classify(0xFFFFFFFFu) != 0) return -1;
    job.short_sample_bits = 1u;
    while ((1ull << job.short_sample_bits) < (uint64_t)job.spp) ++job.short_sample_bits;
    const uint64_t cap_bytes = !short_on ? 0 : sw.short_cap_bytes ? sw.short_cap_bytes : pool_bytes_for_cap(sw, job, s->ctx->n_cus);
    if (counts[3] != 0) {
        // The hard list holds, at worst, every sample of the proven tiles; its bytes are capped at the pool's (or PT_SHORT_CAP_BYTES). Where the cap
        // binds the pass takes the first max_short short tiles in tile order and the rest stay the wavefront's: the classification runs once more
        // with that bound. One tile at least stays the wavefront's, whose forms read the hard list only when PoolD::n_work_pixels is not 0.
        const uint64_t entry_bytes = short_entries_wide(job, counts[5]) ? 8 : 4;
        uint64_t max_short = cap_bytes / entry_bytes / ((uint64_t)64 * job.spp);
        if (counts[0] == 0 && max_short >= counts[5]) max_short = counts[5] - 1u;
        if (max_short < counts[3] && classify((uint32_t)max_short) != 0) return -1;
    }
    // The yield pilot (DESIGN.md §23 "Taking tiles by yield"): where the short-path pass may run, the range is long enough to pay for it and
    // the cap has not already bound on the proven tiles, k_short's counting form renders the first PILOT_SAMPLES samples of every tile of the
    // wavefront's map, and the tiles it finishes at least theta of go to the short list too (select_by_yield). The histogram of the yields says
    // what the selection costs: where the list's bytes, the 4-byte entries (PT_PILOT_NARROW) or the rule that one tile stays the wavefront's
    // do not allow it, the threshold moves up bin by bin — the lowest yields are dropped first — and the selection runs once more.
    if (short_on && !sw.no_pilot && (job.spp >= PILOT_MIN || sw.pilot_any_range) && counts[3] == counts[5] && counts[0] > 1u) {
        const uint32_t n_active = counts[0], n_proven = counts[5], proven_pixels = counts[4], p_eff = std::min(PILOT_SAMPLES, job.spp);
        if (!hip_ok(hipMemsetAsync(job.d_pilot, 0, (size_t)n_tiles * 2 * sizeof(uint32_t), job.st), "hipMemset(pilot counts)")) return -1;
        PoolD pool = short_pool(s, job);
        pool.spp_end = job.spp_begin + p_eff;
        ShortArgsD a = short_args(s, job);
        a.short_list = d_tile_map;
        a.n_short = n_active;
        a.chunk = p_eff;
        a.n_chunks = 1u;
        a.pilot = job.d_pilot;
        timer.begin(5, job.st);
        launch_short(s->gpu->dev.view, job.dc, pool, job.seed, a, job.st);
        timer.end(job.st);
        uint32_t hist[3 * SHORT_YIELD_BINS];
        const uint32_t bin0 = (uint32_t)std::min(17.0, std::max(0.0, std::ceil(sw.pilot_theta * 16.0)));
        if (select_by_yield(s, job, timer, bin0, counts, hist) != 0) return -1;
        uint64_t cap_entries = 0;
        auto fits = [&](uint32_t bin) {
            uint64_t tiles = 0, seen = 0, unfinished = 0;
            for (uint32_t k = bin; k < SHORT_YIELD_BINS; ++k) {
                tiles += hist[3 * k];
                seen += hist[3 * k + 1];
                unfinished += hist[3 * k + 2];
            }
            // the taken tiles' part of the list: their projected hard samples with the margin, at most every sample of theirs
            const uint64_t projected = (unfinished * job.spp + p_eff - 1) / p_eff;
            const uint64_t with_margin = sw.pilot_margin_set ? (uint64_t)std::ceil(sw.pilot_margin * (double)projected) : projected + projected / 2 + 64 * tiles;
            cap_entries = (uint64_t)proven_pixels * job.spp + std::min<uint64_t>(with_margin, seen / p_eff * job.spp);
            const bool wide = short_entries_wide(job, n_proven + tiles);
            return tiles < n_active && !(wide && sw.pilot_narrow) && cap_entries * (wide ? 8 : 4) <= cap_bytes;
        };
        uint32_t bin = bin0;
        while (bin < SHORT_YIELD_BINS && !fits(bin)) ++bin;
        if (bin != bin0 && select_by_yield(s, job, timer, bin, counts, hist) != 0) return -1;
        (void)fits(bin);   // (bin = SHORT_YIELD_BINS takes nothing: the proven tiles' worst case, which fits)
        uint64_t tiles = 0;
        for (uint32_t k = bin; k < SHORT_YIELD_BINS; ++k) tiles += hist[3 * k];
        if (counts[6] != tiles || counts[5] != n_proven) return set_error("pt_render: the yield pilot's tile counts do not add up (internal error)");
        job.pilot_ran = true;
        job.short_cap_entries = cap_entries;
        if (sw.prof) {
            fprintf(stderr, "[pt prof] PILOT  tiles piloted %u, proven %u, threshold bin %u/16 (asked %u/16), taken %u; list entries %llu; bins (tiles, seen, unfinished):", n_active,
                    n_proven, bin, bin0, counts[6], (unsigned long long)cap_entries);
            for (uint32_t k = 0; k < SHORT_YIELD_BINS; ++k) fprintf(stderr, " %u:(%u,%u,%u)", k, hist[3 * k], hist[3 * k + 1], hist[3 * k + 2]);
            fprintf(stderr, "\n");
        }
    }
    if (counts[1] == 0 && counts[3] == 0) return 0;   // neither a sure-sky nor a short tile: the render is the wavefront's, its kernel arguments what they are without the passes
    job.sky = true;
    job.tile_map = d_tile_map;
    job.sky_list = d_sky_list;
    job.short_list = d_short_list;
    adopt_tile_counts(s, job, counts);
    if (!job.pilot_ran) job.short_cap_entries = (uint64_t)job.n_short_pixels * job.spp;   // every sample of the tiles taken (their pixels inside the image)
    return 0;
}

// The short-path pass itself, between the classification and the pool's plan: k_short renders the short tiles' samples into
// the tiled accumulator — cleared here, not by tiled_accum — and appends the hard ones to the scene's list; the host reads back their number
// and the pass's sample and segment counts (one more small synchronisation ahead of k_init) and writes the record K1 / K3 find the list by.
// The list holds every sample of the proven tiles and, of the tiles the pilot took, the projected hard samples with a margin
// (Job::short_cap_entries). k_short checks every store against that size and counts on: when the count read back is larger than the list, the
// planes are cleared again, the selection is undone (select_by_yield with a threshold no tile reaches) and the pass runs once more over the
// proven tiles alone, whose worst case the list holds.
// PT_PROF, diagnostic builds (-DPT_STAMPS): k_short's wave cycles per phase and its walks' counts (pt_k_short.hip)
void short_prof(const Job& job, const unsigned long long* words) {
#ifdef PT_STAMPS
    if (!job.prof) return;
    const unsigned long long* p = words + SHORT_PROF_AT;
    unsigned long long all = 0;
    for (int i = 0; i < 8; ++i) all += p[i];
    fprintf(stderr, "[pt prof] SHORT  defer %d, chunk %u; wave cycles: rng+ray %llu, camera top level %llu, camera walks %llu, shade %llu, bounce top level %llu, bounce walks %llu, environment %llu, rings %llu; sum %llu\n",
            job.short_defer ? 1 : 0, job.short_chunk, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], all);
    for (int w = 0; w < 2; ++w)
        fprintf(stderr, "[pt prof] SHORT  %s walks: wave-samples (passes) %llu, lanes %llu, lane-steps %llu, longest-lane steps %llu, skipped as outcome-neutral %llu\n", w ? "bounce" : "camera",
                p[8 + 8 * w], p[9 + 8 * w], p[10 + 8 * w], p[11 + 8 * w], p[12 + 8 * w]);
#else
    (void)job; (void)words;
#endif
}
int run_short(pt_scene* s, Job& job, EventTimer& timer) {
    if (!job.sky) return 0;
    const size_t n_tile_pixels = (size_t)((job.dc.width + 7) / 8) * ((job.dc.height + 7) / 8) * 64;
    double* planes = s->gpu->tile_accum.as<double>();
    ShortHdrD& hdr = job.short_hdr;   // (the job's: the copy below is asynchronous)
    memset(&hdr, 0, sizeof hdr);
    for (int pass = 0; job.n_short_tiles != 0; ++pass) {
        const uint64_t cap = job.short_cap_entries, all = (uint64_t)job.n_short_pixels * job.spp;
        if (!s->gpu->short_mem.reserve((size_t)cap * (job.short_wide ? 8 : 4), "hipMalloc(hard list)")) return -1;
        if (!hip_ok(hipMemsetAsync(planes, 0, n_tile_pixels * 3 * sizeof(double), job.st), "hipMemset(tiled accumulator)")) return -1;
        if (!hip_ok(hipMemsetAsync(job.short_words, 0, SHORT_WORDS * sizeof(unsigned long long), job.st), "hipMemset(short pass counts)")) return -1;
        const PoolD pool = short_pool(s, job);
        ShortArgsD a = short_args(s, job);
        a.short_list = job.short_list;
        a.n_short = job.n_short_tiles;
        a.chunk = job.short_chunk;
        a.n_chunks = (job.spp + job.short_chunk - 1) / job.short_chunk;
        a.hard = s->gpu->short_mem.as<void>();
        a.cap = cap;
        a.wide = job.short_wide ? 1u : 0u;
        unsigned long long words[SHORT_WORDS] = {};
        timer.begin(4, job.st);
        launch_short(s->gpu->dev.view, job.dc, pool, job.seed, a, job.st);
        timer.end(job.st);
        if (!hip_ok(hipGetLastError(), "short-path pass") ||
            !hip_ok(hipMemcpyAsync(words, job.short_words, sizeof words, hipMemcpyDeviceToHost, job.st), "hipMemcpy(short pass counts)") ||
            !hip_ok(hipStreamSynchronize(job.st), "hipStreamSynchronize(short-path pass)"))
            return -1;
        timer.drain();
        if (words[0] > all || words[0] + words[1] != all) return set_error("pt_render: the short-path pass's sample counts do not add up (internal error)");
        if (words[0] > cap) {   // more hard samples than the pilot projected, margin included: the proven tiles alone
            if (pass != 0 || !job.pilot_ran) return set_error("pt_render: the short-path pass's hard list is too small (internal error)");
            uint32_t counts[8], hist[3 * SHORT_YIELD_BINS];
            if (select_by_yield(s, job, timer, SHORT_YIELD_BINS, counts, hist) != 0) return -1;
            if (counts[6] != 0) return set_error("pt_render: the yield pilot's tile counts do not add up (internal error)");
            adopt_tile_counts(s, job, counts);
            job.short_cap_entries = (uint64_t)job.n_short_pixels * job.spp;
            job.short_fallback = true;
            continue;
        }
        job.n_hard = words[0];
        job.short_samples = words[1];
        job.short_segments = words[2];
        job.short_walks = words[3];
        job.short_walk_passes = words[4];
        job.short_direct_tiles = words[5];
        short_prof(job, words);
        hdr.hard = s->gpu->short_mem.as<void>();
        hdr.short_list = job.short_list;
        hdr.wide = a.wide;
        hdr.sample_bits = a.sample_bits;
        hdr.n_hard = job.n_hard;
        break;
    }
    return hip_ok(hipMemcpyAsync(short_hdr_behind(planes, n_tile_pixels), &hdr, sizeof hdr, hipMemcpyHostToDevice, job.st), "hipMemcpy(hard list record)") ? 0 : -1;
}

// Pool sizing (arithmetic only). slots_per_pixel = 0 (default): DYNAMIC work assignment — a fixed pool that fills
// the machine several times over; finished paths pull the next (pixel, sample) from a global
// counter. slots_per_pixel = k >= 1: STATIC ownership (deterministic; k = 1 is the reference's
// exact per-pixel sample order).
struct PoolPlan {
    bool dynamic;
    uint32_t k;   // static mode: slots per pixel as clamped here
    uint32_t tiles_x, n_tile_pixels;
    uint64_t total_work;
    uint32_t n_slots;
};
int plan_pool(const Switches& sw, const Job& job, int n_cus, PoolPlan& p) {
    uint32_t k = sw.slots_per_pixel;
    p.dynamic = k == 0;
    const uint32_t tiles_y = (job.dc.height + 7) / 8;
    p.tiles_x = (job.dc.width + 7) / 8;
    const uint64_t n_tile_pixels64 = (uint64_t)p.tiles_x * tiles_y * 64;
    if (n_tile_pixels64 > 0x7FFFFFFFull) return set_error("pt_render: image too large");
    p.n_tile_pixels = (uint32_t)n_tile_pixels64;
    // (the sky pass: the work items cover the active tiles only)
    p.total_work = p.dynamic ? (job.list ? (uint64_t)job.n_list : job.sky ? (uint64_t)job.n_active_tiles * 64 : n_tile_pixels64) * job.spp : (uint64_t)job.n_items * job.spp;
    if (p.dynamic && job.sky) p.total_work += job.n_hard;   // (the short-path pass's hard samples, behind the tile items)
    uint64_t n_slots64;
    if (p.dynamic) {
        // Resident paths: enough that per-launch fixed costs and kernel tails amortise (16.8M slots are 9% faster than
        // 4.2M on the 4000-spp frame, 33.6M another 2%), few enough that the frame's end — when the sample budget is
        // handed out and slots die — stays short: between 16K and 128K slots per CU (3.5 GB of path state at 33.6M).
        // [r3] about 64 samples per slot (was 128; 32 gained another 5-15 % on scene 6 below 500 spp but lost 4 % on scene 5 at 4K): re-measured for the sample ranges ONE RANK of an 8-GPU frame renders — scene 6
        // FHD @ 500 spp: 4.2 M slots 489 ms, 8.4 M (the old rule's choice) 426, 16.8 M 407.5, 33.6 M 409; @ 1000 spp: 8.4 M 846,
        // 16.8 M (old) 785.5, 33.6 M 779 — the long, thin end of a frame costs less than running the whole frame on a small pool.
        // [r3, last afternoon] re-measured once more with the 512-thread K3, its 8192-slot windows and the half windows at the end of K2's
        // queue (every launch's END costs less, so deeper pools pay): about 30 samples per slot and up to 512 K slots per CU — scene 6
        // FHD @ 4000 spp: 33.6 M slots 2905, 67 M 2940, 134 M 2984, 268 M 2957 Msamples/s; @ 2000: 2886 / 2903 / 2923; @ 1000: 33.6 M 2822,
        // 67 M 2836, 134 M 2752; @ 500: 16.8 M 2688, 33.6 M 2750, 67 M 2694; @ 250: 8.4 M 2484, 16.8 M 2574; scene 3 1920x1920 @ 4000:
        // 1314 / 1328 / 1359; scene 5 4K @ 1000: 4355 / 4431 / 4499 (profiles/r03_pool_sweep.txt). 134 M slots are 14 GB of path records.
        // The sky pass thins total_work, but the rule keeps reading the WHOLE frame's work: the slots hold the paths of the
        // active tiles, which are as long as they were, and a pool sized from the thinner list came out a step smaller just where the
        // steps lie — scene 6 at 1000 spp 33.5 M slots for 67 M (K2 +2 %, the frame's gain cut from 3 % to 1.3 %), at 500 spp -1.3 %.
        const uint64_t rule_work = job.list ? p.total_work : n_tile_pixels64 * job.spp;
        uint64_t per_cu = 16384;   // a power of two (the tile-ordered work items and the 64 counter shards divide it evenly)
        while (per_cu < 524288 && per_cu * 2 * (uint64_t)std::max(1, n_cus) * 30 <= rule_work) per_cu *= 2;
        // one more doubling (268 M slots, 28 GB) only from 48 samples per slot: scene 3 1920x1920 @ 4000 spp (55 per slot) 1335 -> 1362,
        // while at 31 per slot scene 6 FHD @ 4000 loses 0.7 % and scene 5 4K @ 1000 0.5 % (initialising and compacting the pool costs 58 ms there)
        if (per_cu == 524288 && per_cu * 2 * (uint64_t)std::max(1, n_cus) * 48 <= rule_work) per_cu *= 2;
        uint64_t target = (uint64_t)n_cus * per_cu;
        if (sw.pool_slots_set) {
            target = sw.pool_slots;
            if (target == 0) return set_error("pt_render: PT_POOL_SLOTS must be positive");
        }
        n_slots64 = std::min<uint64_t>(target, std::max<uint64_t>(p.total_work, 1));
    } else {
        if (k > job.spp) k = job.spp;
        if (k == 0) k = 1;
        while ((uint64_t)k * job.n_items > 0x40000000ull && k > 1) --k;
        n_slots64 = (uint64_t)k * job.n_items;
    }
    if (n_slots64 > 0x7FFFFFC0ull) return set_error("pt_render: image too large for the path pool");
    p.k = k;
    p.n_slots = (uint32_t)n_slots64;
    return 0;
}

// The bytes the hard list of the short-path pass is capped at: the pool's records and state words for the whole frame's plan
uint64_t pool_bytes_for_cap(const Switches& sw, const Job& job, int n_cus) {
    PoolPlan p;
    Job whole = job;
    whole.sky = false;
    if (plan_pool(sw, whole, n_cus, p) != 0) return 0;
    const uint64_t n_al = ((uint64_t)p.n_slots + 8191) & ~(uint64_t)8191;
    return n_al * (sizeof(RayRec) + sizeof(PathRec) + 2 * sizeof(uint32_t));
}

// The kernels of a render: the form of k_init / k_shade that exists for it, K2's variant, the persistent grids.
struct Kernels {
    ShadeForm form;
    bool ordered;      // shading-order output (PoolD::reorder)
    int extend_code;   // -1 = batch, -(stack*10 + blocks) = two-phase
    int blocks_shade;  // resident blocks per CU of the form's k_shade; 0: there is no such kernel (render_core refuses)
    int grid_extend, grid_shade;
};
// the two-phase K2's instantiation for this scene's BVHs (stack*10 + blocks per CU), 0 when its LDS stack does not cover them
int extend2_code(const pt_scene* s, const Switches& sw) {
    const int need = (int)s->stack_need_extend2;
    if (need > 32) return 0;
    // four blocks per CU where the LDS allows it (stacks of 16 and 20 entries): the kernel then runs at 128 registers with
    // 64 B of spills per lane and is still 7.5 % faster than at three blocks and 149 registers (round 2; in round 1, at
    // 166 registers, the same bound meant 168 B of spills and lost 11 %)
    // [r3, last] stacks of <= 16 entries: blocks of 128 threads over 1024-slot windows (code 2164, eight blocks per CU) — with the
    // queue's end in half windows the smaller block's shorter barrier waits win on every pool size: K2 -1.0 % (16.8 M slots), -1.8 %
    // (67 M, 134 M) against 256 threads; 64 threads: +1 % / -2.0 % / -2.5 % (worse on shallow pools); 512 threads: +5 %
    int code = need <= 16 ? 2164 : need <= 20 ? 204 : need <= 24 ? 243 : need <= 28 ? 283 : 323;
    if (const int c = sw.ext2) {
        if (c / 10 >= need && (c == 163 || c == 164 || c == 204 || c == 243 || c == 283 || c == 323)) code = c;
        if ((c == 1164 || c == 2164 || c == 8164) && need <= 16) code = c;
    }
    return code;
}
Kernels choose_kernels(const Switches& sw, const pt_scene* s, const Job& job, const PoolPlan& p) {
    Kernels kn;
    kn.form = job.form;
    // Shading-order output (PoolD::reorder): the dynamic mode's sorted whole-frame k_shade writes every path to its position in the
    // window's sorted order in a second record area, and the two areas swap after each launch — K2's chunks are then K3's groups: a tile's
    // camera rays in pixel order, or 64 paths of one material class. Static mode, pixel lists and PT_POOL_IN_PLACE write in place.
    kn.ordered = p.dynamic && !job.list && shade_form_sorts(kn.form) && !sw.pool_in_place;
    // K2 variant: two-phase kernel when there are meshes to defer and its LDS stack covers the scene's BVHs, else the
    // batch kernel (the experiment switches: Switches::k2, ext2)
    const int two_phase = extend2_code(s, sw);
    kn.extend_code = (s->n_mesh_entries > 0 && two_phase != 0) ? -two_phase : -1;
    if (sw.k2 == Switches::K2_BATCH) kn.extend_code = -1;
    else if (sw.k2 == Switches::K2_TWOPHASE && two_phase != 0) kn.extend_code = -two_phase;
    const int blocks_extend = extend_occupancy_blocks(kn.extend_code == -1 && s->gpu->dev.view.tlas_flat ? (s->gpu->dev.view.flat_pairs ? -3 : -2) : kn.extend_code, kn.form.motion);
    kn.blocks_shade = shade_occupancy_blocks(kn.form);
    kn.grid_extend = sw.k2_blocks ? sw.k2_blocks : s->ctx->n_cus * blocks_extend * sw.grid_mult;
    kn.grid_shade = s->ctx->n_cus * kn.blocks_shade * sw.grid_mult;
    return kn;
}

// The pool's memory: the scene's cached buffer grown to what THIS render needs and carved from this render's n_al (never from the cached
// capacity: a small render after a large one lays its arrays out as a fresh scene would), the scene's counters, PoolD's scalar fields.
int bind_pool(pt_scene* s, const Switches& sw, const Job& job, const PoolPlan& p, const Kernels& kn, PoolD& pool) {
    // one allocation: the two record arrays (RayRec, PathRec), the static mode's f64 arrays, the two u32 state arrays (+ the output area)
    const size_t n_al = ((size_t)p.n_slots + 8191) & ~(size_t)8191;   // whole windows: 2048 slots (k_extend2, k_shade) / 4096 (k_shade with 512 threads)
    const size_t n_f64 = p.dynamic ? 0 : 6;   // the per-slot sample sums and radiances exist in the static mode only (the dynamic mode adds into the frame)
    const size_t bytes = n_al * (sizeof(RayRec) + sizeof(PathRec) + n_f64 * sizeof(double) + 2 * sizeof(uint32_t)) +
                         (kn.ordered ? n_al * (sizeof(RayRec) + sizeof(PathRec) + sizeof(uint32_t)) : 0);
    if (!s->gpu->pool_mem.reserve(bytes, "hipMalloc(path pool)")) return -1;
    if (!s->gpu->counters()) {
        if (!s->gpu->d_counters.alloc(sizeof(CountersD), "hipMalloc(counters)")) return -1;
        if (!s->gpu->h_counters.reserve(sizeof(CountersD), "hipHostMalloc(counters)")) return -1;
    }
    memset(&pool, 0, sizeof pool);
    {
        char* m = s->gpu->pool_mem.as<char>();   // hipMalloc memory is 256-B aligned; records first (64-B aligned)
        pool.ray = (RayRec*)m; m += n_al * sizeof(RayRec);
        pool.path = (PathRec*)m; m += n_al * sizeof(PathRec);
        double* d = (double*)m;
        double** f64s[6] = {&pool.ax, &pool.ay, &pool.az, &pool.rx, &pool.ry, &pool.rz};
        for (auto f : f64s) { *f = n_f64 ? d : nullptr; d += n_f64 ? n_al : 0; }
        uint32_t* u = (uint32_t*)d;
        uint32_t** u32s[2] = {&pool.hit_prim, &pool.bounce};
        for (auto f : u32s) { *f = u; u += n_al; }
        pool.ray_out = pool.ray;
        pool.path_out = pool.path;
        pool.bounce_out = pool.bounce;
        if (kn.ordered) {   // (u is 64-B aligned: n_al is a multiple of 8192)
            m = (char*)u;
            pool.ray_out = (RayRec*)m; m += n_al * sizeof(RayRec);
            pool.path_out = (PathRec*)m; m += n_al * sizeof(PathRec);
            pool.bounce_out = (uint32_t*)m;
            pool.reorder = 1u;
        }
    }
    pool.n_slots = p.n_slots;
    pool.n_alloc = (uint32_t)n_al;
    pool.n_pixels = job.n_pixels;
    pool.k = p.dynamic ? 0u : p.k;
    pool.spp_begin = job.spp_begin;
    pool.spp_end = job.spp_end;
    pool.dynamic = p.dynamic ? 1u : 0u;
    pool.defer_regen = (p.dynamic && !sw.no_defer_regen) ? 1u : 0u;
    pool.compact = (job.dc.motionless && !sw.no_compact_records) ? 1u : 0u;
    pool.total_work = p.total_work;
    pool.width = job.dc.width;
    pool.height = job.dc.height;
    pool.inv_width = 1.0 / (double)job.dc.width;
    pool.tiles_x = p.tiles_x;
    pool.n_tile_pixels = p.n_tile_pixels;
    pool.n_work_pixels = job.sky ? job.n_active_tiles * 64u : 0u;
    pool.list = job.d_list;
    pool.n_list = job.list ? job.n_list : 0u;
    pool.list_store = job.list && job.opts.accum_on_device && job.opts.overwrite ? 1u : 0u;   // (a host accumulator is written by copy_back, pixel by pixel)
    // experiment (PT_INIT_SHUFFLE=1): k_init hands the initial items out permuted inside each 8192-slot granule (an odd multiplier), so
    // that the first K2 launch traces incoherent chunks — the measure of what tile-ordered chunks are worth
    if (p.dynamic && !job.list && sw.init_shuffle) pool.init_perm = 0x9E3779B1u;
    return 0;
}

// The frame accumulator on the device: the caller's, or one of this call's (`own` frees it on every return path), cleared where the
// render is to overwrite. d_accum is null when this fails.
double* device_accum(const Job& job, double* accum, DevMem& own) {
    const size_t bytes = (size_t)job.n_pixels * 3 * sizeof(double);
    double* d_accum = accum;
    if (!job.opts.accum_on_device) {
        if (!own.alloc(bytes, "hipMalloc(accum)")) return nullptr;
        d_accum = own.as<double>();
        if (!hip_ok(hipMemsetAsync(d_accum, 0, bytes, job.st), "hipMemset(accum)")) return nullptr;
    } else if (job.opts.overwrite && !job.list) {   // (a list render stores its pixels instead: the others are not written)
        if (!hip_ok(hipMemsetAsync(d_accum, 0, bytes, job.st), "hipMemset(accum)")) return nullptr;
    }
    return d_accum;
}
// dynamic mode: the kernels add into channel planes in work-item (tile) order (PoolD::accum_tiled); k_detile adds them to d_accum.
// (tiled_accum_bytes, above: the tile map behind the planes is written by classify_sky and never cleared here)
int tiled_accum(pt_scene* s, const Job& job, PoolD& pool) {
    const size_t tb = (size_t)pool.n_tile_pixels * 3 * sizeof(double);
    if (!s->gpu->tile_accum.reserve(tiled_accum_bytes(pool.n_tile_pixels), "hipMalloc(tiled accumulator)")) return -1;
    // (the short-path pass has cleared the planes ahead of its kernel, whose sums they hold by now: run_short)
    if (job.n_short_tiles == 0 && !hip_ok(hipMemsetAsync(s->gpu->tile_accum.as<double>(), 0, tb, job.st), "hipMemset(tiled accumulator)")) return -1;
    pool.accum = s->gpu->tile_accum.as<double>();
    pool.accum_tiled = 1u;
    // the kernels find the map behind THIS accumulator's planes (pool_tile_map): the buffer classify_sky wrote into may not have moved
    if (job.sky && tile_map_behind(pool.accum, pool.n_tile_pixels) != job.tile_map) return set_error("pt_render: the sky pass's tile map is not behind the tiled accumulator (internal error)");
    return 0;
}
// (init_cnt is the caller's: the copy is asynchronous, so it has to live until the render's next synchronise)
int start_counters(pt_scene* s, const Job& job, uint32_t n_slots, CountersD& init_cnt) {
    memset(&init_cnt, 0, sizeof init_cnt);
    init_cnt.alive = job.spp == 0 || (job.sky && job.n_active_tiles == 0) ? 0 : n_slots;   // every slot starts with one sample (k <= spp / n_slots <= total_work)
    for (uint32_t sh = 0; sh < WORK_SHARDS; ++sh) {   // dynamic mode: items 0 .. n_slots-1 were handed out by k_init
        const uint64_t row = (uint64_t)WORK_SHARDS * 64, rows = n_slots / row, rem = n_slots % row;
        const uint64_t part = rem > (uint64_t)sh * 64 ? std::min<uint64_t>(rem - (uint64_t)sh * 64, 64) : 0;
        init_cnt.work[sh].next = rows * 64 + part;
    }
    return hip_ok(hipMemcpyAsync(s->gpu->counters(), &init_cnt, sizeof init_cnt, hipMemcpyHostToDevice, job.st), "hipMemcpy(counters)") ? 0 : -1;
}

// the frame's end: once half of the slots still covered are dead the survivors move to the front and the launches shrink with them
// (k_compact_scan / k_compact_move). The count is the last poll's — stale only towards MORE live slots, which errs on the safe side.
int compact_pool(pt_scene* s, hipStream_t st, uint64_t n_alive, PoolD& pool, EventTimer& timer) {
    const uint32_t new_end = (uint32_t)((n_alive + 8191) & ~(uint64_t)8191);
    const uint32_t cap = new_end;                                  // holes and movers are both at most the live count
    if (!s->gpu->compact_scratch.reserve((2 * (size_t)cap + 2) * sizeof(uint32_t), "hipMalloc(compaction lists)")) return -1;
    uint32_t* scratch = s->gpu->compact_scratch.as<uint32_t>();
    timer.begin(2, st);
    launch_compact(pool, new_end, scratch, scratch + cap, scratch + 2 * (size_t)cap, cap, s->ctx->n_cus * 8, st);
    timer.end(st);
    pool.n_alloc = new_end;
    pool.n_slots = std::min(pool.n_slots, new_end);
    return 0;
}

struct RunResult { uint64_t iterations = 0; uint32_t compactions = 0; double ms_total = 0.0; };
// init -> {extend, shade}* -> detile / resolve on the job's stream, with a poll of the live-slot counter every few iterations
int run_wavefront(pt_scene* s, const Switches& sw, const Job& job, const PoolPlan& p, const Kernels& kn, PoolD& pool, double* d_accum, EventTimer& timer,
                  RunResult& r) {
    hipStream_t st = job.st;
    const CamD& dc = job.dc;
    (void)hipStreamSynchronize(st);
    const auto t0 = std::chrono::steady_clock::now();

    if (job.sky && job.n_sky_tiles != 0 && job.spp != 0) {   // the sure-sky tiles' samples, ahead of the wavefront
        timer.begin(3, st);
        launch_sky(s->gpu->dev.view, dc, pool, s->gpu->counters(), job.seed, job.sky_list, job.n_sky_tiles, job.sky_chunk, st);
        timer.end(st);
    }
    const bool wavefront = !(job.sky && job.n_active_tiles == 0);   // a frame that is all sky has none
    if (wavefront) {
        timer.begin(2, st);
        if (!launch_init(dc, pool, job.seed, kn.grid_shade, st, kn.form)) return set_error("pt_render: no k_init form for this render");
        timer.end(st);
    }
    const uint64_t per_slot = p.dynamic ? (p.total_work + p.n_slots - 1) / std::max<uint64_t>(p.n_slots, 1) + 1 : (job.spp + p.k - 1) / p.k;
    const uint64_t max_iterations = per_slot * ((uint64_t)std::max(1u, dc.max_depth) + 1) + 4;   // + 1: a parked slot idles one iteration
    uint32_t poll_every = 8;
    const bool compact_ok = p.dynamic && !sw.no_compact_pool;
    // max_depth = 0: trace() returns zero radiance for every sample (camera.rs:177); nothing to launch
    bool alive = job.spp != 0 && dc.max_depth != 0 && wavefront;
    while (alive) {
        for (uint32_t i = 0; i < poll_every; ++i) {
            timer.begin(0, st);
            launch_extend(s->gpu->dev.view, pool, s->gpu->counters(), kn.grid_extend, kn.extend_code, st, kn.form.motion, sw.k2_split);
            timer.end(st);
            timer.begin(1, st);
            if (!launch_shade(s->gpu->dev.view, dc, pool, s->gpu->counters(), job.seed, kn.grid_shade, kn.form, st, sw.wide_window_min, mode_has_table(job.mode) ? &job.env : nullptr))
                return set_error("pt_render: no k_shade form for this render");
            timer.end(st);
            if (kn.ordered) {   // what K3 wrote is the pool K2, the compaction and the next K3 read
                std::swap(pool.ray, pool.ray_out);
                std::swap(pool.path, pool.path_out);
                std::swap(pool.bounce, pool.bounce_out);
            }
            ++r.iterations;
        }
        if (!hip_ok(hipMemcpyAsync(s->gpu->host_counters(), s->gpu->counters(), sizeof(CountersD), hipMemcpyDeviceToHost, st), "hipMemcpy(counters)")) return -1;
        if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(render)")) return -1;
        timer.drain();
        const uint64_t n_alive = s->gpu->host_counters()->alive;
        alive = n_alive != 0;
        if (alive && r.iterations > max_iterations + 128) return set_error("pt_render: iteration bound exceeded (internal error)");
        if (poll_every < sw.poll_cap) poll_every *= 2;     // (a poll is a pipeline drain of some tens of microseconds: every 8 iterations costs <= 0.5 %)
        if (compact_ok && alive && n_alive * sw.compact_den <= (uint64_t)pool.n_alloc * sw.compact_num && pool.n_alloc > 4 * 8192u) {
            if (compact_pool(s, st, n_alive, pool, timer) != 0) return -1;
            ++r.compactions;
        }
    }
    if (!p.dynamic || pool.accum_tiled) {
        timer.begin(2, st);
        if (pool.accum_tiled) launch_detile(pool, d_accum, s->ctx->n_cus * 8, st);
        else launch_resolve(pool, d_accum, s->ctx->n_cus * 8, st);
        timer.end(st);
    }
    if (!hip_ok(hipMemcpyAsync(s->gpu->host_counters(), s->gpu->counters(), sizeof(CountersD), hipMemcpyDeviceToHost, st), "hipMemcpy(counters)")) return -1;
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(resolve)")) return -1;
    timer.drain();
    r.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return hip_ok(hipGetLastError(), "kernel launch") ? 0 : -1;
}

// a host accumulator gets the frame back: the whole of it, or only the listed pixels of the caller's frame
int copy_back(const Job& job, const double* d_accum, double* accum) {
    if (job.opts.accum_on_device) return 0;
    const size_t n = (size_t)job.n_pixels * 3, bytes = n * sizeof(double);
    if (job.opts.overwrite && !job.list) return hip_ok(hipMemcpy(accum, d_accum, bytes, hipMemcpyDeviceToHost), "hipMemcpy(accum)") ? 0 : -1;
    std::vector<double> tmp(n);
    if (!hip_ok(hipMemcpy(tmp.data(), d_accum, bytes, hipMemcpyDeviceToHost), "hipMemcpy(accum)")) return -1;
    if (job.list) {
        for (uint32_t i = 0; i < job.n_list; ++i)
            for (uint32_t c = 0; c < 3; ++c) {
                const size_t j = 3 * (size_t)job.h_list[i] + c;
                accum[j] = job.opts.overwrite ? tmp[j] : accum[j] + tmp[j];
            }
    } else {
        for (size_t i = 0; i < n; ++i) accum[i] += tmp[i];
    }
    return 0;
}

// PT_PROF, diagnostic builds (-DPT_STAMPS): wave-cycle sums per k_shade class
void print_prof(const CountersD* cnt) {
    static const char* names[N_CLASSES + 1] = {"miss", "diffuse", "metal", "glass", "principled", "light", "sheen", "clearcoat", "mix", "idle", "dead", "WINDOW"};
    for (uint32_t c = 0; c <= N_CLASSES; ++c) {
        const unsigned long long* p = cnt->prof[c];
        if (p[0] && c == CLASS_DEAD)
            fprintf(stderr, "[pt prof] K2 window  n %10llu  phase A %8.0f  barrier %8.0f  phase B %8.0f  barrier %8.0f  candidates %6.1f (cycles per window and wave)\n", p[0],
                    (double)p[1] / p[0], (double)p[2] / p[0], (double)p[3] / p[0], (double)p[4] / p[0], (double)p[5] / p[0])
#ifdef PT_STAMPS
            // the list's overflow (pt_k2_extend.h "rounds of a window"): sums over the frame, and the full windows by eighths of candidates
            , fprintf(stderr, "[pt prof] K2 overflow  wave cycles: phase A %llu (of it chunk ends with a walk %llu)  barriers %llu  phase B %llu  barriers %llu; rays: phase B %llu (per wave-window sums: x waves per block)  walked in phase A %llu\n",
                      p[1], p[7], p[2], p[3], p[4], p[5], p[6]),
              fprintf(stderr, "[pt prof] K2 full windows by candidates in eighths of the window, 0 .. 8: %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", p[8] & 0xFFFFFFFFull,
                      p[8] >> 32, p[9] & 0xFFFFFFFFull, p[9] >> 32, p[10] & 0xFFFFFFFFull, p[10] >> 32, p[11] & 0xFFFFFFFFull, p[11] >> 32, p[12] & 0xFFFFFFFFull)
#endif
            ;
        else if (p[0] && c < N_CLASSES)
            fprintf(stderr, "[pt prof] %-10s n %10llu  body %8.0f = hit %7.0f + env/tex %7.0f + direction %7.0f + pdf/eval/ray %7.0f  dequeue %8.0f  regen+store %8.0f  whole %8.0f (cycles per wave-group)\n",
                    names[c], p[0], (double)p[2] / p[0], (double)p[1] / p[0], (double)p[6] / p[0], (double)p[7] / p[0], (double)(p[2] - p[1] - p[6] - p[7]) / p[0],
                    (double)p[3] / p[0], (double)p[4] / p[0], (double)p[5] / p[0]),
            fprintf(stderr, "[pt prof] %-10s   lanes per group: live %5.1f  on a surface %5.1f  with a next direction %5.1f  regenerated %5.1f\n", names[c], (double)p[8] / p[0],
                    (double)p[9] / p[0], (double)p[10] / p[0], (double)p[11] / p[0])
#ifdef PT_STAMPS
            , fprintf(stderr, "[pt prof] %-10s   groups of one primitive %10llu (%5.1f %%), of one sphere / quad %10llu (%5.1f %%)\n", names[c], p[12], 100.0 * (double)p[12] / p[0],
                      p[13], 100.0 * (double)p[13] / p[0])
#endif
            ;
        else if (p[0])
            fprintf(stderr, "[pt prof] WINDOW     n %10llu  sort %8.0f  shade %8.0f  barrier wait %8.0f  groups %8.0f  record wait %8.0f (cycles per window and wave)\n", p[0],
                    (double)p[1] / p[0], (double)p[2] / p[0], (double)p[3] / p[0], (double)p[4] / p[0], (double)p[5] / p[0]);
    }
}

void fill_stats(const pt_scene* s, const Job& job, const PoolPlan& p, const Kernels& kn, const PoolD& pool, const EventTimer& timer, const RunResult& r, pt_render_stats* stats) {
    memset(stats, 0, sizeof *stats);
    stats->samples = s->gpu->host_counters()->samples + job.short_samples;   // (k_short counts into words of its own: the counters start after it)
    stats->segments = s->gpu->host_counters()->segments + job.short_segments;
    stats->iterations = r.iterations;
    stats->n_slots = p.n_slots;
    stats->slots_per_pixel = p.dynamic ? 0u : p.k;
    stats->ms_total = r.ms_total;
    stats->ms_extend = timer.ms[0];
    stats->ms_shade = timer.ms[1];
    stats->ms_other = timer.ms[2];
    stats->launches_extend = timer.launches[0];
    stats->launches_shade = timer.launches[1];
    stats->extend_variant = kn.extend_code <= -100 ? 0u : 1u;
    stats->shade_variant = (uint32_t)kn.form.variant;
    stats->blocks_extend = (uint32_t)kn.grid_extend;
    stats->blocks_shade = (uint32_t)kn.grid_shade;
    stats->compactions = r.compactions;
    stats->n_alloc_end = pool.n_alloc;
    stats->k2_split_windows = s->gpu->host_counters()->k2_split_windows;
    stats->k2_overflow_rays = s->gpu->host_counters()->k2_overflow_rays;
    stats->pilot_tiles = job.n_pilot_tiles;
    stats->short_fallback = job.short_fallback ? 1u : 0u;
    stats->short_list_bytes = job.n_short_tiles ? job.short_cap_entries * (job.short_wide ? 8 : 4) : 0u;
    stats->short_pixels = job.n_short_pixels;
    stats->short_direct_tiles = job.short_direct_tiles;
    stats->short_self_prims = job.n_short_tiles ? job.short_self_prims : 0u;
    stats->short_walks = job.short_walks;
    stats->short_walk_passes = job.short_walk_passes;
    stats->ms_pilot = timer.ms[5];
    stats->short_tiles = job.n_short_tiles;
    stats->short_samples = job.short_samples;
    stats->hard_samples = job.n_hard;
    stats->ms_short = timer.ms[4];
    stats->sky_tiles = job.sky ? job.n_sky_tiles : 0u;
    stats->sky_samples = job.sky ? (uint64_t)job.n_sky_pixels * job.spp : 0u;
    stats->ms_sky = timer.ms[3];
}
// the statistics of an adaptive render: its passes' counts and times added up, the pool and the kernels of the last pass
void add_stats(pt_render_stats& sum, const pt_render_stats& ps) {
    sum.samples += ps.samples;
    sum.segments += ps.segments;
    sum.iterations += ps.iterations;
    sum.n_slots = std::max(sum.n_slots, ps.n_slots);
    sum.slots_per_pixel = ps.slots_per_pixel;
    sum.ms_extend += ps.ms_extend;
    sum.ms_shade += ps.ms_shade;
    sum.ms_other += ps.ms_other;
    sum.launches_extend += ps.launches_extend;
    sum.launches_shade += ps.launches_shade;
    sum.extend_variant = ps.extend_variant;
    sum.shade_variant = ps.shade_variant;
    sum.blocks_extend = ps.blocks_extend;
    sum.blocks_shade = ps.blocks_shade;
    sum.compactions += ps.compactions;
    sum.n_alloc_end = ps.n_alloc_end;
    sum.k2_split_windows += ps.k2_split_windows;
    sum.k2_overflow_rays += ps.k2_overflow_rays;
    sum.pilot_tiles = std::max(sum.pilot_tiles, ps.pilot_tiles);
    sum.short_fallback += ps.short_fallback;
    sum.short_list_bytes = std::max(sum.short_list_bytes, ps.short_list_bytes);
    sum.short_pixels = std::max(sum.short_pixels, ps.short_pixels);
    sum.short_direct_tiles = std::max(sum.short_direct_tiles, ps.short_direct_tiles);
    sum.short_self_prims = std::max(sum.short_self_prims, ps.short_self_prims);
    sum.short_walks += ps.short_walks;
    sum.short_walk_passes += ps.short_walk_passes;
    sum.ms_pilot += ps.ms_pilot;
    sum.short_tiles = std::max(sum.short_tiles, ps.short_tiles);
    sum.short_samples += ps.short_samples;
    sum.hard_samples += ps.hard_samples;
    sum.ms_short += ps.ms_short;
    sum.sky_tiles = std::max(sum.sky_tiles, ps.sky_tiles);
    sum.sky_samples += ps.sky_samples;
    sum.ms_sky += ps.ms_sky;
}

// The render core behind pt_render, pt_render_pixels and the passes of pt_render_adaptive. d_list (device) / h_list (host, the same
// pixels) / n_list: a pixel-list render (PoolD::list; d_list sorted by tiled index, n_list > 0), or null: the whole frame — then the
// path below is exactly pt_render's. When several things are wrong at once the first refusal in this order is the one returned:
// arguments, camera, size, mode, pool, then form.
int render_core(pt_scene* s, const pt_camera* cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* accum, const pt_render_opts* opts_in,
                pt_render_stats* stats, const uint32_t* d_list, const uint32_t* h_list, uint32_t n_list) {
    if (!s || !s->built) return set_error("pt_render: world not built (call pt_world_build)");
    if (!accum) return set_error("pt_render: null accumulator");
    if (spp_end < spp_begin) return set_error("pt_render: spp_end < spp_begin");
    Job job;
    memset(&job.opts, 0, sizeof job.opts);
    if (opts_in) job.opts = *opts_in;
    if (!hip_ok(hipSetDevice(s->ctx->device), "hipSetDevice")) return -1;
    job.st = job.opts.stream ? (hipStream_t)job.opts.stream : s->ctx->stream;
    job.seed = seed;
    job.spp_begin = spp_begin; job.spp_end = spp_end; job.spp = spp_end - spp_begin;
    job.d_list = d_list; job.h_list = h_list; job.n_list = n_list; job.list = d_list != nullptr;
    if (make_camd(s, cam, job.dc) != 0) return -1;
    const uint64_t n_pixels64 = (uint64_t)job.dc.width * job.dc.height;
    if (n_pixels64 == 0 || n_pixels64 > 0x7FFFFFFFull) return set_error("pt_render: bad image size");
    job.n_pixels = (uint32_t)n_pixels64;
    job.n_items = job.list ? n_list : job.n_pixels;
    memset(&job.env, 0, sizeof job.env);
    if (render_mode(s, job.dc, job.st, job.mode, job.env) != 0) return -1;

    const Switches sw = read_switches(job.opts);
    job.form = shade_form(ShadeForm{sw.shade_variant, s->gpu->dev.view.n_lights != 0u, job.list, s->sampler == 1 /* the Sobol sampler: DESIGN.md §11 */, job.mode, s->motion_on(), s->punctual_on()});
    EventTimer timer;
    timer.enabled = job.opts.profile != 0;
    if (classify_sky(s, sw, job, timer) != 0) return -1;
    if (run_short(s, job, timer) != 0) return -1;
    PoolPlan plan;
    if (plan_pool(sw, job, s->ctx->n_cus, plan) != 0) return -1;
    const Kernels kn = choose_kernels(sw, s, job, plan);
    PoolD pool;
    if (bind_pool(s, sw, job, plan, kn, pool) != 0) return -1;
    DevMem own_accum;
    double* d_accum = device_accum(job, accum, own_accum);
    if (!d_accum) return -1;
    // (refused here and no earlier: a failed allocation above has always been reported first)
    if (kn.blocks_shade < 1) return set_error("pt_render: no k_shade form for this combination of pixel list, environment sampling, sampler and media");
    pool.accum = d_accum;
    if (plan.dynamic && !sw.accum_linear && tiled_accum(s, job, pool) != 0) return -1;
    CountersD init_cnt;
    if (start_counters(s, job, plan.n_slots, init_cnt) != 0) return -1;

    RunResult run;
    if (run_wavefront(s, sw, job, plan, kn, pool, d_accum, timer, run) != 0) return -1;
    if (copy_back(job, d_accum, accum) != 0) return -1;
    if (sw.prof) print_prof(s->gpu->host_counters());
    if (stats) fill_stats(s, job, plan, kn, pool, timer, run, stats);
    return 0;
}
}  // namespace

extern "C" int pt_render(pt_scene* s, const pt_camera* cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* accum,
                         const pt_render_opts* opts, pt_render_stats* stats) {
    return render_core(s, cam, seed, spp_begin, spp_end, accum, opts, stats, nullptr, nullptr, 0);
}

namespace {
uint32_t tiled_key(uint32_t p, uint32_t width, uint32_t tiles_x) {   // row-major pixel -> its tiled index (k_detile's tiled_index)
    const uint32_t y = p / width, x = p % width;
    return ((y >> 3) * tiles_x + (x >> 3)) * 64u + ((y & 7u) << 3) + (x & 7u);
}
}  // namespace

extern "C" int pt_render_pixels(pt_scene* s, const pt_camera* cam, uint64_t seed, const uint32_t* pixels, uint32_t n, uint32_t spp_begin,
                                uint32_t spp_end, double* accum, const pt_render_opts* opts, pt_render_stats* stats) {
    if (!s || !s->built) return set_error("pt_render_pixels: world not built (call pt_world_build)");
    if (!accum) return set_error("pt_render_pixels: null accumulator");
    if (spp_end < spp_begin) return set_error("pt_render_pixels: spp_end < spp_begin");
    CamDerived cd;
    if (derive_camera(cam, cd) != 0) return -1;
    const uint64_t n_pixels = (uint64_t)cam->image_width * cd.height;
    if (n_pixels > 0x7FFFFFFFull) return set_error("pt_render_pixels: bad image size");
    if (n == 0) {
        if (stats) memset(stats, 0, sizeof *stats);
        return 0;
    }
    if (!pixels) return set_error("pt_render_pixels: null pixel list");
    for (uint32_t i = 0; i < n; ++i) {
        if (pixels[i] >= n_pixels) return set_error("pt_render_pixels: pixel index out of range (must be < width * height)");
        if (i > 0 && pixels[i] <= pixels[i - 1]) return set_error("pt_render_pixels: the pixel list must be strictly ascending (sorted, no duplicates)");
    }
    // the device list in tiled order: a run of 64 work items then covers an 8x8 tile, as in a whole-frame render
    const uint32_t width = cam->image_width, tiles_x = (width + 7) / 8;
    std::vector<uint32_t> sorted(pixels, pixels + n);
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return tiled_key(a, width, tiles_x) < tiled_key(b, width, tiles_x); });
    if (!hip_ok(hipSetDevice(s->ctx->device), "hipSetDevice")) return -1;
    if (!s->gpu->pixel_list.reserve((size_t)n * sizeof(uint32_t), "hipMalloc(pixel list)")) return -1;   // (re-used like the pool)
    if (!hip_ok(hipMemcpy(s->gpu->pixel_list.as<uint32_t>(), sorted.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(pixel list)")) return -1;
    return render_core(s, cam, seed, spp_begin, spp_end, accum, opts, stats, s->gpu->pixel_list.as<uint32_t>(), sorted.data(), n);
}

extern "C" int pt_adaptive_schedule(uint32_t min_spp, uint32_t max_spp, uint32_t* bounds, uint32_t cap) {
    if (min_spp < 2) return set_error("pt_adaptive_schedule: min_spp must be at least 2");
    if (max_spp < min_spp) return set_error("pt_adaptive_schedule: max_spp must be at least min_spp");
    if (cap && !bounds) return set_error("pt_adaptive_schedule: null bounds");
    uint32_t count = 0;
    auto put = [&](uint32_t b) {
        if (count < cap) bounds[count] = b;
        ++count;
    };
    const uint32_t half = min_spp / 2;
    put(0);
    put(half);
    uint32_t b = min_spp;
    put(b);
    while (b < max_spp) {
        b = (uint32_t)std::min<uint64_t>(max_spp, (uint64_t)b + std::max(half, b / 2));
        put(b);
    }
    return (int)count;
}

extern "C" int pt_render_adaptive(pt_scene* s, const pt_camera* cam, uint64_t seed, const pt_adaptive_opts* ao, double* accum,
                                  uint32_t* spp_per_pixel, pt_render_stats* stats) {
    if (!s || !s->built) return set_error("pt_render_adaptive: world not built (call pt_world_build)");
    if (!ao) return set_error("pt_render_adaptive: null options");
    if (!accum || !spp_per_pixel) return set_error("pt_render_adaptive: null output buffer");
    const int n_bounds = pt_adaptive_schedule(ao->min_spp, ao->max_spp, nullptr, 0);
    if (n_bounds < 0) return set_error((std::string("pt_render_adaptive: ") + pt_last_error()).c_str());
    std::vector<uint32_t> b((size_t)n_bounds);
    (void)pt_adaptive_schedule(ao->min_spp, ao->max_spp, b.data(), (uint32_t)n_bounds);
    CamDerived cd;
    if (derive_camera(cam, cd) != 0) return -1;
    const uint32_t width = cam->image_width, height = cd.height;
    const uint64_t n64 = (uint64_t)width * height;
    if (n64 > 0x7FFFFFFFull) return set_error("pt_render_adaptive: bad image size");
    const uint32_t n_pixels = (uint32_t)n64;
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = ao->stream ? (hipStream_t)ao->stream : ctx->stream;
    auto t0 = std::chrono::steady_clock::now();

    // device state: E, O (3 f64 per pixel each), the error map, two pixel lists, the stop counts, the select kernels' block counts
    const uint32_t n_blocks = adapt_select_blocks(width, height);
    const size_t f64s = (size_t)n_pixels * 7, u32s = (size_t)n_pixels * 3 + n_blocks + 1;
    DevMem mem;
    if (!mem.alloc(f64s * sizeof(double) + u32s * sizeof(uint32_t), "hipMalloc(adaptive state)")) return -1;
    double* E = mem.as<double>();
    double* O = E + 3 * (size_t)n_pixels;
    double* err = O + 3 * (size_t)n_pixels;
    uint32_t* list_a = (uint32_t*)(err + n_pixels);
    uint32_t* list_b = list_a + n_pixels;
    uint32_t* stop = list_b + n_pixels;
    uint32_t* block_counts = stop + n_pixels;
    uint32_t* d_active = block_counts + n_blocks;
    if (!hip_ok(hipMemsetAsync(E, 0, 6 * (size_t)n_pixels * sizeof(double), st), "hipMemset(adaptive sums)") ||
        !hip_ok(hipMemsetAsync(stop, 0, (size_t)n_pixels * sizeof(uint32_t), st), "hipMemset(adaptive counts)"))
        return -1;
    std::vector<uint32_t> all;   // every pixel, in tiled order
    all.reserve(n_pixels);
    const uint32_t tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx)
            for (uint32_t i = 0; i < 64; ++i) {
                const uint32_t x = tx * 8 + (i & 7), y = ty * 8 + (i >> 3);
                if (x < width && y < height) all.push_back(y * width + x);
            }
    if (!hip_ok(hipMemcpyAsync(list_a, all.data(), (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, st), "hipMemcpy(pixel list)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(adaptive)"))
        return -1;

    pt_render_opts po;
    memset(&po, 0, sizeof po);
    po.slots_per_pixel = ao->slots_per_pixel;
    po.accum_on_device = 1;
    po.profile = ao->profile;
    po.stream = (void*)st;
    pt_render_stats sum;
    memset(&sum, 0, sizeof sum);
    uint32_t n_active = n_pixels;
    double n_e = 0.0, n_o = 0.0;
    const uint32_t max_spp = ao->max_spp;
    for (int i = 0; i + 1 < n_bounds && n_active != 0; ++i) {
        const uint32_t lo = b[(size_t)i], hi = b[(size_t)i + 1];
        pt_render_stats ps;
        if (render_core(s, cam, seed, lo, hi, (i & 1) ? O : E, &po, &ps, list_a, nullptr, n_active) != 0) return -1;
        add_stats(sum, ps);
        ((i & 1) ? n_o : n_e) += (double)(hi - lo);
        if (i >= 1 && hi < max_spp) {   // the test: who goes on into round i + 1
            launch_adapt_error(E, O, stop, n_pixels, n_e, n_o, err, st);
            launch_adapt_select(err, stop, width, height, ao->threshold, hi, block_counts, list_b, d_active, st);
            if (!hip_ok(hipMemcpyAsync(&n_active, d_active, sizeof n_active, hipMemcpyDeviceToHost, st), "hipMemcpy(active count)") ||
                !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(adaptive select)"))
                return -1;
            std::swap(list_a, list_b);
        }
    }
    launch_adapt_final(E, O, stop, n_pixels, max_spp, list_b, st);
    if (!hip_ok(hipMemcpyAsync(accum, E, (size_t)n_pixels * 3 * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(accum)") ||
        !hip_ok(hipMemcpyAsync(spp_per_pixel, list_b, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "hipMemcpy(spp per pixel)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(adaptive)") || !hip_ok(hipGetLastError(), "kernel launch"))
        return -1;
    sum.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = sum;
    return 0;
}

extern "C" int pt_render_aovs(pt_scene* s, const pt_camera* cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov,
                              const pt_render_opts* opts_in) {
    if (!s || !s->built) return set_error("pt_render_aovs: world not built (call pt_world_build)");
    if (!aov) return set_error("pt_render_aovs: null aov buffer");
    if (!cam) return set_error("pt_render_aovs: null camera");
    if (spp_end < spp_begin) return set_error("pt_render_aovs: spp_end < spp_begin");
    pt_render_opts opts;
    memset(&opts, 0, sizeof opts);
    if (opts_in) opts = *opts_in;
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = opts.stream ? (hipStream_t)opts.stream : ctx->stream;
    CamD dc;
    if (make_camd(s, cam, dc) != 0) return -1;
    const uint64_t n_pixels = (uint64_t)dc.width * dc.height;
    if (n_pixels == 0 || n_pixels > 0x7FFFFFFFull) return set_error("pt_render_aovs: bad image size");
    const size_t bytes = (size_t)n_pixels * 8 * sizeof(double);
    DevMem own;
    double* d_aov = aov;
    if (!opts.accum_on_device) {   // a host buffer: its sums travel to the device and back, the kernel adds to them there
        if (!own.alloc(bytes, "hipMalloc(aov)")) return -1;
        d_aov = own.as<double>();
        if (!opts.overwrite && !hip_ok(hipMemcpyAsync(d_aov, aov, bytes, hipMemcpyHostToDevice, st), "hipMemcpy(aov)")) return -1;
    }
    ShadeForm aov_form;   // of a form, the AOV walk looks at the sampler only
    aov_form.qmc = s->sampler == 1;
    aov_form.motion = s->motion_on();   // moving instances are posed at each sample's time, taken through the shutter
    if (!launch_aov(s->gpu->dev.view, dc, seed, spp_begin, spp_end, d_aov, opts.overwrite != 0, ctx->n_cus * 8, st, aov_form))
        return set_error("pt_render_aovs: no k_aov form for this sampler");
    if (!hip_ok(hipGetLastError(), "kernel launch")) return -1;
    if (!opts.accum_on_device && !hip_ok(hipMemcpyAsync(aov, d_aov, bytes, hipMemcpyDeviceToHost, st), "hipMemcpy(aov)")) return -1;
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(aov)") ? 0 : -1;
}
