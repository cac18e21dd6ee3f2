// Context management and the wavefront render loop (host side of Camera::render,
// camera.rs:79-126): size the path pool, launch init -> {extend, shade}* -> resolve on one HIP
// stream, poll the live-slot counter every few iterations, report per-kernel HIP-event times.
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
#include "pt_scene.h"

using namespace pt;
using namespace pt::host;

extern "C" const char* pt_last_error(void) { return pt::last_error(); }
extern "C" int pt_set_error_message(const char* msg) { return set_error(msg); }

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
    return s;
}
extern "C" void pt_scene_destroy(pt_scene* s) { delete s; }
extern "C" pt_ctx* pt_scene_ctx(pt_scene* s) { return s ? s->ctx : nullptr; }
extern "C" int pt_find_registered_image(pt_scene* s, const char* name) {
    auto it = s->images.find(name);
    return it == s->images.end() ? -1 : it->second;
}

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

namespace {
struct EventTimer {   // per-launch HIP-event timing, drained at the polling syncs
    struct Pending {
        hipEvent_t a, b;
        int kind;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_list;
    double ms[3] = {0, 0, 0};
    uint64_t launches[3] = {0, 0, 0};
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
static int make_camd(pt_scene* s, const pt_camera* cam, CamD& dc) {
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
    dc.n_lights = s->dev.view.n_lights;
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
static int env_tables(pt_scene* s, const CamD& dc, hipStream_t st, EnvTabD& e) {
    memset(&e, 0, sizeof e);
    if (s->env_tab_tex != dc.env_tex) {
        TexD T;
        if (!hip_ok(hipMemcpyAsync(&T, s->dev.view.tex + dc.env_tex, sizeof T, hipMemcpyDeviceToHost, st), "hipMemcpy(env texture)") ||
            !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(env texture)"))
            return -1;
        if (s->env_tab) (void)hipFree(s->env_tab);
        s->env_tab = nullptr;
        s->env_tab_bytes = 0;
        s->env_tab_tex = -1;
        s->env_tab_w = T.w;
        s->env_tab_h = T.h;
        s->env_tab_z = 0.0;
        if (T.w != 0 && T.h != 0) {
            const size_t n_col = (size_t)T.h * (T.w + 1), bytes = (n_col + T.h + 1) * sizeof(double);
            if (!hip_ok(hipMalloc((void**)&s->env_tab, bytes), "hipMalloc(env tables)")) return -1;
            s->env_tab_bytes = bytes;
            launch_env_tables(s->dev.view, T, s->env_tab, s->env_tab + n_col, st);
            if (!hip_ok(hipGetLastError(), "env tables") ||
                !hip_ok(hipMemcpyAsync(&s->env_tab_z, s->env_tab + n_col + T.h, sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(env Z)") ||
                !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(env tables)"))
                return -1;
        }
        s->env_tab_tex = dc.env_tex;
    }
    e.w = s->env_tab_w;
    e.h = s->env_tab_h;
    e.f = s->env_f;
    if (s->env_tab && std::isfinite(s->env_tab_z) && s->env_tab_z > 0.0) {
        e.col = s->env_tab;
        e.row = s->env_tab + (size_t)e.h * (e.w + 1);
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
    mode = dsp ? MODE_DSP : lse ? MODE_LSE : !med ? (env_on ? MODE_ENV : MODE_PLAIN) : s->interior_on() ? MODE_INT : s->grid_media_on() ? MODE_HET : MODE_MED;
    return 0;
}

// The render core behind pt_render, pt_render_pixels and the passes of pt_render_adaptive. d_list (device) / h_list (host, the same
// pixels) / n_list: a pixel-list render (PoolD::list; d_list sorted by tiled index, n_list > 0), or null: the whole frame — then the
// path below is exactly pt_render's.
static int render_core(pt_scene* s, const pt_camera* cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* accum,
                       const pt_render_opts* opts_in, pt_render_stats* stats, const uint32_t* d_list, const uint32_t* h_list, uint32_t n_list) {
    if (!s || !s->built) return set_error("pt_render: world not built (call pt_world_build)");
    if (!accum) return set_error("pt_render: null accumulator");
    if (spp_end < spp_begin) return set_error("pt_render: spp_end < spp_begin");
    pt_render_opts opts;
    memset(&opts, 0, sizeof opts);
    if (opts_in) opts = *opts_in;
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    hipStream_t st = opts.stream ? (hipStream_t)opts.stream : ctx->stream;

    CamD dc;
    if (make_camd(s, cam, dc) != 0) return -1;
    const uint64_t n_pixels64 = (uint64_t)dc.width * dc.height;
    if (n_pixels64 == 0 || n_pixels64 > 0x7FFFFFFFull) return set_error("pt_render: bad image size");
    const uint32_t n_pixels = (uint32_t)n_pixels64;
    const uint32_t spp = spp_end - spp_begin;
    const bool list = d_list != nullptr;
    const uint32_t n_items = list ? n_list : n_pixels;   // pixels rendered
    ShadeMode mode;
    EnvTabD env{};   // the table argument of a mode that has one
    if (render_mode(s, dc, st, mode, env) != 0) return -1;

    // pool sizing. slots_per_pixel = 0 (default): DYNAMIC work assignment — a fixed pool that fills
    // the machine several times over; finished paths pull the next (pixel, sample) from a global
    // counter. slots_per_pixel = k >= 1: STATIC ownership (deterministic; k = 1 is the reference's
    // exact per-pixel sample order).
    uint32_t k = opts.slots_per_pixel;
    if (k == 0)   // an explicit option wins over the experiment switch
        if (const char* e = exp_env("PT_SLOTS_PER_PIXEL")) k = (uint32_t)atoi(e);
    const bool dynamic = k == 0;
    const uint32_t tiles_x = (dc.width + 7) / 8, tiles_y = (dc.height + 7) / 8;
    const uint64_t n_tile_pixels64 = (uint64_t)tiles_x * tiles_y * 64;
    if (n_tile_pixels64 > 0x7FFFFFFFull) return set_error("pt_render: image too large");
    const uint64_t total_work = dynamic ? (list ? (uint64_t)n_list : n_tile_pixels64) * spp : (uint64_t)n_items * spp;
    uint64_t n_slots64;
    if (dynamic) {
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
        uint64_t per_cu = 16384;   // a power of two (the tile-ordered work items and the 64 counter shards divide it evenly)
        while (per_cu < 524288 && per_cu * 2 * (uint64_t)std::max(1, ctx->n_cus) * 30 <= total_work) per_cu *= 2;
        // one more doubling (268 M slots, 28 GB) only from 48 samples per slot: scene 3 1920x1920 @ 4000 spp (55 per slot) 1335 -> 1362,
        // while at 31 per slot scene 6 FHD @ 4000 loses 0.7 % and scene 5 4K @ 1000 0.5 % (initialising and compacting the pool costs 58 ms there)
        if (per_cu == 524288 && per_cu * 2 * (uint64_t)std::max(1, ctx->n_cus) * 48 <= total_work) per_cu *= 2;
        uint64_t target = (uint64_t)ctx->n_cus * per_cu;
        if (const char* e = exp_env("PT_POOL_SLOTS")) {
            target = strtoull(e, nullptr, 10);
            if (target == 0) return set_error("pt_render: PT_POOL_SLOTS must be positive");
        }
        n_slots64 = std::min<uint64_t>(target, std::max<uint64_t>(total_work, 1));
    } else {
        if (k > spp) k = spp;
        if (k == 0) k = 1;
        while ((uint64_t)k * n_items > 0x40000000ull && k > 1) --k;
        n_slots64 = (uint64_t)k * n_items;
    }
    if (n_slots64 > 0x7FFFFFC0ull) return set_error("pt_render: image too large for the path pool");
    const uint32_t n_slots = (uint32_t)n_slots64;
    int shade_variant = 42;   // k_shade<sort, min waves/SIMD>: sort*10 + waves (12 = windowed material sort with 256 threads / 2048-slot windows, 2 = plain;
                              // [r3] 22 = the same with 512 threads / 4096-slot windows: K3 -2 % on scenes 6, 3 and 5; 32 = 8192-slot windows: another
                              // -1.6 % on scene 6's 33.6 M-slot pool, +2.5 % on scene 5's 16.8 M; 42 = per launch, 32 while the pool holds >= 16 such
                              // windows per block launched, else 22)
    if (const char* e = exp_env("PT_SHADE_VARIANT")) shade_variant = atoi(e);
    const ShadeForm form = shade_form(ShadeForm{shade_variant, s->dev.view.n_lights != 0u, list, s->sampler == 1 /* the Sobol sampler: DESIGN.md §11 */, mode});   // the form of k_init / k_shade that exists for it
    shade_variant = form.variant;
    // Shading-order output (PoolD::reorder): the dynamic mode's sorted whole-frame k_shade writes every path to its position in the
    // window's sorted order in a second record area, and the two areas swap after each launch — K2's chunks are then K3's groups: a tile's
    // camera rays in pixel order, or 64 paths of one material class. Static mode, pixel lists and PT_POOL_IN_PLACE write in place.
    const bool ordered = dynamic && !list && shade_form_sorts(form) && !exp_env("PT_POOL_IN_PLACE");
    // one allocation: the two record arrays (RayRec, PathRec), the static mode's f64 arrays, the two u32 state arrays (+ the output area)
    const size_t n_al = ((size_t)n_slots + 8191) & ~(size_t)8191;   // whole windows: 2048 slots (k_extend2, k_shade) / 4096 (k_shade with 512 threads)
    const size_t n_f64 = dynamic ? 0 : 6;   // the per-slot sample sums and radiances exist in the static mode only (the dynamic mode adds into the frame)
    const size_t bytes = n_al * (sizeof(RayRec) + sizeof(PathRec) + n_f64 * sizeof(double) + 2 * sizeof(uint32_t)) +
                         (ordered ? n_al * (sizeof(RayRec) + sizeof(PathRec) + sizeof(uint32_t)) : 0);
    if (bytes > s->pool_bytes) {
        if (s->pool_mem) (void)hipFree(s->pool_mem);
        s->pool_mem = nullptr;
        s->pool_bytes = 0;
        if (!hip_ok(hipMalloc(&s->pool_mem, bytes), "hipMalloc(path pool)")) return -1;
        s->pool_bytes = bytes;
    }
    if (!s->d_counters) {
        if (!hip_ok(hipMalloc((void**)&s->d_counters, sizeof(CountersD)), "hipMalloc(counters)")) return -1;
        if (!hip_ok(hipHostMalloc((void**)&s->h_counters, sizeof(CountersD), hipHostMallocDefault), "hipHostMalloc(counters)")) return -1;
    }
    PoolD pool;
    memset(&pool, 0, sizeof pool);
    {
        char* m = (char*)s->pool_mem;   // hipMalloc memory is 256-B aligned; records first (64-B aligned)
        pool.ray = (RayRec*)m; m += n_al * sizeof(RayRec);
        pool.path = (PathRec*)m; m += n_al * sizeof(PathRec);
        double* d = (double*)m;
        double** f64s[6] = {&pool.ax, &pool.ay, &pool.az, &pool.rx, &pool.ry, &pool.rz};
        for (auto p : f64s) { *p = n_f64 ? d : nullptr; d += n_f64 ? n_al : 0; }
        uint32_t* u = (uint32_t*)d;
        uint32_t** u32s[2] = {&pool.hit_prim, &pool.bounce};
        for (auto p : u32s) { *p = u; u += n_al; }
        pool.ray_out = pool.ray;
        pool.path_out = pool.path;
        pool.bounce_out = pool.bounce;
        if (ordered) {   // (u is 64-B aligned: n_al is a multiple of 8192)
            m = (char*)u;
            pool.ray_out = (RayRec*)m; m += n_al * sizeof(RayRec);
            pool.path_out = (PathRec*)m; m += n_al * sizeof(PathRec);
            pool.bounce_out = (uint32_t*)m;
            pool.reorder = 1u;
        }
    }
    pool.n_slots = n_slots;
    pool.n_alloc = (uint32_t)n_al;
    pool.n_pixels = n_pixels;
    pool.k = dynamic ? 0u : k;
    pool.spp_begin = spp_begin;
    pool.spp_end = spp_end;
    pool.dynamic = dynamic ? 1u : 0u;
    pool.defer_regen = (dynamic && !exp_env("PT_NO_DEFER_REGEN")) ? 1u : 0u;
    pool.compact = (dc.motionless && !exp_env("PT_NO_COMPACT_RECORDS")) ? 1u : 0u;
    pool.total_work = total_work;
    pool.width = dc.width;
    pool.height = dc.height;
    pool.tiles_x = tiles_x;
    pool.n_tile_pixels = (uint32_t)n_tile_pixels64;
    pool.list = d_list;
    pool.n_list = list ? n_list : 0u;
    pool.list_store = list && opts.accum_on_device && opts.overwrite ? 1u : 0u;   // (a host accumulator is written below, pixel by pixel)
    // experiment (PT_INIT_SHUFFLE=1): k_init hands the initial items out permuted inside each 8192-slot granule (an odd multiplier), so
    // that the first K2 launch traces incoherent chunks — the measure of what tile-ordered chunks are worth
    if (dynamic && !list && exp_env("PT_INIT_SHUFFLE")) pool.init_perm = 0x9E3779B1u;

    // accumulator on the device (freed on every return path when it is ours)
    double* d_accum = accum;
    const size_t accum_bytes = (size_t)n_pixels * 3 * sizeof(double);
    struct AccumGuard {
        double* p = nullptr;
        ~AccumGuard() { if (p) (void)hipFree(p); }
    } own_accum;
    if (!opts.accum_on_device) {
        if (!hip_ok(hipMalloc((void**)&d_accum, accum_bytes), "hipMalloc(accum)")) return -1;
        own_accum.p = d_accum;
        if (!hip_ok(hipMemsetAsync(d_accum, 0, accum_bytes, st), "hipMemset(accum)")) return -1;
    } else if (opts.overwrite && !list) {   // (a list render stores its pixels instead: the others are not written)
        if (!hip_ok(hipMemsetAsync(d_accum, 0, accum_bytes, st), "hipMemset(accum)")) return -1;
    }

    // persistent grids: resident blocks per CU x CUs
    int mult = 1;
    if (const char* e = exp_env("PT_GRID_MULT")) mult = std::max(1, atoi(e));
    uint32_t wide_window_min = 16;
    if (const char* e = exp_env("PT_WIDE_WINDOW_MIN")) wide_window_min = (uint32_t)std::max(1, atoi(e));
    // K2 variant: two-phase kernel when there are meshes to defer and its LDS stack covers the scene's BVHs, else the
    // batch kernel. Experiment switches: PT_K2=batch forces the batch kernel; PT_EXT2 = stack*10 + blocks per CU picks
    // the instantiation. extend_code: -1 = batch, -(stack*10 + blocks) = two-phase.
    auto extend2_code = [&]() -> int {
        const int need = (int)s->stack_need_extend2;
        if (need > 32) return 0;
        // four blocks per CU where the LDS allows it (stacks of 16 and 20 entries): the kernel then runs at 128 registers with
        // 64 B of spills per lane and is still 7.5 % faster than at three blocks and 149 registers (round 2; in round 1, at
        // 166 registers, the same bound meant 168 B of spills and lost 11 %)
        // [r3, last] stacks of <= 16 entries: blocks of 128 threads over 1024-slot windows (code 2164, eight blocks per CU) — with the
        // queue's end in half windows the smaller block's shorter barrier waits win on every pool size: K2 -1.0 % (16.8 M slots), -1.8 %
        // (67 M, 134 M) against 256 threads; 64 threads: +1 % / -2.0 % / -2.5 % (worse on shallow pools); 512 threads: +5 %
        int code = need <= 16 ? 2164 : need <= 20 ? 204 : need <= 24 ? 243 : need <= 28 ? 283 : 323;
        if (const char* e = exp_env("PT_EXT2")) {
            const int c = atoi(e);
            if (c / 10 >= need && (c == 163 || c == 164 || c == 204 || c == 243 || c == 283 || c == 323)) code = c;
            if ((c == 1164 || c == 2164 || c == 8164) && need <= 16) code = c;
        }
        return code;
    };
    int extend_code = (s->n_mesh_entries > 0 && extend2_code() != 0) ? -extend2_code() : -1;
    if (const char* e = exp_env("PT_K2")) {
        if (!strcmp(e, "batch")) extend_code = -1;
        else if (!strcmp(e, "twophase") && extend2_code() != 0) extend_code = -extend2_code();
    }
    const int blocks_extend = extend_occupancy_blocks(extend_code == -1 && s->dev.view.tlas_flat ? (s->dev.view.flat_pairs ? -3 : -2) : extend_code), blocks_shade = shade_occupancy_blocks(form);
    if (blocks_shade < 1) return set_error("pt_render: no k_shade form for this combination of pixel list, environment sampling, sampler and media");
    const int grid_extend = ctx->n_cus * blocks_extend * mult, grid_shade = ctx->n_cus * blocks_shade * mult;

    pool.accum = d_accum;
    // dynamic mode: the kernels add into channel planes in work-item (tile) order (PoolD::accum_tiled); k_detile adds them to d_accum
    const bool tiled = dynamic && !exp_env("PT_ACCUM_LINEAR");
    if (tiled) {
        const size_t tb = (size_t)n_tile_pixels64 * 3 * sizeof(double);
        if (tb > s->tile_accum_bytes) {
            if (s->tile_accum) (void)hipFree(s->tile_accum);
            s->tile_accum = nullptr;
            s->tile_accum_bytes = 0;
            if (!hip_ok(hipMalloc((void**)&s->tile_accum, tb), "hipMalloc(tiled accumulator)")) return -1;
            s->tile_accum_bytes = tb;
        }
        if (!hip_ok(hipMemsetAsync(s->tile_accum, 0, tb, st), "hipMemset(tiled accumulator)")) return -1;
        pool.accum = s->tile_accum;
        pool.accum_tiled = 1u;
    }
    pool.inv_width = 1.0 / (double)dc.width;
    CountersD init_cnt;
    memset(&init_cnt, 0, sizeof init_cnt);
    init_cnt.alive = spp == 0 ? 0 : n_slots;   // every slot starts with one sample (k <= spp / n_slots <= total_work)
    for (uint32_t sh = 0; sh < WORK_SHARDS; ++sh) {   // dynamic mode: items 0 .. n_slots-1 were handed out by k_init
        const uint64_t row = (uint64_t)WORK_SHARDS * 64, rows = n_slots / row, rem = n_slots % row;
        const uint64_t part = rem > (uint64_t)sh * 64 ? std::min<uint64_t>(rem - (uint64_t)sh * 64, 64) : 0;
        init_cnt.work[sh].next = rows * 64 + part;
    }
    if (!hip_ok(hipMemcpyAsync(s->d_counters, &init_cnt, sizeof init_cnt, hipMemcpyHostToDevice, st), "hipMemcpy(counters)")) return -1;

    EventTimer timer;
    timer.enabled = opts.profile != 0;
    auto t0 = std::chrono::steady_clock::now();
    (void)hipStreamSynchronize(st);
    t0 = std::chrono::steady_clock::now();

    timer.begin(2, st);
    if (!launch_init(dc, pool, seed, grid_shade, st, form)) return set_error("pt_render: no k_init form for this render");
    timer.end(st);
    uint64_t iterations = 0;
    const uint64_t per_slot = dynamic ? (total_work + n_slots - 1) / std::max<uint64_t>(n_slots, 1) + 1 : (spp + k - 1) / k;
    const uint64_t max_iterations = per_slot * ((uint64_t)std::max(1u, dc.max_depth) + 1) + 4;   // + 1: a parked slot idles one iteration
    uint32_t poll_every = 8;
    const bool compact_ok = dynamic && !exp_env("PT_NO_COMPACT_POOL");
    uint32_t compactions = 0;
    uint64_t compact_num = 1, compact_den = 2;      // compact when live <= num/den of the slots still covered (25 % .. 85 % measured level: within 0.5 %)
    uint32_t poll_cap = 8;
    if (const char* e = exp_env("PT_COMPACT_AT")) { compact_num = (uint64_t)std::max(1, atoi(e)); compact_den = 100; }   // per cent
    if (const char* e = exp_env("PT_POLL_CAP")) poll_cap = (uint32_t)std::max(1, atoi(e));
    bool alive = spp != 0 && dc.max_depth != 0;
    if (spp != 0 && dc.max_depth == 0) {
        // max_depth = 0: trace() returns zero radiance for every sample (camera.rs:177); nothing to launch
        alive = false;
    }
    while (alive) {
        for (uint32_t i = 0; i < poll_every; ++i) {
            timer.begin(0, st);
            launch_extend(s->dev.view, pool, s->d_counters, grid_extend, extend_code, st);
            timer.end(st);
            timer.begin(1, st);
            if (!launch_shade(s->dev.view, dc, pool, s->d_counters, seed, grid_shade, form, st, wide_window_min, mode_has_table(mode) ? &env : nullptr)) return set_error("pt_render: no k_shade form for this render");
            timer.end(st);
            if (ordered) {   // what K3 wrote is the pool K2, the compaction and the next K3 read
                std::swap(pool.ray, pool.ray_out);
                std::swap(pool.path, pool.path_out);
                std::swap(pool.bounce, pool.bounce_out);
            }
            ++iterations;
        }
        if (!hip_ok(hipMemcpyAsync(s->h_counters, s->d_counters, sizeof(CountersD), hipMemcpyDeviceToHost, st), "hipMemcpy(counters)")) return -1;
        if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(render)")) return -1;
        timer.drain();
        const uint64_t n_alive = s->h_counters->alive;
        alive = n_alive != 0;
        if (alive && iterations > max_iterations + 128) return set_error("pt_render: iteration bound exceeded (internal error)");
        if (poll_every < poll_cap) poll_every *= 2;     // (a poll is a pipeline drain of some tens of microseconds: every 8 iterations costs <= 0.5 %)
        // the frame's end: once half of the slots still covered are dead the survivors move to the front and the launches shrink with them
        // (k_compact_scan / k_compact_move). The count is the last poll's — stale only towards MORE live slots, which errs on the safe side.
        if (compact_ok && alive && n_alive * compact_den <= (uint64_t)pool.n_alloc * compact_num && pool.n_alloc > 4 * 8192u) {
            const uint32_t new_end = (uint32_t)((n_alive + 8191) & ~(uint64_t)8191);
            const uint32_t cap = new_end;                                  // holes and movers are both at most the live count
            const size_t words = 2 * (size_t)cap + 2;
            if (words > s->compact_scratch_words) {
                if (s->compact_scratch) (void)hipFree(s->compact_scratch);
                s->compact_scratch = nullptr;
                s->compact_scratch_words = 0;
                if (!hip_ok(hipMalloc((void**)&s->compact_scratch, words * sizeof(uint32_t)), "hipMalloc(compaction lists)")) return -1;
                s->compact_scratch_words = words;
            }
            timer.begin(2, st);
            launch_compact(pool, new_end, s->compact_scratch, s->compact_scratch + cap, s->compact_scratch + 2 * (size_t)cap, cap, ctx->n_cus * 8, st);
            timer.end(st);
            pool.n_alloc = new_end;
            pool.n_slots = std::min(pool.n_slots, new_end);
            ++compactions;
        }
    }
    if (!dynamic || tiled) {
        timer.begin(2, st);
        if (tiled) launch_detile(pool, d_accum, ctx->n_cus * 8, st);
        else launch_resolve(pool, d_accum, ctx->n_cus * 8, st);
        timer.end(st);
    }
    if (!hip_ok(hipMemcpyAsync(s->h_counters, s->d_counters, sizeof(CountersD), hipMemcpyDeviceToHost, st), "hipMemcpy(counters)")) return -1;
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(resolve)")) return -1;
    timer.drain();
    auto t1 = std::chrono::steady_clock::now();
    if (!hip_ok(hipGetLastError(), "kernel launch")) return -1;

    if (!opts.accum_on_device && list) {   // only the listed pixels of the caller's frame are written
        std::vector<double> tmp((size_t)n_pixels * 3);
        if (!hip_ok(hipMemcpy(tmp.data(), d_accum, accum_bytes, hipMemcpyDeviceToHost), "hipMemcpy(accum)")) return -1;
        for (uint32_t i = 0; i < n_list; ++i)
            for (uint32_t c = 0; c < 3; ++c) {
                const size_t j = 3 * (size_t)h_list[i] + c;
                accum[j] = opts.overwrite ? tmp[j] : accum[j] + tmp[j];
            }
    } else if (!opts.accum_on_device) {
        if (opts.overwrite) {
            if (!hip_ok(hipMemcpy(accum, d_accum, accum_bytes, hipMemcpyDeviceToHost), "hipMemcpy(accum)")) return -1;
        } else {
            std::vector<double> tmp((size_t)n_pixels * 3);
            if (!hip_ok(hipMemcpy(tmp.data(), d_accum, accum_bytes, hipMemcpyDeviceToHost), "hipMemcpy(accum)")) return -1;
            for (size_t i = 0; i < tmp.size(); ++i) accum[i] += tmp[i];
        }
    }
    if (exp_env("PT_PROF")) {   // diagnostic builds (-DPT_STAMPS): wave-cycle sums per k_shade class
        static const char* names[N_CLASSES + 1] = {"miss", "diffuse", "metal", "glass", "principled", "light", "sheen", "clearcoat", "mix", "idle", "dead", "WINDOW"};
        for (uint32_t c = 0; c <= N_CLASSES; ++c) {
            const unsigned long long* p = s->h_counters->prof[c];
            if (p[0] && c == CLASS_DEAD)
                fprintf(stderr, "[pt prof] K2 window  n %10llu  phase A %8.0f  barrier %8.0f  phase B %8.0f  barrier %8.0f  candidates %6.1f (cycles per window and wave)\n", p[0],
                        (double)p[1] / p[0], (double)p[2] / p[0], (double)p[3] / p[0], (double)p[4] / p[0], (double)p[5] / p[0]);
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
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->samples = s->h_counters->samples;
        stats->segments = s->h_counters->segments;
        stats->iterations = iterations;
        stats->n_slots = n_slots;
        stats->slots_per_pixel = dynamic ? 0u : k;
        stats->ms_total = std::chrono::duration<double, std::milli>(t1 - t0).count();
        stats->ms_extend = timer.ms[0];
        stats->ms_shade = timer.ms[1];
        stats->ms_other = timer.ms[2];
        stats->launches_extend = timer.launches[0];
        stats->launches_shade = timer.launches[1];
        stats->extend_variant = extend_code <= -100 ? 0u : 1u;
        stats->shade_variant = (uint32_t)shade_variant;
        stats->blocks_extend = (uint32_t)grid_extend;
        stats->blocks_shade = (uint32_t)grid_shade;
        stats->compactions = compactions;
        stats->n_alloc_end = pool.n_alloc;
    }
    return 0;
}

extern "C" int pt_render(pt_scene* s, const pt_camera* cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* accum,
                         const pt_render_opts* opts, pt_render_stats* stats) {
    return render_core(s, cam, seed, spp_begin, spp_end, accum, opts, stats, nullptr, nullptr, 0);
}

namespace {
uint32_t tiled_key(uint32_t p, uint32_t width, uint32_t tiles_x) {   // row-major pixel -> its tiled index (k_detile's tiled_index)
    const uint32_t y = p / width, x = p % width;
    return ((y >> 3) * tiles_x + (x >> 3)) * 64u + ((y & 7u) << 3) + (x & 7u);
}
// the scene's device pixel list (re-used like tile_accum), at least n entries
bool pixel_list_buffer(pt_scene* s, size_t n) {
    if (n <= s->pixel_list_words) return true;
    if (s->pixel_list) (void)hipFree(s->pixel_list);
    s->pixel_list = nullptr;
    s->pixel_list_words = 0;
    if (!hip_ok(hipMalloc((void**)&s->pixel_list, n * sizeof(uint32_t)), "hipMalloc(pixel list)")) return false;
    s->pixel_list_words = n;
    return true;
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
    if (!pixel_list_buffer(s, n)) return -1;
    if (!hip_ok(hipMemcpy(s->pixel_list, sorted.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(pixel list)")) return -1;
    return render_core(s, cam, seed, spp_begin, spp_end, accum, opts, stats, s->pixel_list, sorted.data(), n);
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
    struct Mem {
        void* p = nullptr;
        ~Mem() { if (p) (void)hipFree(p); }
    } mem;
    if (!hip_ok(hipMalloc(&mem.p, f64s * sizeof(double) + u32s * sizeof(uint32_t)), "hipMalloc(adaptive state)")) return -1;
    double* E = (double*)mem.p;
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

extern "C" int pt_resolve_u8_counts(pt_ctx* ctx, const double* accum, uint32_t n_pixels, const uint32_t* spp_per_pixel, uint8_t* rgb8) {
    if (!ctx) return set_error("pt_resolve_u8_counts: null context");
    if (!accum || !spp_per_pixel || !rgb8) return set_error("pt_resolve_u8_counts: null buffer");
    for (uint32_t p = 0; p < n_pixels; ++p)
        if (spp_per_pixel[p] == 0) return set_error("pt_resolve_u8_counts: a pixel has no samples");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    const size_t n = (size_t)n_pixels * 3;
    double* d_in = nullptr;
    uint32_t* d_cnt = nullptr;
    uint8_t* d_out = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_in, n * sizeof(double) + 8), "hipMalloc") && hip_ok(hipMalloc((void**)&d_cnt, (size_t)n_pixels * 4 + 4), "hipMalloc") &&
              hip_ok(hipMalloc((void**)&d_out, n + 1), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_in, accum, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy") &&
              hip_ok(hipMemcpyAsync(d_cnt, spp_per_pixel, (size_t)n_pixels * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_quantise_counts(d_in, n_pixels, d_cnt, d_out, ctx->stream);
        ok = hip_ok(hipMemcpyAsync(rgb8, d_out, n, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_in) (void)hipFree(d_in);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_out) (void)hipFree(d_out);
    return ok ? 0 : -1;
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
    struct Mem {
        double* p = nullptr;
        ~Mem() { if (p) (void)hipFree(p); }
    } own;
    double* d_aov = aov;
    if (!opts.accum_on_device) {   // a host buffer: its sums travel to the device and back, the kernel adds to them there
        if (!hip_ok(hipMalloc((void**)&own.p, bytes), "hipMalloc(aov)")) return -1;
        d_aov = own.p;
        if (!opts.overwrite && !hip_ok(hipMemcpyAsync(d_aov, aov, bytes, hipMemcpyHostToDevice, st), "hipMemcpy(aov)")) return -1;
    }
    ShadeForm aov_form;   // of a form, the AOV walk looks at the sampler only
    aov_form.qmc = s->sampler == 1;
    if (!launch_aov(s->dev.view, dc, seed, spp_begin, spp_end, d_aov, opts.overwrite != 0, ctx->n_cus * 8, st, aov_form))
        return set_error("pt_render_aovs: no k_aov form for this sampler");
    if (!hip_ok(hipGetLastError(), "kernel launch")) return -1;
    if (!opts.accum_on_device && !hip_ok(hipMemcpyAsync(aov, d_aov, bytes, hipMemcpyDeviceToHost, st), "hipMemcpy(aov)")) return -1;
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(aov)") ? 0 : -1;
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
    struct Mem {
        double* p = nullptr;
        ~Mem() { if (p) (void)hipFree(p); }
    } mem;
    if (!hip_ok(hipMalloc((void**)&mem.p, n * 29 * sizeof(double)), "hipMalloc(denoise)")) return -1;
    double* d_tmp = mem.p;
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
    struct Mem {
        void* p = nullptr;
        ~Mem() { if (p) (void)hipFree(p); }
    } mem;
    if (f64s + tail > 0 && !hip_ok(hipMalloc(&mem.p, f64s * sizeof(double) + tail), "hipMalloc(film)")) return -1;
    double* at = (double*)mem.p;
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

extern "C" int pt_resolve_u8(pt_ctx* ctx, const double* accum, uint32_t n_pixels, uint32_t total_spp, uint8_t* rgb8) {
    if (!ctx) return set_error("pt_resolve_u8: null context");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    const uint32_t n = n_pixels * 3;
    double* d_in = nullptr;
    uint8_t* d_out = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_in, (size_t)n * sizeof(double)), "hipMalloc") && hip_ok(hipMalloc((void**)&d_out, n), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_in, accum, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_quantise(d_in, n, 1.0 / (double)total_spp, d_out, ctx->stream);   // pixel_sample_scale camera.rs:53
        ok = hip_ok(hipMemcpyAsync(rgb8, d_out, n, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return ok ? 0 : -1;
}

extern "C" int pt_intersect(pt_scene* s, const double* rays, uint32_t n, double* out) {
    if (!s || !s->built) return set_error("pt_intersect: world not built");
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    double *d_r = nullptr, *d_o = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_r, (size_t)n * 7 * sizeof(double) + 8), "hipMalloc") &&
              hip_ok(hipMalloc((void**)&d_o, (size_t)n * 15 * sizeof(double) + 8), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_r, rays, (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_probe(s->dev.view, d_r, n, d_o, ctx->stream);
        ok = hip_ok(hipMemcpyAsync(out, d_o, (size_t)n * 15 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_r) (void)hipFree(d_r);
    if (d_o) (void)hipFree(d_o);
    return ok ? 0 : -1;
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
    if (!hip_ok(hipMemcpyAsync(&T, s->dev.view.tex + dc.env_tex, sizeof T, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") ||
        !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))
        return -1;
    const size_t n_in = (size_t)n * (which == 0 ? 2 : 3), n_out = (size_t)n * (which == 0 ? 4 : 1);
    double *d_i = nullptr, *d_o = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_i, n_in * sizeof(double) + 8), "hipMalloc") &&
              hip_ok(hipMalloc((void**)&d_o, n_out * sizeof(double) + 8), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_i, in, n_in * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_env_probe(s->dev.view, T, e, which, d_i, n, d_o, ctx->stream);
        ok = hip_ok(hipMemcpyAsync(out, d_o, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_i) (void)hipFree(d_i);
    if (d_o) (void)hipFree(d_o);
    return ok ? 0 : -1;
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
    double *d_i = nullptr, *d_o = nullptr;
    GridD* d_g = nullptr;
    float* d_v = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_i, n_in * sizeof(double)), "hipMalloc") && hip_ok(hipMalloc((void**)&d_o, n_out * sizeof(double)), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_i, in, n_in * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok && grid) {   // the medium's own grid, uploaded for the call (the world need not be built)
        const HostGrid& hg = s->grids[(size_t)s->mats[mat].p[6] - 1];
        ok = hip_ok(hipMalloc((void**)&d_g, sizeof(GridD)), "hipMalloc") && hip_ok(hipMalloc((void**)&d_v, hg.vals.size() * sizeof(float)), "hipMalloc") &&
             hip_ok(hipMemcpyAsync(d_g, &hg.d, sizeof(GridD), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy") &&
             hip_ok(hipMemcpyAsync(d_v, hg.vals.data(), hg.vals.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    }
    if (ok) {
        if (grid) launch_grid_probe(which, d_g, d_v, d_i, n, d_o, ctx->stream);
        else if (which == 4) launch_absorb_probe(s->mats[mat].p + 7, d_i, n, d_o, ctx->stream);
        else launch_medium_probe(which, s->mats[mat].p[0], s->mats[mat].p[1], d_i, n, d_o, ctx->stream);
        ok = hip_ok(hipGetLastError(), "kernel launch") &&
             hip_ok(hipMemcpyAsync(out, d_o, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_i) (void)hipFree(d_i);
    if (d_o) (void)hipFree(d_o);
    if (d_g) (void)hipFree(d_g);
    if (d_v) (void)hipFree(d_v);
    return ok ? 0 : -1;
}

extern "C" int pt_light_probe(pt_scene* s, int which, const double* in, uint32_t n, double* out) {
    if (!s || !s->built) return set_error("pt_light_probe: world not built");
    if (which != 0 && which != 1) return set_error("pt_light_probe: which must be 0 or 1");
    if (s->dev.view.n_lights == 0u) return set_error("pt_light_probe: the world has no lights list");
    const bool exact = s->light_sampling == 1;
    if (exact && s->light_mesh_bad_area) return set_error("pt_light_probe: exact light sampling needs light meshes of finite, positive area");
    if (exact && s->light_blas_depth > (uint32_t)LIGHT_STACK) return set_error("pt_light_probe: exact light sampling: a light mesh's BVH is deeper than the 24 levels its pdf walk's stack holds");
    if (n == 0) return 0;
    if (!in || !out) return set_error("pt_light_probe: null buffer");
    const size_t n_in = (size_t)n * (which == 0 ? 4 : 7), n_out = (size_t)n * (which == 0 ? 6 : 1);
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    double *d_i = nullptr, *d_o = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_i, n_in * sizeof(double)), "hipMalloc") && hip_ok(hipMalloc((void**)&d_o, n_out * sizeof(double)), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_i, in, n_in * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_light_probe(s->dev.view, exact, which, d_i, n, d_o, ctx->stream);
        ok = hip_ok(hipGetLastError(), "kernel launch") &&
             hip_ok(hipMemcpyAsync(out, d_o, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_i) (void)hipFree(d_i);
    if (d_o) (void)hipFree(d_o);
    return ok ? 0 : -1;
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
    double *d_i = nullptr, *d_o = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_i, n_in * sizeof(double)), "hipMalloc") && hip_ok(hipMalloc((void**)&d_o, n_out * sizeof(double)), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_i, in, n_in * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_dispersion_probe(s->sampler, which, seed, m.ior, m.p[1], m.p[2], d_w, d_i, n, d_o, ctx->stream);
        ok = hip_ok(hipGetLastError(), "kernel launch") &&
             hip_ok(hipMemcpyAsync(out, d_o, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_i) (void)hipFree(d_i);
    if (d_o) (void)hipFree(d_o);
    return ok ? 0 : -1;
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
    pt_ctx* ctx = s->ctx;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    double *d_i = nullptr, *d_o = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_i, (size_t)n * 2 * sizeof(double)), "hipMalloc") && hip_ok(hipMalloc((void**)&d_o, (size_t)n * 8 * sizeof(double)), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_i, in, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_camera_probe(dc, s->sampler, seed, d_i, n, d_o, ctx->stream);
        ok = hip_ok(hipGetLastError(), "kernel launch") &&
             hip_ok(hipMemcpyAsync(out, d_o, (size_t)n * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_i) (void)hipFree(d_i);
    if (d_o) (void)hipFree(d_o);
    return ok ? 0 : -1;
}

extern "C" int pt_sampler_probe(pt_ctx* ctx, int kind, uint64_t seed, uint32_t pixel, uint32_t sample_begin, uint32_t n_samples, uint32_t draw_begin,
                                uint32_t n_draws, uint64_t* out) {
    if (!ctx) return set_error("pt_sampler_probe: null context");
    if (kind != 0 && kind != 1) return set_error("pt_sampler_probe: kind must be 0 (independent) or 1 (Sobol)");
    const uint64_t n = (uint64_t)n_samples * n_draws;
    if (n == 0) return 0;
    if (!out || n > (1ull << 28)) return set_error("pt_sampler_probe: null output or more than 2^28 values");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    uint64_t* d_o = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_o, n * sizeof(uint64_t)), "hipMalloc");
    if (ok) {
        launch_sampler_probe(kind, seed, pixel, sample_begin, n_samples, draw_begin, n_draws, d_o, ctx->stream);
        ok = hip_ok(hipGetLastError(), "kernel launch") &&
             hip_ok(hipMemcpyAsync(out, d_o, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_o) (void)hipFree(d_o);
    return ok ? 0 : -1;
}

extern "C" int pt_math_probe(pt_ctx* ctx, int which, const double* in, uint32_t n, double* out) {
    if (!ctx) return set_error("pt_math_probe: null context");
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return -1;
    double *d_i = nullptr, *d_o = nullptr;
    bool ok = hip_ok(hipMalloc((void**)&d_i, (size_t)n * 2 * sizeof(double) + 8), "hipMalloc") &&
              hip_ok(hipMalloc((void**)&d_o, (size_t)n * sizeof(double) + 8), "hipMalloc") &&
              hip_ok(hipMemcpyAsync(d_i, in, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy");
    if (ok) {
        launch_math_probe(which, d_i, n, d_o, ctx->stream);
        ok = hip_ok(hipMemcpyAsync(out, d_o, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy") &&
             hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (d_i) (void)hipFree(d_i);
    if (d_o) (void)hipFree(d_o);
    return ok ? 0 : -1;
}
