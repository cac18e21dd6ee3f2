// CLI with the reference's two flags (src/main.rs:620-645): -q/--quality toggles
// 1920 px @ 4000 spp vs 600 px @ 100 spp, -s/--scene N picks the scene script. Extra,
// explicit overrides (not in the reference): --width, --spp, --seed, --out, --assets, --device, --float-hdr
// (.hdr environments keep their f32 samples instead of the reference's .to_rgb8() squash, texture.rs:67),
// --adaptive T [--min-spp M] (adaptive sampling to the noise target T, pt_render_adaptive; --spp is then the cap),
// --denoise [--aov-spp N] (two half-frames + first-hit AOVs over min(N, spp) samples through pt_denoise; N defaults to 16).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "scenes.hpp"

using namespace path_tracer;

int main(int argc, char** argv) {
    bool quality = false, float_hdr = false;
    int scene = 1, device = 0;
    long width = -1, spp = -1, min_spp = 16;
    double adaptive = 0.0, env_sampling = 0.0;
    bool use_adaptive = false, use_denoise = false;
    int sampler = 0;
    long aov_spp = 16;
    uint64_t seed = 1;
    std::string out, assets = "assets";
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) { std::cerr << "missing value for " << a << "\n"; exit(2); }
            return argv[++i];
        };
        if (a == "-q" || a == "--quality") quality = true;
        else if (a == "-s" || a == "--scene") scene = atoi(next());
        else if (a == "--width") width = atol(next());
        else if (a == "--spp") spp = atol(next());
        else if (a == "--seed") seed = strtoull(next(), nullptr, 10);
        else if (a == "--out") out = next();
        else if (a == "--assets") assets = next();
        else if (a == "--device") device = atoi(next());
        else if (a == "--float-hdr") float_hdr = true;
        else if (a == "--env-sampling") {
            env_sampling = atof(next());
            if (!(env_sampling >= 0.0 && env_sampling < 1.0)) { std::cerr << "--env-sampling must be in [0, 1)\n"; return 2; }
        }
        else if (a == "--sampler") {
            const std::string v = next();
            if (v == "independent") sampler = 0;
            else if (v == "sobol") sampler = 1;
            else { std::cerr << "--sampler must be independent or sobol\n"; return 2; }
        }
        else if (a == "--adaptive") { adaptive = atof(next()); use_adaptive = true; }
        else if (a == "--min-spp") min_spp = atol(next());
        else if (a == "--denoise") use_denoise = true;
        else if (a == "--aov-spp") aov_spp = atol(next());
        else if (a == "-h" || a == "--help") {
            std::cout << "usage: pt_render [-q] [-s N] [--width W] [--spp S] [--seed K] [--out file.png] [--assets DIR] [--device D] [--float-hdr] [--env-sampling F] [--sampler independent|sobol] [--adaptive T [--min-spp M]] [--denoise [--aov-spp N]]\n";
            return 0;
        } else { std::cerr << "unknown argument " << a << "\n"; return 2; }
    }
    size_t w = quality ? 1920 : 600, s = quality ? 4000 : 100;   // main.rs:633
    if (width > 0) w = (size_t)width;
    if (spp > 0) s = (size_t)spp;
    if (use_denoise && use_adaptive) { std::cerr << "--denoise and --adaptive cannot be combined\n"; return 2; }
    if (use_denoise && s < 2) { std::cerr << "--denoise needs at least 2 samples per pixel\n"; return 2; }
    if (use_denoise && aov_spp < 1) { std::cerr << "--aov-spp must be positive\n"; return 2; }
    if (scene < 1 || scene > 7) return 0;   // `_ => ()` main.rs:643
    pt_ctx* ctx = nullptr;
    if (pt_ctx_create(device, &ctx) != 0) {
        std::cerr << "fatal: " << pt_last_error() << "\n";
        return 1;
    }
    try {
        SceneSetup setup = make_scene(scene, w, s, assets, 1);
        setup.world.float_hdr = float_hdr;
        setup.world.env_sampling = env_sampling;
        setup.world.sampler = sampler;
        setup.world.build_bvh(ctx, setup.camera.environment.is_map ? setup.camera.environment.map : nullptr);
        setup.camera.init();
        std::cerr << "rendering production\n";   // camera.rs:101
        if (use_adaptive) {
            const uint32_t m = (uint32_t)std::max(2L, std::min(min_spp, (long)s));
            setup.camera.render_adaptive(setup.world, out.empty() ? setup.output : out, adaptive, m, seed);
        } else if (use_denoise) {
            setup.camera.render_denoised(setup.world, out.empty() ? setup.output : out, (uint32_t)aov_spp, seed);
        } else {
            setup.camera.render(setup.world, out.empty() ? setup.output : out, seed);
        }
        setup.world.release();
    } catch (const std::exception& e) {
        std::cerr << "panic: " << e.what() << "\n";   // the reference unwrap()s asset errors
        pt_ctx_destroy(ctx);
        return 101;
    }
    pt_ctx_destroy(ctx);
    return 0;
}
