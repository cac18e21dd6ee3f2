// Host-callable launchers of the HIP kernels: one per stage. K2 is in pt_k2.hip, K1 / K3 / the AOV walk in pt_k3.hip and the units
// pt_forms.h form_unit names (pt_k3_*.hip: the Sobol sampler's forms and one unit per shading mode), the small kernels in pt_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "pt_types.h"

namespace pt {
// What a render asks of K1 / K3 / the AOV walk. variant: k_shade's shape code (pt_forms.h SHADE_SHAPES; PT_SHADE_VARIANT); lights: the scene
// has a lights list; list: pixel-list render (PoolD::list); qmc: the Sobol sampler (pt_scene_set_sampler); mode: the
// shading mode (pt_types.h ShadeMode); motion: motion is in effect (pt_scene_motion); punctual: punctual lights are in effect
// (pt_light_point ...). Which forms exist: pt_forms.h shade_form_exists.
struct ShadeForm { int variant = 0; bool lights = false, list = false, qmc = false; ShadeMode mode = MODE_PLAIN; bool motion = false, punctual = false; };
// The form a render gets: pixel lists, qmc and every mode but the plain one exist for the default variant's shapes only — any other variant becomes 42.
// The launchers and queries below take the form this returns.
ShadeForm shade_form(ShadeForm asked);
// whether the form's k_shade sorts its windows by class (the shading-order output, PoolD::reorder, needs the sort's positions)
bool shade_form_sorts(const ShadeForm& form);
// whether the form's K1 / K3 read the sky pass's tile map (pt_types.h sky_pass_form): the pass is off for a render whose form does not
bool shade_form_maps_tiles(const ShadeForm& form);
// The launchers that take a form return false, having launched nothing, when no kernel of that form exists.
bool launch_init(const CamD& cam, const PoolD& pool, uint64_t seed, int max_blocks, hipStream_t st, const ShadeForm& form);
// K2 variant code (`code` of launch_extend / extend_occupancy_blocks): -1 = batch kernel (-2 / -3 ask extend_occupancy_blocks for its
// flat-top-level instantiation without / with pair passes), -(stack*10 + blocks) = two-phase kernel k_extend2<stack, blocks> for stack in {16, 20, 24}.
// motion: the MOT forms (instances posed at each ray's time). They exist for the batch kernel and the default two-phase codes; another
// two-phase code becomes the default one for its stack.
// split: the two-phase kernel's rule for mid-window rounds (pt_k2_extend.h K2_SPLIT_*; 0: none, 1: at half a window, 2: drain); the batch kernel has none.
void launch_extend(const SceneD& sc, const PoolD& pool, CountersD* cnt, int max_blocks, int code, hipStream_t st, bool motion = false, uint32_t split = 1);
// wide_window_min (variant 42): 8192-slot windows while the pool holds at least that many of them per block launched, 4096-slot ones below
// env: the table argument of a mode that has one (pt_types.h mode_has_table) — the ENV forms' tables; the DSP forms' weight table (device, DSP_BINS x 3) in `col` — else null
bool launch_shade(const SceneD& sc, const CamD& cam, const PoolD& pool, CountersD* cnt, uint64_t seed, int max_blocks, const ShadeForm& form, hipStream_t st,
                  uint32_t wide_window_min = 16, const EnvTabD* env = nullptr);
// resident blocks per CU of the K2 / K3 kernel a render launches (shade: 0 when no kernel of that form exists)
int extend_occupancy_blocks(int code, bool motion = false);
int shade_occupancy_blocks(const ShadeForm& form);
// pt_medium_probe: the medium functions k_shade's MED forms call (which 0: n x (u1, u2, dir.xyz) -> n x (new_dir.xyz, ph); 1: n x u ->
// n free-flight distances); in / out: device
void launch_medium_probe(int which, double density, double g, const double* in, uint32_t n, double* out, hipStream_t st);
// ... and the grid-density functions the HET forms call (which 2: n points -> sigma; 3: n x (o.xyz, dir.xyz, t) -> n x (collided, s, draws
// consumed), row i with the independent sampler's draws of (seed 0, pixel i, sample 0) from draw 0); grid, vals: device
void launch_grid_probe(int which, const GridD* grid, const float* vals, const double* in, uint32_t n, double* out, hipStream_t st);
// ... and the attenuation the INT forms apply (which 4: n lengths -> n x 3 factors exp(-(a_c * l)), exactly 1 where a_c == 0)
void launch_absorb_probe(const double absorption[3], const double* in, uint32_t n, double* out, hipStream_t st);
// pt_light_probe: lights.sample / lights.pdf as k_shade calls them (exact: the LSE forms' functions, else the reference's; which 0: n x
// (origin.xyz, time) -> n x (dir.xyz, light index, face or -1, draws consumed), row i with the independent sampler's draws of (seed 0,
// pixel i, sample 0) from draw 0; which 1: n x (origin.xyz, direction.xyz, time) -> n lights.pdf values); in / out: device
// (a scene with moving instances — SceneD::inst_motion — is probed with every instance posed at the row's time)
void launch_light_probe(const SceneD& sc, bool exact, int which, const double* in, uint32_t n, double* out, hipStream_t st);
// pt_dispersion_probe: the device functions k_shade's DSP forms call (which 0: n x (pixel, sample) -> n x (u, lambda, bin, W_r, W_g, W_b, n(lambda)) under
// sampler `kind`; 1: n wavelengths in nm -> n values n(lambda)); n_d, b, inv2_d: the glass's MatD::ior, p[1], p[2]; w: the weight table; in / out / w: device
void launch_dispersion_probe(int kind, int which, uint64_t seed, double n_d, double b, double inv2_d, const double* w, const double* in, uint32_t n, double* out, hipStream_t st);
// pt_sampler_probe: the 64-bit values of single draws, by the draw functions the kernels call (kind 0: Rng, 1: RngQ); out: device
void launch_sampler_probe(int kind, uint64_t seed, uint32_t pixel, uint32_t sample_begin, uint32_t n_samples, uint32_t draw_begin, uint32_t n_draws, uint64_t* out,
                          hipStream_t st);
// pt_envmap.hip: the environment-sampling tables of image texture `tex` (device TexD values; col: H * (W + 1), row: H + 1 doubles),
// and the probe behind pt_env_probe (which 0: (u1, u2) pairs -> {dir.xyz, pdf}; 1: directions -> env_pdf)
void launch_env_tables(const SceneD& sc, const TexD& tex, double* col, double* row, hipStream_t st);
void launch_env_probe(const SceneD& sc, const TexD& tex, const EnvTabD& e, int which, const double* in, uint32_t n, double* out, hipStream_t st);
void launch_resolve(const PoolD& pool, double* accum, int max_blocks, hipStream_t st);
// the frame's end (dynamic mode): live slots beyond new_end move into dead slots below it; holes / movers: scratch lists of `cap` entries, counts: 2 words
void launch_compact(const PoolD& pool, uint32_t new_end, uint32_t* holes, uint32_t* movers, uint32_t* counts, uint32_t cap, int max_blocks, hipStream_t st);
void launch_detile(const PoolD& pool, double* accum, int max_blocks, hipStream_t st);
// pt_k_sky.hip: the sky pass. launch_sky_classify: the tile test of every tile against the boxes (device, six doubles each), then
// tile_map (active-tile index -> tile), sky_list (the sure-sky tiles), both in tile order, and counts = {active tiles, sure-sky tiles, pixels of
// the sure-sky tiles inside the image}; flags: n_tiles bytes of scratch. launch_sky: samples [spp_begin, spp_end) of every pixel of the listed
// tiles, `chunk` samples per wave, added to the tiled accumulator and to the sample and segment counts.
// The short-path pass: `shadeable` = the boxes (bit b = box b) of the entries k_short can shade, 0 = none: only sure-sky and
// wavefront tiles come out. Of the SHORT tiles — every box not cleared is shadeable — the first max_short in tile order go to short_list, the
// rest stay in tile_map; counts[3..5] = short tiles taken, their pixels inside the image, short tiles found. launch_short (pt_k_short.hip):
// samples [spp_begin, spp_end) of every pixel of the short tiles, finished where the path is camera -> (miss | shadeable hit -> miss), else
// appended to the hard list (pt_types.h ShortArgsD).
struct SkyCam;
struct ReachOrder;
void launch_sky_classify(const SkyCam& cam, uint32_t n_boxes, const double* boxes6, unsigned long long shadeable, uint32_t max_short, uint32_t n_tiles, uint8_t* flags,
                         uint32_t* tile_map, uint32_t* sky_list, uint32_t* short_list, uint32_t* counts, uint32_t* reach, const ReachOrder& order, hipStream_t st);   // (reach: null, or the tiles' reach masks in `order`)
void launch_sky_scan(uint32_t width, uint32_t height, uint32_t max_short, uint32_t n_tiles, const uint8_t* flags, uint32_t* tile_map, uint32_t* sky_list,
                     uint32_t* short_list, uint32_t* counts, hipStream_t st);   // (the scan of launch_sky_classify alone; counts: 8 words)
void launch_short(const SceneD& sc, const CamD& cam, const PoolD& pool, uint64_t seed, const ShortArgsD& a, hipStream_t st);
// the pilot's selection (pt_k_short.hip k_short_select): flags of the piloted wavefront tiles -> SKY_TILE_TAKEN where the yield bin >= min_bin; hist: 3 * SHORT_YIELD_BINS words
void launch_short_select(uint8_t* flags, uint32_t n_tiles, const uint32_t* pilot, uint32_t min_bin, uint32_t* hist, hipStream_t st);
void launch_sky(const SceneD& sc, const CamD& cam, const PoolD& pool, CountersD* cnt, uint64_t seed, const uint32_t* sky_list, uint32_t n_sky, uint32_t chunk,
                hipStream_t st);
// pt_adaptive.hip: the adaptive render's per-round kernels (see there)
void launch_adapt_error(const double* E, const double* O, const uint32_t* stop, uint32_t n_pixels, double n_e, double n_o, double* err, hipStream_t st);
void launch_adapt_select(const double* err, uint32_t* stop, uint32_t width, uint32_t height, double threshold, uint32_t stop_value, uint32_t* block_counts,
                         uint32_t* list_out, uint32_t* n_out, hipStream_t st);
void launch_adapt_final(double* E, const double* O, const uint32_t* stop, uint32_t n_pixels, uint32_t max_spp, uint32_t* counts, hipStream_t st);
void launch_quantise_counts(const double* accum, uint32_t n_pixels, const uint32_t* counts, uint8_t* rgb8, hipStream_t st);
uint32_t adapt_select_blocks(uint32_t width, uint32_t height);   // entries of launch_adapt_select's block_counts
void launch_quantise(const double* accum, uint32_t n, double scale, uint8_t* rgb8, hipStream_t st);
void launch_probe(const SceneD& sc, const double* rays, uint32_t n, double* out, hipStream_t st);
// pt_render_aovs: first-hit feature sums of samples [spp_begin, spp_end) of every pixel (aov: device, 8 doubles per pixel); of `form`, qmc matters
bool launch_aov(const SceneD& sc, const CamD& cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov, bool overwrite, int max_blocks,
                hipStream_t st, const ShadeForm& form);
// pt_denoise.hip: the a-trous denoiser (see there). Device buffers; tmp: 12 doubles per pixel of scratch
void launch_denoise(uint32_t width, uint32_t height, const double* sum_a, double n_a, const double* sum_b, double n_b, const double* aov, double n_aov,
                    uint32_t iterations, double sigma_l, double sigma_z, double* tmp, double* out, hipStream_t st);
// pt_film.hip: the film stage (see there). Device buffers. bright / glare: 3 planes of n_pixels doubles; counts: per-pixel sample counts or
// null (then scale = 1 / total_spp); launch_film_conv: one transposing pass (in: 3 planes rows x cols, out: 3 planes cols x rows, taps: 2 r + 1
// weights), false when the radius needs more LDS than a CU has; launch_film_develop: glare null = no glare, hdr or rgb8 may be null
void launch_film_prepare(const double* sums, uint32_t n_pixels, double scale, const uint32_t* counts, double k, double thr, double* bright, hipStream_t st);
bool launch_film_conv(const double* in, double* out, uint32_t rows, uint32_t cols, uint32_t r, const double* taps, double scale, bool accumulate, hipStream_t st);
void launch_film_develop(const double* sums, uint32_t n_pixels, double scale, const uint32_t* counts, double k, double thr, double s, const double* glare,
                         uint32_t tonemap, double white, double* hdr, uint8_t* rgb8, hipStream_t st);
// pt_camera_probe: generate_ray as k_init calls it under sampler `kind` (n x (pixel, sample) -> n x (origin.xyz, direction.xyz, time, draws consumed)); in / out: device
// motion: the shutter is applied (motion is in effect)
// the light grid's table: g.cells rows of n doubles into `table`; stage: through LDS (the default) or lane-per-cell stores
void launch_punctual_grid(const PunctualD* lights, uint32_t n, const PunctualGridBuild& g, double* table, bool stage, hipStream_t st);
// pt_punctual_probe: the punctual lights' device functions as k_shade's PLT forms call them (which 0: n x point.xyz -> n x (k, w.xyz, D, E.rgb, draws
// consumed), row i with the independent sampler's draws of (seed 0, pixel i, sample 0) from draw 0; 1: n x (k, point.xyz) -> n x (w.xyz, D, E.rgb)); in / out: device
// (the light grid in effect: 2: n x point.xyz -> n x (cell, k, p, draws consumed, w.xyz, D, E.rgb); 3: n x (cell, k) -> n x C[cell][k])
void launch_punctual_probe(const SceneD& sc, int which, const double* in, uint32_t n, double* out, hipStream_t st);
void launch_camera_probe(const CamD& cam, int kind, uint64_t seed, const double* in, uint32_t n, double* out, hipStream_t st, bool motion = false);
void launch_math_probe(int which, const double* in, uint32_t n, double* out, hipStream_t st);
}  // namespace pt
