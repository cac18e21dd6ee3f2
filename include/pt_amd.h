/* pt_amd.h — C ABI of the MI355X-native wavefront path tracer (libpt_amd.so).
 *
 * Drop-in boundary for ONE path of chiefchewie/thu-acg-f2024-path-tracer: the per-pixel
 * integrator entered through `Camera::render(&self, world: &World, filename)`
 * (src/camera.rs:79) and everything below it (camera.rs trace loop, hittable/ BVH traversal
 * and primitive intersection, bsdf/ sample+pdf+eval). The scene / material / camera builder
 * calls mirror the reference's constructors one-to-one so that its main.rs scene scripts map
 * onto this header line by line (INTEGRATION.md shows the Rust `extern "C"` binding).
 *
 * Conventions: plain C types only; every call returns 0 (or a handle >= 0) on success and
 * -1 on error with pt_last_error() describing it; nothing panics or throws across the ABI.
 * Handles (textures, materials, objects) are small ints local to one pt_scene. A pt_ctx and
 * its scenes are not thread-safe: one render at a time per context. There is NO CPU
 * fallback: every entry point that computes needs the HIP device and fails loudly without.
 *
 * Arithmetic: the reference computes in f64 (src/vec3.rs:3-6); so do these kernels.
 */
#ifndef PT_AMD_H
#define PT_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_ctx pt_ctx;       /* one HIP device + stream */
typedef struct pt_scene pt_scene;   /* World + its textures/materials/objects (hittable/world.rs:5-8) */

/* The 12 public fields of `Camera` (src/camera.rs:23-36). environment: Color(Vec3) or
 * Map(ImageTexture) (camera.rs:16-19) -> env_is_map + env_color / env_tex. */
typedef struct pt_camera {
    double aspect_ratio;
    uint32_t image_width, samples_per_pixel, max_depth, env_is_map;
    double vfov;
    double look_from[3], look_at[3], vup[3];
    double blur_strength, focal_length, defocus_angle;
    double env_color[3];
    int32_t env_tex;
    int32_t _pad;
} pt_camera;

typedef struct pt_render_opts {
    uint32_t slots_per_pixel;   /* resident paths per pixel; 0 = auto (fills the GPU; about one path per 30 samples of the
                                   frame, at most 1 M paths per CU: 134 M paths = 14 GB of device memory for 1920x1080 @
                                   4000 spp on an MI355X, 28 GB at most, kept by the scene until pt_scene_destroy); 1 = the reference's
                                   exact per-pixel sample order */
    uint32_t accum_on_device;   /* accum points to device memory (e.g. a torch tensor) */
    uint32_t profile;           /* time every kernel launch with HIP events */
    uint32_t overwrite;         /* 0: the frame's sums are ADDED to accum (sample ranges accumulate); 1: accum is overwritten */
    void* stream;               /* hipStream_t to launch on; NULL = the context's own stream */
} pt_render_opts;

typedef struct pt_render_stats {
    uint64_t samples, segments, iterations;
    uint32_t n_slots, slots_per_pixel;
    double ms_total;                       /* wall time inside pt_render (host clock, synced) */
    double ms_extend, ms_shade, ms_other;  /* HIP-event time per kernel family (profile=1) */
    uint64_t launches_extend, launches_shade;
    uint32_t extend_variant, shade_variant;   /* K2: 0 two-phase k_extend2, 1 batch k_extend; K3: sort*10 + min waves/SIMD */
    uint32_t blocks_extend, blocks_shade;
    uint32_t compactions;                  /* times the thinning pool was compacted at the frame's end (dynamic mode) */
    uint32_t n_alloc_end;                  /* slots the last launches still covered */
    /* the sky pass (pt_sky_tiles below): 8x8 pixel tiles rendered outside the path pool, their samples — the tiles' pixels inside
       the image x the samples per pixel, counted in `samples` and `segments` as well — and the HIP-event time of their kernel (profile=1).
       All zero when the pass is off. */
    /* the short-path pass (pt_short_tiles below): tiles whose camera rays can enter only boxes of shadeable entries, rendered
       ahead of the path pool as far as a sample's path is camera -> miss or camera -> one diffuse hit -> miss — short_samples, counted in
       `samples` and `segments` as well; the other samples of those tiles (hard_samples) are the path pool's; the HIP-event time of the pass's
       kernel (profile=1). All zero when the pass is off. (In front of the sky pass's fields, which stay the structure's last: a caller built
       against the header before these four must be rebuilt, the sky fields' offsets having moved by 32 bytes.)
       Device memory: the pass keeps a list sized for EVERY sample of the tiles it takes by proof (4 bytes each, 8 where tile, pixel and sample do not
       fit in 32 bits; the tiles taken by yield add what short_list_bytes says), capped at the bytes of the path pool's records — scene 6 at 1920x1080 @ 4000 spp: 7.9 GB beside a 27 GB pool; where the
       cap binds the pass takes fewer tiles. PT_EXPERIMENT=1 PT_SHORT_CAP_BYTES=n lowers the cap for a host with less memory. */
    /* the pass's yield pilot: on a sample range of 256 samples per pixel or more the pass first renders 8 samples of every tile
       of the path pool's, counting only, and takes the tiles it finishes half of as well. pilot_tiles: the tiles taken that way (counted in
       short_tiles too); short_fallback: 1 when the pass found more hard samples than its list held and ran again with the proven tiles alone
       (pilot_tiles is then 0); short_list_bytes: the bytes of the hard list — every sample of the proven tiles, and of the taken tiles 1.5
       times the pilot's projection and 64 entries per tile; short_pixels: the pixels of the short tiles that lie inside the image
       (short_samples + hard_samples = short_pixels x the samples per pixel); ms_pilot: the HIP-event time of the pilot's kernel (profile=1). */
    /* the pass's deferred miss proofs: a bounce ray that enters a mesh's box waits, with up to 63 others of its wave, for a
       pass in which every lane proves one ray's miss. short_walks: the rays that waited; short_walk_passes: the passes that walked them
       (their mean fill is short_walks / (64 x short_walk_passes)). Zero with PT_EXPERIMENT=1 PT_SHORT_DEFER=0. (In front of the pilot's
       fields: a caller built against the header before these two must be rebuilt.) */
    /* the pass's reach masks (pt_tile_reach below). short_direct_tiles: the tiles of the pass whose mask names one shadeable entry
       and nothing else, whose camera rays are tested against that primitive alone; short_self_prims: the shadeable quads a bounce that left them
       does not test again (the numbers of quad and camera keep the proof's bound). Under PT_EXPERIMENT=1: short_direct_tiles is zero with
       PT_SHORT_REACH=0 or PT_SHORT_DIRECT=0; short_self_prims is zero with PT_SHORT_SELF=0 (PT_SHORT_REACH=0 leaves it as it is). (In front of the deferred proofs' fields: a caller built against the header
       before these two must be rebuilt.) */
    /* K2's rounds: the two-phase kernel k_extend2 collects the rays of a window that enter mesh boxes in a list and walks the
       meshes in a second phase; a ray that finds the list full is walked where it was found, which is slow. k2_overflow_rays: those rays, over
       all launches. A full window whose first half has filled more than half of the list runs the second phase there and again at its end:
       k2_split_windows counts them. Under PT_EXPERIMENT=1, PT_K2_SPLIT=0 splits no window and PT_K2_SPLIT=2 runs the second phase after any
       chunk that leaves less than a chunk of room (k2_split_windows then counts those rounds); PT_K2_BLOCKS=n launches K2 on n blocks. Both zero
       for the batch kernel. (In front of the short pass's fields: a caller built against the header before these two must be rebuilt.) */
    uint64_t k2_split_windows, k2_overflow_rays;
    uint64_t short_direct_tiles, short_self_prims;
    uint64_t short_walks, short_walk_passes;
    uint64_t pilot_tiles, short_fallback, short_list_bytes, short_pixels;
    double ms_pilot;
    uint64_t short_tiles, short_samples, hard_samples;
    double ms_short;
    uint64_t sky_tiles, sky_samples;
    double ms_sky;
} pt_render_stats;

const char* pt_last_error(void);
int pt_set_error_message(const char* msg);   /* host layers above the ABI report through the same channel; returns -1 */
/* Fails (-1) when no HIP device is present: there is no host fallback. */
int pt_ctx_create(int device, pt_ctx** out);
void pt_ctx_destroy(pt_ctx*);
int pt_device_name(pt_ctx*, char* buf, uint32_t n);

pt_scene* pt_scene_create(pt_ctx*);
void pt_scene_destroy(pt_scene*);
pt_ctx* pt_scene_ctx(pt_scene*);

/* ---- textures: src/texture.rs ---------------------------------------------------------- */
int pt_tex_solid_rgb(pt_scene*, double r, double g, double b);          /* SolidTexture<Vec3> :11-25 */
int pt_tex_solid_f(pt_scene*, double v);                                /* SolidTexture<f64>       */
int pt_tex_checker(pt_scene*, double scale, int tex1, int tex2);        /* CheckerTexture::new :34-40 */
int pt_tex_image_rgb8(pt_scene*, uint32_t w, uint32_t h, const uint8_t* rgb);   /* ImageTexture (decoded, RGB8) :56-70 */
/* The float-HDR option: an ImageTexture that keeps the decoder's f32 samples instead of `.to_rgb8()`
 * (texture.rs:67) — same nearest-texel lookup (texture.rs:73-91), values not clamped to [0,1]. Usable wherever an image texture
 * is (colour, normal map, Camera::environment). pt_scene_set_float_hdr(scene, 1) makes the scene scripts (pt_build_scene) and the
 * host mirrors load Radiance .hdr files this way; the default (0) is the reference's RGB8 behaviour. */
int pt_tex_image_rgbf32(pt_scene*, uint32_t w, uint32_t h, const float* rgb);
int pt_scene_set_float_hdr(pt_scene*, int on);
int pt_scene_float_hdr(pt_scene*);
/* Environment importance sampling (no counterpart in the reference). Opt-in, a setting of the scene: f = the
 * mixture weight p_env, 0 <= f < 1 and finite (else -1); the default 0 is off. It is IN EFFECT for a render when f > 0, the
 * camera's environment is a map (env_is_map) and that map's weight Z (below) is finite and > 0. When it is not in effect every
 * render is the estimator of camera.rs:177-226 bit for bit; pt_render_aovs never uses it.
 *
 * Distribution, over the W x H texels of the environment texture (texel (i, j) = the one sample_environment reads: row j covers
 * theta in [j pi/H, (j+1) pi/H), column i covers phi in [-pi + 2 pi i/W, -pi + 2 pi (i+1)/W)):
 *   lum_ij = max(0, 0.2126 r + 0.7152 g + 0.0722 b) of the texel value as tex_image returns it (RGB8 * (1/255), or f32 widened;
 *            NaN -> 0), summed left to right;  c_j = cos(j pi / H) (the argument formed as (j * pi) / H);
 *   w_ij = (lum_ij * (c_j - c_{j+1})) * ((2 pi) / W);
 *   row j: P_j[0] = 0, P_j[i+1] = P_j[i] + w_ij for i = 0 .. W-1 in order, R_j = P_j[W];
 *   rows:  Q[0] = 0, Q[j+1] = Q[j] + R_j for j = 0 .. H-1 in order, Z = Q[H];
 *   env_pdf(d) = lum(texel(d)) / Z per steradian.
 * Sampling, draws u1 then u2 in [0, 1): x = u1 * Z (if x >= Z: the largest double below Z); j = the smallest row with x < Q[j+1];
 *   t1 = (x - Q[j]) / (Q[j+1] - Q[j]); cos_t = c_j - t1 * (c_j - c_{j+1}); y = u2 * R_j (same rule against R_j); i = the smallest
 *   column with y < P_j[i+1]; t2 = (y - P_j[i]) / (P_j[i+1] - P_j[i]); phi = -pi + ((2 pi) * (i + t2)) / W;
 *   sin_t = sqrt(max(0, 1 - cos_t^2)); d = (sin_t cos(phi), cos_t, sin_t sin(phi)); its pdf = lum_ij / Z. Zero-weight rows and
 *   texels are never chosen.
 * Estimator, at every surface bounce after Russian roulette whose material is in the env set E: one selector draw r;
 *   p_env = f, p_light = lights ? (1 - f) / 2 : 0, p_bsdf = 1 - p_light - p_env; r < p_light: lights.sample, r < p_light + p_env:
 *   an env sample (two more draws), else mat.sample. q_env(d) = env_pdf(d) if d lies on the positive side of the material's local
 *   frame (z > 0 after make_local_frame's rotation), else 0; an env direction with q_env = 0 ends the path.
 *   pdf = p_bsdf * s_b + p_light * light_pdf + p_env * q_env(d), throughput *= eval * k / pdf, where s_b is the BSDF sampler's
 *   density and k = (today's density / today's pdf) at d: diffuse: s_b = its pdf, k = 1; metal (its sampler draws GGX visible
 *   normals with alpha = roughness^2 while its pdf uses alpha = roughness): s_b = G1_s(v) D_s(h) / (4 v.z) with alpha_s =
 *   roughness^2 for l.z > 0 (0 below), k = (p0_bsdf s_b + p0_light light_pdf) / (p0_bsdf bsdf_pdf + p0_light light_pdf) with
 *   today's weights p0 (0.5 / 0.5 with lights, else 1 / 0). So the expectation is today's wherever light_pdf is the light
 *   sampler's density. A bounce whose pdf is 0 (or metal's today-pdf is 0), or whose new throughput is exactly (0, 0, 0), ends
 *   the path.
 *   E = diffuse, and metal with roughness >= 0.05 seen from the front of its frame (v.z > 0). Every other hit (glass, lights,
 *   principled, sheen, clearcoat, mixes, near-mirror metal) bounces exactly as today. */
int pt_scene_set_env_sampling(pt_scene*, double f);
double pt_scene_env_sampling(pt_scene*);
/* The sampler: where a path's random numbers come from. kind 0 (default) = independent draws, the reference's thread_rng stand-in:
 * draw d of sample s of pixel p is half of Philox4x32-10(counter = (d >> 1, s, seed_hi, 0), key = (seed_lo, p)); every entry point
 * is then the code it was before this setting existed, bit for bit. kind 1 = an Owen-scrambled Sobol (0,2)-sequence per pixel and
 * per pair of draws, padded across pairs by independent keys (hash-based Owen scrambling: Burley 2020, Laine-Karras hash). Any
 * other kind returns -1 and leaves the setting. In effect for pt_render, pt_render_pixels, pt_render_adaptive, pt_render_multi
 * and pt_render_aovs (whose camera ray stays the one pt_render traces for (pixel, s)). The sample index is the global one, so
 * sample ranges, pixel lists, adaptive rounds, the denoiser's halves and multi-GPU shards stay pieces of one sequence — and
 * renders of DIFFERENT ranges of one seed are stratified against each other, not independent: independent estimates need
 * different seeds. The rule of kind 1, all arithmetic on uint32 (wrapping):
 *   rev(x)     = the 32 bits of x in reverse order
 *   lk(x, k)   : x += k; x ^= x * 0x6c50b47c; x ^= x * 0xb82f1e52; x ^= x * 0xc7afe638; x ^= x * 0x8d22f6e6
 *   owen(x, k) = rev(lk(rev(x), k))
 *   sobol0(i)  = rev(i);   sobol1(i) = rev(y), y = i; y ^= (y & 0xAAAAAAAA) >> 1; y ^= (y & 0xCCCCCCCC) >> 2;
 *                y ^= (y & 0xF0F0F0F0) >> 4; y ^= (y & 0xFF00FF00) >> 8; y ^= (y & 0xFFFF0000) >> 16   (Sobol's second dimension)
 *   draw d: pair k = d >> 1, component c = d & 1;  K[0..3] = Philox4x32-10(counter = (k, 0, seed_hi, 1), key = (seed_lo, p))
 *   j = owen(s, K[0]);  x = owen(c == 0 ? sobol0(j) : sobol1(j), K[1 + c]);  value = (uint64(x) << 32) | lk(x, K[3] + c)
 * The 64-bit value is consumed exactly where the Philox value is (the same conversions to f64, ranges and indices, the same
 * draws made and not used), at every draw of a path — there is no depth beyond which the sampler falls back to independent
 * draws. One addition, kind 1 only: a two-value draw (the pixel offsets, the lens offsets, the environment sample, the two
 * numbers of a BSDF direction or of a point on a quad light) first advances the draw index to the next even one, so that
 * its two coordinates are the two components of one pair; the draw indices of a Sobol path therefore differ from those of an
 * independent one. The 2^m points of a pair for samples [a 2^m, (a+1) 2^m) put one point into every elementary interval
 * 2^-q x 2^-(m-q). */
int pt_scene_set_sampler(pt_scene*, int kind);
int pt_scene_sampler(pt_scene*);
/* Light sampling: how lights.sample / lights.pdf treat the mesh and sphere entries of the lights list. kind 0 (default) = the
 * reference's (mesh.rs:122-141, sphere.rs:110-135: a uniformly chosen triangle with u, v drawn in the unit square, the whole sphere
 * surface; O(n) triangle tests per pdf); kind 1 = exact; any other kind returns -1 and leaves the setting. Changing it needs no
 * pt_world_build. Kind 1 is IN EFFECT for a render when kind == 1 and the lights list holds at least one mesh or sphere entry,
 * directly or under instances; otherwise every entry point launches exactly the kernels it launches without the setting and
 * produces the same bits. In effect for pt_render, pt_render_pixels, pt_render_adaptive and pt_render_multi; pt_render_aovs does
 * not change. With kind 1 in effect a render returns -1 when environment importance sampling or participating media are in effect
 * too, when a light mesh's area A is 0 or not finite, or when a light mesh's BVH is deeper than 24 levels. The rule of kind 1:
 *   The light-index draw (gen_range(0..n_lights)) and the instance chain (origin, and for the pdf the direction, into the entry's
 *   local space, the sampled direction back out) are made exactly as with kind 0; quad and cuboid entries keep kind 0's rule.
 *   Mesh entry of n faces in pt_mesh's face order, vertices v0, v1, v2 in the mesh's local space (instance chains are rigid, so one
 *   table serves every placement). Table, built by pt_world_build for every mesh in the lights list: c_i = cross(v1 - v0, v2 - v0),
 *   A_i = 0.5 * length(c_i), C[0] = 0, C[i+1] = C[i] + A_i summed in order in f64, A = C[n].
 *     sample: one single draw u0, x = u0 * A (if x >= A: the largest double below A); face j = the smallest j with x < C[j+1] (a
 *       zero-area face is never chosen); one two-value draw (u1, u2) (pair-aligned under the Sobol sampler); s = sqrt(u1),
 *       b0 = 1 - s, b1 = s * (1 - u2), b2 = s * u2; point = v0 * b0 + v1 * b1 + v2 * b2 (left to right); dir = normalize(point - origin).
 *     pdf: r = Ray::new(origin, direction, time) in local space; over EVERY face f that the triangle test of mesh.rs:50-82 accepts
 *       with t_min = 0, at distance t: term = (t * t) / (|dot(r.d, normalize(c_f))| * A) — the geometric normal; the entry's pdf is
 *       the sum of the terms, in the order the mesh's BVH yields them (two trees agree to rounding). All hits count, not only the
 *       first: a direction towards any point of the mesh has that density whether the point is occluded or not.
 *   Sphere entry, centre c at `time`, radius r: L = c - origin, d2 = length_squared(L), r2 = r * r; one two-value draw (u1, u2).
 *     d2 <= r2 (origin inside or on the sphere): cos_t = 1 - 2 u1, sin_t = sqrt(max(0, 1 - cos_t^2)), phi = (2 pi) u2,
 *       dir = (sin_t cos phi, sin_t sin phi, cos_t); pdf = 1 / (4 pi) for every direction.
 *     d2 > r2: x = r2 / d2, cm = sqrt(1 - x), k = x / (1 + cm) (= 1 - cm without the cancellation); cos_t = 1 - u1 * k, sin_t and
 *       phi as above; dir = that vector rotated from +z onto normalize(L) (the shortest-arc frame the medium's phase sampling uses);
 *       pdf = 1 / ((2 pi) * k) when the sphere test of sphere.rs:64-87 accepts Ray::new(origin, direction, time) with t_min = 0, else 0.
 *   lights.pdf averages the entries' pdfs over the list as with kind 0. */
int pt_scene_set_light_sampling(pt_scene*, int kind);
int pt_scene_light_sampling(pt_scene*);
/* The projection: how a (pixel, sample) becomes a camera ray. kind 0 (default) = perspective, the reference's pinhole / thin-lens camera
 * (camera.rs:153-168): every entry point is then the code it was before this setting existed, bit for bit. 1 = orthographic, 2 = fisheye
 * (equidistant), 3 = panorama (equirectangular lat-long); any other kind returns -1 and leaves the setting. Changing it needs no
 * pt_world_build. In effect for pt_render, pt_render_pixels, pt_render_adaptive, pt_render_multi and pt_render_aovs (and so for the
 * denoiser's features), in every shading mode, under both samplers, in static and dynamic pools. pt_camera and pt_camera_init do not
 * change. The rule. forward, right, up, pixel00, pixel_du, pixel_dv, center are pt_camera_init's; W, H the image size; F = focal_length;
 * dof_right, dof_up = right, up times the lens radius tan((defocus_angle / 2) * (PI / 180)) * F. f64, one IEEE rounding per written
 * operation; (sin, cos) are the deterministic ones of the kernels (pt_math_probe which 3 / 4).
 *   Every kind makes exactly the draws kind 0 makes, in its order: the two-value pixel draw (u0, u1): radius = sqrt(u0), angle =
 *   u1 * 2 * PI, bx = (radius * cos(angle)) * blur_strength, by = (radius * sin(angle)) * blur_strength; the two-value lens draw, the
 *   same way without the factor: (px, py), made and not used when the lens radius is zero; the time draw (made by index only when
 *   nothing in the scene moves). So draw indices, the Sobol sampler's pair alignment and dispersion's wavelength stream do not move.
 *   fy = row + bx, fx = col + by: continuous pixel coordinates, integer at a pixel centre (bx belongs to rows, as in the reference).
 *   1 orthographic: S = pixel00 + pixel_dv * fy + pixel_du * fx (kind 0's sample location); O = S + forward * F, a point of the plane
 *     through center; with a non-zero lens O = (O + dof_right * px) + dof_up * py; ray = Ray::new(O, S - O, time). The camera frames the
 *     rectangle kind 0 sees on its focal plane: an object at distance F keeps its size, the focal plane is sharp, defocus works as in kind 0.
 *   2 fisheye: vfov is the full angle across the image HEIGHT. xn = (2 * (fx + 0.5) - W) / H, yn = (H - 2 * (fy + 0.5)) / H,
 *     rho = sqrt(xn * xn + yn * yn); theta = fmin(rho * th, PI), th = (vfov * (PI / 180)) / 2 formed on the host; a = rho > 0 ?
 *     sin(theta) / rho : 0; w = (right * (xn * a) + up * (yn * a)) - forward * cos(theta); ray = Ray::new(center, w, time).
 *   3 panorama, in WORLD axes (look_at, vup and vfov must be valid for pt_camera_init and are otherwise not read; only look_from
 *     matters): phi = -PI + ((2 * PI) * (fx + 0.5)) / W; theta = fmin(fmax((PI * (fy + 0.5)) / H, 0), PI);
 *     w = (sin(theta) * cos(phi), cos(theta), sin(theta) * sin(phi)); ray = Ray::new(center, w, time). This is the direction
 *     convention of the environment lookup (camera.rs:140-151) and of pt_scene_set_env_sampling's table: pixel (i, j) looks along the
 *     centre of texel (i, j) of an environment map of the same size, so the image IS an environment map of the scene around look_from,
 *     at any aspect ratio.
 * A render (and pt_render_aovs, pt_camera_probe) returns -1, writing nothing: kinds 2 and 3 with defocus_angle != 0 (a lens disc has no
 * natural plane there); kind 2 when vfov is not finite or not > 0, or when sqrt((W / H)^2 + 1) * th > PI: the image circle must cover
 * the frame, so that no sample is without a ray. Jitter beyond the frame is covered by the clamps. */
int pt_scene_set_projection(pt_scene*, int kind);
int pt_scene_projection(pt_scene*);
/* ---- materials: src/bsdf/, src/material.rs ---------------------------------------------- */
int pt_mat_diffuse(pt_scene*, int color_tex, int normal_map_tex);       /* DiffuseBRDF::{new,from_rgb,from_textures} diffuse.rs:21-47; -1 = no map */
int pt_mat_metal(pt_scene*, int color_tex, int rough_tex);              /* MetalBRDF::new metal.rs:23-35 */
int pt_mat_glass(pt_scene*, int color_tex, int rough_tex, double anisotropic, double ior);   /* GlassBSDF::new glass.rs:28-40 */
int pt_mat_principled(pt_scene*, int color_tex, const double params[11]);   /* PrincipledBSDF::new principled.rs:45-73, same argument order */
int pt_mat_light(pt_scene*, int emission_tex);                          /* DiffuseLight::new material.rs:155-164 */
/* ---- homogeneous participating media: fog, smoke (the reference's commented-out volume.rs `HomogeneousVolume`) ----
 * A medium is a material. density = sigma_t, finite and > 0; (r, g, b) = the single-scattering albedo sigma_s / sigma_t, each in
 * [0, 1]; hg_g = the Henyey-Greenstein asymmetry, |hg_g| < 1 (0 = isotropic). Anything else returns -1, and so does a handle that
 * would reach 4094 (a path keeps its medium in 12 bits: create media early in scenes with thousands of materials). Any closed object
 * (sphere, cuboid, mesh, an instance of these) may carry it: its surface is then the medium's BOUNDARY — invisible — and the medium
 * fills its inside. A medium inside pt_mat_mix and a medium object in the lights list are refused (-1).
 * pt_scene_set_camera_medium: the medium camera rays start in — the camera inside a fog box, or an unbounded fog when no boundary
 * carries that material; -1 (default) = none; a handle that is not a medium returns -1 and leaves the setting.
 * Media are IN EFFECT for a render when some world object's material is a medium or the camera medium is set; otherwise every
 * entry point runs exactly the kernels it ran before media existed (a medium material nothing uses does not count).
 * Not supported: nested or overlapping media (leaving ANY boundary puts the path into "no medium"), boundaries that touch or lie
 * within 2e-3 of each other, chromatic density (chromatic absorption: pt_mat_medium_tinted), textured albedo, emission from media;
 * a transmissive object inside a medium is treated as filled by it (a glass object with a medium of its own: pt_mat_glass_set_interior). Environment importance sampling together with media in effect: the render returns -1. max_depth must
 * be below 2^20 then.
 *
 * The estimator: analog tracking with the reference's one-sample MIS. Each path carries m, a medium or none; a camera ray starts with
 * m = the camera medium. Whenever K3 visits a live path whose segment is resolved (a hit at distance t = HitInfo::dist, or a miss,
 * t = +inf), with o, dir the segment's ray:
 *  1 Free flight, only if m is set: one draw u in [0, 1) (converted like every unit draw: (v >> 11) * 2^-53);
 *    d = -log(1 - u) / density with the deterministic log of pt_detmath.h. d < t: a MEDIUM VERTEX at x = o + d * dir (step 2). Else
 *    the surface hit or miss is processed unweighted (step 3 or 4): transmittance and free-flight density cancel.
 *    One exception, before the draw: a MISS while m is a medium that some world object bounds. A boundary is closed, so such a
 *    ray is not inside m: the path lost a crossing — an exit closer than the 1e-3 of K2's t_min to an offset entry point, which
 *    happens at the edges of cuboids and meshes — and would scatter for ever outside. m becomes none, no draw is made, and the
 *    miss is processed (step 4). Until its ray leaves the scene such a path carries the wrong medium; about 1 crossing in 10^4.
 *  2 Medium vertex. No emission. Russian roulette exactly as at a surface (bounce > 5: p = clamp(luminance(thr), 0.01, 1), one draw,
 *    end if draw > p, else thr /= p). Then the selector draw (camera.rs:199-201; made even without lights). Below p_light (0.5 with a
 *    lights list, else 0): w = lights.sample(x). Otherwise a two-value draw (u1, u2) (pair-aligned under the Sobol sampler):
 *      cos_t = 1 - 2 u1 when |g| < 1e-3, else (1 + g^2 - ((1 - g^2) / (1 - g + 2 g u1))^2) / (2 g); clamped to [-1, 1];
 *      sin_t = sqrt(max(0, 1 - cos_t^2)); phi = (2 pi) u2; w = the local vector (sin_t cos phi, sin_t sin phi, cos_t) taken to the
 *      world by the shading frame built around dir (the shortest-arc quaternion of vec3.rs:23-29): g > 0 scatters forward.
 *    ph(c) = (1 - g^2) / (4 pi s sqrt(s)), s = 1 + g^2 - 2 g c, c = dot(dir, w). pdf = p_bsdf ph + p_light lights.pdf(x, w).
 *    A zero or non-finite pdf ends the path. thr *= albedo * ph / pdf. The new ray starts at x (no offset) along w (normalised as
 *    Ray::new does). m is unchanged. ++bounce; the depth bound applies as at a surface.
 *  3 Boundary hit (the surface's material is a medium k): no draw, no roulette, no emission, no change of throughput.
 *    m = (m == k) ? none : k — a toggle, independent of face orientation, so cuboid faces and meshes of either winding work. The
 *    ray continues with the same direction from point + 1e-3 * signum(dot(dir, gn)) * gn (the offset camera.rs:217-222 applies to
 *    every continued ray). ++bounce, and the depth bound applies: counting a crossing as a bounce guarantees termination, needs no
 *    extra state, and is what a glass surface of ior 1 would cost.
 *  4 Any other surface hit, or a miss: exactly the code without media. m is kept.
 * A miss inside an unbounded medium is only reached through d >= +inf, i.e. never: such a path scatters until roulette or the
 * depth bound ends it. pt_render_aovs and pt_intersect see a boundary as an ordinary first hit (albedo (1, 1, 1)). */
int pt_mat_medium(pt_scene*, double density, double r, double g, double b, double hg_g);
/* ---- grid-density participating media: smoke plumes, clouds, uneven haze (no counterpart in the reference) ----
 * A medium whose extinction varies in space: sigma(x) = scale * V(x), V the trilinear interpolation of a 3-D grid of f32 samples.
 * The handle is a medium material like pt_mat_medium's and works wherever that one does: carried by a closed object (its boundary),
 * or set with pt_scene_set_camera_medium — then, with no boundary object, an unbounded medium that is empty outside the grid's box.
 * Every refusal of pt_mat_medium applies (handle limit 4094, no mix child, no lights list); (r, g, b) and hg_g as there.
 * values[(k * ny + j) * nx + i] is the sample at the centre of cell (i, j, k) of the world-space axis-aligned box [box_lo, box_hi];
 * the values are copied. Returns -1, creating nothing, when: scale is not finite or not > 0; a value is negative or not finite; all
 * values are 0; some n_a < 2; nx * ny * nz > 2^28; box_lo[a] >= box_hi[a] or a box coordinate is not finite; the albedo or hg_g is
 * outside pt_mat_medium's ranges; or the majorant optical diagonal scale * max(values) * |box_hi - box_lo| exceeds 4096 — a design
 * limit that bounds the expected trip count of the longest tracking loop a lane can run (a medium that thick is opaque: model it as
 * a surface).
 * Grid media are IN EFFECT for a render when some world object's material is one or the camera medium is one; otherwise every
 * render runs exactly the kernels it ran before they existed, and a homogeneous medium keeps pt_mat_medium's rule and bits either way.
 * Not supported, besides pt_mat_medium's list, which carries over unchanged: a grid that follows an instance's transform or a moving
 * sphere — the grid is fixed in world space whatever carries the medium.
 *
 * Density, all in f64. For x outside the box (any x_a < lo_a or x_a > hi_a; a NaN coordinate counts as outside): sigma(x) = 0.
 * Inside, per axis a with c_a = (double)n_a / (hi_a - lo_a):  q_a = (x_a - lo_a) * c_a - 0.5, clamped to [0, n_a - 1];
 * i_a = min(floor(q_a), n_a - 2); f_a = q_a - i_a. With v_xyz the sample at (i_x + x, i_y + y, i_z + z) widened to f64, every blend
 * written as lerp(a, b, f) = a + f * (b - a):  x pairs first: c_yz = lerp(v_0yz, v_1yz, f_x); then y: c_z = lerp(c_0z, c_1z, f_y);
 * then z: V = lerp(c_0, c_1, f_z).  sigma(x) = scale * V.  The majorant is mu = scale * (double)max(values).
 *
 * Estimator: step 1 of pt_mat_medium's rule when m is a grid medium; steps 2-4, the "miss while m is bounded" exception before any
 * draw, the boundary toggle and roulette are unchanged. With o, dir, t the resolved segment (t = +inf on a miss):
 *   Clip to the box by the slab test: start from near = 0, far = t. Per axis with dir_a != 0: inv = 1 / dir_a, ta = (lo_a - o_a) * inv,
 *   tb = (hi_a - o_a) * inv; near = max(near, min(ta, tb)), far = min(far, max(ta, tb)). An axis with dir_a == 0 changes nothing when
 *   lo_a <= o_a <= hi_a and empties the interval otherwise. [t0, t1] = [near, far]. Unless t0 < t1 and t1 is finite — and always when
 *   a component of o or dir is not finite — no draw is made and the surface or miss is processed.
 *   Otherwise s = t0 and repeat: a single draw u, s += -log(1 - u) / mu (the deterministic log); if s >= t1 there is no collision:
 *   the surface or miss is processed unweighted; else a single draw v: if v * mu < sigma(o + s * dir), a MEDIUM VERTEX at o + s * dir
 *   (step 2, with the medium's albedo and g); else continue.
 * Both draws are single draws (not pair-aligned under the Sobol sampler). A miss inside an UNBOUNDED grid medium is reachable: the
 * ray leaves the box without a collision and the environment is added. pt_render_aovs and pt_intersect do not change. */
int pt_mat_medium_grid(pt_scene*, double scale, double r, double g, double b, double hg_g, uint32_t nx, uint32_t ny, uint32_t nz, const float* values,
                       const double box_lo[3], const double box_hi[3]);
int pt_scene_set_camera_medium(pt_scene*, int mat);
int pt_scene_camera_medium(pt_scene*);
/* ---- interior media and chromatic absorption: coloured glass, whisky, tea, milk, wax, jade (no counterpart in the reference, whose
 * GlassBSDF::eval ignores base_color) ----
 * pt_mat_medium_tinted: a homogeneous medium like pt_mat_medium's with an extra absorption coefficient per channel. density >= 0 and
 * finite (0 = no scattering, pure absorption; pt_mat_medium itself goes on refusing 0); albedo and hg_g as in pt_mat_medium, also when
 * density is 0; each absorption[c] finite and >= 0; density + max(absorption) > 0. pt_mat_medium's handle limit (4094) and its mix and
 * lights refusals apply. A refused call returns -1 and creates nothing. There is no tinted grid medium.
 * pt_mat_glass_set_interior: the medium that fills objects of glass material glass_mat: medium_mat = any medium handle (homogeneous,
 * tinted or grid), or -1 to detach. Returns -1 and leaves the setting when glass_mat is not a pt_mat_glass handle, when medium_mat is
 * neither a medium nor -1, or when the glass is a child of a mix; pt_mat_mix with a child that has an interior returns -1. The world
 * must be (re)built after the call. pt_mat_glass_interior: the medium handle, or -1.
 * Media are IN EFFECT for a render (pt_mat_medium) also when a world object's material is a glass whose interior is set. The code of
 * this section runs only when some world object's glass has an interior, or a tinted medium is the material of a world object or the
 * camera medium; otherwise every render launches exactly the kernels it launched before and produces the same bits (a tinted medium
 * nothing uses, or an interior set and detached again, does not count). An interior medium is bounded — an object carries it — so
 * step 1's exception applies to it unchanged: a miss while inside resets the medium. pt_scene_set_camera_medium(interior) puts the
 * camera inside such a body.
 *
 * The rule: additions to pt_mat_medium's steps. No step makes a new draw; draw indices and Sobol pair alignment do not move.
 *  Absorption, in step 1, before anything else at this visit uses the throughput. At the start of the visit m is a tinted medium with
 *    coefficients a_c; l is the distance travelled on this segment: d at a medium vertex, otherwise t, +inf on a miss (traced rays are
 *    unit length). For each channel with a_c > 0: thr_c *= exp(-(a_c * l)), with the deterministic exp of pt_detmath.h and the product
 *    formed first; a channel with a_c == 0 is not touched (no 0 * inf). So the emission of a light hit inside the medium, the
 *    environment on a miss and the roulette probability are attenuated. When density == 0, step 1 makes no draw and d = +inf; a miss
 *    inside an unbounded density-0 medium is reachable and its absorbed channels arrive as exactly 0. The lost-crossing reset (a miss
 *    while m is bounded: m becomes none) happens first, and that segment is not attenuated.
 *  Interior, in step 4, at a surface hit whose own material is a glass with interior k. The hit is processed exactly as without one
 *    (roulette, selector, light or BSDF direction, eval / pdf, the offset e = 1e-3 * signum(dot(dir, gn))), with one addition: the
 *    bounce CROSSED the surface when signum(dot(dir, gn)) is not NaN and equals signum(dot(ray.d, gn)) — the continued ray starts on
 *    the side the incoming ray was heading to. That covers refraction, and a lights-list direction that happens to go through. On a
 *    crossing at a front-face hit (HitInfo::front_face, which glass uses for eta): m = k; at a back-face hit: m = none. Without a
 *    crossing (reflection outside, internal reflection inside) m is kept. Front face, not step 3's toggle: glass needs correct
 *    winding for its eta anyway, and the state heals itself at the next crossing after a lost one.
 *  The free flight and the absorption inside the body are step 1 of the next visit, unchanged.
 * Not supported, besides pt_mat_medium's list: a glass with an interior that stands inside another medium (entering forgets the outer
 * medium, leaving gives "no medium"); hollow or nested glass shells; interiors on principled or mix materials; a grid interior that
 * moves with an instance (as for pt_mat_medium_grid). pt_render_aovs does not change: glass stays albedo (1, 1, 1). */
int pt_mat_medium_tinted(pt_scene*, double density, double r, double g, double b, double hg_g, const double absorption[3]);
int pt_mat_glass_set_interior(pt_scene*, int glass_mat, int medium_mat);
int pt_mat_glass_interior(pt_scene*, int glass_mat);
/* ---- spectral dispersion of glass: prisms, diamonds, the coloured rim of a lens (no counterpart in the reference, whose glass has one
 * index of refraction for all light) ----
 * pt_mat_glass_set_dispersion: the ior given to pt_mat_glass is read as n_d, the index at lambda_d = 587.56 nm; abbe is the Abbe number
 * V_d = (n_d - 1) / (n_F - n_C), lambda_F = 486.13 nm, lambda_C = 656.27 nm; 0 = off (the default). Two-term Cauchy, wavelengths in um,
 * all f64, the operations in the order written:
 *   inv2(l) = 1.0 / (l * l);  b = (n_d - 1) / (abbe * (inv2(0.48613) - inv2(0.65627)));
 *   n(lambda) = n_d + b * (inv2(lambda_nm * 1e-3) - inv2(0.58756))      (the host computes b and inv2(0.58756), the device the rest)
 * Returns -1 and leaves the setting when glass_mat is not a pt_mat_glass handle, when abbe is negative or not finite, when abbe > 0 and
 * n(380) or n(730) is not finite or is <= 1, or when the glass is a child of a mix; pt_mat_mix with a dispersive child returns -1. The
 * world must be (re)built after the call. pt_mat_glass_dispersion: V_d, 0 when off, -1 on a bad handle.
 * Dispersion is IN EFFECT for a render when some world object's own material is a glass with abbe > 0; otherwise every entry point
 * launches exactly the kernels it launches without this setting and produces the same bits (a dispersive glass nothing uses, or a
 * dispersion set and cleared again, does not count). In effect for pt_render, pt_render_pixels, pt_render_adaptive and pt_render_multi;
 * pt_render_aovs and pt_intersect do not change. With dispersion in effect a render returns -1 when environment importance sampling,
 * participating media (a glass interior among them) or exact light sampling are in effect too, or when max_depth >= 2^31.
 *
 * The wavelength of a path is a function of (seed, pixel, global sample index s) alone — no draw of the path's own stream is made; draw
 * indices and Sobol pair alignment do not move:
 *   sampler kind 0: K = Philox4x32-10(counter = (0, s, seed_hi, 2), key = (seed_lo, pixel));  v = (uint64(K[0]) << 32) | K[1]
 *   sampler kind 1: K = Philox4x32-10(counter = (0, 0, seed_hi, 2), key = (seed_lo, pixel));  x = owen(sobol0(s), K[0]);
 *                   v = (uint64(x) << 32) | lk(x, K[1])   (owen, sobol0, lk: pt_scene_set_sampler's rule) — so the 2^m samples of an
 *                   aligned block of one pixel put one wavelength into every stratum of width 2^-m
 *   (counter word 3 = 2 is a stream of its own: 0 and 1 are the two samplers')
 *   u = (v >> 11) * 2^-53;  lambda = 380 + u * 350 (nm);  bin j = min(floor(u * 64), 63)
 * The weight table W[64][3], the same for every scene, built on the host in f64. At the centre of bin j, l_j = 380 + (j + 0.5) * (350 / 64),
 * with the piecewise Gaussian g(l; mu, s1, s2) = exp(-0.5 * ((l - mu) / s)^2), s = s1 for l < mu, else s2:
 *   x = 1.056 g(599.8, 37.9, 31.0) + 0.362 g(442.0, 16.0, 26.7) - 0.065 g(501.1, 20.4, 26.2)
 *   y = 0.821 g(568.8, 46.9, 40.5) + 0.286 g(530.9, 16.3, 31.1)
 *   z = 1.217 g(437.0, 11.8, 36.0) + 0.681 g(459.0, 26.0, 13.8)
 *   r =  3.2404542 x - 1.5371385 y - 0.4985314 z;  g = -0.9692660 x + 1.8760108 y + 0.0415560 z;  b = 0.0556434 x - 0.2040259 y + 1.0572252 z
 *   raw_c(j) = max(0, .);  W[j][c] = raw_c(j) * 64 / (sum of raw_c(k), k = 0 .. 63 in order) — the mean of every channel over the bins is 1.
 * (The numbers follow the multi-lobe fit of Wyman, Sloan and Shirley 2013 to the CIE 1931 observer and the XYZ -> linear sRGB matrix;
 * this text defines them.)
 * The estimator: one addition to the surface bounce. Every path carries one flag, MONO, clear on a camera ray. At a surface hit whose
 * own material is a glass with abbe > 0 the bounce is processed exactly as without dispersion (roulette, selector, light or BSDF
 * direction, pdf, eval, offset) except that every read of the glass's ior at this bounce — eta_i / eta_o in sample, pdf and eval — takes
 * n(lambda) of the path's wavelength. If the bounce continues the path and MONO is clear: MONO is set and the new throughput is
 * (thr * attenuation) * W[j], componentwise, in that order. A path whose MONO is set is not weighted again. Every other hit, every miss,
 * roulette, emission and the environment are unchanged; the principled material's glass lobe is not dispersive. With all V_d -> infinity
 * the expectation is the one without dispersion: lambda is independent of everything the path does before its first dispersive visit and
 * the mean of W is (1, 1, 1).
 * Not supported: dispersion together with an interior, with media, environment sampling or exact light sampling; dispersive principled or
 * mix materials; wavelength-dependent emission or textures; more than the two Cauchy terms. */
int pt_mat_glass_set_dispersion(pt_scene*, int glass_mat, double abbe);
double pt_mat_glass_dispersion(pt_scene*, int glass_mat);
/* the three bsdf/ materials no reference scene instantiates */
int pt_mat_mix(pt_scene*, double t, int mat1, int mat2);                /* MixBxDf::new mix.rs:14-20; a child may itself be a mix of non-mix materials (two levels) */
int pt_mat_sheen(pt_scene*, double r, double g, double b, double sheen_tint);   /* SheenBRDF::new sheen.rs:17-22 */
int pt_mat_clearcoat(pt_scene*, double clearcoat_gloss);                /* ClearcoatBRDF::new clearcoat.rs:14-18 */
/* ---- geometry: src/hittable/ ------------------------------------------------------------ */
int pt_sphere(pt_scene*, double radius, const double p1[3], const double p2[3], int mat);   /* Sphere::new_still/new_moving sphere.rs:22-46 */
int pt_quad(pt_scene*, const double q[3], const double u[3], const double v[3], int mat);   /* Quad::new quad.rs:17-36 */
int pt_cuboid(pt_scene*, const double a[3], const double b[3], int mat);                    /* Cuboid::new cuboid.rs:11-58 */
/* TriangleMesh::from_obj mesh.rs:149-197: f32 positions (and optional normals / texcoords,
 * all indexed by the position index as the reference does) + u32 index triples. */
int pt_mesh(pt_scene*, double scale, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
            uint32_t n_nrm, const float* nrm, uint32_t n_uv, const float* uv, int mat);
int pt_instance(pt_scene*, int obj, const double axis[3], double angle, const double translation[3]);   /* Instance::new instance.rs:20-30 */
/* ---- motion blur of instances: keyframed poses and a camera shutter (not in the reference, opt-in) ----
 * A ray's `time` is drawn per sample (camera.rs:165) and the reference reads it only in Sphere::center. pt_instance_moving makes an
 * Instance whose pose depends on it, so that a quad, a cuboid, a mesh or a light under it blurs like a moving sphere does.
 * The pose at `time`. Keys: axis, angle0, angle1, tr0, tr1. da = angle1 - angle0 and dtr = tr1 - tr0 (componentwise) are formed once on
 *   the host. angle = angle0 + da * time; tr = tr0 + dtr * time, componentwise. The forward matrix and its analytic inverse are then built
 *   by exactly pt_instance's operation sequence: (sn, cs) = the deterministic sincos(angle * 0.5) (pt_math_probe which 3 / 4), v = axis * sn,
 *   q = (v, cs), x2 = qx + qx .. wz = qw * z2, c0 = (1 - (yy + zz), xy + wz, xz - wy), c1 = (xy - wz, 1 - (xx + zz), yz + wx),
 *   c2 = (xz + wy, yz - wx, 1 - (xx + yy)), t = tr; i* = the transposed columns, it = -(i0 * t.x, then i1 * t.y + that, then i2 * t.z + that).
 *   So a moving instance at time t is, bit for bit, pt_instance(obj, axis, angle, tr) of those two lerped values. An instance with
 *   angle0 == angle1 ("translates only") keeps the rotation columns of angle0 + da * 0 and recomputes only t and it. Every level of a
 *   chain uses the ray's one time; moving and static instances nest in any order.
 * The shutter. pt_scene_set_shutter(scene, open, close), 0 <= open <= close <= 1, both finite; the default is (0, 1). Where motion is in
 *   effect a camera ray's time is open + (close - open) * u, u the value generate_ray draws today (the number and order of draws are
 *   unchanged); with (0, 1) those are u's bits, open == close freezes the scene at that instant. The shutter scales moving spheres too.
 * In effect (pt_scene_motion, after pt_world_build): some placed object's chain holds an instance made by pt_instance_moving, even one
 *   whose two keys are equal, or the shutter is not (0, 1) and something in the scene moves. Otherwise no new code runs.
 * Boxes. The world box of a placement covers every time in [0, 1]. A level that translates only: the union of the transformed box at
 *   time 0 and at time 1 (exact: the box is linear in time). A level that spins: rho = the largest corner norm of the child box, the union
 *   of tr(0) +- rho and tr(1) +- rho (rho widened by 1e-14 relative and the box by four ulps of its largest coordinate, for rounding).
 *   Levels above transform that box as they do a static one. (A mesh under ONE instance that translates only gets the bounds of its
 *   transformed vertices at times 0 and 1, as a mesh under a static instance gets those of its transformed vertices.)
 * Limits. With motion in effect a render returns -1 when environment importance sampling, any participating or interior medium, exact
 *   light sampling or dispersion is in effect too. A moving instance in the lights list is allowed under light-sampling kind 0: its
 *   sample / pdf (instance.rs:64-75) use the pose at the path's time. pt_intersect and pt_light_probe take the ray's time as given, with no
 *   shutter, and are defined for time in [0, 1] (pt_light_probe under kind 1 returns -1 when an instance moves, as a render does);
 *   pt_camera_probe and pt_render_aovs apply the shutter when motion is in effect. */
int pt_instance_moving(pt_scene*, int obj, const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3]);
int pt_scene_set_shutter(pt_scene*, double open, double close);
int pt_scene_shutter(pt_scene*, double out[2]);
int pt_scene_motion(pt_scene*);         /* 1: motion is in effect, 0: not, -1: the world is not built */
/* Host only, no context needed. pt_motion_pose: the InstD numbers of the pose at `time` (c0, c1, c2, t, i0, i1, i2, it: 24 doubles).
 * pt_motion_swept_box: one level of the box rule for box = (lo.xyz, hi.xyz). */
int pt_motion_pose(const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3], double time, double out24[24]);
/* Host only, no context needed. The sky pass's tile test: out_tiles[ty * tiles_x + tx] (tiles_x = ceil(width / 8), ceil(height / 8) rows) = 1 when NO
   ray the perspective camera can generate for any pixel of the 8x8 tile (ty, tx), any sample — any lens point, any jitter within blur_strength —
   can enter any of the n_boxes world-space boxes (six doubles each: lo.xyz, hi.xyz), else 0. Conservative: a 1 is a proof (the test and the proof are in
   csrc/pt_sky_tiles.h), a 0 promises nothing. More than 64 boxes are tested as their union. n_boxes = 0 clears every tile; a camera inside or touching a
   box clears none. A dynamic-mode pt_render of the whole frame in the plain shading mode (independent sampler, perspective projection, nothing
   moving, no camera medium) applies the test to the boxes of the world's entries (pt_world_entry_box) and renders the cleared tiles — every sample of
   theirs is the environment in the camera ray's direction — outside the path pool; the frame's sums and counts are what they are without. */
int pt_sky_tiles(const pt_camera* cam, uint32_t n_boxes, const double* boxes6, uint8_t* out_tiles);
/* Host only, no context needed. The same test read per box (csrc/pt_sky_tiles.h sky_tile_class): out_tiles = 1 for a sure-sky tile as above, 2 for a
   SHORT tile — every box the test could NOT clear has shadeable[b] != 0, so a camera ray of the tile enters boxes of shadeable entries or none — and 0
   for every other tile (the path pool's). shadeable: n_boxes bytes, or null for none. More than 64 boxes, a NaN or an infinity, a camera inside or touching a
   box that is not shadeable: no tile is 2. A render as described above, on a scene without a lights list whose top level is walked flat, renders the
   short tiles' samples ahead of the path pool where their path is camera -> miss or camera -> one hit of a shadeable entry (a still world-level
   sphere or quad, diffuse, no normal map, no instance) -> miss; sums and counts are what they are without (PT_SHORT_PASS=0 under PT_EXPERIMENT=1). */
int pt_short_tiles(const pt_camera* cam, uint32_t n_boxes, const double* boxes6, const uint8_t* shadeable, uint8_t* out_tiles);
/* Host only, no context needed. The same test, its answer per box (csrc/pt_sky_tiles.h sky_tile_reach): bit b of out_masks[ty * tiles_x + tx] is 0 when NO
   camera ray of the tile can enter box b (a proof, as above) and 1 when the test could not clear it. The mask is 0 exactly where pt_sky_tiles says 1.
   All ones (every one of the 64 bits) wherever the test says nothing: a NaN or an infinity among the boxes or in the camera, the lens's centre or a
   corner of it inside or on a box, and, with more than 64 boxes, every tile whose union of boxes is not cleared. A render that runs the short-path pass
   keeps these masks on the device and its pass tests, per tile, only the entries a camera ray can reach (PT_SHORT_REACH=0,
   PT_SHORT_DIRECT=0 and PT_SHORT_SELF=0 under PT_EXPERIMENT=1 switch its steps off): sums and counts are what they are without. */
int pt_tile_reach(const pt_camera* cam, uint32_t n_boxes, const double* boxes6, uint64_t* out_masks);
int pt_motion_swept_box(const double box[6], const double axis[3], double angle0, double angle1, const double tr0[3], const double tr1[3], double out[6]);
/* test probe: the f64 world box (lo.xyz, hi.xyz) of world entry `entry` (lights list first, then objects), before the f32 rounding */
int pt_world_entry_box(pt_scene*, uint32_t entry, double out[6]);
/* ---- punctual lights: point, spot and directional "sun" lights (the reference's unfinished hittable/light.rs PointLight { position, power },
 *      finished, with two siblings; opt-in) ----
 * Arithmetic: f64, one IEEE rounding per written operation. A scene keeps a list of n <= 2048 punctual lights, each a record formed on the host:
 *   kind 0, pt_light_point(position, power), mirrors PointLight::new: I_c = power_c / (4 * PI), in W/sr.
 *   kind 1, pt_light_spot(position, target, inner_deg, outer_deg, intensity): axis = normalize(target - position), 0 <= inner_deg <= outer_deg < 180
 *     (angles from the axis), cos_i = cos(inner_deg * (PI / 180)) and cos_o likewise, by the deterministic cosine of pt_instance's angles
 *     (pt_math_probe which 4); I = the on-axis intensity.
 *   kind 2, pt_light_directional(direction, irradiance): axis = normalize(direction), the way the light travels; I = the irradiance on a plane
 *     facing the light.
 *   Each call returns the light's index k >= 0, or -1 and adds nothing: a non-finite or negative colour, a non-finite position, a zero-length
 *   axis, angles out of range, the list full. pt_scene_clear_punctual_lights empties the list, pt_scene_punctual_count is its length,
 *   pt_scene_punctual_light(k, out16) the record as stored: kind, pos.xyz, axis.xyz, I.rgb, cos_i, cos_o, four zeros. The list takes effect at the
 *   next pt_world_build. pt_scene_set_punctual_fraction(f), 0 < f < 1 and finite (else -1, the setting stays), default 0.5, takes effect at once.
 * In effect: n > 0 at the last build. Otherwise every entry point launches the kernels it launches without this feature and produces the same
 *   bits, whatever f is. In effect for pt_render, pt_render_pixels, pt_render_adaptive and pt_render_multi, static and dynamic pools, with and
 *   without a lights list, both samplers. pt_render_aovs and pt_intersect do not change. A render returns -1 when environment importance
 *   sampling, any participating or interior medium, exact light sampling, dispersion or motion is in effect too, or max_depth >= 2^20. The sky
 *   pass stays off.
 * At a surface bounce, after emission and roulette, the selector draw r is made as without: p_punct = f, p_light = lights ? (1 - f) / 2 : 0,
 *   p_bsdf = 1 - p_light - p_punct. r < p_light: lights.sample; r < p_light + p_punct: the punctual branch; otherwise mat.sample — the order of
 *   the environment-sampling mixture. The light and BSDF branches are the bounce without this feature with pdf = p_bsdf * bsdf_pdf + p_light *
 *   light_pdf under these weights (a punctual direction has measure zero there and adds no term).
 * The punctual branch. One index draw k = gen_range(0..n), the conversion of the lights list's index draw (under the Sobol sampler a single
 *   draw, not pair-aligned). With x the hit point — kinds 0, 1: L = pos - x, d2 = dot(L, L), D = sqrt(d2), w = L / D, E_c = I_c / d2; kind 1 in
 *   addition c = -dot(w, axis), s = cos_i > cos_o ? clamp((c - cos_o) / (cos_i - cos_o), 0, 1) : (c >= cos_o ? 1 : 0), fall = (s * s) * (3 - 2 * s),
 *   E_c = (I_c * fall) / d2; kind 2: w = -axis, E = I. Then e = mat.eval(wo, w), the material's own eval with its cosine factor (the call the
 *   lights branch makes), pm = f / (double)n, thr' = ((thr * e) * E) / pm componentwise. The path ends when d2 is 0 or not finite, or thr' is
 *   exactly (0, 0, 0). Otherwise it continues as a SHADOW segment: the ray Ray::new(point + (1e-3 * signum(dot(w, gn))) * gn, w, time) — the
 *   offset of every continued ray —, ++bounce, and the depth bound as at any bounce: a shadow segment that would be the max_depth-th ray is never
 *   resolved, so max_depth = 2 is the first depth at which these lights show, as for area lights.
 * Resolving a SHADOW segment, when K3 next visits the path, before anything else (no emission, no roulette, no draw). With o the stored ray
 *   origin: D' = length(pos_k - o) for kinds 0 and 1, +inf for kind 2. The light is visible iff the ray missed or hit.dist >= D' (a surface
 *   behind the light does not shadow it). If visible, radiance += thr; the environment is not added on a miss. The path ends either way.
 * Consequences. The lights are invisible to camera and BSDF rays. Any surface occludes, glass included: no caustics from them and no light
 *   through windows. Selection is uniform, not by power. The sample's expectation is direct lighting by the list plus the estimator of
 *   everything else as it is without: each branch is divided by its own probability. */
int pt_light_point(pt_scene*, const double position[3], const double power[3]);
int pt_light_spot(pt_scene*, const double position[3], const double target[3], double inner_deg, double outer_deg, const double intensity[3]);
int pt_light_directional(pt_scene*, const double direction[3], const double irradiance[3]);
int pt_scene_clear_punctual_lights(pt_scene*);
int pt_scene_punctual_count(pt_scene*);
int pt_scene_punctual_light(pt_scene*, int k, double out[16]);
int pt_scene_set_punctual_fraction(pt_scene*, double f);
double pt_scene_punctual_fraction(pt_scene*);
/* test probe: the punctual branch's device functions as k_shade calls them. which 0: in = n x point.xyz; row i uses the independent sampler's
 * draws of (seed 0, pixel i, sample 0) from draw 0; out = n x (k, w.xyz, D, E.rgb, draws consumed). which 1: in = n x (k, point.xyz), out = n x
 * (w.xyz, D, E.rgb). -1 when the world was built without punctual lights. */
int pt_punctual_probe(pt_scene*, int which, const double* in, uint32_t n, double* out);
/* Host only, no context needed: the device's light evaluation compiled for the host. rec16: a record as pt_scene_punctual_light returns it;
 * out7 = (w.xyz, D, E.rgb). */
int pt_punctual_eval(const double rec16[16], const double point[3], double out7[7]);
/* ---- light shafts: punctual lights that light participating media (a spot light's cone in haze, a lamp in fog, sun beams through smoke; opt-in;
 *      DESIGN.md section 22) ----
 * pt_scene_set_punctual_media(on): 0 (default) or 1; any other value returns -1 and leaves the setting. It takes effect at once, without a rebuild.
 *   pt_scene_punctual_media reads it.
 * In effect for a render: the setting is 1, punctual lights are in effect (n > 0 at the last build) and media are in effect with homogeneous
 *   (pt_mat_medium) or grid (pt_mat_medium_grid) media only, as the material of a boundary object or as the camera medium. With the setting 0
 *   everything is as without it, the refusal of the pair included. With the setting 1 and only one of the two features in effect, that feature's
 *   kernels run and produce its bits. With a glass interior or a tinted medium in effect the render is still refused (-1); so it is with
 *   environment importance sampling, exact light sampling, dispersion or motion, as for either feature. max_depth must be at most 255 then: a path
 *   keeps its medium (12 bits), the SHADOW flag, the light's index (11 bits) and its bounce number (8 bits) in one word. In effect for pt_render,
 *   pt_render_pixels, pt_render_adaptive and pt_render_multi, static and dynamic pools, with and without a lights list, both samplers.
 *   pt_render_aovs, pt_intersect and the sky pass do not change.
 * The rule is pt_mat_medium's steps 1-4 (pt_mat_medium_grid's step 1 for a grid medium) and the punctual rule above, with these additions and
 *   nothing else. f64, one rounding per written operation; draws are converted as those rules convert them.
 * Medium vertex (step 2), at x with the segment's direction dir. Roulette as there. The selector draw r is READ (without this feature a medium
 *   vertex without a lights list only advances the counter). The shares are the surface bounce's under punctual lights: p_punct = f, p_light =
 *   lights ? (1 - f) / 2 : 0, p_bsdf = 1 - p_light - p_punct. r < p_light: lights.sample; r < p_light + p_punct: the punctual branch; otherwise
 *   the phase sample. The lights and phase branches are step 2's with pdf = p_bsdf * ph + p_light * light_pdf under these weights.
 *   The punctual branch: one index draw k, the surface rule's (a single draw under the Sobol sampler); (w, D, d2, E) of light k at x as there;
 *   ph = hg_phase(g, dot(dir, w)) — the phase function stands where the surface has its eval, and there is no cosine —; pm = f / (double)n;
 *   thr' = ((thr * (albedo * ph)) * E) / pm componentwise. The path ends when d2 is 0 or not finite, or thr' is exactly (0, 0, 0). Otherwise it
 *   continues as a SHADOW segment Ray::new(x, w, time) — no offset, as for a scattered ray —, ++bounce, the depth bound as at any bounce; m is kept.
 * Surface bounce (step 4): the punctual rule as it is. The SHADOW segment keeps the path's m.
 * Resolving a SHADOW segment, when K3 next visits the path, before anything else. With o the stored origin: D' = length(pos_k - o) (+inf for a
 *   directional light), t = the hit distance or +inf on a miss, t_end = t < D' ? t : D'. In this order:
 *   1 Lost crossing: m is a medium that some world object bounds and the ray missed: m becomes none, no draw (step 1's exception, unchanged).
 *   2 Free flight, if m is set: step 1's over [0, t_end) with its draws — a homogeneous medium one draw, d = -log(1 - u) / density; a grid
 *     medium grid_track with t_end in place of t. A collision at a distance below t_end: the light is BLOCKED, the path ends, nothing is added.
 *   3 Boundary crossing: otherwise, if the ray hit a medium's boundary at t < D', the segment goes on: m toggles exactly as in step 3, the
 *     origin moves to the offset hit point, ++bounce and the depth bound (a segment the bound cuts contributes nothing, like any ray beyond
 *     max_depth). The path stays a SHADOW segment towards light k; the throughput is unchanged. D' is formed again from the new origin.
 *   4 Resolution: otherwise the light is visible iff the ray missed or t >= D'. If visible, radiance += thr. The path ends either way; the
 *     environment is never added.
 * Consequences. In expectation a shadow segment carries the transmittance exp(-integral of sigma) of everything between its origin and the
 *   light: the analog free flight collides before t_end with probability 1 - exp(-integral), so the estimate is unbiased — for grids too, by
 *   delta tracking. A sun in an UNBOUNDED homogeneous medium is always blocked (D' = t = +inf): use a bounded fog box. A shadow segment spends
 *   one bounce of depth per boundary it crosses. Everything the punctual rule states stays true: the lights are invisible to camera, phase and
 *   BSDF rays, every surface blocks them, selection is uniform. */
int pt_scene_set_punctual_media(pt_scene*, int on);
int pt_scene_punctual_media(pt_scene*);
/* ---- the light grid: punctual lights picked by importance per scene cell (a street of lamps, a string of spots, a chandelier; opt-in;
 *      DESIGN.md section 26) ----
 * The two sections above stay what they are: with the selection kind 0, the default, every bit and every draw is theirs. Kind 1 replaces one
 * thing, the choice of the light k and its probability, at the surface bounce's punctual branch and at the light-shaft medium vertex's.
 * Arithmetic: f64, one IEEE rounding per written operation, no contraction.
 * Settings. pt_scene_set_punctual_selection(kind): 0 uniform (default), 1 the light grid; any other value returns -1 and leaves the setting;
 *   pt_scene_punctual_selection reads it. pt_scene_set_punctual_grid(nx, ny, nz, box6_or_NULL): the dims are 0, 0, 0 (automatic, the default) or
 *   each in 1..64; a box (lo.xyz, hi.xyz), when given, must be finite with hi >= lo per axis; NULL (default) means the world's bounds at the
 *   build. A refused call returns -1 and changes nothing. Like the light list, both settings take effect at the next pt_world_build; they do
 *   not clear `built`. pt_scene_punctual_grid(dims3, box6) reports what the LAST BUILD used (either pointer may be NULL); -1 when the grid is
 *   not in effect.
 * In effect: the kind was 1 at the last build and n > 0. Otherwise nothing new runs and no table exists. pt_render's refusals are the two
 *   sections' own, unchanged.
 * Build (pt_world_build). Box: the one given, or the union of pt_world_entry_box over all entries; if that union is not finite the build fails
 *   (-1) and asks for a box. Automatic dims: R = 16; an axis of extent ext gets clamp(ceil(R * ext / ext_max), 1, R) cells — the longest R —,
 *   an axis of extent 0 one cell; R is halved until cells * n <= 2^25. Explicit dims with cells * n > 2^25 fail the build (2^25 entries are
 *   256 MiB of doubles).
 *   Cell (ix, iy, iz) has index (iz * ny + iy) * nx + ix. Per axis s = (hi - lo) / (double)n_axis, a = lo + i * s, b = lo + (i + 1) * s (i and
 *   i + 1 as doubles), m = (a + b) * 0.5, h = (b - a) * 0.5; rc2 = (hx * hx + hy * hy) + hz * hz.
 *   Weight of light k for the cell: Y = (I_r + I_g) + I_b. Kind 2: w = Y. Kinds 0 and 1: per axis t = p < a ? a - p : (p > b ? p - b : 0) with p
 *   the light's position, dmin2 = (tx * tx + ty * ty) + tz * tz, w = Y / (dmin2 + rc2). Kind 1 adds a cone cull: v = m - pos, d2 = (vx * vx +
 *   vy * vy) + vz * vz, and only when d2 > rc2: d = sqrt(d2), sa = sqrt(rc2) / d, ca = sqrt(1 - sa * sa), c_m = ((vx * ax + vy * ay) + vz * az) / d
 *   with a the light's axis, so = sqrt(max(0, 1 - cos_o * cos_o)), c_far = cos_o * ca - so * sa; if cos_o > -ca && c_m < c_far - 1e-9 then
 *   w = 0. c_far is cos(theta_o + alpha): the cull fires when the cell's bounding sphere lies wholly outside the outer cone.
 *   Row of the cell: W = the sum of the w_k in ascending k. If W is not finite or not > 0, every p_k = 1 / (double)n; otherwise p_k = 0.875 *
 *   (w_k / W) + 0.125 / (double)n. C[k] = C[k-1] + p_k in ascending k with C[-1] = 0, and C[n-1] is stored as exactly 1.0. The one-eighth
 *   uniform floor gives every light a probability of at least 1 / (8n) in every cell: the importance may be wrong — it ignores occlusion and
 *   the material, and its cone test is a bound on a sphere — and the estimator stays unbiased.
 * Selection at a vertex x. Cell: per axis inv = (hi > lo) ? n_axis / (hi - lo) : 0, q = (x - lo) * inv, i = q >= 0 ? (q < (double)n_axis ?
 *   (uint32)q : n_axis - 1) : 0 — a NaN and every point outside the box take a border cell (the vertices of an unbounded medium are such
 *   points). Draw: u = one draw by the rand Standard f64 conversion ((v >> 11) * 2^-53); under the Sobol sampler a single draw, not
 *   pair-aligned, like the index draw it replaces. k = the smallest index with u < C[k] (it exists: C[n-1] = 1), p = C[k] - (k > 0 ? C[k-1] :
 *   0). Weight: pm = f * p, thr' = ((thr * e) * E) / pm; at a medium vertex albedo * ph stands where e stands. Everything after that —
 *   endings, the SHADOW segment, the bounce word, resolution — is the two sections' own; k is an index below n.
 *   The probability that u lands in [C[k-1], C[k]) is that difference up to u's 2^-53 lattice: against p >= 1 / 16384 (n <= 2048) the relative
 *   error is below 2e-12.
 * Exactly one draw is made (gen_range rejects half of its draws when n is a power of two). */
int pt_scene_set_punctual_selection(pt_scene*, int kind);
int pt_scene_punctual_selection(pt_scene*);
int pt_scene_set_punctual_grid(pt_scene*, uint32_t nx, uint32_t ny, uint32_t nz, const double* box6_or_null);
int pt_scene_punctual_grid(pt_scene*, uint32_t dims3[3], double box6[6]);
/* pt_punctual_probe with the light grid in effect (-1 otherwise). which 2: in = n x point.xyz; row i uses the independent sampler's draws of
 * (seed 0, pixel i, sample 0) from draw 0; out = n x (cell, k, p, draws consumed, w.xyz, D, E.rgb). which 3: in = n x (cell, k), out = n x
 * C[cell][k]. */
/* Host only, no context needed: the device's functions compiled for the host. pt_punctual_grid_row: recs16 = n records as
 * pt_scene_punctual_light returns them (1 <= n <= 2048), box6 finite with hi >= lo, dims3 each in 1..64, cell < nx * ny * nz; out_cdf = the
 * cell's n values C[0..n-1]. pt_punctual_grid_select: table = the WHOLE table, row after row in cell order, nx * ny * nz rows of n doubles;
 * for each of the m (point.xyz, u) pairs out3 = (cell, k, p). */
int pt_punctual_grid_row(const double* recs16, uint32_t n, const double box6[6], const uint32_t dims3[3], uint32_t cell, double* out_cdf);
int pt_punctual_grid_select(const double box6[6], const uint32_t dims3[3], const double* table, uint32_t n, const double* points, const double* u, uint32_t m, double* out3);
/* ---- world: src/hittable/world.rs:10-29 -------------------------------------------------- */
int pt_world_add_object(pt_scene*, int obj);
int pt_world_add_light(pt_scene*, int obj);
int pt_world_build(pt_scene*);          /* build_bvh: flatten to SoA, build BVHs, upload to HBM */
uint32_t pt_world_prim_count(pt_scene*);
/* BVH::build (bvh.rs:24-121) for large meshes on the GPU: meshes with at least min_triangles triangles get an LBVH built
 * by HIP kernels at the next pt_world_build (default 2^19; 0 = always the host's binned-SAH builder). Any conservative
 * tree gives the same hits; an LBVH is cheaper to build and costlier to traverse. _info: meshes the GPU builder handled
 * in the last build and the depth of the deepest of them. */
int pt_world_set_device_bvh_threshold(pt_scene*, uint32_t min_triangles);
int pt_world_device_bvh_info(pt_scene*, uint32_t* n_meshes, uint32_t* deepest);

/* ---- asset ingest (host): the roles of tobj::load_obj (main.rs:408) and
 * ImageReader::open().decode().to_rgb8() (texture.rs:62-67) for .obj / Radiance .hdr ------- */
int pt_load_obj(const char* path, float** pos, uint32_t* n_pos, uint32_t** idx, uint32_t* n_idx, float** uv, uint32_t* n_uv);
/* OBJ with vn and separate v/vt/vn index streams, expanded to ONE index per corner (tobj's single_index): the fix of
 * mesh.rs:173-184's position-indexed normals / texcoords. Feed the result to pt_mesh. */
int pt_load_obj_single_index(const char* path, float** pos, uint32_t* n_pos, uint32_t** idx, uint32_t* n_idx, float** nrm, uint32_t* n_nrm,
                             float** uv, uint32_t* n_uv);
int pt_load_hdr_rgb8(const char* path, uint8_t** rgb, uint32_t* w, uint32_t* h);
int pt_load_hdr_rgbf32(const char* path, float** rgb, uint32_t* w, uint32_t* h);   /* the same decode without .to_rgb8(): f32 RGB, free with pt_free */
int pt_load_png_rgb8(const char* path, uint8_t** rgb, uint32_t* w, uint32_t* h);   /* PNG -> RGB8 (alpha dropped like to_rgb8, texture.rs:67) */
/* JPEG -> RGB8: baseline and progressive Huffman JPEG (the reference's earthmap.jpg / envmap.jpg, main.rs:100,365) with libjpeg's
 * reference arithmetic (ISLOW integer IDCT, fixed-point YCbCr->RGB, fancy chroma upsampling): csrc/pt_jpeg.cpp */
int pt_load_jpeg_rgb8(const char* path, uint8_t** rgb, uint32_t* w, uint32_t* h);
void pt_free(void*);
/* images decoded by the caller (any format this library has no decoder for — or pixels a host wants to substitute): hand them
 * over decoded, under the file name the reference's scene opens ("envmap.jpg", "earthmap.jpg", "bricks/color.png", ...); a
 * registered image takes precedence over the file */
int pt_register_image(pt_scene*, const char* name, uint32_t w, uint32_t h, const uint8_t* rgb);
int pt_find_registered_image(pt_scene*, const char* name);   /* texture handle or -1 */
int pt_save_png(const char* path, uint32_t w, uint32_t h, const uint8_t* rgb);   /* imgbuf.save camera.rs:118 */

/* ---- the reference's scene scripts main.rs:14-618 (`-s N`); fills the camera the script sets
 * up. scene_seed replaces the unseeded build-time RNG of scene 1 (main.rs:38-47). ----------- */
int pt_build_scene(pt_scene*, int scene_id, uint32_t width, uint32_t spp, const char* asset_dir, uint64_t scene_seed,
                   pt_camera* out_cam);

/* Camera::init camera.rs:51-77; out6x3 = forward,right,up,pixel00,pixel_du,pixel_dv */
int pt_camera_init(const pt_camera*, double out6x3[18], uint32_t* image_height);

/* Camera::render camera.rs:79-126, the hot path. Adds to accum[(y*W+x)*3+c] the SUM over
 * samples [spp_begin, spp_end) of trace(y, x) — sums, not means, so that sample ranges
 * rendered on different GPUs add up (one reduce) before pt_resolve_u8. */
int pt_render(pt_scene*, const pt_camera*, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* accum,
              const pt_render_opts* opts, pt_render_stats* stats);
/* camera.rs:109-114,128-130: mean, sqrt gamma, clamp(0,0.999)*256 as u8. Host buffers. */
int pt_resolve_u8(pt_ctx*, const double* accum, uint32_t n_pixels, uint32_t total_spp, uint8_t* rgb8);

/* ---- pixel lists and adaptive sampling (no counterpart in the reference) ----------------------------------------------
 * pt_render restricted to the listed pixels (row-major y*W+x, strictly ascending, < W*H; n == 0 is a no-op). Adds (or, with
 * opts->overwrite, stores) the sums of samples [spp_begin, spp_end) of each LISTED pixel into accum (the full W*H*3 frame, host
 * or device as opts says); the values of pixels that are not listed are not written. A listed pixel's sums are those pt_render
 * computes for it (static mode: bit for bit). An unsorted, duplicated or out-of-range list returns -1. */
int pt_render_pixels(pt_scene*, const pt_camera*, uint64_t seed, const uint32_t* pixels, uint32_t n, uint32_t spp_begin,
                     uint32_t spp_end, double* accum, const pt_render_opts* opts, pt_render_stats* stats);
/* Render to a noise target. Schedule (all integer divisions): b_0 = 0, b_1 = min_spp/2, b_2 = min_spp,
 * b_{i+1} = min(max_spp, b_i + max(min_spp/2, b_i/2)); round i renders [b_i, b_{i+1}) of the active pixels as one
 * pt_render_pixels pass, even rounds into sums E, odd rounds into sums O. After each round i >= 1 with b_{i+1} < max_spp,
 * with n_E, n_O the samples of the even / odd rounds so far: A_c = E_c / n_E, B_c = O_c / n_O,
 * M = (E_r+O_r + E_g+O_g + E_b+O_b) / (n_E+n_O), err = (|A_r-B_r| + |A_g-B_g| + |A_b-B_b|) / (1e-4 + sqrt(M)) (left to right,
 * one IEEE rounding per operation); an active pixel stays active if !(err < threshold) holds for itself or for any active
 * pixel among its 8 neighbours, else it stops for good with b_{i+1} samples. */
typedef struct pt_adaptive_opts {
    uint32_t min_spp;          /* >= 2: samples every pixel gets before its first test */
    uint32_t max_spp;          /* >= min_spp: no pixel gets more */
    double threshold;          /* a pixel stops once err < threshold; <= 0: none stops early */
    uint32_t slots_per_pixel;  /* as pt_render_opts (1 = the reference's per-pixel order, bit-exact mode) */
    uint32_t profile;
    void* stream;              /* hipStream_t; NULL = the context's own stream */
} pt_adaptive_opts;
/* round boundaries b_0 = 0 < b_1 < ... < b_R = max_spp: writes the first min(R + 1, cap) of them and returns R + 1, or -1
 * (min_spp < 2, max_spp < min_spp) */
int pt_adaptive_schedule(uint32_t min_spp, uint32_t max_spp, uint32_t* bounds, uint32_t cap);
/* accum: host W*H*3 sums E + O (overwritten); spp_per_pixel: host W*H, the samples each pixel received.
 * stats: summed over the passes (samples == sum of spp_per_pixel). Device memory on top of the path pool: 68 B per pixel. */
int pt_render_adaptive(pt_scene*, const pt_camera*, uint64_t seed, const pt_adaptive_opts* opts, double* accum,
                       uint32_t* spp_per_pixel, pt_render_stats* stats);
/* pt_resolve_u8 with each pixel's own count (> 0): mean = sum * (1.0 / n_p), then pt_resolve_u8's arithmetic. Host buffers. */
int pt_resolve_u8_counts(pt_ctx*, const double* accum, uint32_t n_pixels, const uint32_t* spp_per_pixel, uint8_t* rgb8);

/* ---- feature buffers and denoising (no counterpart in the reference) ----------------------------------------------------
 * First-hit AOVs. For every pixel and each sample s in [spp_begin, spp_end), the camera ray is the one pt_render traces for
 * (pixel, s): same seed, same RNG draws. The ray's first hit adds to aov[(y*W+x)*8 + k]. These are SUMS over samples, like
 * accum, so sample ranges add up:
 *   k = 0..2  albedo r,g,b   (every sample): diffuse / metal / principled: the colour texture at the hit; sheen: its base colour;
 *             glass, clearcoat, light, a medium's boundary and a miss: (1, 1, 1) (glass's base colour reaches no radiance, emitted
 *             and environment light is not reflected, a boundary is a first hit like glass); mix: (1 - t) * A(child1) + t * A(child2), recursively over the two levels allowed
 *   k = 3..5  normal x,y,z   (hits only: the shading normal of the hit, normal map applied)
 *   k = 6     depth          (hits only: t of the first hit; camera rays are unit length)
 *   k = 7     hits           (number of samples whose camera ray hit something)
 * opts: accum_on_device, overwrite and stream as pt_render; the other fields are ignored. Deterministic (no atomics).
 * A null aov, an unbuilt world or spp_end < spp_begin returns -1; an empty range adds nothing (overwrite: stores zeros). */
int pt_render_aovs(pt_scene*, const pt_camera*, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov,
                   const pt_render_opts* opts);
/* Variance-guided a-trous denoiser (edge-avoiding wavelet filter on demodulated colour). Host buffers, W*H row-major.
 * sum_a / sum_b: the W*H*3 sums of two DISJOINT sample sets of n_a / n_b samples (e.g. pt_render over [0, n/2) and [n/2, n));
 * aov: pt_render_aovs sums over n_aov samples; out: W*H*3 MEANS. The rule, per pixel (f64, one IEEE rounding per operation):
 *   L(c) = 0.2126 r + 0.7152 g + 0.0722 b;  mu = (sum_a + sum_b) / (n_a + n_b)
 *   background: hits == 0. Foreground: z = depth / hits, N = normal / sqrt(x^2 + y^2 + z^2) (0 if that length is 0),
 *     a = max(albedo / n_aov, 1e-3) per channel, c = mu / a, cA = (sum_a / n_a) / a, cB = (sum_b / n_b) / a,
 *     v = (L(cA) - L(cB))^2 * (n_a n_b / (n_a + n_b)^2)   (the variance of the mean the two halves imply)
 *   level k = 0 .. K-1, step s = 2^k, for each foreground pixel p (background pixels keep c and v):
 *     g_p = the 3x3 filter (1/4, 1/2, 1/4)^2 of v over the in-image foreground neighbours, divided by the weight present
 *     taps q = p + s*(i, j), j then i in -2..2, in the image and foreground, with h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *     w = h_i h_j * exp(-|L(c_p) - L(c_q)| / (sigma_l sqrt(g_p) + 1e-10) - |z_p - z_q| / (sigma_z z_p + 1e-10)) * max(0, N_p.N_q)^128
 *     (one deterministic exp; the power as seven squarings);  c'_p = sum w c_q / sum w,  v'_p = sum w^2 v_q / (sum w)^2
 *     (sum w == 0, possible only with a zero normal: c and v are kept)
 *   out = c^(K) * a on the foreground, mu on the background.
 * Defaults (opts NULL), calibrated on scenes 3 and 6: K = 5, sigma_l = 4, sigma_z = 0.1.
 * Returns -1 for a null pointer, W or H = 0, n_a, n_b or n_aov = 0, K > 10, sigma_l or sigma_z <= 0 or NaN.
 * Device memory: 232 B per pixel for the call's duration. */
typedef struct pt_denoise_opts {
    uint32_t iterations;   /* a-trous levels K (steps 1, 2, ..., 2^(K-1)); <= 10. Default 5 */
    double sigma_l;        /* luminance edge-stopping, in standard deviations. Default 4 */
    double sigma_z;        /* relative-depth edge-stopping. Default 0.1 */
} pt_denoise_opts;
int pt_denoise(pt_ctx*, uint32_t width, uint32_t height, const double* sum_a, uint32_t n_a, const double* sum_b, uint32_t n_b,
               const double* aov, uint32_t n_aov, const pt_denoise_opts* opts, double* out);

/* ---- the film stage: exposure, glare, tone mapping and HDR output (no counterpart in the reference, whose camera.rs:109-130 is the
 * default options' case) ----
 * pt_film_develop turns W*H*3 sample SUMS (row-major, as pt_render leaves them) into the scene-linear image hdr_out (W*H*3 f64) and / or
 * the display image rgb8_out (W*H*3 bytes); either may be null, not both. n = counts ? counts[p] : total_spp per pixel p. Host buffers,
 * or with opts->on_device device pointers (a torch tensor, the accumulator of pt_render with accum_on_device). Like pt_denoise the call
 * returns when the work is done; sums is not written. With default options (opts NULL) rgb8_out holds pt_resolve_u8's bytes, or
 * pt_resolve_u8_counts's when counts is given.
 * The rule. f64, one IEEE rounding per written operation; lum(c) = 0.2126 r + 0.7152 g + 0.0722 b.
 *  1 Mean and exposure: m_c = sum_c * (1.0 / n), as pt_resolve_u8 / pt_resolve_u8_counts form it; k = exp2(exposure_ev), computed on the
 *    host; x_c = fmax(m_c * k, 0.0): NaN and negative values become 0, +inf stays.
 *  2 Bright part: Y = lum(x); w = (Y > T and Y is finite) ? (Y - T) / Y : 0, T = bloom_threshold; B_c = x_c * w.
 *  3 Glare, only when s = bloom_strength > 0. For level l = 0 .. L-1 (L = bloom_levels): sigma_l = bloom_sigma * 2^l, r_l = ceil(3 sigma_l),
 *    k_l[i] = exp(-(i * i) / (2 sigma_l^2)) for i = -r_l .. r_l, divided by their sum taken in that order (host).
 *    H_l[y][x] = sum_i k_l[i] B[y][x + i], then V_l[y][x] = sum_i k_l[i] H_l[y + i][x]; taps outside the image contribute 0 and the weights
 *    are NOT renormalised: light scattered past the frame is lost and none comes in. G = sum_l (1 / L) V_l. The order of the sums is the
 *    implementation's: every term is non-negative, so any order agrees to about (2 r + 1) * 2^-53 relative.
 *    o_c = (x_c - s * B_c) + s * G_c. With s == 0: o = x, no kernel of this step runs and no scratch for it is allocated.
 *  4 hdr_out = o: scene-linear, after exposure and glare, before the tone curve.
 *  5 Tone curve. For tonemap 1-3 first o_c = fmin(o_c, 1e150). oetf(t) = t <= 0.0031308 ? 12.92 t : 1.055 * pow(t, 1 / 2.4) - 0.055 (the
 *    deterministic pow of pt_detmath.h).
 *      0 reference: v_c = sqrt(o_c)                          1 srgb: v_c = oetf(fmin(o_c, 1))
 *      2 reinhard (extended, on luminance): Y = lum(o), sc = (1 + Y / (white * white)) / (1 + Y), v_c = oetf(fmin(o_c * sc, 1))
 *      3 aces (Narkowicz's fit): t = (o (2.51 o + 0.03)) / (o (2.43 o + 0.59) + 0.14), v_c = oetf(clamp(t, 0, 1))
 *  6 Quantiser, every mode: rgb8 = (uint8)(clamp(v_c, 0, 0.999) * 256) (NaN -> 0), pt_resolve_u8's.
 * Returns -1, writing nothing, for a null context or sums, both outputs null, W or H = 0, counts null and total_spp = 0, a host-side count
 * of 0 (device counts are not inspected), an option outside the range its field states (NaN included; pt_film_opts_check is that test
 * alone: 0, or -1 and pt_last_error; NULL = the defaults), or, with s > 0, a W or H above 524280 (the convolution's launch grid).
 * Device memory for the call's duration: with s > 0, 72 B per pixel of scratch (B, the transposed row pass, G: three f64 planes each)
 * plus the weights (8 B per tap); with s == 0 none. Host buffers add their device copies: 55 B per pixel. */
typedef struct pt_film_opts {
    double   exposure_ev;      /* image is scaled by 2^ev first. Default 0. Finite, |ev| <= 100 */
    uint32_t tonemap;          /* 0 reference (sqrt), 1 srgb, 2 reinhard, 3 aces. Default 0 */
    double   white;            /* tonemap 2: the luminance that maps to 1. Default 4. Finite, >= 1e-3 */
    double   bloom_strength;   /* s in [0, 1]; 0 = no glare (default) */
    double   bloom_threshold;  /* T >= 0, finite: luminance above which light spreads. Default 1 */
    double   bloom_sigma;      /* sigma_0 in pixels, in [0.5, 64]. Default 2 */
    uint32_t bloom_levels;     /* L in 1..6, sigma_0 * 2^(L-1) <= 128. Default 5 */
    uint32_t on_device;        /* sums, counts, hdr_out, rgb8_out are device pointers */
    void*    stream;           /* hipStream_t; NULL = the context's */
} pt_film_opts;
int pt_film_opts_check(const pt_film_opts* /* NULL = defaults */);
int pt_film_develop(pt_ctx*, uint32_t width, uint32_t height, const double* sums, uint32_t total_spp, const uint32_t* counts /* or NULL */,
                    const pt_film_opts* /* NULL = defaults */, double* hdr_out /* W*H*3 or NULL */, uint8_t* rgb8_out /* W*H*3 or NULL */);
/* Float image files (host). pt_save_hdr: Radiance RGBE, readable by pt_load_hdr_rgbf32: the "#?RADIANCE" / "FORMAT=32-bit_rle_rgbe" /
 * "-Y h +X w" header and flat scanlines; per pixel the shared exponent comes from its largest channel by frexp, mantissas are truncated;
 * negative, NaN and below-1e-38 values encode as 0. pt_save_pfm: "PF", little-endian (scale -1.0), rows bottom to top, the f32 bits as they
 * are. Both return -1 for a null pointer, a zero size or a file that cannot be written. */
int pt_save_hdr(const char* path, uint32_t w, uint32_t h, const float* rgb);
int pt_save_pfm(const char* path, uint32_t w, uint32_t h, const float* rgb);

/* ---- the physical sky: Preetham daylight, a ground and a sun disc, baked into a float lat-long map (no counterpart in the reference) ----
 * A stage of its own: it produces a W x H x 3 f32 map in the layout of an environment texture; the render kernels never see anything else.
 * pt_tex_sky bakes and hands the map to pt_tex_image_rgbf32, so the handle it returns is usable as pt_camera.env_tex (env_is_map = 1), with
 * pt_scene_set_env_sampling, the panorama projection and the film stage unchanged.
 * The rule. f64, one IEEE rounding per written operation, no contraction; exp, sincos, acos, pow are pt_detmath.h's on host and device.
 *  s = v' / |v'| with v' = sun_dir / (its largest |component|), |v'| = sqrt((x^2 + y^2) + z^2); T = turbidity; c_s = clamp(s.y, 0, 1),
 *  theta_s = acos(c_s): a sun below the horizon is held at the horizon for the sky's formulas. dot(d, s) = (d.x s.x + d.y s.y) + d.z s.z.
 *  Texel (i, j) (column, row; sample_environment's, PROJ_PANORAMA's and the environment sampler's geometry): centre theta = ((j + 0.5) pi) / H,
 *  phi = -pi + ((2 pi) (i + 0.5)) / W, d = (sin theta cos phi, cos theta, sin theta sin phi);
 *  solid angle w_ij = (cos((j pi) / H) - cos(((j + 1) pi) / H)) * ((2 pi) / W).
 *  Sky, d.y > 0 (Preetham, Shirley, Smits 1999; directions are used as given, unit length is the caller's business):
 *   c_g = clamp(dot(d, s), -1, 1), gamma = acos(c_g);
 *   F(c_t, gamma, c_g; A..E) = (1 + A exp(B / c_t)) * ((1 + C exp(D gamma)) + E (c_g c_g));
 *   A..E = a T + b with (a, b):
 *     Y: (0.1787, -1.4630) (-0.3554, 0.4275) (-0.0227, 5.3251) (0.1206, -2.5771) (-0.0670, 0.3703)
 *     x: (-0.0193, -0.2592) (-0.0665, 0.0008) (-0.0004, 0.2125) (-0.0641, -0.8989) (-0.0033, 0.0452)
 *     y: (-0.0167, -0.2608) (-0.0950, 0.0092) (-0.0079, 0.2102) (-0.0441, -1.6537) (-0.0109, 0.0529)
 *   zenith: chi = (4/9 - T/120) (pi - 2 theta_s); Yz = ((4.0453 T - 4.9710) (sin chi / cos chi) - 0.2155 T) + 2.4192;
 *     xz = ((T T) p_0 + T p_1) + p_2 with p_r = ((M_r0 theta_s^3 + M_r1 theta_s^2) + M_r2 theta_s) + M_r3, theta_s^2 = theta_s theta_s,
 *     theta_s^3 = theta_s^2 theta_s, Mx = (0.00166, -0.00375, 0.00209, 0; -0.02903, 0.06377, -0.03202, 0.00394; 0.11693, -0.21196, 0.06052, 0.25886);
 *     yz likewise with My = (0.00275, -0.00610, 0.00317, 0; -0.04214, 0.08970, -0.04153, 0.00516; 0.15346, -0.26756, 0.06670, 0.26688);
 *   q = (qz F(d.y, gamma, c_g)) / F(1, theta_s, c_s) for q in Y, x, y (the zenith values and the denominators are formed once, on the host);
 *   X = (x / y) Y, Z = (((1 - x) - y) / y) Y; linear sRGB (D65): r = (3.2404542 X - 1.5371385 Y) - 0.4985314 Z,
 *   g = (-0.9692660 X + 1.8760108 Y) + 0.0415560 Z, b = (0.0556434 X - 0.2040259 Y) + 1.0572252 Z; each max(0, .), then times `scale`.
 *   Model units are kcd/m^2 (klx for irradiance); `scale` brings them to the renderer's.
 *  Sun irradiance E_sun (an approximation: Preetham's Rayleigh and Angstrom terms only; ozone, gas and water vapour are left out). s.y > 0:
 *   m = 1 / (s.y + 0.15 pow(93.885 - (theta_s 180) / pi, -1.253)); beta = 0.04608 T - 0.04586; lambda = (0.610, 0.550, 0.465) um for r, g, b;
 *   tau_c = 0.008735 pow(lambda_c, -4.08) + beta pow(lambda_c, -1.3); E_sun,c = 127.5 exp(-(tau_c m)). s.y <= 0: E_sun = 0.
 *   pt_sky_sun_irradiance = (scale sun_scale) E_sun,c.
 *  Ground, d.y <= 0 (a Lambertian plane lit by this sky): G_c = ((scale albedo_c) (E_sky,c + (sun_scale E_sun,c) max(0, s.y))) / pi, where
 *   E_sky,c = sum_a sum_b sky_c(d_ab) wgt_a of the unscaled sky (scale = 1) over 16 x 64 midpoints theta_a = ((a + 0.5) (pi/2)) / 16,
 *   phi_b = -pi + ((2 pi) (b + 0.5)) / 64, wgt_a = (cos theta_a (cos((a (pi/2)) / 16) - cos(((a + 1) (pi/2)) / 16))) * ((2 pi) / 64), b inner, a outer,
 *   in order: it does not depend on W and H.
 *  The disc, pt_sky_bake only (sun_scale > 0 and E_sun > 0, else nothing is added): each texel has 8 x 8 sub-directions
 *   theta = ((j + (a + 0.5) / 8) pi) / H, phi = -pi + ((2 pi) (i + (b + 0.5) / 8)) / W; n_ij = how many have dot(d_sub, s) >= cos(alpha),
 *   alpha = (sun_radius_deg pi) / 180 (sub-directions below the horizon count too). If every n_ij is 0, the texel sample_environment reads
 *   for direction s gets n = 64. Omega = sum_j (((sum_i n_ij) / 64) (cos((j pi) / H) - cos(((j + 1) pi) / H))) * ((2 pi) / W), rows in order
 *   (the row sums are integers: no order to fix); L_sun,c = ((scale sun_scale) E_sun,c) / Omega; texel = (float)(sky-or-ground at the centre +
 *   L_sun,c (n_ij / 64)). So sum_ij disc_ij w_ij = pt_sky_sun_irradiance at every map size, and two bakes of the same options are the same bytes.
 * Every entry point returns -1 for options outside the ranges below (NaN included; pt_sky_opts_check is that test alone and names the field),
 * a null buffer with n > 0, W or H = 0 or W * H > 2^26. NULL options mean the defaults. Device memory of a bake, for the call's duration:
 * the disc's window (1 B per texel of it) and 4 B per row; a host `rgb` adds its device copy (12 B per texel). */
typedef struct pt_sky_opts {
    double sun_dir[3];        /* from the scene towards the sun, world axes (y up), any finite length > 0; normalised once on the host */
    double turbidity;         /* T, finite, 1.7 <= T <= 10. Default 3 */
    double ground_albedo[3];  /* each finite, in [0, 1]. Default 0.3 */
    double sun_radius_deg;    /* angular radius alpha of the disc, 0 < alpha <= 10. Default 0.2665 */
    double sun_scale;         /* >= 0, finite; multiplies the sun's irradiance; 0 = no disc in the map. Default 1 */
    double scale;             /* > 0, finite; multiplies everything (model units are kcd/m^2). Default 0.04 */
} pt_sky_opts;
int pt_sky_opts_default(pt_sky_opts*);              /* sun_dir = (0, 1, 0) */
int pt_sky_opts_check(const pt_sky_opts* /* NULL = defaults */);
/* host only, no context: n directions xyz -> n x rgb: the sky above, the ground below, NO disc */
int pt_sky_eval(const pt_sky_opts*, const double* dirs, uint32_t n, double* out_rgb);
int pt_sky_sun_irradiance(const pt_sky_opts*, double out[3]);   /* zeros when the sun is not above the horizon */
/* device: pt_sky_eval by the bake kernel's device function (the same bits); the bake (w*h*3 floats, row-major, disc included; `rgb` a host
 * buffer, or with rgb_on_device a device pointer); and the bake followed by exactly pt_tex_image_rgbf32 of its result, whose handle it returns */
int pt_sky_probe(pt_ctx*, const pt_sky_opts*, const double* dirs, uint32_t n, double* out_rgb);
int pt_sky_bake(pt_ctx*, const pt_sky_opts*, uint32_t w, uint32_t h, float* rgb, int rgb_on_device);
int pt_tex_sky(pt_scene*, const pt_sky_opts*, uint32_t w, uint32_t h);

/* ---- mesh tessellation and displacement mapping (not in the reference, opt-in) ----
 * A stage of its own in front of pt_mesh: a coarse mesh and a height image in, an ordinary fine mesh out. No render kernel knows of it.
 * pt_mesh_tessellate runs on the GPU (csrc/pt_tess.hip), pt_mesh_tessellate_host is its host twin; the two return the same bytes.
 * Input: pt_mesh's: f32 positions, u32 index triples, optional f32 normals and texcoords indexed by the position index. The attribute
 *  arrays are brought to n = n_pos entries first (entries past n_pos dropped, missing ones zero: no index refers to them).
 * Arithmetic: f64 on the f32 values widened, in the order written here, no fused operation; each written vertex attribute is rounded
 *  to f32 once (so level l + 1 reads the f32 values level l wrote). sqrt and floor are the IEEE operations.
 * One level, n vertices and F faces -> n + E vertices and 4F faces:
 *  face f = (a, b, c) has the edges e0 = (a, b), e1 = (b, c), e2 = (c, a); an edge's key is (min << 32) | max (a == b is an edge like any
 *  other). The E distinct keys in ascending order: the midpoint of the key of rank r is vertex n + r. Old vertices keep their indices,
 *  unreferenced ones stay. Midpoint position and texcoord: (A + B) * 0.5 per component. Midpoint normal: s = A + B per component,
 *  L = sqrt((s.x s.x + s.y s.y) + s.z s.z); L finite and > 0: s / L per component, else the normal of the endpoint with the smaller index.
 *  Children, winding kept: 4f = (a, ab, ca), 4f + 1 = (ab, b, bc), 4f + 2 = (ca, bc, c), 4f + 3 = (ab, bc, ca).
 * Smooth normals of a mesh: per vertex, the corners 3f + k that refer to it in ascending order; sum = 0, then sum += c_f componentwise
 *  with c_f = (p1 - p0) x (p2 - p0) of face f (e1 = p1 - p0, e2 = p2 - p0, c = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *  e1.x e2.y - e1.y e2.x)): area weighting. L as above; L finite and > 0: sum / L, else the normal the vertex had, else (0, 1, 0).
 * Displacement (height != NULL), after the last level, per vertex with texcoord (u, v) and normal N: N is the carried (interpolated)
 *  normal as stored, not renormalised; an input without normals gets the smooth normals of the subdivided, undisplaced mesh (rounded
 *  to f32 like any attribute), and those are then its carried normals. The image is height_w x height_h f32, row 0 at v = 1.
 *  wrap 0 (clamp): u, v clamped to [0, 1], texel indices clamped to the image; wrap 1 (repeat): u - floor(u), indices modulo W / H
 *  (a true modulo). x = u W - 0.5, y = (1 - v) H - 0.5, i0 = floor(x), tx = x - i0, j0 = floor(y), ty = y - j0, i1 = i0 + 1, j1 = j0 + 1;
 *  h = (h00 (1 - tx) + h10 tx) (1 - ty) + (h01 (1 - tx) + h11 tx) ty with hab = texel (ia, jb); d = scale (h - midlevel);
 *  p' = p + N d per component. d = 0 where u, v or h is not finite.
 * Normals written (`normals`): 0 auto = smooth when displacing, else the input's if it had any, else none; 1 keep = the carried
 *  normals (none when there are none); 2 smooth = recomputed from the final positions (a vertex without a usable sum keeps its carried
 *  normal); 3 none (pt_mesh then shades flat).
 * Refused with -1 before any device work: a NULL output pointer or a NULL array with a count above 0; n_idx % 3 != 0; an index out of
 *  range for any given array; a height without texcoords or with height_w or height_h = 0; levels > 12; 4^levels F > 0x07FFFFFF
 *  (pt_mesh's cap); n + (4^levels - 1) F > 2^32 - 1 (that bounds n + E at every level); an unknown wrap or normals value. NULL options
 *  mean the defaults. NaN and infinite positions, normals, texcoords and texels are data. Outputs are malloc'd: free them with pt_free;
 *  *out_nrm / *out_uv are NULL where there is none; *out_n_idx counts indices. A failed device allocation returns -1 with nothing held.
 * Device memory, per level of F faces and n vertices: the two meshes (32 B a vertex with both attributes, 12 B a face, old and new)
 *  plus 108 B a face of edge keys, slots, flags, ranks and midpoint indices, and the radix sort's own buffer. A mesh whose vertices are duplicated along texcoord seams
 *  (pt_load_obj_single_index) cracks there under displacement: the duplicates move along different normals. Welding is not done here. */
typedef struct pt_tess_opts {
    uint32_t levels;               /* 0..12. Default 1 */
    uint32_t height_w, height_h;
    const float* height;           /* NULL: no displacement */
    double scale, midlevel;        /* Defaults 1 and 0.5 */
    int wrap;                      /* 0 clamp (default), 1 repeat */
    int normals;                   /* 0 auto (default), 1 keep, 2 smooth, 3 none */
} pt_tess_opts;
int pt_tess_opts_default(pt_tess_opts*);
int pt_mesh_tessellate(pt_ctx*, const pt_tess_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                       uint32_t n_nrm, const float* nrm, uint32_t n_uv, const float* uv,
                       float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm, float** out_uv);
int pt_mesh_tessellate_host(const pt_tess_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                            uint32_t n_nrm, const float* nrm, uint32_t n_uv, const float* uv,
                            float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm, float** out_uv);
/* host only: the drop-in mesh for pt_quad(q, u, v). Vertex (i, j), 0 <= i <= nu, 0 <= j <= nv, has index j (nu + 1) + i, position
 * (q + u (i / nu)) + v (j / nv) and texcoord (i / nu, j / nv), all f64 rounded to f32 once; every vertex has the normal c / L,
 * c = cross(u, v), L as above. Cell (i, j) has the faces (v00, v10, v11) and (v00, v11, v01), cells in row order. -1 for nu or nv = 0,
 * more than 0x07FFFFFF faces, or u x v without a finite length above 0. */
int pt_mesh_grid(const double q[3], const double u[3], const double v[3], uint32_t nu, uint32_t nv,
                 float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm, float** out_uv);
/* host only: w x h RGB8 -> w x h heights ((0.2126 r + 0.7152 g) + 0.0722 b) / 255, f64 rounded to f32 */
int pt_height_from_rgb8(uint32_t w, uint32_t h, const uint8_t* rgb, float* out);

/* ---- Loop subdivision surfaces: creases, corners, limit projection (not in the reference, opt-in) ----
 * A stage of its own in front of pt_mesh, and in front of pt_mesh_tessellate when displacement follows: a coarse control cage in, a
 * rounder fine mesh out. No render kernel knows of it. pt_mesh_subdivide runs on the GPU (csrc/pt_subdiv.hip), pt_mesh_subdivide_host
 * is its host twin; the two return the same bytes.
 * Input: f32 positions, u32 index triples, optional f32 texcoords indexed by the position index (brought to n = n_pos entries first:
 *  entries past n_pos dropped, missing ones zero), optional crease flags: n_idx bytes, crease[3f + k] != 0 marks edge k of face f as
 *  sharp, edges numbered as in section 27: e0 = (a, b), e1 = (b, c), e2 = (c, a). Flags are read as 0 or 1.
 * Arithmetic: f64 on the f32 values widened, in the order written here, no fused operation; each written vertex attribute is rounded to
 *  f32 once per level. sqrt is the IEEE operation. dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z. No trigonometry anywhere: the caller
 *  turns angles into cosines.
 * Topology of a level is section 27's: the same edge keys, the E distinct keys in ascending order, the midpoint of the key of rank r
 *  is vertex n + r, the same four children in the same order: n' = n + E, F' = 4F, and out_idx is what pt_mesh_tessellate writes.
 * An edge's run: the slots 3f + k that carry its key, in ascending order. An edge is sharp when its run's length is not 2 (boundary and
 *  non-manifold edges), or its endpoints are equal (a == b), or any slot of its run is flagged.
 * Creasing by angle, once, on the input mesh, before the first level (and before the limit projection when levels = 0): an edge of
 *  run length 2 with a != b, whose slots lie in the faces f0 and f1, c_i = (p1 - p0) x (p2 - p0) of face f_i (section 27's cross
 *  product): all of its slots are flagged when dot(c0, c1) < crease_cos * sqrt(dot(c0, c0) * dot(c1, c1)). False for NaN. Faces of
 *  opposed winding across an edge therefore read as a fold: that is data, not an error.
 * Child flags travel with the slots: with e_k = 1 when any slot of the run of the parent's edge k is flagged (the parent's own slot
 *  is one of them), else 0: child 4f = (a, ab, ca) has the flags (e0, 0, e2), 4f + 1 = (ab, b, bc) has (e0, e1, 0), 4f + 2 =
 *  (ca, bc, c) has (0, e1, e2), 4f + 3 = (ab, bc, ca) has (0, 0, 0). A crease flagged on one side only is then carried by both.
 * Odd vertices: the midpoint of key (A, B), A the smaller index: sharp edge: (A + B) * 0.5; otherwise (A + B) * 0.375 + (C + D) * 0.125
 *  with C, D the vertices opposite the edge in the first and the second slot of its run: for slot 3f + k that is idx[3f + (k + 2) % 3].
 * Neighbours of v: one entry per distinct key with a != b that contains v, in ascending order of the other endpoint's index; k is
 *  their number, s the number of them that are sharp. Self-edges give no neighbour.
 * Even vertices: k = 0: the vertex keeps its value. s >= 3: a corner, kept. s == 2, the sharp neighbours w0 < w1: d0 = P[w0] - P[v],
 *  d1 = P[w1] - P[v]; a corner, kept, when dot(d0, d1) > corner_cos * sqrt(dot(d0, d0) * dot(d1, d1)) (false for NaN); otherwise the
 *  crease rule P[v] * 0.75 + (P[w0] + P[w1]) * 0.125. s <= 1: Warren's weights: beta = 0.1875 for k == 3, else 0.375 / (double)k;
 *  S = 0, then S += P[w] over the neighbours in ascending order; the value is P[v] * (1.0 - (double)k * beta) + S * beta.
 *  All masks read the level's input values. Unreferenced vertices stay.
 * Texcoords go through the same masks (the same edge classes, the same w0, w1, k, beta) as positions; classification uses positions only.
 * Limit projection (limit = 1): once, after the last level, on the last mesh's own edges and flags, the same classification:
 *  s <= 1: chi = 0.2 for k == 3, else 0.5 / (double)k: P[v] * (1.0 - (double)k * chi) + S * chi; crease: P[v] * (2.0 / 3.0) +
 *  (P[w0] + P[w1]) * (1.0 / 6.0); corners and k = 0: kept. It reads the unprojected values and writes new ones; texcoords go with it.
 * Normals (`normals`): 0 smooth: section 27's smooth normals of the final positions, (0, 1, 0) where the sum is unusable; 1 none.
 * out_crease (when wanted): the flags of the output mesh, 0 or 1 per slot: subdividing the output again with them continues the same
 *  surface. With levels = 0 they are the input's flags after creasing by angle.
 * Refused with -1 before any device work: a NULL output pointer (out_crease alone may be NULL: not wanted) or a NULL array with a count
 *  above 0; n_idx % 3 != 0; an index out of range for positions or for given texcoords; levels > 12; 4^levels F > 0x07FFFFFF;
 *  n + (4^levels - 1) F > 2^32 - 1; crease_cos or corner_cos NaN; an unknown limit or normals value. NULL options mean the defaults.
 *  NaN and infinite coordinates are data. Outputs are malloc'd: free them with pt_free; *out_nrm / *out_uv are NULL where there is none.
 * Device memory, per level of F faces, n vertices and E edges: the two meshes (20 B a vertex with texcoords, 15 B a face, old and new),
 *  108 B a face of edge keys, slots, flags, ranks and midpoint indices, 48 B an edge of neighbour pairs, 2 B an edge of classes,
 *  4 B a vertex of run starts, and the radix sort's own buffer.
 * A mesh whose vertices are duplicated along texcoord seams (pt_load_obj_single_index) turns its seams into creases: boundary edges on
 *  both sides. They stay closed (both copies compute the same crease positions) but are visible. Welding is not done here. */
typedef struct pt_subdiv_opts {
    uint32_t levels;      /* 0..12. Default 1 */
    double crease_cos;    /* default -2: no edge is creased by angle */
    double corner_cos;    /* default  2: no vertex is a corner by angle */
    int limit;            /* 0 (default); 1: push the last level's vertices to their limit positions */
    int normals;          /* 0 smooth (default): the area-weighted rule of section 27 on the final positions; 1 none */
} pt_subdiv_opts;
int pt_subdiv_opts_default(pt_subdiv_opts*);
int pt_mesh_subdivide(pt_ctx*, const pt_subdiv_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                      uint32_t n_uv, const float* uv, const uint8_t* crease /* n_idx bytes or NULL */,
                      float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx,
                      float** out_nrm, float** out_uv, uint8_t** out_crease /* may be NULL: not wanted */);
int pt_mesh_subdivide_host(const pt_subdiv_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                           uint32_t n_uv, const float* uv, const uint8_t* crease,
                           float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx,
                           float** out_nrm, float** out_uv, uint8_t** out_crease);

/* ---- isosurface extraction: density grids and signed distance fields to meshes (not in the reference, opt-in) ----
 * A stage of its own in front of pt_mesh (and of pt_mesh_subdivide / pt_mesh_tessellate when rounding or displacement follows): a 3-D
 * grid of samples in, the triangle mesh of one of its level sets out. No render kernel knows of it. pt_mesh_isosurface runs on the GPU
 * (csrc/pt_iso.hip), pt_mesh_isosurface_host is its host twin; the two return the same bytes.
 * Arithmetic: f64 on the f32 samples widened, in the order written here, no fused operation; each written attribute is rounded to f32
 *  once. sqrt is the IEEE operation.
 * Grid: pt_mat_medium_grid's: values[(k ny + j) nx + i] is the sample at the centre of cell (i, j, k) of the box, so with
 *  h_a = (hi_a - lo_a) / (double)n_a the point of grid index i_a lies at lo_a + ((double)i_a + 0.5) * h_a per axis. A grid made for a
 *  medium meshes where the medium's density crosses `iso`.
 * Lattice: the sample centres. closed = 1 adds one layer on every side: grid indices -1 .. n_a per axis, the added points read
 *  `outside`, their positions continue the spacing ((double)(-1) + 0.5 = -0.5). NX x NY x NZ points, N_a = n_a + 2 closed; primed
 *  indices count from the first lattice layer; the linear index of a point is (k' NY + j') NX + i'.
 * A point is inside when its value >= iso.
 * Marching tetrahedra. A lattice cube is anchored at its corner of lowest indices (every point with i' < NX - 1, j' < NY - 1,
 *  k' < NZ - 1 anchors one; its linear index is the anchor's); its corners are numbered c = x + 2y + 4z. It is cut into the six
 *  tetrahedra of the Kuhn split around the diagonal 0-7, in this order, corners (v0, v1, v2, v3):
 *    0 (0,1,3,7)   1 (0,1,5,7)   2 (0,2,3,7)   3 (0,2,6,7)   4 (0,4,5,7)   5 (0,4,6,7)
 *  so neighbouring cubes agree on every face diagonal. Tetrahedra 0, 3 and 4 are positive (det(v1 - v0, v2 - v0, v3 - v0) = +1 in
 *  lattice coordinates), 1, 2 and 5 negative.
 * Edges: a lattice edge runs from point A to B = A + d, d one of the seven offsets with d = dx + 2dy + 4dz in 1..7 (axes, face
 *  diagonals, the cube diagonal): every edge of every tetrahedron is one, from the corner with the lower number. An edge crosses when
 *  exactly one endpoint is inside. The crossing edges in ascending order of (A's linear index, B's linear index), which for one A is
 *  ascending d: the edge of rank r gives vertex r, shared by every tetrahedron around it.
 * Vertex: a, b the values at A, B: t = (iso - a) / (b - a) (always from A), P = PA + (PB - PA) * t per component.
 * Triangles, in ascending order of (cube, tetrahedron 0..5, triangle 0..1). Case m of a tetrahedron: bit l set when v_l is inside. Its
 *  edges: 0 = (v0,v1) 1 = (v0,v2) 2 = (v0,v3) 3 = (v1,v2) 4 = (v1,v3) 5 = (v2,v3). One corner a alone on its side, the others b < c < d:
 *  the triangle of the edges (ab, ac, ad). Two inside a < b, two outside c < d: the quad (ac, ad, bd, bc) split by its diagonal ac-bd
 *  into (ac, ad, bd) and (ac, bd, bc). The second and third vertex are then swapped where needed so that, with lattice coordinates for
 *  the corners and edge midpoints for the vertices, (p1 - p0) x (p2 - p0) has a positive dot product with (mean of the outside corners -
 *  mean of the inside corners): normals point towards lower values. For a positive tetrahedron that gives, per case m = 0 .. 15:
 *    0000 -                 0001 (0,1,2)           0010 (0,4,3)           0011 (1,2,4) (1,4,3)
 *    0100 (1,3,5)           0101 (0,5,2) (0,3,5)   0110 (0,4,5) (0,5,1)   0111 (2,4,5)
 *    1000 (2,5,4)           1001 (0,1,5) (0,5,4)   1010 (0,5,3) (0,2,5)   1011 (1,5,3)
 *    1100 (1,3,4) (1,4,2)   1101 (0,3,4)           1110 (0,2,1)           1111 -
 *  (m written v3 v2 v1 v0); a negative tetrahedron swaps the second and third vertex of each triangle. A sample equal to iso makes
 *  several edges meet in one point (t = 0): the zero-area triangles that follow are data, as section 27 keeps a == b edges.
 * Normals (`normals`): 0 gradient: at a lattice point g_a = (v+ - v-) / (2.0 * h_a) per axis, v+ and v- the neighbours along the axis;
 *  where one of them is not in the lattice, the one-sided difference over h_a with the point's own value in its place. At a vertex
 *  G = gA + (gB - gA) * t per component, N = -G, L = sqrt((N.x N.x + N.y N.y) + N.z N.z); N / L when L is finite and > 0, else
 *  (0, 1, 0). 1 smooth: section 27's smooth normals of the finished mesh, (0, 1, 0) where the sum is unusable. 2 none: *out_nrm = NULL.
 * Refused with -1 before any device work: a NULL output pointer, values or box; some n_a < 2; nx ny nz > 2^28; more than 2^29 lattice
 *  points after padding (7 x points then fits 32 bits); a value, iso, outside or a box coordinate that is not finite; lo_a >= hi_a; an
 *  unknown closed or normals value. NULL options mean the defaults. Refused with -1 after the counting pass, with nothing held: more than
 *  0x07FFFFFF triangles (pt_mesh's cap). A grid with no crossing returns 0 and an empty mesh (counts 0). Outputs are malloc'd: free
 *  them with pt_free.
 * Device memory: 13 B a lattice point (the sample, the mask byte, the first vertex, the first triangle), the scan's own buffer, and the
 *  mesh: 12 B a vertex (24 with normals), 12 B a triangle; smooth normals add section 27's 28 B a corner. */
typedef struct pt_iso_opts {
    double iso;       /* the level. Default 0.5 */
    int closed;       /* 0 open (default): the surface ends at the hull of the sample centres; 1: one layer of samples of value
                         `outside` is added on every side, so the surface closes */
    float outside;    /* default 0 */
    int normals;      /* 0 gradient (default), 1 smooth (section 27's rule on the final mesh), 2 none */
} pt_iso_opts;
int pt_iso_opts_default(pt_iso_opts*);
int pt_mesh_isosurface(pt_ctx*, const pt_iso_opts*, uint32_t nx, uint32_t ny, uint32_t nz, const float* values,
                       const double box_lo[3], const double box_hi[3],
                       float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm);
int pt_mesh_isosurface_host(const pt_iso_opts*, uint32_t nx, uint32_t ny, uint32_t nz, const float* values,
                            const double box_lo[3], const double box_hi[3],
                            float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx, float** out_nrm);

/* ---- mesh voxelisation: signed distance, occupancy and density grids of a triangle mesh (not in the reference, opt-in) ----
 * The direction isosurface extraction lacks: a triangle mesh in, a 3-D grid of samples out, in the layout pt_mat_medium_grid and
 * pt_mesh_isosurface read. No render kernel knows of it. pt_mesh_sdf runs on the GPU (csrc/pt_sdf.hip), pt_mesh_sdf_host is its host
 * twin; the two write the same bytes. out_values is the caller's: nx ny nz floats.
 * Arithmetic: f64 on the f32 positions widened, in the order written here, no fused operation; sqrt is the IEEE operation; each output
 *  is rounded to f32 once.
 * Grid: values[(k ny + j) nx + i] is the sample at the centre of cell (i, j, k): x_i = lo_x + ((double)i + 0.5) * h_x, with
 *  h_a = (hi_a - lo_a) / (double)n_a, and so for y_j, z_k.
 * POSITIVE INSIDE is the default: depth = +d inside, -d outside. With pt_mesh_isosurface (inside: value >= iso, normals towards lower
 *  values) iso = 0 gives outward normals, iso = -r grows the body by r, iso = +r shrinks it, and a density is the depth clamped.
 * Sign (skipped for what = 1). The winding number of a sample is the signed count of the surface's crossings of the ray from the sample
 *  towards +x, taken per column (j, k) so that it is an integer and watertight. P = (y_j, z_k). A triangle (A, B, C) is projected to the
 *  (y, z) plane; only a column with min(A.y, B.y, C.y) <= P.y <= max(..) and the same in z (exact comparisons) can cross it. For each
 *  directed edge U -> V of (A -> B, B -> C, C -> A):
 *   1. if (V.y, V.z) < (U.y, U.z) lexicographically, swap U and V and remember `swapped`;
 *   2. dy = V.y - U.y, dz = V.z - U.z, e = dy * (P.z - U.z) - dz * (P.y - U.y);
 *   3. s = +1 when e > 0, or when e == 0 and (dz < 0, or dz == 0 and dy > 0); else s = -1. The tie is P moved by (+eps, +eps^2); an
 *      edge that projects to a point (dy == dz == 0) gets -1;
 *   4. the directed edge's side is swapped ? -s : s, its value swapped ? -e : e.
 *  The two triangles on an edge evaluate the same bits, so exactly one of them owns a column that lies on it. The column crosses the
 *  triangle when the three sides are equal; that value o is the crossing's orientation (+1: the projection is counter-clockwise, the
 *  normal has +x, the ray leaves the body). With wa, wb, wc the directed values of B -> C, C -> A, A -> B:
 *   x* = ((wa * A.x + wb * B.x) + wc * C.x) / ((wa + wb) + wc); a crossing with a zero denominator or a non-finite x* is dropped;
 *   m = the number of i in 0 .. nx - 1 with x_i < x* (by the x_i formula, not a rounded division); the crossing adds o to the winding of
 *   every sample i < m of the column. A sample is inside when its winding is non-zero (fill = 0) or odd (fill = 1).
 *  A degenerate projection never has three equal sides with a non-zero denominator. An open mesh (assets/bunny.obj has 42 boundary
 *  edges) gets a sign that is defined but not meaningful: use what = 1. A face that lies exactly on sample centres makes the body
 *  half-open there: an axis-aligned cube [c0, c1]^3 on sample centres is inside on [c0, c1) per axis.
 * Distance (skipped for what = 2). A triangle with a repeated index, or with n.n == 0 for ab = B - A, ac = C - A (per component, f64),
 *  n = (ab.y ac.z - ab.z ac.y, ab.z ac.x - ab.x ac.z, ab.x ac.y - ab.y ac.x), is dropped from this pass; dot(u, v) =
 *  (u.x v.x + u.y v.y) + u.z v.z throughout. D = the minimum over the other triangles of the squared distance from the sample centre
 *  P to the triangle, by the Voronoi region of the closest point, the first that applies:
 *   ap = P - A; d1 = dot(ab, ap); d2 = dot(ac, ap);               d1 <= 0 and d2 <= 0: dot(ap, ap)                      (vertex A)
 *   bp = ap - ab; d3 = dot(ab, bp); d4 = dot(ac, bp);             d3 >= 0 and d4 <= d3: dot(bp, bp)                     (vertex B)
 *   vc = d1 * d4 - d3 * d2;          vc <= 0, d1 >= 0, d3 <= 0: v = d1 / (d1 - d3), q = ap - ab * v, dot(q, q)          (edge AB)
 *   cp = ap - ac; d5 = dot(ab, cp); d6 = dot(ac, cp);             d6 >= 0 and d5 <= d6: dot(cp, cp)                     (vertex C)
 *   vb = d5 * d2 - d1 * d6;          vb <= 0, d2 >= 0, d6 <= 0: w = d2 / (d2 - d6), q = ap - ac * w, dot(q, q)          (edge AC)
 *   va = d3 * d6 - d5 * d4;          va <= 0, d4 - d3 >= 0, d5 - d6 >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),
 *                                                                         q = bp - (ac - ab) * w, dot(q, q)             (edge BC)
 *   else den = (va + vb) + vc; v = vb / den; w = vc / den; q = ap - (ab * v + ac * w), dot(q, q)                        (the face)
 *  (vector operations per component). The minimum of f64 values does not depend on the order of the triangles, nor on leaving out
 *  triangles that cannot hold it: the GPU stage culls, the twin does not cull by brick, and the bytes are the same.
 * Outputs: d = sqrt(D), and d = band where band > 0 and not d < band; depth = inside ? d : -d. what = 0: (float)depth, (float)(-depth)
 *  with negate; what = 1: (float)d; what = 2: 1.0f inside, 0.0f outside; what = 3: (float)(min(d, ramp) / ramp) inside, 0.0f outside.
 * Refused with -1, nothing written, before any device work: a NULL pointer (NULL options mean the defaults); n_idx that is 0 or not a
 *  multiple of 3; more than 0x07FFFFFF triangles; an index >= n_pos; a position or box coordinate that is not finite; lo_a >= hi_a; some
 *  n_a < 2; nx ny nz > 2^28; an unknown what or fill; a band that is negative or not finite; what = 3 with a ramp that is not finite or
 *  not > 0; for what != 2, no triangle left after the degenerate ones are dropped.
 * Limits: coordinates whose products overflow or underflow f64 are the caller's problem (f32 positions and a box of their size never do).
 * Device memory: 96 B a triangle (the 72-B record A, ab, ac and the 24-B f32 box), 4 B x (nx + 1) ny nz for the deltas, which the inside
 *  flags then replace, 4 B a sample for the output, and the mesh as uploaded (12 B a position, 4 B an index).
 * pt_mesh_fit_grid (host only) gives cubic cells around a mesh: lo_a / hi_a the bounds of the positions (widened to f64),
 *  ext_a = hi_a - lo_a, E = the largest ext_a, h = E / ((double)n_longest - 2.0 * margin_cells),
 *  n_a = max(2, ceil(ext_a / h + 2.0 * margin_cells)), c_a = lo_a + 0.5 * ext_a, half_a = 0.5 * ((double)n_a * h),
 *  out_lo_a = c_a - half_a, out_hi_a = c_a + half_a. Refused with -1: a NULL pointer, no positions, a position that is not finite, a
 *  margin that is negative or not finite, n_longest <= 2 margin_cells + 1, E == 0, nx ny nz > 2^28. */
typedef struct pt_sdf_opts {
    int what;      /* 0 depth: signed distance, POSITIVE INSIDE (default); 1 distance (unsigned; no sign pass, open meshes welcome);
                      2 occupancy: 1.0f inside, 0.0f outside (no distance pass); 3 density: a ramp for pt_mat_medium_grid */
    int fill;      /* which winding numbers are inside: 0 non-zero (default), 1 odd */
    int negate;    /* what = 0 only: 1 writes -depth (the usual "negative inside" convention) */
    double band;   /* > 0: distances are capped at band (what 0, 1); 0 (default): exact everywhere */
    double ramp;   /* what = 3: density = min(d, ramp) / ramp inside, 0 outside; must be given, > 0 (no default) */
} pt_sdf_opts;
int pt_sdf_opts_default(pt_sdf_opts*);
int pt_mesh_sdf(pt_ctx*, const pt_sdf_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                uint32_t nx, uint32_t ny, uint32_t nz, const double box_lo[3], const double box_hi[3], float* out_values);
int pt_mesh_sdf_host(const pt_sdf_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                     uint32_t nx, uint32_t ny, uint32_t nz, const double box_lo[3], const double box_hi[3], float* out_values);
int pt_mesh_fit_grid(uint32_t n_pos, const float* pos, uint32_t n_longest, double margin_cells,
                     uint32_t out_dims[3], double out_lo[3], double out_hi[3]);

/* ---- mesh welding and simplification: quadric vertex clustering (not in the reference, opt-in) ----
 * The stage that makes a mesh smaller, and the welding sections 27 and 28 leave out: vertices are grouped (by equal position, or by
 * the cubic cell they lie in), each group becomes one vertex, faces that lose a corner go. A stage of its own in front of pt_mesh,
 * pt_mesh_subdivide, pt_mesh_tessellate and pt_mesh_sdf; no render kernel knows of it. pt_mesh_simplify runs on the GPU
 * (csrc/pt_simplify.hip), pt_mesh_simplify_host is its host twin; the two return the same bytes.
 * Input: f32 positions, u32 index triples, optional f32 texcoords indexed by the position index (brought to n = n_pos entries first:
 *  entries past n_pos dropped, missing ones zero).
 * Arithmetic: f64 on the f32 values widened, in the order written here, no fused operation; each written attribute is rounded to f32
 *  once. floor is the IEEE operation; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z and the cross product are section 27's.
 * TSUM(t_0 .. t_{L-1}), L >= 1, the only summation order used: tile j holds t_{16j} .. t_{16j+15}, missing entries read +0.0. A tile's
 *  value is the balanced pairwise tree s0_i = t_i, s(l+1)_i = s(l)_{2i} + s(l)_{2i+1}, l = 0 .. 3, taken at s4_0. TSUM is tile 0's
 *  value, then += tile 1's, tile 2's, ... in order. (Sixteen lanes take a tile in four xor-butterfly steps: f64 addition is
 *  commutative bit for bit. A run of L terms then costs L / 16 sequential additions.)
 * 1. Referenced vertices: only vertices some index names take part; the others are ignored and dropped.
 * 2. Keys. mode 0 (weld): two vertices are equal when their three components compare equal as floats (-0 equals +0). mode 1
 *  (cluster): lo_a = the minimum of the referenced positions per axis, hi_a the maximum, ext_a = hi_a - lo_a, E the largest ext_a;
 *  cell = `cell` when that is > 0, else E / (double)grid_n; c_a = floor(((double)p_a - lo_a) / cell); two vertices are equal when
 *  their (c_x, c_y, c_z) are (key = (c_z << 42) | (c_y << 21) | c_x).
 * 3. Clusters: a cluster is the set of referenced vertices of one key, its members in ascending vertex index, its head the lowest
 *  member. Cluster ids ascend with the head's vertex index. Welding an already welded, fully referenced mesh is the identity.
 * 4. Triangles: face (a, b, c) maps to the cluster ids (A, B, C), rotation kept; it is dropped when two ids are equal. With `dedup`
 *  the surviving faces are grouped by vertex set {A, B, C}. In a group, in ascending face index, e faces are even permutations of the
 *  sorted triple and o are odd: e > o: the first e - o even faces survive; o > e: the first o - e odd faces; e = o: none. Survivors
 *  are written in ascending input face index. Every directed edge of the output is then as often used as its reverse when that held
 *  for the input: a closed input gives a closed output with the same winding numbers. It need NOT be manifold: a thin wall that
 *  collapses into one layer of cells cancels, a handle narrower than a cell pinches into a shared edge or vertex.
 * 5. Output vertices: the clusters a surviving face names, in cluster-id order. out_map[v] (when wanted; n_pos entries) is the output
 *  vertex of input vertex v, 0xFFFFFFFF for an unreferenced vertex and for one whose cluster was dropped.
 * 6. Placement. mode 0: the head's position bits and the head's texcoord. mode 1, per cluster of `count` members:
 *  o_a = lo_a + ((double)c_a + 0.5) * cell; m_a = TSUM over the members of ((double)p_a - o_a) / (double)count; texcoord: per
 *  component (float)(TSUM over the members / (double)count). placement 1 (mean): x = m. placement 0 (quadric): the cluster's corners
 *  are the slots 3f + k of the input index array that name a member, in ascending order (a face with two corners in the cluster counts
 *  twice; dropped faces count). Each corner gives nine terms from face f's vertices in index order, o subtracted from each
 *  (p' = (double)p - o per component): e1 = p1' - p0', e2 = p2' - p0', n = e1 x e2, d = dot(n, p0'); the terms n.x n.x, n.x n.y,
 *  n.x n.z, n.y n.y, n.y n.z, n.z n.z, n.x d, n.y d, n.z d. The TSUM of each over the corners: a00 a01 a02 a11 a12 a22 b0 b1 b2.
 *  T = (a00 + a11) + a22; T not finite or not > 0: x = m. Otherwise lambda = reg * T; a00, a11, a22 each + lambda;
 *  r_a = b_a + lambda * m_a;
 *   c00 = a11 a22 - a12 a12   c01 = a02 a12 - a01 a22   c02 = a01 a12 - a02 a11
 *   c11 = a00 a22 - a02 a02   c12 = a01 a02 - a00 a12   c22 = a00 a11 - a01 a01
 *   det = (a00 c00 + a01 c01) + a02 c02
 *   x0 = ((c00 r0 + c01 r1) + c02 r2) / det   x1 = ((c01 r0 + c11 r1) + c12 r2) / det   x2 = ((c02 r0 + c12 r1) + c22 r2) / det
 *  accepted when det > 0, every x_a is finite and |x_a| <= cell (the optimum may leave its cell by half a cell); otherwise x = m.
 *  Position = (float)(o_a + x_a). reg is bounded because Cramer's rule in f64 loses the in-plane block of a flat cluster below about 1e-8.
 * Normals (`normals`): 0 smooth: section 27's smooth normals of the result, (0, 1, 0) where the sum is unusable; 1 none.
 * Refused with -1 before any device work: a NULL output pointer (out_map alone may be NULL: not wanted) or a NULL array with a count
 *  above 0; n_idx that is 0 or not a multiple of 3; more than 0x07FFFFFF faces; an index out of range for positions or for given
 *  texcoords; a position that is not finite (texcoords are data); an unknown mode, placement, dedup or normals value; mode 1 with a
 *  cell that is negative or not finite, with cell == 0 and grid_n == 0, with E == 0, with floor(ext_a / cell) >= 2^21 on some axis,
 *  or with reg outside [1e-6, 1] or NaN. NULL options mean the defaults. pt_mesh_simplify alone also refuses n_pos above 2^31 - 2
 *  (its sorts count in 31 bits). A mesh that collapses entirely returns 0 and an empty mesh (counts 0). Outputs are malloc'd: free
 *  them with pt_free; *out_nrm / *out_uv are NULL where there is none. A failed device allocation returns -1 with nothing held.
 * Device memory: the mesh as uploaded (12 B a vertex, 8 more with texcoords, 12 B a face); 48 B a vertex of flags, keys, sorted
 *  vertices, ranks and cluster ids (mode 0: 12 more during its first sort); quadric placement 48 B a face of (cluster, corner) pairs;
 *  8 B a face of survivor flags and ranks, with dedup 45 B a face more of group keys and sorted faces; 32 B a cluster (40 with
 *  texcoords); the result, section 27's 28 B a corner of it for smooth normals, and the radix sorts' own buffers. */
typedef struct pt_simplify_opts {
    int mode;          /* 0 weld: merge vertices of equal position; 1 cluster (default) */
    double cell;       /* mode 1: edge of the cubic cells; > 0 wins over grid_n. Default 0 */
    uint32_t grid_n;   /* mode 1, cell == 0: cell = E / (double)grid_n, E the longest extent. Default 64 */
    int placement;     /* mode 1: 0 quadric (default), 1 mean */
    double reg;        /* quadric: Tikhonov weight towards the mean, in [1e-6, 1]. Default 1e-3 */
    int dedup;         /* 1 (default): coincident triangles cancel by orientation; 0: only degenerate ones go */
    int normals;       /* 0 smooth (section 27's rule on the result, (0, 1, 0) where unusable; default), 1 none */
} pt_simplify_opts;
int pt_simplify_opts_default(pt_simplify_opts*);
int pt_mesh_simplify(pt_ctx*, const pt_simplify_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                     uint32_t n_uv, const float* uv,
                     float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx,
                     float** out_nrm, float** out_uv, uint32_t** out_map /* may be NULL: not wanted */);
int pt_mesh_simplify_host(const pt_simplify_opts*, uint32_t n_pos, const float* pos, uint32_t n_idx, const uint32_t* idx,
                          uint32_t n_uv, const float* uv,
                          float** out_pos, uint32_t* out_n_pos, uint32_t** out_idx, uint32_t* out_n_idx,
                          float** out_nrm, float** out_uv, uint32_t** out_map);

/* ---- multi-GPU: one process per GPU, spp sharding, ONE RCCL reduce over xGMI --------------------------------------
 * The reference is a single process (rayon over pixels, camera.rs:102); samples of a pixel are only summed
 * (camera.rs:106-108), so rank r of N renders the sample range pt_shard_range(spp, r, N) of every pixel and one
 * ncclReduce(sum, f64, root 0) of the W*H*3 sample SUMS lands the frame on rank 0. RCCL is called directly from
 * /opt/rocm on the device accumulator, on the render stream: no torch, no host bounce. */
typedef struct pt_comm pt_comm;       /* one rank of an RCCL communicator, bound to a pt_ctx's device and stream */
void pt_shard_range(uint32_t spp, int rank, int world, uint32_t* lo, uint32_t* hi);   /* contiguous, disjoint, near-equal */
/* Rendezvous of the `world` processes of one launch (rank / world as torchrun's RANK / WORLD_SIZE): rank 0 creates the
 * RCCL unique id and publishes it in the file `id_path` (any path all ranks agree on and no earlier launch used), the
 * others wait for it up to timeout_s (<= 0: 120 s); then ncclCommInitRank. world == 1 needs no file. */
int pt_comm_create(pt_ctx*, int rank, int world, const char* id_path, double timeout_s, pt_comm** out);
void pt_comm_destroy(pt_comm*);
int pt_comm_rank(pt_comm*);
int pt_comm_world(pt_comm*);
int pt_comm_barrier(pt_comm*);        /* all ranks have arrived and every device is idle */
int pt_comm_allreduce_f64(pt_comm*, double* host_values, uint32_t n /* <= 64 */, int op /* 0 sum, 1 max */);
int pt_bootstrap_exchange(const char* path, int rank, void* bytes, uint32_t n, double timeout_s);   /* the file rendezvous itself (host only) */
/* Camera::render on all ranks of the communicator: samples [0, spp_total) split by pt_shard_range, rendered into a
 * device accumulator, reduced onto rank 0 and ADDED there to accum_root (host, W*H*3 sums; ignored on other ranks;
 * opts->overwrite: stored instead of added). stats are this rank's. A failure on any rank is agreed on before the
 * reduce is posted: every rank returns -1 and no rank waits; a failure inside a collective aborts the communicator. */
int pt_render_multi(pt_scene*, const pt_camera*, uint64_t seed, uint32_t spp_total, pt_comm*, double* accum_root,
                    const pt_render_opts* opts, pt_render_stats* stats);

/* ---- parity probes (tests only) ---------------------------------------------------------- */
/* closest hit of n rays {o.xyz, d.xyz, time} against the built world (World::intersect_all,
 * world.rs:47-62, ray_t = [1e-3, inf)); out[15*i] = {hit, t, prim_id, u, v, front_face,
 * point.xyz, geometric_normal.xyz, shading_normal.xyz} */
int pt_intersect(pt_scene*, const double* rays, uint32_t n, double* out);
/* elementwise device arithmetic: which = 0 sqrt(a) 1 a/b 2 a*b+a 3 sin 4 cos 5 acos 6 atan2(a,b)
 * 7 pow(a,b) 8 log2 9 rng uniform(seed=a, pixel=b, sample=7, draw=i); in = n pairs (a,b) */
int pt_math_probe(pt_ctx*, int which, const double* in, uint32_t n, double* out);
/* the device functions of environment sampling that k_shade calls (pt_scene_set_env_sampling's rule): which = 0: in = n pairs
 * (u1, u2), out = n x {dir.xyz, pdf}; which = 1: in = n directions xyz, out = n env_pdf values. Builds the scene's tables if
 * needed (the world must be built). -1 when the camera's environment is not a map or its Z is 0. */
int pt_env_probe(pt_scene*, const pt_camera*, int which, const double* in, uint32_t n, double* out);
/* the samplers' draw functions as the kernels call them (pt_scene_set_sampler's rule): out[i * n_draws + j] = the 64-bit value of
 * the single draw draw_begin + j (no two-value alignment) of sample sample_begin + i of `pixel` under `seed`; kind as there
 * (0: the Philox values). At most 2^28 values a call. */
int pt_sampler_probe(pt_ctx*, int kind, uint64_t seed, uint32_t pixel, uint32_t sample_begin, uint32_t n_samples, uint32_t draw_begin,
                     uint32_t n_draws, uint64_t* out);

/* the device functions of participating media that k_shade calls (pt_mat_medium's rule), for medium material `mat`:
 * which = 0: in = n x (u1, u2, dir.xyz), out = n x (w.xyz, ph(dot(dir, w))); which = 1: in = n x u, out = n free-flight distances.
 * For a grid medium (pt_mat_medium_grid's rule; -1 for a medium without a grid): which = 2: in = n points xyz, out = n sigma values;
 * which = 3: in = n x (o.xyz, dir.xyz, t), |dir| <= 1 (else -1); row i is tracked with the independent sampler's draws of (seed 0,
 * pixel i, sample 0) from draw 0; out = n x (collided 0 / 1, s or 0, draws consumed). which = 4 (any medium; pt_mat_medium_tinted's
 * rule): in = n segment lengths, out = n x 3 factors exp(-(a_c * l)), exactly 1 where a_c == 0. The world need not be built. */
int pt_medium_probe(pt_scene*, int mat, int which, const double* in, uint32_t n, double* out);
/* lights.sample / lights.pdf as k_shade calls them, of the scene's current light-sampling kind (pt_scene_set_light_sampling's rule).
 * The world must be built; -1 without a lights list. which = 0: in = n x (origin.xyz, time); row i runs lights.sample with the
 * independent sampler's draws of (seed 0, pixel i, sample 0) from draw 0; out = n x (dir.xyz, light index, face index or -1 for a
 * non-mesh entry (and always under kind 0), draws consumed). which = 1: in = n x (origin.xyz, direction.xyz, time), out = n
 * lights.pdf values. */
int pt_light_probe(pt_scene*, int which, const double* in, uint32_t n, double* out);
/* the device functions of dispersion that k_shade calls (pt_mat_glass_set_dispersion's rule), for dispersive glass `glass_mat` (-1 when it
 * is not one), under the scene's current sampler kind. which = 0: in = n x (pixel, sample) as doubles (32-bit unsigned integers), out =
 * n x (u, lambda, j, W_r, W_g, W_b, n(lambda)) of a path of `seed`; which = 1: in = n wavelengths in nm, out = n values n(lambda).
 * The world need not be built. */
int pt_dispersion_probe(pt_scene*, int glass_mat, int which, uint64_t seed, const double* in, uint32_t n, double* out);
/* generate_ray as k_init calls it, under the scene's projection (pt_scene_set_projection's rule) and sampler: in = n x (pixel, sample) as
 * doubles (pixel < W * H, sample a 32-bit unsigned integer, else -1); out = n x (origin.xyz, direction.xyz, time, draws consumed) of the
 * sample's stream of `seed` from draw 0. The camera's refusals are the renders'. The world need not be built (time is then drawn). */
int pt_camera_probe(pt_scene*, const pt_camera*, uint64_t seed, const double* in, uint32_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif
