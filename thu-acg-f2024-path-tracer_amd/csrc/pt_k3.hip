// K1 / K3 forms of the plain and ENV modes without the Sobol sampler (unit_forms<UNIT_PLAIN>: k_init<LIST>, k_shade's shapes x LIGHTS and the
// LIST / ENV forms of the default shapes), k_probe, k_aov, and the launchers of K1, K3 and the AOV walk, which pick a form's kernel from the unit that owns it.
#include "pt_forms.h"
#include "pt_k_trace.h"

namespace pt {

// Debug/parity probe: closest hit + reconstructed HitInfo for a batch of arbitrary rays.
// out[15*i..] = {hit, t, prim_id, u, v, front, p.xyz, gn.xyz, sn.xyz}
// MOT: the scene has moving instances (SceneD::inst_motion): every instance is posed at the ray's time, taken as given (no shutter)
template <bool MOT>
__global__ __launch_bounds__(BLOCK) void k_probe(SceneD sc, const double* rays /* o.xyz d.xyz time */, uint32_t n, double* out) {
    __shared__ uint32_t stack[TRAVERSAL_STACK * BLOCK];
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const double* q = rays + 7 * (size_t)i;
        RayD r = make_ray(V3{q[0], q[1], q[2]}, V3{q[3], q[4], q[5]}, q[6]);
        Closest c = closest_hit<MOT>(sc, r, 1e-3, &stack[threadIdx.x]);
        double* o = out + 15 * (size_t)i;
        for (int j = 0; j < 15; ++j) o[j] = 0.0;
        HitD h;
        if (c.id != HIT_NONE && reconstruct_hit<true, MOT>(sc, r, c.id, 1e-3, h)) {
            o[0] = 1.0; o[1] = c.t; o[2] = (double)c.id; o[3] = h.u; o[4] = h.v; o[5] = h.front ? 1.0 : 0.0;
            o[6] = h.point.x; o[7] = h.point.y; o[8] = h.point.z;
            o[9] = h.gn.x; o[10] = h.gn.y; o[11] = h.gn.z;
            o[12] = h.sn.x; o[13] = h.sn.y; o[14] = h.sn.z;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_aov(SceneD sc, CamD cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov, uint32_t overwrite) {
    aov_pixels<false>(sc, cam, seed, spp_begin, spp_end, aov, overwrite);
}

FormKernels forms_plain(const ShadeForm& f) { return unit_forms<UNIT_PLAIN>(f, k_aov); }
static FormKernels form_kernels(const ShadeForm& f) {   // asks the unit that owns the form's k_shade, and the one that owns its k_init (pt_forms.h)
    constexpr FormKernels (*unit[])(const ShadeForm&) = {forms_plain, forms_qmc, forms_med, forms_het, forms_int, forms_lse, forms_dsp, forms_mot, forms_plt, forms_shf};   // in FormUnit's order
    const FormUnit k3 = form_unit(f.mode, f.qmc, f.motion, f.punctual), k1 = form_unit(mode_has_media(f.mode) ? MODE_MED : MODE_PLAIN, f.qmc, f.motion);   // K1 has a plain, a MED and a MOT form only
    FormKernels k = unit[k3](f);
    if (k1 != k3) k.init = k.shade ? unit[k1](f).init : nullptr;
    return k;
}

ShadeForm shade_form(ShadeForm f) {
    if (!shade_form_exists(SHADE_SHAPES[shade_row(f.variant)], f.lights, f.list, f.qmc, f.mode, f.motion, f.punctual)) f.variant = 42;
    return f;
}
bool shade_form_sorts(const ShadeForm& f) { return SHADE_SHAPES[shade_row(f.variant)].sort; }
bool shade_form_maps_tiles(const ShadeForm& f) { return sky_pass_form(f.list, f.mode, f.qmc, f.motion || f.punctual, SHADE_SHAPES[shade_row(f.variant)].minw == 2); }

bool launch_init(const CamD& cam, const PoolD& pool, uint64_t seed, int max_blocks, hipStream_t st, const ShadeForm& form) {
    const init_fn k = form_kernels(form).init;
    if (k) hipLaunchKernelGGL(k, grid_for(pool.n_alloc, max_blocks), dim3(BLOCK), 0, st, cam, pool, seed);
    return k != nullptr;
}
bool launch_shade(const SceneD& sc, const CamD& cam, const PoolD& pool, CountersD* cnt, uint64_t seed, int max_blocks, const ShadeForm& form, hipStream_t st,
                  uint32_t wide_window_min, const EnvTabD* env) {
    ShadeForm f = form;
    // 42: 8192-slot windows while the pool holds at least PT_WIDE_WINDOW_MIN of them per block launched, 4096-slot windows below
    // (a thinner pool — smaller frames, one rank's share, the frame's end after compaction — levels its end better with more, smaller windows)
    if (f.variant == 42) f.variant = pool.n_alloc / 8192u >= (uint32_t)max_blocks * (wide_window_min ? wide_window_min : 1u) ? 32 : 22;
    const ShadeShape sh = SHADE_SHAPES[shade_row(f.variant)];
    const uint32_t blocks = clamp_blocks(sh.sort ? pool.n_alloc / (uint32_t)(sh.kb * sh.per) : (pool.n_alloc + (uint32_t)sh.kb - 1u) / (uint32_t)sh.kb, max_blocks);   // one block per window / chunk
    const shade_fn k = form_kernels(f).shade;
    if (k) hipLaunchKernelGGL(k, dim3(blocks), dim3((uint32_t)sh.kb), 0, st, sc, cam, pool, cnt, seed, env ? *env : EnvTabD{});
    return k != nullptr;
}
int shade_occupancy_blocks(const ShadeForm& f) {
    const shade_fn k = form_kernels(f).shade;
    return k ? occupancy_blocks((const void*)k, SHADE_SHAPES[shade_row(f.variant)].kb) : 0;
}
void launch_probe(const SceneD& sc, const double* rays, uint32_t n, double* out, hipStream_t st) {
    if (sc.inst_motion) hipLaunchKernelGGL(k_probe<true>, grid_for(n, 2048), dim3(BLOCK), 0, st, sc, rays, n, out);
    else hipLaunchKernelGGL(k_probe<false>, grid_for(n, 2048), dim3(BLOCK), 0, st, sc, rays, n, out);
}
bool launch_aov(const SceneD& sc, const CamD& cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov, bool overwrite, int max_blocks,
                hipStream_t st, const ShadeForm& form) {
    const aov_fn k = form_kernels(form).aov;
    if (k) hipLaunchKernelGGL(k, grid_for(cam.width * cam.height, max_blocks), dim3(BLOCK), 0, st, sc, cam, seed, spp_begin, spp_end, aov, overwrite ? 1u : 0u);
    return k != nullptr;
}

}  // namespace pt
