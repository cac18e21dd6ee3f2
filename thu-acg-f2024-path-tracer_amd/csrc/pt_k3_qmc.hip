// The Sobol sampler's forms of K1 / K3 (unit_forms<UNIT_QMC>: the plain and ENV modes with QMC), k_aov_qmc and the sampler probe.
#include "pt_forms.h"
#include "pt_k_trace.h"

namespace pt {

__global__ __launch_bounds__(BLOCK) void k_aov_qmc(SceneD sc, CamD cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov, uint32_t overwrite) {
    aov_pixels<true>(sc, cam, seed, spp_begin, spp_end, aov, overwrite);
}
// pt_sampler_probe: out[i * n_draws + j] = the single draw (no two-value alignment) sample_begin + i, draw_begin + j of `pixel` — the
// draw functions K1 / K3 call
template <class R>
__global__ __launch_bounds__(BLOCK) void k_sampler_probe(uint64_t seed, uint32_t pixel, uint32_t sample_begin, uint32_t n_samples, uint32_t draw_begin, uint32_t n_draws,
                                                         unsigned long long* out) {
    const unsigned long long n = (unsigned long long)n_samples * n_draws;
    for (unsigned long long i = blockIdx.x * (unsigned long long)BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK) {
        R g{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample_begin + (uint32_t)(i / n_draws), draw_begin + (uint32_t)(i % n_draws)};
        out[i] = rng_u64(g);
    }
}
void launch_sampler_probe(int kind, uint64_t seed, uint32_t pixel, uint32_t sample_begin, uint32_t n_samples, uint32_t draw_begin, uint32_t n_draws, uint64_t* out,
                          hipStream_t st) {
    const unsigned long long n = (unsigned long long)n_samples * n_draws;
    const dim3 grid = grid_for((uint32_t)(n > 0xFFFFFF00ull ? 0xFFFFFF00ull : n), 2048);
    if (kind == 1) hipLaunchKernelGGL(k_sampler_probe<RngQ>, grid, dim3(BLOCK), 0, st, seed, pixel, sample_begin, n_samples, draw_begin, n_draws, (unsigned long long*)out);
    else hipLaunchKernelGGL(k_sampler_probe<Rng>, grid, dim3(BLOCK), 0, st, seed, pixel, sample_begin, n_samples, draw_begin, n_draws, (unsigned long long*)out);
}

FormKernels forms_qmc(const ShadeForm& f) { return unit_forms<UNIT_QMC>(f, k_aov_qmc); }

}  // namespace pt
