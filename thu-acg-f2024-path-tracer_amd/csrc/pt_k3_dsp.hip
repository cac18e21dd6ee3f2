// The spectral-dispersion forms of K3 (unit_forms<UNIT_DSP>: the mode DSP, with or without LIGHTS, LIST and QMC)
// and the dispersion probe.
#include "pt_forms.h"

namespace pt {

// pt_dispersion_probe: the wavelength, its bin and weights and the Cauchy index as shade_slot's DSP forms compute them
template <bool QMC>
__global__ __launch_bounds__(BLOCK) void k_dispersion_probe(int which, uint64_t seed, double n_d, double b, double inv2_d, const double* w, const double* in, uint32_t n, double* out) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        if (which == 0) {
            const WavelengthD wl = dsp_wavelength<QMC>((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)in[2 * (size_t)i], (uint32_t)in[2 * (size_t)i + 1]);
            const double* row = w + 3u * wl.bin;
            double* o = out + 7 * (size_t)i;
            o[0] = wl.u; o[1] = wl.lambda; o[2] = (double)wl.bin; o[3] = row[0]; o[4] = row[1]; o[5] = row[2];
            o[6] = dsp_ior(n_d, b, inv2_d, wl.lambda);
        } else {
            out[i] = dsp_ior(n_d, b, inv2_d, in[i]);
        }
    }
}
void launch_dispersion_probe(int kind, int which, uint64_t seed, double n_d, double b, double inv2_d, const double* w, const double* in, uint32_t n, double* out, hipStream_t st) {
    if (kind == 1) hipLaunchKernelGGL(k_dispersion_probe<true>, grid_for(n, 2048), dim3(BLOCK), 0, st, which, seed, n_d, b, inv2_d, w, in, n, out);
    else hipLaunchKernelGGL(k_dispersion_probe<false>, grid_for(n, 2048), dim3(BLOCK), 0, st, which, seed, n_d, b, inv2_d, w, in, n, out);
}

FormKernels forms_dsp(const ShadeForm& f) { return unit_forms<UNIT_DSP>(f, nullptr); }

}  // namespace pt
