// The PLT forms of K3 (unit_forms<UNIT_PLT>: punctual lights in effect — point, spot and directional lights; plain mode, the default
// variant's shapes x LIGHTS x LIST x QMC) and the punctual probe. K1 and the AOV walk have no PLT form: the lights change no camera ray and no first hit.
#include "pt_forms.h"

namespace pt {

// pt_punctual_probe: the punctual branch's index draw and light evaluation as shade_slot makes them
__global__ __launch_bounds__(BLOCK) void k_punctual_probe(SceneD sc, int which, const double* in, uint32_t n, double* out) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        if (which == 0) {
            const double* q = in + 3 * (size_t)i;
            Rng rng{0u, 0u, i, 0u, 0u};
            const uint32_t k = rng_index(rng, sc.n_punctual) & PLT_INDEX_MASK;
            const PunctualEval e = punctual_eval(sc.punctual[k], q);
            double* o = out + 9 * (size_t)i;
            o[0] = (double)k; o[1] = e.w[0]; o[2] = e.w[1]; o[3] = e.w[2]; o[4] = e.D; o[5] = e.E[0]; o[6] = e.E[1]; o[7] = e.E[2]; o[8] = (double)rng.draw;
        } else {
            const double* q = in + 4 * (size_t)i;
            const uint32_t k = (uint32_t)q[0];                        // (the host checked k < n_punctual)
            const PunctualEval e = punctual_eval(sc.punctual[k], q + 1);
            double* o = out + 7 * (size_t)i;
            o[0] = e.w[0]; o[1] = e.w[1]; o[2] = e.w[2]; o[3] = e.D; o[4] = e.E[0]; o[5] = e.E[1]; o[6] = e.E[2];
        }
    }
}
void launch_punctual_probe(const SceneD& sc, int which, const double* in, uint32_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_punctual_probe, grid_for(n, 2048), dim3(BLOCK), 0, st, sc, which, in, n, out);
}

FormKernels forms_plt(const ShadeForm& f) { return unit_forms<UNIT_PLT>(f, nullptr); }

}  // namespace pt
