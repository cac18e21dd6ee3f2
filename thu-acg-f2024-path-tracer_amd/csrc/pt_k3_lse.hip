// The exact-light-sampling forms of K3 (unit_forms<UNIT_LSE>: the mode LSE, with or without LIST and QMC)
// and the light probe.
#include "pt_forms.h"

namespace pt {

// pt_light_probe: lights.sample / lights.pdf as shade_slot calls them — the LSE forms' functions (EXACT) or the reference's
// MOT (never with EXACT): the scene has moving instances, posed at the row's time
template <bool EXACT, bool MOT = false>
__global__ __launch_bounds__(BLOCK) void k_light_probe(SceneD sc, int which, const double* in, uint32_t n, double* out) {
    __shared__ uint32_t stack[LIGHT_STACK * BLOCK];
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        if (which == 0) {
            const double* q = in + 4 * (size_t)i;
            Rng rng{0u, 0u, i, 0u, 0u};
            uint32_t light = 0u;
            int32_t face = -1;
            V3 d;
            if constexpr (EXACT) {
                d = lights_sample_exact(sc, V3{q[0], q[1], q[2]}, q[3], rng, &light, &face);
            } else {
                Rng first = rng;                                   // the index draw is lights.sample's first: the same value
                light = rng_index(first, sc.n_lights);
                d = lights_sample<MOT>(sc, V3{q[0], q[1], q[2]}, q[3], rng);
            }
            double* o = out + 6 * (size_t)i;
            o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = (double)light; o[4] = (double)face; o[5] = (double)rng.draw;
        } else {
            const double* q = in + 7 * (size_t)i;
            const V3 o{q[0], q[1], q[2]}, d{q[3], q[4], q[5]};
            if constexpr (EXACT) out[i] = lights_pdf_exact<BLOCK>(sc, o, d, q[6], &stack[threadIdx.x]);
            else out[i] = lights_pdf<MOT>(sc, o, d, q[6]);
        }
    }
}
void launch_light_probe(const SceneD& sc, bool exact, int which, const double* in, uint32_t n, double* out, hipStream_t st) {
    if (exact) hipLaunchKernelGGL(k_light_probe<true>, grid_for(n, 2048), dim3(BLOCK), 0, st, sc, which, in, n, out);
    else if (sc.inst_motion) hipLaunchKernelGGL((k_light_probe<false, true>), grid_for(n, 2048), dim3(BLOCK), 0, st, sc, which, in, n, out);
    else hipLaunchKernelGGL(k_light_probe<false>, grid_for(n, 2048), dim3(BLOCK), 0, st, sc, which, in, n, out);
}

FormKernels forms_lse(const ShadeForm& f) { return unit_forms<UNIT_LSE>(f, nullptr); }

}  // namespace pt
