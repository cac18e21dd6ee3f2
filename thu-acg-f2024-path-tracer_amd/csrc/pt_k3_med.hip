// The participating-media forms of K1 / K3 (unit_forms<UNIT_MED>: the mode MED, with or without QMC) and the medium probe.
#include "pt_forms.h"

namespace pt {

// pt_medium_probe: which 0: in = n x (u1, u2, dir.xyz) -> out = n x (new_dir.xyz, ph); which 1: in = n x u -> out = n free-flight
// distances — the functions shade_slot's MED forms call
__global__ __launch_bounds__(BLOCK) void k_medium_probe(int which, double density, double g, const double* in, uint32_t n, double* out) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        if (which == 0) {
            const double* q = in + 5 * (size_t)i;
            const V3 axis{q[2], q[3], q[4]};
            const V3 d = hg_sample(g, q[0], q[1], axis);
            double* o = out + 4 * (size_t)i;
            o[0] = d.x; o[1] = d.y; o[2] = d.z;
            o[3] = hg_phase(g, dot(axis, d));
        } else {
            out[i] = medium_free_flight(in[i], density);
        }
    }
}
void launch_medium_probe(int which, double density, double g, const double* in, uint32_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_medium_probe, grid_for(n, 2048), dim3(BLOCK), 0, st, which, density, g, in, n, out);
}

FormKernels forms_med(const ShadeForm& f) { return unit_forms<UNIT_MED>(f, nullptr); }

}  // namespace pt
