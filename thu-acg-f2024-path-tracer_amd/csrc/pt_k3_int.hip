// The interior-media forms of K3 (unit_forms<UNIT_INT>: the mode INT, with or without QMC) and the
// absorption probe.
#include "pt_forms.h"

namespace pt {

// pt_medium_probe which 4: in = n lengths -> out = n x 3 throughput factors of a segment of that length — the function shade_slot's
// INT forms call, applied to a throughput of (1, 1, 1)
__global__ __launch_bounds__(BLOCK) void k_absorb_probe(V3 a, const double* in, uint32_t n, double* out) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const V3 f = medium_absorb(a, V3{1.0, 1.0, 1.0}, in[i]);
        double* o = out + 3 * (size_t)i;
        o[0] = f.x; o[1] = f.y; o[2] = f.z;
    }
}
void launch_absorb_probe(const double absorption[3], const double* in, uint32_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_absorb_probe, grid_for(n, 2048), dim3(BLOCK), 0, st, V3{absorption[0], absorption[1], absorption[2]}, in, n, out);
}

FormKernels forms_int(const ShadeForm& f) { return unit_forms<UNIT_INT>(f, nullptr); }

}  // namespace pt
