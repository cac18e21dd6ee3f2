// The grid-density-media forms of K3 (unit_forms<UNIT_HET>: the mode HET, with or without QMC) and the grid probe.
#include "pt_forms.h"

namespace pt {

// pt_medium_probe: which 2: in = n points xyz -> out = n sigma values; which 3: in = n x (o.xyz, dir.xyz, t) -> out = n x (collided,
// s or 0, draws consumed), row i tracked with the independent sampler's draws of (seed 0, pixel i, sample 0) from draw 0 — the
// functions shade_slot's HET forms call
__global__ __launch_bounds__(BLOCK) void k_grid_probe(int which, const GridD* grid, const float* vals, const double* in, uint32_t n, double* out) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        if (which == 2) {
            const double* q = in + 3 * (size_t)i;
            out[i] = grid_sigma(*grid, vals, V3{q[0], q[1], q[2]});
        } else {
            const double* q = in + 7 * (size_t)i;
            const GridTrack tr = grid_track(grid, vals, V3{q[0], q[1], q[2]}, V3{q[3], q[4], q[5]}, q[6], Rng{0u, 0u, i, 0u, 0u});
            double* o = out + 3 * (size_t)i;
            o[0] = tr.collided ? 1.0 : 0.0;
            o[1] = tr.s;
            o[2] = (double)tr.draw;
        }
    }
}
void launch_grid_probe(int which, const GridD* grid, const float* vals, const double* in, uint32_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_grid_probe, grid_for(n, 2048), dim3(BLOCK), 0, st, which, grid, vals, in, n, out);
}

FormKernels forms_het(const ShadeForm& f) { return unit_forms<UNIT_HET>(f, nullptr); }

}  // namespace pt
