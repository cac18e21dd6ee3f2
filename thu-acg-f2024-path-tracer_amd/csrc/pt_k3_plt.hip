// The PLT forms of K3 (unit_forms<UNIT_PLT>: punctual lights in effect — point, spot and directional lights; plain mode, the default
// variant's shapes x LIGHTS x LIST x QMC), the punctual probe and the light grid's build kernel. K1 and the AOV walk have no PLT form:
// the lights change no camera ray and no first hit.
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
        } else if (which == 2) {                                      // the light grid's selection at a point (the host checked that the grid is in effect)
            const double* q = in + 3 * (size_t)i;
            Rng rng{0u, 0u, i, 0u, 0u};
            const uint32_t cell = punctual_grid_cell(sc.punctual_grid, q);
            double p;
            const uint32_t k = punctual_grid_pick(sc, q, rng_f64(rng), p) & PLT_INDEX_MASK;
            const PunctualEval e = punctual_eval(sc.punctual[k], q);
            double* o = out + 11 * (size_t)i;
            o[0] = (double)cell; o[1] = (double)k; o[2] = p; o[3] = (double)rng.draw; o[4] = e.w[0]; o[5] = e.w[1]; o[6] = e.w[2]; o[7] = e.D; o[8] = e.E[0]; o[9] = e.E[1]; o[10] = e.E[2];
        } else if (which == 3) {                                      // C[cell][k] (the host checked both indices)
            const double* q = in + 2 * (size_t)i;
            out[i] = sc.punctual_cdf[(size_t)(uint32_t)q[0] * sc.punctual_grid.stride + (uint32_t)q[1]];
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

// The light grid's table (the rule: pt_amd.h): row `cell` = the cell's CDF over the n lights, formed by punctual_grid_row — the
// function pt_punctual_grid_row runs on the host. One lane per cell, one wave per block: the sum and the running CDF go in ascending k inside
// a lane (the rule's order), so the work is split over cells only. Every lane reads the same record in the same step: ldu brings it through
// the scalar cache, once per wave. Rows lie [cell][k], so a lane's own stores are n * 8 bytes apart from its neighbour's — 64 write requests
// of 8 bytes per wave instruction. STAGE: the lanes park GRID_TILE consecutive values each in LDS (row pitch GRID_TILE + 1 doubles: a lane's
// 8-byte write lands on its own pair of banks) and the wave writes the tile out cell after cell, GRID_TILE * 8 = 256 contiguous bytes per
// cell, two cells per wave instruction. The direct form stays behind PT_GRID_DIRECT for the measurement.
constexpr int GRID_WAVE = 64, GRID_TILE = 32;
template <bool STAGE>
__global__ __launch_bounds__(GRID_WAVE) void k_punctual_grid(const PunctualD* __restrict__ lights, uint32_t n, PunctualGridBuild g, double* __restrict__ table) {
    __shared__ double tile[STAGE ? GRID_WAVE : 1][GRID_TILE + 1];
    const uint32_t lane = threadIdx.x, base = blockIdx.x * GRID_WAVE, cell = base + lane;
    const bool active = cell < g.cells;
    const PunctualCell c = punctual_grid_geometry(g.box, g.dims, active ? cell : g.cells - 1u);   // (an idle lane of the last block repeats the last cell and stores nothing)
    auto light = [&](uint32_t k) { return ldu(&lights[k]); };
    if constexpr (STAGE) {
        punctual_grid_row(light, n, c, [&](uint32_t k, double C) {     // (k and n are wave-uniform: every lane reaches the barriers together)
            const uint32_t j = k % GRID_TILE;
            tile[lane][j] = C;
            if (j + 1u == (uint32_t)GRID_TILE || k + 1u == n) {
                __syncthreads();
                const uint32_t cnt = j + 1u, k0 = k - j;
                for (uint32_t idx = lane; idx < GRID_WAVE * cnt; idx += GRID_WAVE) {
                    const uint32_t cc = idx / cnt, jj = idx % cnt;
                    if (base + cc < g.cells) table[(size_t)(base + cc) * n + k0 + jj] = tile[cc][jj];
                }
                __syncthreads();
            }
        });
    } else {
        punctual_grid_row(light, n, c, [&](uint32_t k, double C) {
            if (active) table[(size_t)cell * n + k] = C;
        });
    }
}
void launch_punctual_grid(const PunctualD* lights, uint32_t n, const PunctualGridBuild& g, double* table, bool stage, hipStream_t st) {
    const dim3 blocks((g.cells + GRID_WAVE - 1) / GRID_WAVE);
    if (stage) hipLaunchKernelGGL(k_punctual_grid<true>, blocks, dim3(GRID_WAVE), 0, st, lights, n, g, table);
    else hipLaunchKernelGGL(k_punctual_grid<false>, blocks, dim3(GRID_WAVE), 0, st, lights, n, g, table);
}

FormKernels forms_plt(const ShadeForm& f) { return unit_forms<UNIT_PLT>(f, nullptr); }

}  // namespace pt
