// The small kernels around the three stages — k_resolve, k_detile, the pool compaction, k_quantise, k_math_probe, k_camera_probe — and their launchers.
#include "pt_k_common.h"

namespace pt {

// accum[p*3+c] += sum over the k slots of pixel p, in slot order (k == 1: the exact
// sample-order sum the reference computes at camera.rs:106-108)
// LIST: the slots of list entry i are j * n_list + i; only the listed pixels are written (stored with PoolD::list_store)
template <bool LIST = false>
__global__ __launch_bounds__(BLOCK) void k_resolve(PoolD pool, double* accum) {
    const uint32_t n = LIST ? pool.n_list : pool.n_pixels;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (uint32_t j = 0; j < pool.k; ++j) {
            const uint32_t s = j * n + i;
            if (j == 0) { sx = pool.ax[s]; sy = pool.ay[s]; sz = pool.az[s]; }
            else { sx += pool.ax[s]; sy += pool.ay[s]; sz += pool.az[s]; }
        }
        const uint32_t p = LIST ? pool.list[i] : i;
        if (LIST && pool.list_store) {
            accum[3 * (size_t)p] = sx;
            accum[3 * (size_t)p + 1] = sy;
            accum[3 * (size_t)p + 2] = sz;
        } else {
            accum[3 * (size_t)p] += sx;
            accum[3 * (size_t)p + 1] += sy;
            accum[3 * (size_t)p + 2] += sz;
        }
    }
}

// dynamic mode with the tiled frame accumulator (PoolD::accum_tiled): accum[p*3+c] += plane c's sum of pixel p — once per render
// LIST: the listed pixels only (stored with PoolD::list_store)
template <bool LIST = false>
__global__ __launch_bounds__(BLOCK) void k_detile(PoolD pool, double* accum) {
    const uint32_t n = LIST ? pool.n_list : pool.n_pixels;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const uint32_t p = LIST ? pool.list[i] : i;
        const double* a = pool.accum + tiled_index(pool, p);
        if (LIST && pool.list_store) {
            accum[3 * (size_t)p] = a[0];
            accum[3 * (size_t)p + 1] = a[pool.n_tile_pixels];
            accum[3 * (size_t)p + 2] = a[2 * (size_t)pool.n_tile_pixels];
        } else {
            accum[3 * (size_t)p] += a[0];
            accum[3 * (size_t)p + 1] += a[pool.n_tile_pixels];
            accum[3 * (size_t)p + 2] += a[2 * (size_t)pool.n_tile_pixels];
        }
    }
}

// ---- the frame's END: compaction of the thinning pool (dynamic mode) -----------------------------------------------------------
// When the sample budget is handed out the slots die one by one, and for the last ~60 iterations both kernels sweep a pool
// that is mostly dead — every window pays its sort and its barriers for a handful of live paths (3-6 % of a frame on the pool
// sizes one rank of a multi-GPU frame uses). The host, which polls the live count anyway, then moves the survivors to the
// FRONT: the live slots beyond the new end L ("movers") go into the dead slots below it ("holes"), and every later launch covers
// [0, L) only. k_compact_scan lists both kinds (one atomic per wave and list, any order); k_compact_move copies mover i's two
// records and its state into hole i and marks the old slot dead. Which slot a path sits in decides nothing (the RNG is keyed by
// pixel and sample, the frame accumulator by pixel): no result changes.
__global__ __launch_bounds__(BLOCK) void k_compact_scan(PoolD pool, uint32_t new_end, uint32_t* holes, uint32_t* movers, uint32_t* counts /* [0] holes, [1] movers */,
                                                        uint32_t cap) {
    // [r3] A block takes 4096 slots at a time (n_alloc is a multiple of 8192), keeps their sixteen states per thread in registers,
    // ranks its holes and movers inside the block and reserves the block's stretch of each list with ONE atomic: one atomic per wave and
    // list on two addresses (the first form) serialised — 8 M of them, 47 ms, on a 268 M-slot pool (rocprofv3, config 2).
    constexpr int PER = 16, SUPER = PER * BLOCK;
    __shared__ uint32_t s_wave[2][BLOCK / 64], s_base[2];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (uint32_t base = blockIdx.x * SUPER; base < pool.n_alloc; base += gridDim.x * SUPER) {
        uint32_t hole_bits = 0, mover_bits = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const uint32_t s = base + (uint32_t)j * BLOCK + threadIdx.x;
            const bool dead = pool.bounce[s] == SLOT_DEAD;
            hole_bits |= (uint32_t)(s < new_end && dead) << j;
            mover_bits |= (uint32_t)(s >= new_end && !dead) << j;
        }
        uint32_t mine[2] = {(uint32_t)__popc(hole_bits), (uint32_t)__popc(mover_bits)}, before[2];
        for (int which = 0; which < 2; ++which) {              // exclusive prefix of the threads' counts inside the wave, wave totals to LDS
            uint32_t incl = mine[which];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                if (lane >= d) incl += up;
            }
            before[which] = incl - mine[which];
            if (lane == 63) s_wave[which][wave] = incl;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            uint32_t tot = 0;
            for (int w = 0; w < BLOCK / 64; ++w) tot += s_wave[threadIdx.x][w];
            s_base[threadIdx.x] = tot ? atomicAdd(&counts[threadIdx.x], tot) : 0u;
        }
        __syncthreads();
        for (int which = 0; which < 2; ++which) {
            uint32_t at = s_base[which] + before[which];
            for (int w = 0; w < wave; ++w) at += s_wave[which][w];
            uint32_t bits = which == 0 ? hole_bits : mover_bits;
            uint32_t* list = which == 0 ? holes : movers;
            while (bits) {
                const int j = __ffs((int)bits) - 1;
                bits &= bits - 1u;
                if (at < cap) list[at] = base + (uint32_t)j * BLOCK + threadIdx.x;
                ++at;
            }
        }
        __syncthreads();                                        // s_wave / s_base are reused by the next 4096 slots
    }
}
__global__ __launch_bounds__(BLOCK) void k_compact_move(PoolD pool, const uint32_t* holes, const uint32_t* movers, const uint32_t* counts, uint32_t cap) {
    const uint32_t n = counts[1] < counts[0] ? counts[1] : counts[0];          // movers <= holes by construction (live slots <= new end)
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n && i < cap; i += gridDim.x * BLOCK) {
        const uint32_t src = movers[i], dst = holes[i];
        const u4v* r = reinterpret_cast<const u4v*>(&pool.ray[src]);
        u4v* w = reinterpret_cast<u4v*>(&pool.ray[dst]);
        const u4v a = r[0], b = r[1], c = r[2], d = r[3];
        w[0] = a; w[1] = b; w[2] = c; w[3] = d;
        const u4v* pr = reinterpret_cast<const u4v*>(&pool.path[src]);
        u4v* pw = reinterpret_cast<u4v*>(&pool.path[dst]);
        for (unsigned k = 0; k < sizeof(PathRec) / 16; ++k) pw[k] = pr[k];
        pool.bounce[dst] = pool.bounce[src];
        pool.bounce[src] = SLOT_DEAD;
    }
}

// camera.rs:109-114,128-130: mean, sqrt gamma, clamp, truncate to u8
__global__ __launch_bounds__(BLOCK) void k_quantise(const double* accum, uint32_t n, double scale, uint8_t* rgb8) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        double c = accum[i] * scale;
        double g = sqrt(fmax(c, 0.0));
        double q = clampd(g, 0.0, 0.999) * 256.0;
        rgb8[i] = (q != q) ? (uint8_t)0 : (uint8_t)q;
    }
}

// Elementwise probes of the device arithmetic (sqrt/div/fma-free mul-add, libm calls, RNG)
// so that tests can compare them with the host bit for bit / ulp for ulp.
__global__ void k_math_probe(int which, const double* in, uint32_t n, double* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double a = in[2 * (size_t)i], b = in[2 * (size_t)i + 1], r = 0.0;
        switch (which) {
        case 0: r = sqrt(a); break;
        case 1: r = a / b; break;
        case 2: r = a * b + a; break;      // must NOT be fused
        case 3: r = detmath::sin(a); break;
        case 4: r = detmath::cos(a); break;
        case 5: r = detmath::acos(a); break;
        case 6: r = detmath::atan2(a, b); break;
        case 7: r = detmath::pow(a, b); break;
        case 8: r = detmath::log2(a); break;
        case 10: r = detmath::log(a); break;
        case 11: r = detmath::exp(a); break;
        case 9: {
            Rng g{(uint32_t)(long long)a, 0u, (uint32_t)(long long)b, 7u, (uint32_t)i};
            r = rng_f64(g);
            break;
        }
        }
        out[i] = r;
    }
}

// pt_camera_probe: generate_ray as k_init calls it (the sample's stream from draw 0), under the camera's projection
template <bool QMC, bool MOT = false>   // MOT: motion is in effect, the shutter is applied
__global__ __launch_bounds__(BLOCK) void k_camera_probe(CamD cam, uint64_t seed, const double* in, uint32_t n, double* out) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const uint32_t pixel = (uint32_t)in[2 * (size_t)i], sample = (uint32_t)in[2 * (size_t)i + 1];
        uint32_t row, col;
        divmod_u31(pixel, cam.width, row, col);
        std::conditional_t<QMC, RngQ, Rng> rng{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample, 0u};
        const RayD r = generate_ray<MOT>(cam, row, col, rng);
        double* o = out + 8 * (size_t)i;
        o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z; o[6] = r.time; o[7] = (double)rng.draw;
    }
}

// ------------------------------------------------------------------------------- launchers
void launch_camera_probe(const CamD& cam, int kind, uint64_t seed, const double* in, uint32_t n, double* out, hipStream_t st, bool motion) {
    if (motion) {
        if (kind == 1) hipLaunchKernelGGL((k_camera_probe<true, true>), grid_for(n, 2048), dim3(BLOCK), 0, st, cam, seed, in, n, out);
        else hipLaunchKernelGGL((k_camera_probe<false, true>), grid_for(n, 2048), dim3(BLOCK), 0, st, cam, seed, in, n, out);
    } else if (kind == 1) hipLaunchKernelGGL(k_camera_probe<true>, grid_for(n, 2048), dim3(BLOCK), 0, st, cam, seed, in, n, out);
    else hipLaunchKernelGGL(k_camera_probe<false>, grid_for(n, 2048), dim3(BLOCK), 0, st, cam, seed, in, n, out);
}
void launch_resolve(const PoolD& pool, double* accum, int max_blocks, hipStream_t st) {
    hipLaunchKernelGGL(pool.list ? k_resolve<true> : k_resolve<false>, grid_for(pool.list ? pool.n_list : pool.n_pixels, max_blocks), dim3(BLOCK), 0, st, pool, accum);
}
void launch_compact(const PoolD& pool, uint32_t new_end, uint32_t* holes, uint32_t* movers, uint32_t* counts, uint32_t cap, int max_blocks, hipStream_t st) {
    (void)hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), st);
    hipLaunchKernelGGL(k_compact_scan, grid_for(pool.n_alloc / 16u, max_blocks), dim3(BLOCK), 0, st, pool, new_end, holes, movers, counts, cap);
    hipLaunchKernelGGL(k_compact_move, grid_for(cap, max_blocks), dim3(BLOCK), 0, st, pool, holes, movers, counts, cap);
}
void launch_detile(const PoolD& pool, double* accum, int max_blocks, hipStream_t st) {
    hipLaunchKernelGGL(pool.list ? k_detile<true> : k_detile<false>, grid_for(pool.list ? pool.n_list : pool.n_pixels, max_blocks), dim3(BLOCK), 0, st, pool, accum);
}
void launch_quantise(const double* accum, uint32_t n, double scale, uint8_t* rgb8, hipStream_t st) {
    hipLaunchKernelGGL(k_quantise, grid_for(n, 4096), dim3(BLOCK), 0, st, accum, n, scale, rgb8);
}
void launch_math_probe(int which, const double* in, uint32_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_math_probe, grid_for(n, 2048), dim3(BLOCK), 0, st, which, in, n, out);
}

}  // namespace pt
