// The sky pass: the tiles no camera ray of which can enter a box of the world (pt_sky_tiles.h) never enter the path pool.
//   k_sky_classify  one thread per 8x8 pixel tile: the tile test
//   k_sky_scan      one block: the flags -> the wavefront's tile map (active-tile index -> tile), the sure-sky tile list, the short-path
//                   pass's tile list (k_short is in pt_k_short.hip), the counts
//   k_sky           one wave per (sure-sky tile, chunk of samples): what K3 does for a camera ray that left the scene, and nothing else
#include "pt_k_common.h"
#include "pt_sky_tiles.h"

namespace pt {

// reach (null: not wanted): the tile's reach mask (pt_sky_tiles.h sky_tile_reach) for the short-path pass, DESIGN.md §23.3, one word per tile —
// every tile, whatever its class — with box b's bit at position order.at[b]: the place of entry b in SceneD::entry_box, the order
// flat_top_level's loop runs in (the host only asks for it when every entry has its own box and there are at most TLAS_FLAT_MAX of them).
__global__ __launch_bounds__(BLOCK) void k_sky_classify(SkyCam cam, uint32_t n_boxes, const double* boxes6, unsigned long long shadeable, uint32_t tiles_x,
                                                         uint32_t n_tiles, uint8_t* flags, uint32_t* reach, ReachOrder order) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_tiles) return;
    uint32_t ty, tx;
    divmod_u31(t, tiles_x, ty, tx);
    const unsigned long long todo = sky_tile_uncleared(cam, ty, tx, n_boxes, boxes6);
    flags[t] = sky_tile_class_of(cam, ty, tx, n_boxes, boxes6, shadeable, todo);   // (shadeable = 0: sure sky or wavefront, the sky pass's two kinds)
    if (reach) {
        uint32_t m = 0xFFFFFFFFu;
        if (n_boxes <= 32u && !sky_tile_says_nothing(cam, ty, tx, n_boxes, boxes6)) {
            m = 0u;
            for (uint32_t b = 0; b < n_boxes; ++b)
                if ((todo >> b) & 1ull) m |= 1u << (order.at[b] & 31u);
        }
        reach[t] = m;
    }
}

// Thread i ranks the tiles [i * per, (i + 1) * per): the three lists come out in tile order. Of the SHORT tiles the first max_short (in
// tile order) go to short_list; the others stay the wavefront's (the hard list's cap). counts[0] = active tiles, [1] =
// sure-sky tiles, [2] = the pixels of the sure-sky tiles that lie inside the image, [3] = short tiles taken, [4] = their pixels inside the
// image, [5] = short tiles found (proven ones: SKY_TILE_SHORT). A tile k_short_select took by its pilot yield (SKY_TILE_TAKEN)
// is listed with the proven ones, in tile order, and counted in [3] and [4]; [6] = those tiles alone, [7] = their pixels inside the image.
__global__ __launch_bounds__(BLOCK) void k_sky_scan(const uint8_t* flags, uint32_t n_tiles, uint32_t width, uint32_t height, uint32_t max_short, uint32_t* tile_map,
                                                     uint32_t* sky_list, uint32_t* short_list, uint32_t* counts) {
    __shared__ uint32_t s_sky[BLOCK], s_short[BLOCK], s_pixels, s_short_pixels, s_proven, s_taken, s_taken_pixels;
    const uint32_t tiles_x = (width + 7u) / 8u;
    const uint32_t per = (n_tiles + BLOCK - 1) / BLOCK, t0 = threadIdx.x * per, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    uint32_t mine = 0, mine_short = 0, pixels = 0, proven = 0;
    if (threadIdx.x == 0) s_pixels = s_short_pixels = s_proven = s_taken = s_taken_pixels = 0;
    auto tile_pixels = [&](uint32_t t) {
        uint32_t ty, tx;
        divmod_u31(t, tiles_x, ty, tx);
        const uint32_t w = width - tx * 8u < 8u ? width - tx * 8u : 8u, h = height - ty * 8u < 8u ? height - ty * 8u : 8u;
        return w * h;
    };
    for (uint32_t t = t0; t < t1; ++t) {
        if (flags[t] == SKY_TILE_SKY) {
            ++mine;
            pixels += tile_pixels(t);
        } else if (flags[t] == SKY_TILE_SHORT || flags[t] == SKY_TILE_TAKEN) {
            ++mine_short;
            if (flags[t] == SKY_TILE_SHORT) ++proven;
        }
    }
    s_sky[threadIdx.x] = mine;
    s_short[threadIdx.x] = mine_short;
    __syncthreads();
    if (pixels) atomicAdd(&s_pixels, pixels);
    if (proven) atomicAdd(&s_proven, proven);
    for (uint32_t d = 1; d < BLOCK; d <<= 1) {   // inclusive scans of the threads' sky and short counts
        const uint32_t v = threadIdx.x >= d ? s_sky[threadIdx.x - d] : 0u, u = threadIdx.x >= d ? s_short[threadIdx.x - d] : 0u;
        __syncthreads();
        s_sky[threadIdx.x] += v;
        s_short[threadIdx.x] += u;
        __syncthreads();
    }
    uint32_t sky_at = s_sky[threadIdx.x] - mine, short_at = s_short[threadIdx.x] - mine_short;
    uint32_t act_at = (t0 < n_tiles ? t0 : n_tiles) - sky_at - (short_at < max_short ? short_at : max_short);
    uint32_t short_pixels = 0, by_yield = 0, by_yield_pixels = 0;
    for (uint32_t t = t0; t < t1; ++t) {
        if (flags[t] == SKY_TILE_SKY) {
            sky_list[sky_at++] = t;
        } else if ((flags[t] == SKY_TILE_SHORT || flags[t] == SKY_TILE_TAKEN) && short_at++ < max_short) {
            short_list[short_at - 1u] = t;
            short_pixels += tile_pixels(t);
            if (flags[t] == SKY_TILE_TAKEN) {
                ++by_yield;
                by_yield_pixels += tile_pixels(t);
            }
        } else {
            tile_map[act_at++] = t;
        }
    }
    if (short_pixels) atomicAdd(&s_short_pixels, short_pixels);
    if (by_yield) {
        atomicAdd(&s_taken, by_yield);
        atomicAdd(&s_taken_pixels, by_yield_pixels);
    }
    __syncthreads();
    if (threadIdx.x == BLOCK - 1) {
        const uint32_t n_short = s_short[BLOCK - 1], taken = n_short < max_short ? n_short : max_short;
        counts[0] = n_tiles - s_sky[BLOCK - 1] - taken;
        counts[1] = s_sky[BLOCK - 1];
        counts[2] = s_pixels;
        counts[3] = taken;
        counts[4] = s_short_pixels;
        counts[5] = s_proven;
        counts[6] = s_taken;
        counts[7] = s_taken_pixels;
    }
}

// Lane = pixel of the tile (the tiled accumulator's order), so the 64 environment texels of an iteration are neighbours and the wave's
// three atomics cover 64 consecutive words of a plane each. Per sample exactly K1 / K3's arithmetic for a camera ray that left the scene:
// Rng{seed, pixel, sample, 0}, generate_ray, sample_environment, times the throughput (1, 1, 1), exact zeros skipped (add_radiance).
// The samples of a chunk are summed in registers (the dynamic mode's order of additions is free: DESIGN.md §numerics).
__global__ __launch_bounds__(BLOCK) void k_sky(SceneD sc, CamD cam, PoolD pool, CountersD* cnt, uint64_t seed, const uint32_t* sky_list, uint32_t n_sky,
                                                uint32_t chunk, uint32_t n_chunks) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)));
    uint32_t ti, ci;
    divmod_u31(wv, n_chunks, ti, ci);
    if (ti >= n_sky) return;   // (wave-uniform)
    const uint32_t tile = ldu(&sky_list[ti]);
    uint32_t ty, tx;
    divmod_u31(tile, pool.tiles_x, ty, tx);
    const uint32_t col = tx * 8u + (lane & 7u), row = ty * 8u + (lane >> 3);
    const bool in_image = col < pool.width && row < pool.height;
    const uint32_t pixel = row * pool.width + col;
    const uint32_t s0 = pool.spp_begin + ci * chunk, s1 = pool.spp_end - s0 < chunk ? pool.spp_end : s0 + chunk;
    if (in_image) {
        V3 sum{0.0, 0.0, 0.0};
        bool any = false;
        for (uint32_t sample = s0; sample < s1; ++sample) {
            Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample, 0u};
            const RayD r = generate_ray<false>(cam, row, col, rng);
            const V3 c = V3{1.0, 1.0, 1.0} * sample_environment(sc, cam, r.d);
            if (!(c.x == 0.0 && c.y == 0.0 && c.z == 0.0)) {
                sum = sum + c;
                any = true;
            }
        }
        if (any) {
            double* a = pool.accum + (size_t)tile * 64u + lane;
            unsafeAtomicAdd(a, sum.x);
            unsafeAtomicAdd(a + pool.n_tile_pixels, sum.y);
            unsafeAtomicAdd(a + 2 * (size_t)pool.n_tile_pixels, sum.z);
        }
    }
    // every one of these samples had exactly one segment
    const unsigned long long n = (unsigned long long)__popcll(__ballot(in_image)) * (unsigned long long)(s1 - s0);
    if (lane == 0u && n != 0ull) {
        atomicAdd(&cnt->samples, n);
        atomicAdd(&cnt->segments, n);
    }
}

void launch_sky_classify(const SkyCam& cam, uint32_t n_boxes, const double* boxes6, unsigned long long shadeable, uint32_t max_short, uint32_t n_tiles, uint8_t* flags,
                         uint32_t* tile_map, uint32_t* sky_list, uint32_t* short_list, uint32_t* counts, uint32_t* reach, const ReachOrder& order, hipStream_t st) {
    hipLaunchKernelGGL(k_sky_classify, dim3((n_tiles + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, cam, n_boxes, boxes6, shadeable, (cam.width + 7u) / 8u, n_tiles, flags, reach, order);
    hipLaunchKernelGGL(k_sky_scan, dim3(1), dim3(BLOCK), 0, st, flags, n_tiles, cam.width, cam.height, max_short, tile_map, sky_list, short_list, counts);
}
// the scan alone, over flags k_short_select has changed
void launch_sky_scan(uint32_t width, uint32_t height, uint32_t max_short, uint32_t n_tiles, const uint8_t* flags, uint32_t* tile_map, uint32_t* sky_list,
                     uint32_t* short_list, uint32_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(k_sky_scan, dim3(1), dim3(BLOCK), 0, st, flags, n_tiles, width, height, max_short, tile_map, sky_list, short_list, counts);
}
void launch_sky(const SceneD& sc, const CamD& cam, const PoolD& pool, CountersD* cnt, uint64_t seed, const uint32_t* sky_list, uint32_t n_sky, uint32_t chunk,
                hipStream_t st) {
    const uint32_t spp = pool.spp_end - pool.spp_begin;
    if (n_sky == 0u || spp == 0u || chunk == 0u) return;
    const uint32_t n_chunks = (spp + chunk - 1u) / chunk;
    const uint64_t waves = (uint64_t)n_sky * n_chunks;   // (the caller keeps this below 2^31: sky_chunk)
    hipLaunchKernelGGL(k_sky, dim3((uint32_t)((waves + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, st, sc, cam, pool, cnt, seed, sky_list, n_sky, chunk, n_chunks);
}

}  // namespace pt
