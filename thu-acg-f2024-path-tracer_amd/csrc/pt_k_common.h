// What every stage of the wavefront path tracer shares: the pool's record loads / stores, the work-item mapping, the wave-wide
// tally, the in-kernel stamps of -DPT_STAMPS builds and the launchers' grid size. One lane = one resident path.
//
//   pt_k_trace.h      closest-hit traversal (K2, k_aov, k_probe) and the first-hit feature walk of k_aov / k_aov_qmc
//   pt_k3_shade.h     k_init     K1 raygen       camera.rs:153-168  fills the pool with the first sample of every slot
//   pt_k2_extend.h    k_extend2  K2 closest hit  world.rs:47-62 -> bvh.rs:123-164 -> sphere/quad/mesh/instance.rs  (two-phase form; k_extend =
//                                                batch form for scenes without meshes)
//   pt_k3_shade.h     k_shade    K3+K4+K1'       camera.rs:177-226 body: miss/env, emission, RR, one-sample MIS,
//                                                BSDF sample+pdf+eval, next ray; finished paths are regenerated in place
//   pt_kernels.hip    k_resolve  K6 (sum part)   camera.rs:106-109: per-pixel sum of the slot accumulators (and the other small kernels)
//
// All kernels are persistent-thread style: a fixed grid sized to the machine walks the pool
// (grid-stride, or windows drawn from a queue). No MFMA anywhere — this is branchy f64 scalar work bounded by
// VALU issue and L2 latency, with the path pool streaming through HBM once per stage.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pt_dev_geom.h"
#include "pt_dev_medium.h"
#include "pt_envmap.h"
#include "pt_kernels.h"

namespace pt {

constexpr int BLOCK = 256;
constexpr int SORT_WINDOW_SLOTS = 2048;   // window size of k_extend2 and k_shade = the granule pt_render.cpp allocates the pool in

// K2 writes its result (one primitive id per slot) once and never re-reads it, while the scene tables
// (BVH, primitives: a few MB) are re-read by every wave: the result leaves with non-temporal stores.
// (Non-temporal LOADS of the path records made no measurable difference and are not used.)
template <class T> PT_DEV void stnt(T* p, T v) { __builtin_nontemporal_store(v, p); }
typedef __attribute__((address_space(3))) void* lds_ptr;      // operands of __builtin_amdgcn_global_load_lds (LDS-DMA)
typedef const __attribute__((address_space(1))) void* glb_ptr;

// ---- path records (pt_types.h RayRec / PathRec): one lane moves one whole record, 16 B per access ----
typedef double d2v __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
// PoolD::compact (scenes in which nothing moves, CamD::motionless: Ray::time reaches no result): the ray record's time slot
// carries (pixel, bounce number) instead, so a path at bounce 0 — throughput (1,1,1) by definition — has no PathRec worth
// writing: a regenerated camera ray costs one 64-byte record, not 96 bytes.
PT_DEV RayD load_ray(const PoolD& pool, uint32_t s) {
    const d2v* p = reinterpret_cast<const d2v*>(&pool.ray[s]);
    const d2v a = p[0], b = p[1], c = p[2], d = p[3];
    return RayD{V3{a.x, a.y, b.x}, V3{b.y, c.x, c.y}, pool.compact ? 0.0 : d.x};
}
// `tail`: the record's words 12, 13 — the bits of Ray::time, or (pixel, bounce) in compact mode
PT_DEV RayD load_ray(const PoolD& pool, uint32_t s, uint32_t& sample, uint32_t& draw, uint32_t (&tail)[2]) {
    const d2v* p = reinterpret_cast<const d2v*>(&pool.ray[s]);
    const d2v a = p[0], b = p[1], c = p[2];
    const u4v d = *reinterpret_cast<const u4v*>(p + 3);
    sample = d.z;
    draw = d.w;
    tail[0] = d.x;
    tail[1] = d.y;
    return RayD{V3{a.x, a.y, b.x}, V3{b.y, c.x, c.y}, pool.compact ? 0.0 : __hiloint2double((int)d.y, (int)d.x)};
}
// `rays` / `paths`: the pool's record area written — PoolD::ray / path, or k_shade's output area PoolD::ray_out / path_out
PT_DEV void store_ray(const PoolD& pool, RayRec* rays, uint32_t s, const RayD& r, uint32_t sample, uint32_t draw, uint32_t pixel, uint32_t bounce) {
    d2v* p = reinterpret_cast<d2v*>(&rays[s]);
    p[0] = d2v{r.o.x, r.o.y};
    p[1] = d2v{r.o.z, r.d.x};
    p[2] = d2v{r.d.y, r.d.z};
    *reinterpret_cast<u4v*>(p + 3) = pool.compact ? u4v{pixel, bounce, sample, draw}
                                                  : u4v{(uint32_t)__double2loint(r.time), (uint32_t)__double2hiint(r.time), sample, draw};
}
PT_DEV V3 load_path(const PoolD& pool, uint32_t s, uint32_t& pixel, uint32_t& bounce) {
    const d2v* p = reinterpret_cast<const d2v*>(&pool.path[s]);
    const d2v a = p[0];
    const u4v b = *reinterpret_cast<const u4v*>(p + 1);
    pixel = b.z;
    bounce = b.w;
    return V3{a.x, a.y, __hiloint2double((int)b.y, (int)b.x)};
}
PT_DEV void store_path(PathRec* paths, uint32_t s, V3 thr, uint32_t pixel, uint32_t bounce) {
    d2v* p = reinterpret_cast<d2v*>(&paths[s]);
    p[0] = d2v{thr.x, thr.y};
    *reinterpret_cast<u4v*>(p + 1) = u4v{(uint32_t)__double2loint(thr.z), (uint32_t)__double2hiint(thr.z), pixel, bounce};
#if PT_PATHREC_BYTES == 64
    p[2] = d2v{0.0, 0.0};                         // the record is one 64-B sector: write all of it
    p[3] = d2v{0.0, 0.0};
#endif
}

// Sum of a per-thread tally over the wave (every lane gets it). The kernels' end-of-launch counters (samples, segments, alive) are added
// once per WAVE instead of once per thread (131 k to 262 k atomics on a single address at the end of every launch). Measured +-0 on
// every pool size — those atomics return nothing and nobody waits for them — unlike k_compact_scan's, whose returns the waves did wait for.
PT_DEV unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// floor(a / b) and a - b * floor(a / b) for a < 2^53, 0 < b < 2^31, by ONE f64 division and an exact integer correction.
// (The compiler's inline expansion of a 64-bit unsigned division is ~100 instructions, a third of them quarter-rate
// integer multiplies, and it ran once per regenerated camera ray.)
PT_DEV void divmod_u53(unsigned long long a, uint32_t b, unsigned long long& q, uint32_t& r) {
    unsigned long long q0 = (unsigned long long)((double)a / (double)b);     // within 1 of the true quotient
    long long rem = (long long)(a - q0 * (unsigned long long)b);
    if (rem < 0) { --q0; rem += (long long)b; }
    else if (rem >= (long long)b) { ++q0; rem -= (long long)b; }
    q = q0;
    r = (uint32_t)rem;
}
PT_DEV void divmod_u31(uint32_t a, uint32_t b, uint32_t& q, uint32_t& r) {   // a, b < 2^31: the f64 quotient floors exactly
    q = (uint32_t)((double)a / (double)b);
    r = a - q * b;
}
// the sky pass's tile map (PoolD::n_work_pixels != 0): active-tile index -> tile
PT_DEV const uint32_t* pool_tile_map(const PoolD& pool) { return reinterpret_cast<const uint32_t*>(pool.accum + 3 * (size_t)pool.n_tile_pixels); }
// ... and behind the map, at the next 8-byte boundary, the short-path pass's record of its hard list (pt_types.h ShortHdrD; the host: short_hdr_behind)
PT_DEV const ShortHdrD* pool_short_hdr(const PoolD& pool) {
    return reinterpret_cast<const ShortHdrD*>(pool_tile_map(pool) + (((size_t)pool.n_tile_pixels / 64u + 1u) & ~(size_t)1u));
}
// dynamic mode: work item -> (pixel, sample) and the pixel's row / column; false when the item lies outside a ragged image edge
// MAP: the form can run with the sky pass on (sky_pass_form, pt_types.h); every other form is compiled without the lookup, as it was
template <bool MAP>
PT_DEV bool work_to_pixel(const PoolD& pool, unsigned long long w, uint32_t& pixel, uint32_t& sample, uint32_t& row, uint32_t& col) {
    unsigned long long q;
    uint32_t in_frame;
    const bool mapped = MAP && pool.n_work_pixels != 0u;   // (a kernel argument: wave-uniform)
    // the short-path pass's hard samples are the items behind the tile items: (tile, pixel in tile, sample) from the list
    const unsigned long long tile_items = (unsigned long long)pool.n_work_pixels * (unsigned long long)(pool.spp_end - pool.spp_begin);
    const bool hard = mapped && w >= tile_items;
    uint32_t tile, in_tile;
    if (hard) {
        const ShortHdrD* h = pool_short_hdr(pool);
        const unsigned long long i = w - tile_items;   // (< n_hard: the caller has checked w < total_work)
        const uint32_t sbits = ldu(&h->sample_bits);
        const void* list = (const void*)ldu((const unsigned long long*)&h->hard);
        const unsigned long long e = ldu(&h->wide) ? ((const unsigned long long*)list)[i] : (unsigned long long)((const uint32_t*)list)[i];
        sample = pool.spp_begin + (uint32_t)(e & ((1ull << sbits) - 1ull));
        in_tile = (uint32_t)(e >> sbits) & 63u;
        tile = ((const uint32_t*)ldu((const unsigned long long*)&h->short_list))[(uint32_t)(e >> (sbits + 6u))];
    } else {
        divmod_u53(w, mapped ? pool.n_work_pixels : pool.n_tile_pixels, q, in_frame);
        sample = pool.spp_begin + (uint32_t)q;
        tile = in_frame >> 6;
        in_tile = in_frame & 63u;
    }
    if (mapped) {
        // the map entries of the calling lanes by SCALAR loads, one per distinct tile: the lanes hold consecutive items of at most two
        // 64-item chunks (two tiles), or of a shuffled granule of k_init (PT_INIT_SHUFFLE) — a per-lane load's address pair cost a form scratch
        // (a hard sample's tile comes from its entry and is left alone)
        const uint32_t* map = pool_tile_map(pool);
        uint32_t mapped_tile = tile;
        unsigned long long todo = __ballot(!hard);
        while (todo != 0ull) {
            const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)tile, __ffsll((long long)todo) - 1);
            const uint32_t m0 = ldu(&map[t0]);
            const bool mine = !hard && tile == t0;
            if (mine) mapped_tile = m0;
            todo &= ~__ballot(mine);
        }
        tile = mapped_tile;
    }
    uint32_t ty, tx;
    divmod_u31(tile, pool.tiles_x, ty, tx);
    const uint32_t x = tx * 8u + (in_tile & 7u), y = ty * 8u + (in_tile >> 3);
    pixel = y * pool.width + x;
    row = y;
    col = x;
    return x < pool.width && y < pool.height;
}
// pixel-list form: every item is a listed (hence real) pixel, so no item idles at a ragged edge
PT_DEV bool work_to_pixel_list(const PoolD& pool, unsigned long long w, uint32_t& pixel, uint32_t& sample, uint32_t& row, uint32_t& col) {
    unsigned long long q;
    uint32_t i;
    divmod_u53(w, pool.n_list, q, i);
    sample = pool.spp_begin + (uint32_t)q;
    pixel = pool.list[i];
    divmod_u31(pixel, pool.width, row, col);
    return true;
}
template <bool LIST, bool MAP = false>
PT_DEV bool work_item(const PoolD& pool, unsigned long long w, uint32_t& pixel, uint32_t& sample, uint32_t& row, uint32_t& col) {
    if constexpr (LIST) return work_to_pixel_list(pool, w, pixel, sample, row, col);
    else return work_to_pixel<MAP>(pool, w, pixel, sample, row, col);
}
// static mode: the pixel slot s owns
template <bool LIST>
PT_DEV uint32_t slot_pixel(const PoolD& pool, uint32_t s) {
    if constexpr (LIST) return pool.list[s % pool.n_list];
    else return s % pool.n_pixels;
}
// shard-local counter value -> global work item: 64-item chunks are dealt round-robin to the shards
PT_DEV unsigned long long shard_item(unsigned long long c, uint32_t shard) {
    return (c >> 6) * (unsigned long long)(WORK_SHARDS * 64u) + (unsigned long long)shard * 64ull + (c & 63ull);
}

// pixel (row-major) -> its index inside a channel plane of the tiled frame accumulator (PoolD::accum)
PT_DEV uint32_t tiled_index(const PoolD& pool, uint32_t pixel) {
    uint32_t y = (uint32_t)((double)pixel * pool.inv_width);           // within 1 of pixel / width
    int32_t x = (int32_t)(pixel - y * pool.width);
    if (x < 0) { --y; x += (int32_t)pool.width; }
    else if (x >= (int32_t)pool.width) { ++y; x -= (int32_t)pool.width; }
    return ((y >> 3) * pool.tiles_x + ((uint32_t)x >> 3)) * 64u + ((y & 7u) << 3) + ((uint32_t)x & 7u);
}

#ifdef PT_STAMPS
// Diagnostic build: where a k_shade wave spends its cycles (s_memtime ticks; MI355X_MICROARCH.md "In-kernel stamps"). The stamp
// after the record loads forces vmcnt(0) so that the first segment is the pure fetch wait. Never part of the product build.
PT_DEV unsigned long long stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
__shared__ unsigned long long g_prof[N_CLASSES + 1][PROF_COLS];
#define PT_STAMP(i) const unsigned long long t_##i = stamp()
#define PT_STAMP_VAR(i) unsigned long long t_##i = 0
#define PT_STAMP_SET(i) t_##i = stamp()
#define PT_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define PT_STAMP(i)
#define PT_STAMP_VAR(i)
#define PT_STAMP_SET(i)
#define PT_DRAIN()
#endif

static inline uint32_t clamp_blocks(uint32_t b, int max_blocks) {
    if (b > (uint32_t)max_blocks) b = (uint32_t)max_blocks;
    return b ? b : 1u;
}
static inline dim3 grid_for(uint32_t n, int max_blocks) { return dim3(clamp_blocks((n + BLOCK - 1) / BLOCK, max_blocks)); }
// resident blocks per CU of kernel `k` launched with `threads` per block
static inline int occupancy_blocks(const void* k, int threads) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, threads, 0) != hipSuccess || nb < 1) nb = 1;
    return nb;
}

}  // namespace pt
