// The short-path pass: the tiles whose camera rays can enter only boxes of SHADEABLE entries (pt_sky_tiles.h sky_tile_class;
// pt_scene.cpp marks the entries: still spheres and quads of the world, a diffuse material without a normal map) are rendered here, ahead of
// the wavefront, as far as their paths are camera -> miss or camera -> one diffuse hit -> miss. Every other sample of those tiles — the HARD
// ones — is appended to a list and rendered by the wavefront from its first draw (pt_k_common.h work_to_pixel).
//   k_short<false>   one wave per (short tile, chunk of samples), lane = pixel of the tile
//   k_short<true>    the yield pilot: the same body, counting only, one wave per tile of the wavefront's map
//   k_short_select   one block: the piloted tiles whose yield reaches the threshold are flagged for k_sky_scan's lists
// Per sample the wave calls what K1, K2 and K3 call, in their order: Rng{seed, pixel, sample, 0} and generate_ray; K2's phase-A walk of the
// flat top level (flat_top_level, the exact tests of the non-mesh entries it enters; an entered mesh box makes the sample hard unless a
// box-only walk of the mesh's BVH proves the miss: mesh_walk_misses); on a hit of
// a shadeable primitive K3's phase A (reconstruct_hit_prim, fetch_tex, make_local_frame), the selector draw that only moves the counter,
// the diffuse sampler and pdf / eval (mat_sample's and leaf_pdf_eval's MAT_DIFFUSE cases, called directly so that no other material's code
// is compiled in), the throughput and the next ray as shade_slot makes them; the walk again for the bounce; sample_environment and
// add_radiance's rule that exact zeros are skipped. A chunk is summed per pixel in registers: one atomic triple per lane, as k_sky does.
#include "pt_k_common.h"
#include "pt_k_trace.h"
#include "pt_k2_extend.h"
#include "pt_sky_tiles.h"

namespace pt {

constexpr uint32_t SHORT_RING = 128;   // hard entries waiting per wave (a flush takes 64 as soon as 64 wait, a sample appends <= 64)
constexpr uint32_t WALK_STEPS = 256;   // nodes one miss proof may visit before it gives up

// The miss proof (DESIGN.md §23 "Proving a mesh miss"): the ray of this lane has entered the box of mesh entry `e`. It goes into the
// instance's frame as K2's phase B takes it there and walks the mesh's BVH with the box tests K2 makes — visit_node: the f32 slabs with
// their proven margin, t in [t_min, t_best], both ends included — and with no triangle test. true: the walk has visited every node whose
// box the ray enters and none of them was a leaf, so K2, whose walk visits a subset of those nodes (its t_best only shrinks), tests no
// triangle of this mesh either: the ray misses it. false — the sample is hard — as soon as a leaf's box is entered, the stack (`cap`
// entries per lane, stk[level * BLOCK]) or the step budget runs out, an instance of the chain moves, or a reference is none of the above.
PT_DEV bool mesh_walk_misses(const SceneD& sc, const RayD& wray, const Entry& e, float t_min_f, double t_best, uint32_t* stk, uint32_t cap) {
    if (sc.inst_motion)
        for (int32_t i = e.inst; i >= 0; i = sc.insts[i].inner)
            if (sc.inst_motion[i].moves) return false;
    const RayD r = ray_to_local_chain<false, false>(sc, e.inst, wray);
    const RayF f = make_rayf(r.o, r.d, e.extent);
    const float t_max_f = t_max_f32(t_best);
    uint32_t cur = e.blas_root, sp = 0;
    for (uint32_t step = 0; step < WALK_STEPS; ++step) {
        if ((cur & REF_TYPE_MASK) != REF_NODE) return false;      // a leaf's box entered (or a root that is a leaf)
        uint32_t c0, c1;
        const int n = visit_node(&sc.nodes[cur], f, t_min_f, t_max_f, c0, c1);
        if (n == 2) {
            if (sp >= cap) return false;
            stk[(sp++) * BLOCK] = c1;
        }
        if (n > 0) cur = c0;
        else if (sp > 0) cur = stk[(--sp) * BLOCK];
        else return true;
    }
    return false;
}

// PILOT: the counting form (DESIGN.md §23 "Taking tiles by yield"): the same body over the tiles of the wavefront's map and the first
// samples of the range, which adds no radiance and appends nothing: per tile it writes how many samples it would finish and how many it saw.
template <bool PILOT>
__global__ __launch_bounds__(BLOCK) void k_short(SceneD sc, CamD cam, PoolD pool, uint64_t seed, ShortArgsD a) {
    __shared__ unsigned long long s_ring[PILOT ? 1 : BLOCK / 64][PILOT ? 1 : SHORT_RING];
    __shared__ uint32_t s_stk[SHORT_WALK_STACK * BLOCK];
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)));
    uint32_t ti, ci;
    divmod_u31(wv, a.n_chunks, ti, ci);
    if (ti >= a.n_short) return;   // (wave-uniform; no block-wide barrier below)
    volatile unsigned long long* ring = s_ring[PILOT ? 0 : threadIdx.x >> 6];
    uint32_t* stk = &s_stk[threadIdx.x];
    const uint32_t tile = ldu(&a.short_list[ti]);
    uint32_t ty, tx;
    divmod_u31(tile, pool.tiles_x, ty, tx);
    const uint32_t col = tx * 8u + ((uint32_t)lane & 7u), row = ty * 8u + ((uint32_t)lane >> 3);
    const bool in_image = col < pool.width && row < pool.height;
    const uint32_t pixel = row * pool.width + col;
    const uint32_t s0 = pool.spp_begin + ci * a.chunk, s1 = pool.spp_end - s0 < a.chunk ? pool.spp_end : s0 + a.chunk;
    const double t_min = 1e-3;                                     // camera.rs:171,179 (K2's)
    const float t_min_f = __double2float_rd(t_min);
    V3 sum{0.0, 0.0, 0.0};
    bool any = false;
    uint32_t n_one = 0, n_two = 0;                                 // this lane's samples finished with one / two segments
    uint32_t head = 0, tail = 0;                                   // the ring's ends (wave-uniform)
    // `n` (<= 64) waiting entries leave for the list: one returning atomic per flush
    auto flush = [&](uint32_t n) {
        wave_lds_order();
        unsigned long long base = 0ull;
        if (lane == 0) base = atomicAdd(a.n_hard, (unsigned long long)n);
        base = __shfl(base, 0);
        if ((uint32_t)lane < n) {
            const unsigned long long e = ring[(head + (uint32_t)lane) % SHORT_RING], pos = base + (unsigned long long)lane;
            if (pos < a.cap) {                                     // (false only where the pilot's projection fell short: the host then runs the pass again, run_short)
                if (a.wide) ((unsigned long long*)a.hard)[pos] = e;
                else ((uint32_t*)a.hard)[pos] = (uint32_t)e;
            }
        }
        head += n;
        wave_lds_order();
    };
    auto add = [&](V3 c) {                                         // add_radiance's rule: exact zeros are skipped
        if (!(c.x == 0.0 && c.y == 0.0 && c.z == 0.0)) {
            sum = sum + c;
            any = true;
        }
    };
    for (uint32_t sample = s0; sample < s1; ++sample) {
        // K1 / phase D: the camera ray
        Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample, 0u};
        const RayD r = generate_ray<false>(cam, row, col, rng);
        // K2, phase A: the flat top level. A mesh box entered = a candidate K2 would record for its phase B: not ours
        bool recorded = false;
        const Closest c = flat_top_level<false, true, false>(sc, in_image, r, make_rayf(r.o, r.d, sc.tlas_extent), t_min, t_min_f, lane, PairLds{},
                                                             [&](uint32_t, const Entry& e, Closest& best) {
                                                                 if (!recorded) recorded = !mesh_walk_misses(sc, r, e, t_min_f, best.t, stk, a.walk_cap);
                                                             });
        bool done = false;
        const bool clean = in_image && !recorded;
        if (clean && c.id == HIT_NONE) {                           // K3: the ray left the scene (camera.rs:180-183)
            if constexpr (!PILOT) add(V3{1.0, 1.0, 1.0} * sample_environment(sc, cam, r.d));
            ++n_one;
            done = true;
        }
        // K3 at a shadeable primitive: phase A, B1, B2 of shade_slot for a diffuse material at bounce 0 without a lights list
        bool have_dir = false;
        RayD r2{};
        V3 thr{1.0, 1.0, 1.0};
        for (uint32_t j = 0; j < a.n_shade; ++j) {
            const uint32_t gid = ldu(&a.shade_prims[j]);
            const bool mine = clean && c.id == gid;
            if (__ballot(mine) == 0ull) continue;
            const PrimRef pr0 = ldu(&sc.prims[gid]);
            HitD hit{};
            if (mine && reconstruct_hit_prim<false, true, false>(sc, r, pr0, 1e-3, hit)) {
                const MatD* um = &sc.mats[pr0.mat];
                const TexVals tv = fetch_tex<true>(sc, *um, hit);
                const LocalFrame lf = make_local_frame(MAT_DIFFUSE, hit, -r.d);
                // (emission: zero for a diffuse material, and zeros are not added; no roulette at bounce 0)
                ++rng.draw;                                        // :201 the selector, which only moves the counter
                const V3 dir = to_world(lf.f, cosine_sample_hemisphere(rng, cam.two_pi_scale));   // diffuse.rs:51-54
                const V3 l = to_local(lf.f, dir);                  // diffuse.rs:56-65
                const double bsdf_pdf = fabs(l.z) / D_PI;
                const V3 brdf = fabs(l.z) * (tv.color / D_PI);
                const double p_light = 0.0, p_bsdf = 1.0 - p_light, light_pdf = 0.0;
                const double pdf = p_bsdf * bsdf_pdf + p_light * light_pdf;
                const V3 attenuation = brdf / pdf;
                const double e = 1e-3 * signum(dot(dir, hit.gn));  // :217-222
                r2 = make_ray(hit.point + e * hit.gn, dir, r.time);
                thr = thr * attenuation;
                have_dir = true;
            }
        }
        if (__ballot(have_dir) != 0ull) {                          // K2 again, for the bounce; then K3's miss
            bool recorded2 = false;
            const Closest c2 = flat_top_level<false, true, false>(sc, have_dir, r2, make_rayf(r2.o, r2.d, sc.tlas_extent), t_min, t_min_f, lane, PairLds{},
                                                                  [&](uint32_t, const Entry& e, Closest& best) {
                                                                      if (!recorded2) recorded2 = !mesh_walk_misses(sc, r2, e, t_min_f, best.t, stk, a.walk_cap);
                                                                  });
            if (have_dir && !recorded2 && c2.id == HIT_NONE) {
                if constexpr (!PILOT) add(thr * sample_environment(sc, cam, r2.d));
                ++n_two;
                done = true;
            }
        }
        // everything else is hard: nothing added, nothing counted, the wavefront renders the sample from its first draw
        const bool hard = in_image && !done;
        const unsigned long long hm = PILOT ? 0ull : __ballot(hard);
        if (hm != 0ull) {
            if (hard) {
                const uint32_t rank = (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
                ring[(tail + rank) % SHORT_RING] =
                    ((unsigned long long)ti << (6u + a.sample_bits)) | ((unsigned long long)lane << a.sample_bits) | (unsigned long long)(sample - pool.spp_begin);
            }
            tail += (uint32_t)__popcll(hm);
            if (tail - head >= 64u) flush(64u);
        }
    }
    if constexpr (PILOT) {
        const unsigned long long fin = wave_sum((unsigned long long)(n_one + n_two));
        const uint32_t seen = (uint32_t)__popcll(__ballot(in_image)) * (s1 - s0);
        if (lane == 0) {
            a.pilot[2u * tile] = (uint32_t)fin;
            a.pilot[2u * tile + 1u] = seen;
        }
        return;
    }
    if (tail != head) flush(tail - head);
    if (any) {
        double* acc = pool.accum + (size_t)tile * 64u + (uint32_t)lane;
        unsafeAtomicAdd(acc, sum.x);
        unsafeAtomicAdd(acc + pool.n_tile_pixels, sum.y);
        unsafeAtomicAdd(acc + 2 * (size_t)pool.n_tile_pixels, sum.z);
    }
    const unsigned long long one = wave_sum((unsigned long long)n_one), two = wave_sum((unsigned long long)n_two);
    if (lane == 0 && one + two != 0ull) {
        atomicAdd(&a.n_hard[1], one + two);                        // (the host adds them to the render's counts: ShortArgsD)
        atomicAdd(&a.n_hard[2], one + 2ull * two);
    }
}

// The pilot's tiles are taken by yield: one block. A tile of the wavefront's class (flag SKY_TILE_WAVEFRONT, or SKY_TILE_TAKEN
// from an earlier selection of this render) whose pilot saw samples falls into bin floor(16 finished / seen) of 0 .. 16; it becomes
// SKY_TILE_TAKEN when its bin is at least min_bin, else SKY_TILE_WAVEFRONT (min_bin = 17: nothing is taken). k_sky_scan then lists the taken
// tiles with the proven short ones. hist[3 * bin + {0, 1, 2}] = the bin's tiles, the samples the pilot saw there, those it did not finish:
// what the host sizes the hard list from, and how it finds the bin to retreat to where a cap binds.
__global__ __launch_bounds__(BLOCK) void k_short_select(uint8_t* flags, uint32_t n_tiles, const uint32_t* pilot, uint32_t min_bin, uint32_t* hist) {
    __shared__ uint32_t s_hist[3 * SHORT_YIELD_BINS];
    for (uint32_t i = threadIdx.x; i < 3u * SHORT_YIELD_BINS; i += BLOCK) s_hist[i] = 0u;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < n_tiles; t += BLOCK) {
        const uint8_t fl = flags[t];
        if (fl != SKY_TILE_WAVEFRONT && fl != SKY_TILE_TAKEN) continue;
        const uint32_t fin = pilot[2u * t], seen = pilot[2u * t + 1u];
        if (seen == 0u || fin > seen) continue;                    // (not piloted: the tile stays what it is, the wavefront's)
        const uint32_t bin = (uint32_t)((16ull * fin) / seen);
        flags[t] = bin >= min_bin ? SKY_TILE_TAKEN : SKY_TILE_WAVEFRONT;
        atomicAdd(&s_hist[3u * bin], 1u);
        atomicAdd(&s_hist[3u * bin + 1u], seen);
        atomicAdd(&s_hist[3u * bin + 2u], seen - fin);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 3u * SHORT_YIELD_BINS; i += BLOCK) hist[i] = s_hist[i];
}

void launch_short(const SceneD& sc, const CamD& cam, const PoolD& pool, uint64_t seed, const ShortArgsD& a, hipStream_t st) {
    if (a.n_short == 0u || a.n_chunks == 0u) return;
    const uint64_t waves = (uint64_t)a.n_short * a.n_chunks;   // (the caller keeps this below 2^31)
    const dim3 grid((uint32_t)((waves + BLOCK / 64 - 1) / (BLOCK / 64)));
    if (a.pilot) hipLaunchKernelGGL(k_short<true>, grid, dim3(BLOCK), 0, st, sc, cam, pool, seed, a);
    else hipLaunchKernelGGL(k_short<false>, grid, dim3(BLOCK), 0, st, sc, cam, pool, seed, a);
}
void launch_short_select(uint8_t* flags, uint32_t n_tiles, const uint32_t* pilot, uint32_t min_bin, uint32_t* hist, hipStream_t st) {
    hipLaunchKernelGGL(k_short_select, dim3(1), dim3(BLOCK), 0, st, flags, n_tiles, pilot, min_bin, hist);
}

}  // namespace pt
