// The short-path pass: the tiles whose camera rays can enter only boxes of SHADEABLE entries (pt_sky_tiles.h sky_tile_class;
// pt_flatten.cpp marks the entries: still spheres and quads of the world, a diffuse material without a normal map) are rendered here, ahead of
// the wavefront, as far as their paths are camera -> miss or camera -> one diffuse hit -> miss. Every other sample of those tiles — the HARD
// ones — is appended to a list and rendered by the wavefront from its first draw (pt_k_common.h work_to_pixel).
//   k_short<false, DEFER>   one wave per (short tile, chunk of samples), lane = pixel of the tile
//   k_short<true, DEFER>    the yield pilot: the same body, counting only, one wave per tile of the wavefront's map
//   k_short_select          one block: the piloted tiles whose yield reaches the threshold are flagged for k_sky_scan's lists
// Per sample the wave calls what K1, K2 and K3 call, in their order: Rng{seed, pixel, sample, 0} and generate_ray; K2's phase-A walk of the
// flat top level (flat_top_level, the exact tests of the non-mesh entries it enters; an entered mesh box makes the sample hard unless a
// box-only walk of the mesh's BVH proves the miss: mesh_walk_misses); on a hit of
// a shadeable primitive K3's phase A (reconstruct_hit_prim, fetch_tex, make_local_frame), the selector draw that only moves the counter,
// the diffuse sampler and pdf / eval (mat_sample's and leaf_pdf_eval's MAT_DIFFUSE cases, called directly so that no other material's code
// is compiled in), the throughput and the next ray as shade_slot makes them; the walk again for the bounce; sample_environment and
// add_radiance's rule that exact zeros are skipped. A chunk is summed per pixel in registers: one atomic triple per lane, as k_sky does.
// DEFER: the bounce rays' miss proofs do not run where the ray enters the mesh's box — a few lanes of the wave walking
// while the rest wait — but wait as records in a per-wave ring in LDS and run 64 at a time, lane i walking record i ("A pass", in k_short below).
#include "pt_k_common.h"
#include "pt_k_trace.h"
#include "pt_k2_extend.h"
#include "pt_sky_tiles.h"

namespace pt {

constexpr uint32_t SHORT_RING = 128;   // hard entries waiting per wave (a flush takes 64 as soon as 64 wait, an append adds <= 64)
constexpr uint32_t WALK_STEPS = 256;   // nodes one miss proof may visit before it gives up
constexpr uint32_t PEND_RING = 64;     // DEFER: bounce rays waiting per wave for their miss proofs (a pass takes all of them)

// The miss proof (DESIGN.md §23 "Proving a mesh miss"): the ray of this lane has entered the box of mesh entry `e`. It goes into the
// instance's frame as K2's phase B takes it there and walks the mesh's BVH with the box tests K2 makes — visit_node: the f32 slabs with
// their proven margin, t in [t_min, t_best], both ends included — and with no triangle test. true: the walk has visited every node whose
// box the ray enters and none of them was a leaf, so K2, whose walk visits a subset of those nodes (its t_best only shrinks), tests no
// triangle of this mesh either: the ray misses it. false — the sample is hard — as soon as a leaf's box is entered, the stack (`cap`
// entries per lane, stk[level * BLOCK]) or the step budget runs out, an instance of the chain moves, or a reference is none of the above.
// `steps` (diagnostic builds): the nodes visited are added to it. U: `e` is wave-uniform, the chain's instances arrive by scalar loads (the
// same arithmetic on the same values).
template <bool U = false>
PT_DEV bool mesh_walk_misses(const SceneD& sc, const RayD& wray, const Entry& e, float t_min_f, double t_best, uint32_t* stk, uint32_t cap,
                             uint32_t* steps = nullptr) {
    if (sc.inst_motion)
        for (int32_t i = e.inst; i >= 0; i = sc.insts[i].inner)
            if (sc.inst_motion[i].moves) return false;
    const RayD r = ray_to_local_chain<U, false>(sc, e.inst, wray);
    const RayF f = make_rayf(r.o, r.d, e.extent);
    const float t_max_f = t_max_f32(t_best);
    uint32_t cur = e.blas_root, sp = 0;
    for (uint32_t step = 0; step < WALK_STEPS; ++step) {
        if ((cur & REF_TYPE_MASK) != REF_NODE) return false;      // a leaf's box entered (or a root that is a leaf)
        if (steps) ++*steps;
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

#ifdef PT_STAMPS
// Diagnostic build (DESIGN.md §23.2 "Where the time goes"): wave cycles per phase and the walks' counts, summed into ShortArgsD::n_hard
// from word SHORT_PROF_AT on: [0..7] the phases (a) .. (h), [8..12] the camera rays' walks, [16..20] the bounces' — wave-samples (DEFER:
// passes) with a walking lane, walking lanes, steps over lanes, the longest lane's steps per wave-sample, walks skipped as outcome-neutral.
__shared__ unsigned long long g_short_walk_t[BLOCK / 64][2];   // cycles inside the walks of the camera rays / of the bounces, per wave
PT_DEV uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
struct WalkTally {
    unsigned long long n[5] = {0, 0, 0, 0, 0};
    PT_DEV void sample(bool walked, uint32_t steps, uint32_t neutral) {
        const unsigned long long m = __ballot(walked);
        if (m != 0ull) {
            n[0] += 1ull;
            n[1] += (unsigned long long)__popcll(m);
            n[2] += wave_sum((unsigned long long)steps);
            n[3] += (unsigned long long)wave_max_u32(steps);
        }
        n[4] += wave_sum((unsigned long long)neutral);
    }
};
// (inside a divergent region: the first active lane adds the wave's cycles)
#define PT_SHORT_WALK_T(which, t0)                                                                                              \
    do {                                                                                                                        \
        const unsigned long long t1_ = stamp();                                                                                 \
        if (lane == __ffsll((long long)__ballot(true)) - 1) ((volatile unsigned long long*)g_short_walk_t[threadIdx.x >> 6])[which] += t1_ - (t0); \
    } while (0)
#endif

// PILOT: the counting form (DESIGN.md §23 "Taking tiles by yield"): the same body over the tiles of the wavefront's map and the first
// samples of the range, which adds no radiance and appends nothing: per tile it writes how many samples it would finish and how many it saw.
// DEFER: the bounces' miss proofs run in dense passes; false: where the ray enters the box, as the camera rays' do (the
// A/B form, PT_SHORT_DEFER=0). What holds in both forms, and what every count of the pass rests on:
//   - a sample's outcome depends on (tile, pixel, sample, budgets) alone, never on which records shared a pass: a record is proven iff
//     every mesh whose box the ray entered proves a miss, each with t_best = +inf, which is what the walk on the spot is given when no
//     non-mesh entry was hit — and when one was hit the sample is hard whatever a walk says, so neither form walks;
//   - no block-wide barrier: waves leave independently. Every ring index is wave-uniform, LDS steps are fenced with wave_lds_order();
//   - every loop is bounded: WALK_STEPS per mesh, <= TLAS_FLAT_MAX meshes per record, one pass at most per append and one drain;
//   - hard entries leave a wave in another order than without DEFER: nothing reads that order (pt_k_common.h work_to_pixel).
template <bool PILOT, bool DEFER>
__global__ __launch_bounds__(BLOCK, 4) void k_short(SceneD sc, CamD cam, PoolD pool, uint64_t seed, ShortArgsD a) {
    __shared__ unsigned long long s_ring[PILOT ? 1 : BLOCK / 64][PILOT ? 1 : SHORT_RING];
    __shared__ uint32_t s_stk[SHORT_WALK_STACK * BLOCK];
    // the waiting bounces, structure of arrays, per wave: origin and direction (f64: the walk converts them as it does on the spot),
    // the FINISHED contribution thr * sample_environment (not the pilot) — the environment is looked up where the wave looks it up anyway,
    // for the lanes that finish on the spot, so a pass holds no second copy of that code and a record is no larger than with thr —, the
    // mask of the mesh entries whose boxes the ray entered (bit EntryBox::entry < TLAS_FLAT_MAX) and pixel << sample_bits | sample
    constexpr uint32_t PEND_D = PILOT ? 6u : 9u;
    __shared__ double s_pend_d[DEFER ? BLOCK / 64 : 1][DEFER ? PEND_D : 1][DEFER ? PEND_RING : 1];
    __shared__ uint32_t s_pend_u[DEFER ? BLOCK / 64 : 1][DEFER ? 2 : 1][DEFER ? PEND_RING : 1];
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)));
    uint32_t ti, ci;
    divmod_u31(wv, a.n_chunks, ti, ci);
    if (ti >= a.n_short) return;   // (wave-uniform; no block-wide barrier below)
    volatile unsigned long long* ring = s_ring[PILOT ? 0 : threadIdx.x >> 6];
    // (plain LDS accesses, so that they stay ds_ instructions with one base address: every step that reads what other lanes wrote stands behind a wave_lds_order())
    auto& pend_d = s_pend_d[DEFER ? threadIdx.x >> 6 : 0];
    auto& pend_u = s_pend_u[DEFER ? threadIdx.x >> 6 : 0];
    uint32_t* stk = &s_stk[threadIdx.x];
    const uint32_t tile = ldu(&a.short_list[ti]);
    uint32_t ty, tx;
    divmod_u31(tile, pool.tiles_x, ty, tx);
    const uint32_t col = tx * 8u + ((uint32_t)lane & 7u), row = ty * 8u + ((uint32_t)lane >> 3);
    const bool in_image = col < pool.width && row < pool.height;
    const uint32_t pixel = row * pool.width + col;
    const uint32_t s0 = pool.spp_begin + ci * a.chunk, s1 = pool.spp_end - s0 < a.chunk ? pool.spp_end : s0 + a.chunk;
    // DESIGN.md §23.3, all wave-uniform (scalar registers). reach: the entries a camera ray of this tile may enter, bit k = entry_box[k]; every
    // other entry's box is entered by none (pt_sky_tiles.h), so its turn of the loop could only fail: it is not taken. direct_gid: the mask
    // names ONE entry and that entry is a shadeable primitive — the loop's one exact test is the rebuild's, which runs anyway.
    // (the host runs the pass on a top level of at most 32 entries, classify_sky: the masks name every entry there is)
    const uint32_t all_entries = sc.n_entries >= 32u ? 0xFFFFFFFFu : (1u << sc.n_entries) - 1u;
    const uint32_t reach = (a.reach ? ldu(&a.reach[tile]) : 0xFFFFFFFFu) & all_entries;
    uint32_t direct_gid = HIT_NONE;
    if (a.direct != 0u && a.shade_at && __popc(reach) == 1)
        for (uint32_t j = 0; j < a.n_shade; ++j)
            if ((ldu(&a.shade_at[j]) & 0xFFu) == (uint32_t)__builtin_ctz(reach)) direct_gid = ldu(&a.shade_prims[j]);
    const double t_min = 1e-3;                                     // camera.rs:171,179 (K2's)
    const float t_min_f = __double2float_rd(t_min);
    V3 sum{0.0, 0.0, 0.0};
    bool any = false;
    uint32_t n_one = 0, n_two = 0;                                 // this lane's samples finished with one / two segments
    uint32_t head = 0, tail = 0;                                   // the ring's ends (wave-uniform)
    uint32_t n_pend = 0, n_walks = 0, n_passes = 0;                // DEFER: records waiting; records walked, passes run (all wave-uniform)
#ifdef PT_STAMPS
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    WalkTally cam_walks, bounce_walks;
    if (lane < 2) ((volatile unsigned long long*)g_short_walk_t[threadIdx.x >> 6])[lane] = 0ull;
    wave_lds_order();
#endif
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
    // the lanes with `hard` set append `code` = (pixel in tile) << sample_bits | sample (32 bits: the host runs the pass up to 2^26 samples per
    // pixel, classify_sky) under this wave's tile; fewer than 64 entries wait before and
    // after, so the ring of 128 holds them
    auto append_hard = [&](bool hard, uint32_t code) {
        const unsigned long long hm = __ballot(hard);
        if (hm == 0ull) return;
        if (hard) {
            const uint32_t rank = (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
            ring[(tail + rank) % SHORT_RING] = ((unsigned long long)ti << (6u + a.sample_bits)) | (unsigned long long)code;
        }
        tail += (uint32_t)__popcll(hm);
        if (tail - head >= 64u) flush(64u);
    };
    auto add = [&](V3 c) {                                         // add_radiance's rule: exact zeros are skipped
        if (!(c.x == 0.0 && c.y == 0.0 && c.z == 0.0)) {
            sum = sum + c;
            any = true;
        }
    };
    // (DEFER: one more turn of the loop after the last sample, which only drains the waiting records — the pass has one place in the code)
    for (uint32_t sample = s0; sample < s1 + (DEFER ? 1u : 0u); ++sample) {
        const bool body = sample < s1;                             // wave-uniform
        bool hard = false, pend = false;
        RayD r2{};
        V3 contrib{0.0, 0.0, 0.0};
        uint32_t pmask = 0u;
        if (body) {
            PT_STAMP(0);
            // K1 / phase D: the camera ray
            Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample, 0u};
            const RayD r = generate_ray<false>(cam, row, col, rng);
            PT_STAMP(1);
            // K2, phase A: the flat top level. A mesh box entered = a candidate K2 would record for its phase B: not ours.
            // Mesh entries come last in entry_box, so when a mesh callback runs `best` is final for the non-mesh entries. A hit of a primitive
            // that is not shadeable then makes the sample hard whatever a walk says (nothing below finishes it): no walk.
            bool recorded = false;
#ifdef PT_STAMPS
            uint32_t w_steps = 0u, w_neutral = 0u;
            bool w_walked = false;
#endif
            //  the direct hit: every in-image lane is a candidate of the tile's one primitive, and the rebuild below decides
            Closest c{D_INF, direct_gid};
            if (direct_gid == HIT_NONE)
                c = flat_top_level<false, true, false, true>(sc, in_image, r, make_rayf(r.o, r.d, sc.tlas_extent), t_min, t_min_f, lane, PairLds{},
                                                                 [&](uint32_t, const Entry& e, Closest& best) {
                                                                     if (recorded) return;
                                                                     if (best.id != HIT_NONE) {
                                                                         bool shadeable = false;
                                                                         for (uint32_t j = 0; j < a.n_shade; ++j) shadeable = shadeable || best.id == ldu(&a.shade_prims[j]);
                                                                         if (!shadeable) {
                                                                             recorded = true;
#ifdef PT_STAMPS
                                                                             ++w_neutral;
#endif
                                                                             return;
                                                                         }
                                                                     }
#ifdef PT_STAMPS
                                                                     const unsigned long long w0 = stamp();
                                                                     w_walked = true;
                                                                     recorded = !mesh_walk_misses(sc, r, e, t_min_f, best.t, stk, a.walk_cap, &w_steps);
                                                                     PT_SHORT_WALK_T(0, w0);
#else
                                                                     recorded = !mesh_walk_misses(sc, r, e, t_min_f, best.t, stk, a.walk_cap);
#endif
                                                                 }, reach);
#ifdef PT_STAMPS
            cam_walks.sample(w_walked, w_steps, w_neutral);
#endif
            PT_STAMP(2);
            bool done = false;
            const bool clean = in_image && !recorded;
            bool miss = clean && c.id == HIT_NONE;                 // K3: the ray left the scene (camera.rs:180-183), finished below
            // K3 at a shadeable primitive: phase A, B1, B2 of shade_slot for a diffuse material at bounce 0 without a lights list
            bool have_dir = false;
            V3 thr{1.0, 1.0, 1.0};
            uint32_t n_left = 0u, left_at = 0u;                    // wave-uniform: the shadeable primitives bounces of this wave leave, the last one's shade_at
            for (uint32_t j = 0; j < a.n_shade; ++j) {
                const uint32_t gid = ldu(&a.shade_prims[j]);
                const bool mine = clean && c.id == gid;
                if (__ballot(mine) == 0ull) continue;
                const PrimRef pr0 = ldu(&sc.prims[gid]);
                HitD hit{};
                // (the direct hit: the walk would have reported this primitive iff the same test on the same ray succeeds here; else it is a miss)
                const bool hit_ok = mine && reconstruct_hit_prim<false, true, false>(sc, r, pr0, 1e-3, hit);
                miss = miss || (mine && !hit_ok && direct_gid != HIT_NONE);
                if (__ballot(hit_ok) != 0ull) {
                    ++n_left;
                    left_at = a.shade_at ? ldu(&a.shade_at[j]) : 0u;
                }
                if (hit_ok) {
                    const MatD* um = &sc.mats[pr0.mat];
                    const TexVals tv = fetch_tex<true>(sc, *um, hit);
                    const LocalFrame lf = make_local_frame(MAT_DIFFUSE, hit, -r.d);
                    // (emission: zero for a diffuse material, and zeros are not added; no roulette at bounce 0)
                    ++rng.draw;                                    // :201 the selector, which only moves the counter
                    const V3 dir = to_world(lf.f, cosine_sample_hemisphere(rng, cam.two_pi_scale));   // diffuse.rs:51-54
                    const V3 l = to_local(lf.f, dir);              // diffuse.rs:56-65
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
            if (miss) {
                if constexpr (!PILOT) add(V3{1.0, 1.0, 1.0} * sample_environment(sc, cam, r.d));
                ++n_one;
                done = true;
            }
            PT_STAMP(3);
#ifdef PT_STAMPS
            unsigned long long t_4 = t_3, t_5 = t_3;
#endif
            if (__ballot(have_dir) != 0ull) {                      // K2 again, for the bounce; then K3's miss
                // (`best` is final for the non-mesh entries here too: after a hit the bounce does not leave the scene and the sample is hard)
                bool recorded2 = false;
#ifdef PT_STAMPS
                w_steps = w_neutral = 0u;
                w_walked = false;
#endif
                //  every bounce of the wave left ONE quad the host has flagged: its exact test has t < 0 (the proof there), so
                // its entry is not tested
                const uint32_t reach2 = n_left == 1u && (left_at & SHADE_AT_SELF_OK) != 0u ? all_entries & ~(1u << (left_at & 31u)) : all_entries;
                const Closest c2 = flat_top_level<false, true, false, true>(sc, have_dir, r2, make_rayf(r2.o, r2.d, sc.tlas_extent), t_min, t_min_f, lane, PairLds{},
                                                                      [&](uint32_t ei, const Entry& e, Closest& best) {
                                                                          if (best.id != HIT_NONE) {
#ifdef PT_STAMPS
                                                                              if (!recorded2) ++w_neutral;
#endif
                                                                              recorded2 = true;
                                                                              return;
                                                                          }
                                                                          if constexpr (DEFER) {
                                                                              if (ei < 32u) pmask |= 1u << ei;   // (always: n_entries <= TLAS_FLAT_MAX)
                                                                              else recorded2 = true;
                                                                          } else if (!recorded2) {
#ifdef PT_STAMPS
                                                                              const unsigned long long w0 = stamp();
                                                                              w_walked = true;
                                                                              recorded2 = !mesh_walk_misses(sc, r2, e, t_min_f, best.t, stk, a.walk_cap, &w_steps);
                                                                              PT_SHORT_WALK_T(1, w0);
#else
                                                                              recorded2 = !mesh_walk_misses(sc, r2, e, t_min_f, best.t, stk, a.walk_cap);
#endif
                                                                          }
                                                                      }, reach2);
#ifdef PT_STAMPS
                if constexpr (!DEFER) bounce_walks.sample(w_walked, w_steps, w_neutral);
                else bounce_walks.sample(false, 0u, w_neutral);
                t_4 = stamp();
#endif
                const bool left = have_dir && !recorded2 && c2.id == HIT_NONE;   // the bounce leaves the scene unless a mesh whose box it entered is hit
                if constexpr (!PILOT)
                    if (left) contrib = thr * sample_environment(sc, cam, r2.d);
                if (left && pmask == 0u) {
                    if constexpr (!PILOT) add(contrib);
                    ++n_two;
                    done = true;
                }
                pend = left && pmask != 0u;                        // (DEFER only: finished with two segments iff every recorded mesh proves a miss)
#ifdef PT_STAMPS
                t_5 = stamp();
#endif
            }
            // everything else is hard: nothing added, nothing counted, the wavefront renders the sample from its first draw
            hard = in_image && !done && !pend;
#ifdef PT_STAMPS
            ph[0] += t_1 - t_0;
            ph[1] += t_2 - t_1;
            ph[3] += t_3 - t_2;
            ph[4] += t_4 - t_3;
            ph[6] += t_5 - t_4;
#endif
        }
        PT_STAMP(6);
        if constexpr (DEFER) {
            const unsigned long long pm = __ballot(pend);
            const uint32_t n_new = (uint32_t)__popcll(pm);
            if (n_pend != 0u && (!body || n_pend + n_new > PEND_RING)) {
                // A pass: lane i takes record i and walks the meshes it names one after the other, each as the walk on the spot would (the
                // same function, its own column of the stack); the first mesh it cannot prove ends it. The wave waits for its longest lane.
                PT_STAMP(7);
                wave_lds_order();
                bool ok = (uint32_t)lane < n_pend;
                RayD pr{};
                uint32_t mask = 0u;
                if (ok) {
                    pr = RayD{V3{pend_d[0][lane], pend_d[1][lane], pend_d[2][lane]}, V3{pend_d[3][lane], pend_d[4][lane], pend_d[5][lane]}, 0.0};
                    mask = pend_u[0][lane];
                }
#ifdef PT_STAMPS
                uint32_t p_steps = 0u;
                const bool p_walked = ok;
#endif
                for (uint32_t k = 0; k < sc.n_entries; ++k) {      // (wave-uniform: the entry arrives by a scalar load)
                    const EntryBox bx = ldu(&sc.entry_box[k]);
                    if (bx.kind != ENTRY_MESH) continue;
                    const bool want = ok && ((mask >> (bx.entry & 31u)) & 1u) != 0u;
                    if (__ballot(want) == 0ull) continue;
                    if (want) {
                        const Entry e{bx.kind, bx.first_prim, bx.inst, bx.blas_root, bx.extent, bx.n_prims, {0u, 0u}};
#ifdef PT_STAMPS
                        ok = mesh_walk_misses<true>(sc, pr, e, t_min_f, D_INF, stk, a.walk_cap, &p_steps);
#else
                        ok = mesh_walk_misses<true>(sc, pr, e, t_min_f, D_INF, stk, a.walk_cap);
#endif
                    }
                }
                const bool mine = (uint32_t)lane < n_pend;
                const uint32_t code = mine ? pend_u[1][lane] : 0u;
                if (ok) {                                          // proven: two segments, the contribution to the owner's pixel
                    ++n_two;                                       // (counted on the pass's lane: only the wave's sum is read)
                    if constexpr (!PILOT) {
                        const V3 cc{pend_d[6][lane], pend_d[7][lane], pend_d[8][lane]};
                        if (!(cc.x == 0.0 && cc.y == 0.0 && cc.z == 0.0)) {
                            double* acc = pool.accum + (size_t)tile * 64u + (code >> a.sample_bits);
                            unsafeAtomicAdd(acc, cc.x);
                            unsafeAtomicAdd(acc + pool.n_tile_pixels, cc.y);
                            unsafeAtomicAdd(acc + 2 * (size_t)pool.n_tile_pixels, cc.z);
                        }
                    }
                }
                n_walks += n_pend;
                ++n_passes;
                n_pend = 0u;
                wave_lds_order();                                  // (the records are read: the ring may be written again)
                if constexpr (!PILOT) append_hard(mine && !ok, code);
#ifdef PT_STAMPS
                bounce_walks.sample(p_walked, p_steps, 0u);
                ph[5] += stamp() - t_7;
#endif
            }
            if (pm != 0ull) {
                if (pend) {
                    const uint32_t at = n_pend + (uint32_t)__popcll(pm & ((1ull << lane) - 1ull));
                    pend_d[0][at] = r2.o.x; pend_d[1][at] = r2.o.y; pend_d[2][at] = r2.o.z;
                    pend_d[3][at] = r2.d.x; pend_d[4][at] = r2.d.y; pend_d[5][at] = r2.d.z;
                    if constexpr (!PILOT) { pend_d[6][at] = contrib.x; pend_d[7][at] = contrib.y; pend_d[8][at] = contrib.z; }
                    pend_u[0][at] = pmask;
                    pend_u[1][at] = ((uint32_t)lane << a.sample_bits) | (sample - pool.spp_begin);
                }
                n_pend += n_new;
            }
        }
        if constexpr (!PILOT)
            if (body) append_hard(hard, ((uint32_t)lane << a.sample_bits) | (sample - pool.spp_begin));
#ifdef PT_STAMPS
        ph[7] += stamp() - t_6;
#endif
    }
#ifdef PT_STAMPS
    {
        wave_lds_order();
        const unsigned long long wc = ((volatile unsigned long long*)g_short_walk_t[threadIdx.x >> 6])[0], wb = ((volatile unsigned long long*)g_short_walk_t[threadIdx.x >> 6])[1];
        ph[2] = wc;                                                // (c), and (b) without it
        ph[1] -= wc < ph[1] ? wc : ph[1];
        ph[5] += wb;                                               // (f): on the spot (not DEFER) or the passes, which (h) then does not hold
        if constexpr (DEFER) ph[7] -= ph[5] < ph[7] ? ph[5] : ph[7];
        else ph[4] -= wb < ph[4] ? wb : ph[4];
        if (lane == 0 && !PILOT) {
            for (int i = 0; i < 8; ++i) atomicAdd(&a.n_hard[SHORT_PROF_AT + i], ph[i]);
            for (int i = 0; i < 5; ++i) {
                atomicAdd(&a.n_hard[SHORT_PROF_AT + 8 + i], cam_walks.n[i]);
                atomicAdd(&a.n_hard[SHORT_PROF_AT + 16 + i], bounce_walks.n[i]);
            }
        }
    }
#endif
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
    if (lane == 0 && ci == 0u && direct_gid != HIT_NONE) atomicAdd(&a.n_hard[5], 1ull);   // (the tiles of the direct hit)
    if (lane == 0 && n_passes != 0u) {
        atomicAdd(&a.n_hard[3], (unsigned long long)n_walks);
        atomicAdd(&a.n_hard[4], (unsigned long long)n_passes);
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
    if (a.pilot) {
        if (a.defer) hipLaunchKernelGGL((k_short<true, true>), grid, dim3(BLOCK), 0, st, sc, cam, pool, seed, a);
        else hipLaunchKernelGGL((k_short<true, false>), grid, dim3(BLOCK), 0, st, sc, cam, pool, seed, a);
    } else {
        if (a.defer) hipLaunchKernelGGL((k_short<false, true>), grid, dim3(BLOCK), 0, st, sc, cam, pool, seed, a);
        else hipLaunchKernelGGL((k_short<false, false>), grid, dim3(BLOCK), 0, st, sc, cam, pool, seed, a);
    }
}
void launch_short_select(uint8_t* flags, uint32_t n_tiles, const uint32_t* pilot, uint32_t min_bin, uint32_t* hist, hipStream_t st) {
    hipLaunchKernelGGL(k_short_select, dim3(1), dim3(BLOCK), 0, st, flags, n_tiles, pilot, min_bin, hist);
}

}  // namespace pt
