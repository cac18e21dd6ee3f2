// K2: closest hit for every live slot of the pool — k_extend (batch form) and k_extend2 (two-phase form), with the flat top level and
// its pair passes. No sampler, pixel-list, environment or medium parameter reaches this stage.
#pragma once
#include "pt_k_trace.h"

namespace pt {

// Resident blocks per CU the batch form of K2 is compiled for. Its register count sits right at the 128-register step
// (4 waves per SIMD) and tipped over it with unrelated edits elsewhere in this file: measured on one build pair, scene 3's
// K2 was 10 % faster at four blocks than at three, scene 5's 16 % — so the bound is stated instead of left to chance.
#ifndef PT_EXTEND_BATCH_BLOCKS
#define PT_EXTEND_BATCH_BLOCKS 4
#endif

// ---- the FLAT top level (SceneD::tlas_flat: at most TLAS_FLAT_MAX world entries), walked by a whole wave ---------------------
// The wave loops over the entry list together — the entry index is wave-uniform, so boxes and entries arrive by scalar loads
// and there is no top-level stack. Round 2 measured what that loop cost when every entry whose box ANY lane entered was
// tested on the spot by the whole wave: 46 % of k_extend2's time on scene 6 (ten entries: each 64-ray chunk ran five sphere
// tests, one quad test and a cuboid's six, with a handful of lanes active in each). Now the box pass only RECORDS
// (ray, primitive) pairs — ray = lane of the chunk, primitive = global id, one pair per cuboid face — in a small per-wave ring
// in LDS, and whenever 64 pairs are waiting the wave tests them in ONE dense pass: lane i takes pair i, fetches that ray from
// its owner lane (ds_bpermute), transforms it into the primitive's frame and runs the primitive's exact f64 test. Results
// meet in LDS: minimum t per ray (64-bit LDS atomic min on the bits of the positive double), ties -> larger id (atomic max) —
// the same order-independent rule as consider(), so the hit is bit-identical. Mesh entries come second, their boxes trimmed
// by the non-mesh result.
#ifndef PT_PAIR_DENSE_MIN
#define PT_PAIR_DENSE_MIN 16        // lanes of a chunk in one entry's box from which the entry is tested on the spot (break-even of the two forms)
#endif
#ifndef PT_PAIR_PASS_ATTR
#define PT_PAIR_PASS_ATTR PT_DEV
#endif
#ifndef PT_FLAT_DIRECT
#define PT_FLAT_DIRECT 1            // 0: on-the-spot tests look the primitive up in prims[] (A/B)
#endif
#ifndef PT_CUBOID_CULL
#define PT_CUBOID_CULL 1            // 0: all six faces of a cuboid are tested (A/B)
#endif
#ifndef PT_PAIR_SINGLE
#define PT_PAIR_SINGLE 1            // 0: only cuboids (six faces behind one transform) go through the pair passes
#endif
constexpr int PAIR_CAP = 128;       // ring of waiting pairs per wave (a pass runs as soon as 64 wait, an append adds <= 64)
// pair word = id << 6 | lane: the host (pt_flatten.cpp) only sets tlas_flat when the ids of spheres / quads / cuboid faces are below 2^26
struct PairLds {                    // per wave
    unsigned long long* bt;         // [64] bits of the closest t so far of every ray of the chunk (+inf: none)
    uint32_t* bid;                  // [64] its primitive id
    uint32_t* pairs;                // [PAIR_CAP]
};
// LDS operations of one wave execute in issue order; this keeps the compiler from moving them across the steps of the protocol
PT_DEV void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
template <bool MOT = false>
PT_PAIR_PASS_ATTR void pair_pass(const SceneD& sc, const RayD& r, double t_min, int lane, const PairLds& L, uint32_t head, uint32_t n) {
    wave_lds_order();
    const bool mine = (uint32_t)lane < n;
    const uint32_t code = ((volatile uint32_t*)L.pairs)[(head + (uint32_t)lane) % PAIR_CAP];
    const int src = mine ? (int)(code & 63u) : lane;
    const uint32_t gid = code >> 6;
    const RayD pr_ray{V3{__shfl(r.o.x, src), __shfl(r.o.y, src), __shfl(r.o.z, src)}, V3{__shfl(r.d.x, src), __shfl(r.d.y, src), __shfl(r.d.z, src)},
                      __shfl(r.time, src)};
    bool hit = false;
    double t = 0.0;
    if (mine) {
        const PrimRef pr = sc.prims[gid];
        const RayD lr = ray_to_local_chain<false, MOT>(sc, pr.inst, pr_ray);
        if ((pr.kind & 0xFFu) == PRIM_SPHERE) {
            V3 c;
            hit = hit_sphere(sc.spheres[pr.index], lr, t_min, t, c);
        } else {
            double a, b;
            hit = hit_quad(sc.quads[pr.index], lr, t_min, t, a, b);
        }
    }
    // t > t_min > 0: the bits of t order like t. Every winner of this pass holds the pass's minimum, so all of them see the same
    // `before` and agree on whether the ray's closest t went down (older ids are void) or stayed (ids compete).
    const unsigned long long tb = (unsigned long long)__double_as_longlong(t);
    volatile unsigned long long* bt = L.bt;
    volatile uint32_t* bid = L.bid;
    unsigned long long before = 0ull;
    if (hit) before = bt[src];
    hit = hit && tb <= before;
    wave_lds_order();
    if (hit) atomicMin(&L.bt[src], tb);
    wave_lds_order();
    const bool win = hit && bt[src] == tb;
    if (win && tb < before) bid[src] = 0u;
    wave_lds_order();
    if (win) atomicMax(&L.bid[src], gid);
    wave_lds_order();
}
// Must be called by whole waves (`alive` = false for lanes without a ray). on_mesh(ei, entry, best): a lane's ray entered the
// box of mesh entry `ei` (wave-uniform index).
// PAIRS: cuboids few rays of the chunk enter go through the pair passes (L must be valid); false: everything on the spot.
// CULL: compile the cuboid face culling in (the instantiation for scenes without cuboids leaves it out: its registers spilled there).
// MOT: instances are posed at each lane's ray time (inst_at); face culling and the pair passes use the per-lane local ray they compute anyway.
// MASKED (k_short): the loop visits the entries whose bit is set in `reach` (bit k = SceneD::entry_box[k], wave-uniform,
// no bit at or above n_entries), in the same ascending order; an entry whose bit is 0 costs not even its box's load. false: every entry.
template <bool PAIRS, bool CULL, bool MOT = false, bool MASKED = false, class OnMesh>
PT_DEV Closest flat_top_level(const SceneD& sc, bool alive, const RayD& r, const RayF& f, double t_min, float t_min_f, int lane, const PairLds& L,
                              OnMesh&& on_mesh, uint32_t reach = 0xFFFFFFFFu) {
    if constexpr (PAIRS) {
        ((volatile unsigned long long*)L.bt)[lane] = (unsigned long long)__double_as_longlong(D_INF);
        ((volatile uint32_t*)L.bid)[lane] = HIT_NONE;
    }
    uint32_t head = 0, tail = 0;                                     // wave-uniform
    Closest best{D_INF, HIT_NONE};                                   // hits of the entries tested on the spot
    float t_max_f = t_max_f32(best.t);
    bool pairs_open = PAIRS;                                         // wave-uniform: pair results not yet merged into `best`
    auto close_pairs = [&]() {
        if (tail != head) pair_pass<MOT>(sc, r, t_min, lane, L, head, tail - head);
        if (tail != 0u) {                                            // some pass ran: its results join the on-the-spot ones (same rule)
            wave_lds_order();
            const double lt = __longlong_as_double((long long)((volatile unsigned long long*)L.bt)[lane]);
            if (lt < D_INF) consider(best, lt, ((volatile uint32_t*)L.bid)[lane]);
            t_max_f = t_max_f32(best.t);
        }
        pairs_open = false;
    };
    for (uint32_t k = 0; MASKED ? reach != 0u : k < sc.n_entries; ++k) {   // SceneD::entry_box: non-mesh entries first
        if constexpr (MASKED) {                                      // the lowest set bit is this turn's entry
            k = (uint32_t)__builtin_ctz(reach);
            reach &= reach - 1u;
        }
        const EntryBox bx = ldu(&sc.entry_box[k]);
        if (PAIRS && pairs_open && bx.kind == ENTRY_MESH) close_pairs();
        float tn;
        const bool hb = alive && slab_f32(bx.lo, bx.hi, f, t_min_f, t_max_f, tn);
        const unsigned long long m = __ballot(hb);
        if (m == 0ull) continue;
        if (bx.kind == ENTRY_MESH) {
            if (hb) {
                const Entry e{bx.kind, bx.first_prim, bx.inst, bx.blas_root, bx.extent, bx.n_prims, {0u, 0u}};
                on_mesh(bx.entry, e, best);
                t_max_f = t_max_f32(best.t);
            }
            continue;
        }
        const uint32_t n_faces = bx.kind == ENTRY_CUBOID ? 6u : 1u;  // cuboid.rs: six quads, linear
        const uint32_t cnt = (uint32_t)__popcll(m);
        if (!PAIRS || (!PT_PAIR_SINGLE && n_faces == 1u) || cnt >= (uint32_t)PT_PAIR_DENSE_MIN) {
            // a box many rays of the chunk enter: the test on the spot, with the primitive's record in scalar registers, is
            // cheaper than that many pairs — and its hits trim the boxes that follow
            if (CULL && PT_CUBOID_CULL && bx.kind == ENTRY_CUBOID && bx.prim_kind == PRIM_QUAD) {
                // the six faces behind one transform: only those the object-space ray can enter or leave through are tested, and
                // a face no lane of the chunk needs costs neither its 128-byte record nor its test (cuboid_face_mask)
                RayD lr{};
                uint32_t fm = 0u;
                if (hb) {
                    lr = ray_to_local_chain<true, MOT>(sc, bx.inst, r);
                    const CuboidBox cb = ldu(&sc.cuboid_box[k]);
                    fm = cuboid_face_mask(cb.lo, cb.hi, make_rayf(lr.o, lr.d, bx.extent), t_min_f, t_max_f);
                }
                for (uint32_t fi = 0; fi < 6u; ++fi) {
                    const bool need = (fm >> fi) & 1u;
                    if (__ballot(need) == 0ull) continue;
                    const QuadD qd = ldu(&sc.quads[bx.prim_index + fi]);
                    double t, a, b;
                    if (need && hit_quad(qd, lr, t_min, t, a, b)) consider(best, t, bx.first_prim + fi);
                }
                t_max_f = t_max_f32(best.t);
                continue;
            }
            if (hb) {
                const RayD lr = ray_to_local_chain<true, MOT>(sc, bx.inst, r);
                if (PT_FLAT_DIRECT && bx.prim_kind == PRIM_SPHERE) {
                    const SphereD sp = ldu(&sc.spheres[bx.prim_index]);
                    double t;
                    V3 c;
                    if (hit_sphere(sp, lr, t_min, t, c)) consider(best, t, bx.first_prim);
                } else if (PT_FLAT_DIRECT && bx.prim_kind == PRIM_QUAD) {
                    for (uint32_t fi = 0; fi < n_faces; ++fi) {
                        const QuadD qd = ldu(&sc.quads[bx.prim_index + fi]);
                        double t, a, b;
                        if (hit_quad(qd, lr, t_min, t, a, b)) consider(best, t, bx.first_prim + fi);
                    }
                } else {
                    for (uint32_t fi = 0; fi < n_faces; ++fi) test_world_prim<true>(sc, lr, t_min, bx.first_prim + fi, best);
                }
                t_max_f = t_max_f32(best.t);
            }
            continue;
        }
        if constexpr (PAIRS) {
            uint32_t fm = 0x3Fu;                                         // faces this lane's ray may hit (all, when not culled)
            if (CULL && PT_CUBOID_CULL && bx.kind == ENTRY_CUBOID && bx.prim_kind == PRIM_QUAD) {
                fm = 0u;
                if (hb) {
                    const RayD lr = ray_to_local_chain<true, MOT>(sc, bx.inst, r);
                    const CuboidBox cb = ldu(&sc.cuboid_box[k]);
                    fm = cuboid_face_mask(cb.lo, cb.hi, make_rayf(lr.o, lr.d, bx.extent), t_min_f, t_max_f);
                }
            }
            for (uint32_t fi = 0; fi < n_faces; ++fi) {
                const bool need = hb && ((fm >> fi) & 1u);
                const unsigned long long mf = __ballot(need);
                if (mf == 0ull) continue;
                const uint32_t rank = (uint32_t)__popcll(mf & ((1ull << lane) - 1ull));
                if (need) ((volatile uint32_t*)L.pairs)[(tail + rank) % PAIR_CAP] = ((bx.first_prim + fi) << 6) | (uint32_t)lane;
                tail += (uint32_t)__popcll(mf);
                if (tail - head >= 64u) {
                    pair_pass<MOT>(sc, r, t_min, lane, L, head, 64u);
                    head += 64u;
                }
            }
        }
    }
    if (PAIRS && pairs_open) close_pairs();
    return best;
}
template <bool PAIRS, bool MOT = false>
PT_DEV Closest closest_hit_flat(const SceneD& sc, bool alive, const RayD& r, double t_min, uint32_t* stk, int lane, const PairLds& L) {
    const float t_min_f = __double2float_rd(t_min);
    const RayF f = make_rayf(r.o, r.d, sc.tlas_extent);
    return flat_top_level<PAIRS, PAIRS, MOT>(sc, alive, r, f, t_min, t_min_f, lane, L,   // (the batch kernel's instantiation without pair passes serves scenes without cuboids)
                                [&](uint32_t, const Entry& e, Closest& best) { blas_pass<BLOCK, MOT>(sc, r, e, t_min, t_min_f, stk, TRAVERSAL_STACK, best); });
}

// K2, batch form: a fixed grid walks the pool with a grid-stride loop; each lane traverses one ray
// at a time, a wave moves on when its slowest lane is done. Lowest overhead; SIMD utilisation
// suffers when traversal lengths inside a wave differ a lot (sky ray next to a mesh ray). Used for
// scenes without meshes (and as the fallback for BVHs deeper than k_extend2's LDS stack).
// FLAT: SceneD::tlas_flat. PAIRS (FLAT only): SceneD::flat_pairs — the scene has cuboids, whose six faces behind one transform
// are what the pair passes of flat_top_level pay for (scene 3: K2 -19 %, scene 7: -11 %); that instantiation runs three blocks
// per CU (its extra state spills at 128 registers and costs more than the fourth block brings), the others four.
// MOT: motion is in effect (pt_amd.h): instances are posed at each ray's time. Forms of their own, so that the others stay what they were.
template <bool FLAT, bool PAIRS, bool MOT = false>
__global__ __launch_bounds__(BLOCK, PAIRS ? 3 : PT_EXTEND_BATCH_BLOCKS) void k_extend(SceneD sc, PoolD pool, CountersD* cnt) {
    __shared__ uint32_t stack[TRAVERSAL_STACK * BLOCK];
    __shared__ unsigned long long s_pair_t[PAIRS ? BLOCK : 1];
    __shared__ uint32_t s_pair_id[PAIRS ? BLOCK : 1], s_pairs[PAIRS ? (BLOCK / 64) * PAIR_CAP : 1];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const PairLds pl{&s_pair_t[PAIRS ? wave * 64 : 0], &s_pair_id[PAIRS ? wave * 64 : 0], &s_pairs[PAIRS ? wave * PAIR_CAP : 0]};
    unsigned long long nseg = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->win_shade = 0;
    if (ldu(&cnt->alive) == 0ull) return;   // the frame is done: the launches the host had already queued behind its last poll cost a few microseconds each
    // n_alloc is a multiple of BLOCK: whole waves run every chunk (closest_hit_flat ballots)
    for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < pool.n_alloc; s += gridDim.x * BLOCK) {
        const uint32_t state = pool.bounce[s];
        const bool alive = state < SLOT_IDLE;
        RayD r{};
        if (alive) r = load_ray(pool, s);
        Closest c{D_INF, HIT_NONE};
        if (FLAT) c = closest_hit_flat<PAIRS, MOT>(sc, alive, r, 1e-3, &stack[threadIdx.x], lane, pl);   // camera.rs:171,179
        else if (alive) c = closest_hit<MOT>(sc, r, 1e-3, &stack[threadIdx.x]);
        stnt(&pool.hit_prim[s], hit_word(sc, alive ? c.id : dead_or_idle(state)));
        if (alive) ++nseg;
    }
    nseg = wave_sum(nseg);
    if (nseg && (threadIdx.x & 63u) == 0u) atomicAdd(&cnt->segments, nseg);
}

// ---------------------------------------------------------------------------------------
// K2, two-phase form (default). The batch kernel above leaves most lanes idle: a sky ray is done
// after ~5 steps while a lane next to it walks a mesh for 50-150 (17 % VALU lane utilisation in the
// first profile). Here a block takes a WINDOW of 2048 slots and
//   phase A: every ray walks only the TOP-LEVEL tree; spheres / quads / cuboids are intersected on
//            the spot, mesh instances whose box it enters are only RECORDED (<= 4 per ray, in LDS);
//   phase B: the rays that recorded something are compacted into an LDS list and the block's waves
//            draw from it (work stealing): each lane walks the recorded meshes of its ray one after
//            the other, starting from the phase-A best hit, and takes the next ray of the list when
//            it is done (lanes are refilled, a wave does not wait for the longest ray of a group).
// Rays that never touch a mesh finish in the short, uniform phase A; the long mesh traversals run in
// dense waves whose lanes all do the same kind of work. The closest hit is order-independent
// (minimum t, ties -> larger id), so the result is bit-identical to the batch kernel's.
// ---------------------------------------------------------------------------------------
// The phase-A best hit of a ray waits in LDS (t and id), and the window's final primitive ids leave
// with ONE coalesced store per slot: k_shade re-intersects the primitive (reconstruct_hit) and never
// needs t, so 4 B per slot is all this kernel writes.
// LDS per block: STACK x 1 KB (traversal stacks) + 18.5 KB, STACK in {16, 20, 24}: the host picks the
// smallest that covers the scene (pt_scene::stack_need_extend2 — only the deepest mesh tree when the top
// level is walked flat); deeper scenes use the batch kernel. The kernel runs three blocks per CU: a
// fourth would cap it at 128 registers and the spills cost more than the extra waves bring (measured).
// Tried and dropped: the two phases as two kernels with a global candidate list; every
// wave on its own 256-slot window without block barriers; warming the next window's ray lines.
#ifndef PT_TAIL_SPLIT
#define PT_TAIL_SPLIT 1             // 0: whole windows to the end of k_extend2's queue (A/B)
#endif
#ifndef PT_TAIL_PARTS
#define PT_TAIL_PARTS 2             // rounds a tail window is handed out in (2: halves, 4: quarters)
#endif
#ifndef PT_TAIL_SPAN
#define PT_TAIL_SPAN 1              // tail = the last PT_TAIL_SPAN windows per block launched
#endif
#ifndef PT_K2_REVERSE
#define PT_K2_REVERSE 1
#endif
#ifndef PT_K2_PREFETCH
#define PT_K2_PREFETCH 0              // 1: phase A holds the next chunk's ray in registers while it walks the current one — the round-1 form,
#endif                               // which at 128 registers costs 60 B of spills per lane: without it K2 runs 7 % faster and writes 0.46 GB less

constexpr int EXT_WINDOW = 2048;   // slots per block window
#ifndef PT_REFILL_MIN
#define PT_REFILL_MIN 16
#endif
constexpr uint32_t REFILL_MIN = PT_REFILL_MIN;   // idle lanes that trigger a refill of the wave in phase B
#ifndef PT_EXT_CAND
#define PT_EXT_CAND 768
#endif
#ifndef PT_EXT_CAND_SMALL
#define PT_EXT_CAND_SMALL 1024
#endif
// Candidate list per 2048 slots (LDS; scaled with the block size); a fuller window walks the rest in phase A, one mesh after the other
// inside the divergent top-level code — expensive: scene 6, 128-thread blocks: 512 entries K2 +8.6 %, 768 (37.5 % of the window, the
// round-1 choice) the reference, 1024 -2.3 %. The 128-thread form has the LDS for 1024 (19.5 KB per block, eight blocks per CU); the
// 256-thread forms with their deeper stacks stay at 768.
// [r27] Those figures are of a pool nearly half sky and ground rays. Since the sky and short-path passes took those away, 17.6 % of the headline
// frame's candidates found the list full; a full window now hands a list that fills early to phase B in mid-window (k_extend2, "rounds of a window").
constexpr int EXT_CAND = PT_EXT_CAND, EXT_CAND_SMALL = PT_EXT_CAND_SMALL;
static_assert(EXT_WINDOW % BLOCK == 0 && EXT_WINDOW <= 65536, "k_extend2: s_cand_sl holds 16-bit slot offsets inside the window");
static_assert(EXT_WINDOW == SORT_WINDOW_SLOTS, "the pool is allocated in whole windows of this size (pt_render.cpp rounds n_alloc to 2048)");

#ifdef PT_STAMPS   // diagnostic build: the cycles since the last lap go to `acc` (k_extend2's phases, summed over a window's rounds)
#define K2_LAP(acc) do { const unsigned long long t_now = stamp(); acc += t_now - t_lap; t_lap = t_now; } while (0)
#else
#define K2_LAP(acc)
#endif
constexpr uint32_t K2_SPLIT_OFF = 0, K2_SPLIT_HALF = 1, K2_SPLIT_DRAIN = 2;   // k_extend2's `split` (PT_K2_SPLIT; pt_render.cpp Switches::k2_split)
// KB: threads per block (256; [r3] other sizes for A/B — the window and the candidate list scale with it; MINB = waves per SIMD, which is what hipcc's launch bound means)
// MOT: as in k_extend
// split ("rounds of a window"): K2_SPLIT_OFF / K2_SPLIT_HALF / K2_SPLIT_DRAIN — whether a full window's phase A may stop at a
// chunk boundary and hand the list it has to phase B (wave-uniform: a kernel argument)
template <int EXT_STACK, int MINB, int KB = BLOCK, bool MOT = false>
__global__ __launch_bounds__(KB, MINB) void k_extend2(SceneD sc, PoolD pool, CountersD* cnt, uint32_t split) {
    constexpr int WIN = EXT_WINDOW / BLOCK * KB, CAND = (KB <= 128 ? EXT_CAND_SMALL : EXT_CAND) / BLOCK * KB;
    constexpr int NSEG = WIN / KB + 1;                             // a window's phase A has at most one segment per chunk
    __shared__ uint32_t stack[EXT_STACK * KB];
    __shared__ uint32_t s_best_id[WIN];                            //  8 KB  closest primitive of every slot of the window
    __shared__ double s_cand_t[CAND];                              //  6 KB  candidates (rays that entered mesh boxes): phase-A best t,
    __shared__ uint32_t s_cand_items[CAND];                        //  3 KB  recorded mesh entries, 8 bit each, 0xFF = none,
    __shared__ uint16_t s_cand_sl[CAND];                           //        slot inside the window
    // s_seg[g]: the candidates phase A found in SEGMENT g of the window — the chunks between two of its barriers. A segment's appends count
    // into a word of their own, so the words of the segments before it are final from their barrier to the window's end: every thread
    // reads the same number from them however late it reads (a single counter would already hold the next segment's first appends).
    __shared__ uint32_t s_seg[NSEG], s_next, s_win, s_stat[2];     // s_stat: this block's {mid-window rounds, overflow rays}, thread 0's
    uint32_t* stk = &stack[threadIdx.x];
    const int lane = (int)(threadIdx.x & 63u);
    const double t_min = 1e-3;                                     // camera.rs:171,179
    const float t_min_f = __double2float_rd(t_min);
    unsigned long long nseg = 0;
    const uint32_t n_windows = pool.n_alloc / WIN;
    // [r3] The queue's END is handed out in HALF windows (PT_TAIL_SPLIT): with ~16 windows per block and launch a block idles half a
    // window on average while the last ones finish; the last gridDim.x windows go out as two rounds of four chunks each, so the spread
    // at the launch's end is half as long: K2 -0.8 % on the 33.6 M-slot pool, -2.1 % on a 16.8 M-slot one (quarters: +2 %; the last TWO
    // windows per block in halves: +1.4 %; both: +5 % — PT_TAIL_PARTS / PT_TAIL_SPAN)
    constexpr uint32_t PARTS = PT_TAIL_SPLIT ? PT_TAIL_PARTS : 1, CH = (uint32_t)(WIN / KB) / PARTS;   // rounds per tail window, chunks per round
    static_assert(PARTS * CH == (uint32_t)(WIN / KB), "");
    const uint32_t n_tail = PT_TAIL_SPLIT ? (n_windows < gridDim.x * PT_TAIL_SPAN ? n_windows : gridDim.x * PT_TAIL_SPAN) : 0u;
    const uint32_t n_full = n_windows - n_tail, n_queue = n_full + PARTS * n_tail;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->win_shade = 0;
    if (ldu(&cnt->alive) == 0ull) return;   // (see k_extend)
#ifdef PT_STAMPS
    if (threadIdx.x < PROF_COLS) g_prof[CLASS_DEAD][threadIdx.x] = 0ull;
#endif
    // (the next window's index is drawn before the barrier that ends a window and published by it: see k_shade)
    if (threadIdx.x == 0) { s_win = (uint32_t)atomicAdd(&cnt->win_extend, 1ull); s_next = 0; s_stat[0] = 0; s_stat[1] = 0; }
    if (threadIdx.x < (uint32_t)NSEG) s_seg[threadIdx.x] = 0;
    __syncthreads();
    for (;;) {
        const uint32_t q = s_win;
        if (q >= n_queue) break;
        const uint32_t win = q < n_full ? q : n_full + (q - n_full) / PARTS;
        const int j_lo = q < n_full ? 0 : (int)(((q - n_full) % PARTS) * CH), j_hi = q < n_full ? WIN / KB : j_lo + (int)CH;   // this round's chunks
        // [r3] K2 walks the pool from its END, k_shade from its beginning: each kernel starts on the windows the other touched last,
        // i.e. on what the 256 MB memory-side cache still holds of the 3-5 GB the previous launch streamed (PT_K2_REVERSE=0: A/B)
        const uint32_t wbase = (PT_K2_REVERSE ? n_windows - 1u - win : win) * WIN;
        // ---- rounds of a window ------------------------------------------------------------------------
        // A window that is mostly mesh fills the list before phase A ends, and what does not fit is walked where it is found (below): in
        // divergent code, without refill. So a FULL window (tail rounds are half windows already) may hand the list to phase B early:
        //   K2_SPLIT_HALF   after half of its chunks, when the list holds more than CAND / 2 rays. In the 128-thread form half a window is
        //                   CAND slots: neither round of a split window can overflow, and each holds more than CAND / 2 rays. A window
        //                   whose first half stays at or below CAND / 2 is not split and may still overflow in its second half.
        //   K2_SPLIT_DRAIN  after every chunk from chunk CAND / KB on, when the list holds more than CAND - KB rays: no full window overflows
        //                   (a tail round of the 256-thread forms — 1024 slots, a list of 768 — still can, under every rule).
        // Invariants. (1) The decision is block-uniform: it is n_list, the sum of the s_seg words of the segments that have ended, each read
        // behind the barrier that ended it and written by nobody until the window's end — so every thread takes the same barriers.
        // (2) A round's list is reused only behind a barrier that follows its phase B. (3) s_best_id covers the whole window; a round's
        // phase B writes the slots of its own candidates only. (4) A ray's tests keep their order — non-mesh entries, then its meshes in
        // item order — whichever round walks it, so every hit word keeps its bits.
        const int j_rule = q >= n_full || split == K2_SPLIT_OFF ? j_hi : split == K2_SPLIT_HALF ? j_lo + (j_hi - j_lo) / 2 : CAND / KB;
        const uint32_t n_rule = split == K2_SPLIT_HALF ? (uint32_t)CAND / 2u : (uint32_t)(CAND - KB);
        uint32_t n_list = 0, seg = 0;                                // block-uniform: the list's rays at the last barrier, the current segment
#ifdef PT_STAMPS
        unsigned long long t_lap = stamp(), p_a = 0, p_wa = 0, p_b = 0, p_wb = 0, p_over = 0;
        uint32_t n_walked = 0, n_window = 0;
#endif
        // ---- phase B: mesh traversals, 64 rays per pull ------------------------------------------------
        auto phase_b = [&](const uint32_t n_rays) {
            // Lanes are refilled: a lane whose ray is done does not wait for the longest ray of a fixed group of 64 —
            // when at least REFILL_MIN lanes of the wave are idle they draw the next candidates from the list (one
            // LDS atomic per wave) and the wave goes on with every lane at its own ray. s_next counts RAYS here.
            bool busy = false, exhausted = false;                   // exhausted: wave-uniform, the list has run out
            uint32_t sl = 0, items = 0, item_k = 0, cur = REF_EMPTY, first_prim = 0;
            int sp = 0;
            RayD wr{}, r{};
            RayF f{};
            Closest best{D_INF, HIT_NONE};
            float t_max_f = 0.0f;
            auto start_item = [&]() -> bool {                       // enters mesh number item_k of this lane's ray, if any
                const uint32_t ei = item_k < 4u ? (items >> (8u * item_k)) & 0xFFu : 0xFFu;
                if (ei == 0xFFu) return false;
                const Entry e = sc.entries[ei];
                r = ray_to_local_chain<false, MOT>(sc, e.inst, wr);
                first_prim = e.first_prim;
                f = make_rayf(r.o, r.d, e.extent);
                t_max_f = t_max_f32(best.t);
                cur = e.blas_root;
                sp = 0;
                return true;
            };
            for (;;) {
                const unsigned long long idle = __ballot(!busy);
                const uint32_t n_idle = (uint32_t)__popcll(idle);
                if (!exhausted && (n_idle >= REFILL_MIN || n_idle == 64u)) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&s_next, n_idle);
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    exhausted = base + n_idle >= n_rays;
                    if (!busy) {
                        const uint32_t idx = base + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                        if (idx < n_rays) {
                            sl = s_cand_sl[idx];
                            items = s_cand_items[idx];
                            wr = load_ray(pool, wbase + sl);
                            best = Closest{s_cand_t[idx], s_best_id[sl]};
                            item_k = 0;
                            busy = start_item();                    // a candidate always has at least one item
                        }
                    }
                }
                if (__ballot(busy) == 0ull) {
                    if (exhausted) break;
                    continue;                                       // everybody idle: the refill above was forced, go again
                }
                // descend until every busy lane holds a triangle leaf or has run out of nodes in this mesh
                while (busy && (cur & REF_TYPE_MASK) == REF_NODE) {
                    uint32_t c0, c1;
                    const int n = visit_node(&sc.nodes[cur], f, t_min_f, t_max_f, c0, c1);
                    if (n == 2 && sp < EXT_STACK) stk[(sp++) * KB] = c1;
                    if (n > 0) cur = c0;
                    else if (sp > 0) cur = stk[(--sp) * KB];
                    else cur = REF_EMPTY;
                }
                if (busy) {
                    if ((cur & REF_TYPE_MASK) == REF_TRIS) {
                        const uint32_t first = cur & 0x07FFFFFFu, count = ((cur >> 27) & 7u) + 1u;
                        test_leaf(sc, first, count, r, t_min, first_prim, best);
                        t_max_f = t_max_f32(best.t);
                        cur = sp > 0 ? stk[(--sp) * KB] : REF_EMPTY;
                    }
                    if (cur == REF_EMPTY) {                         // this mesh is done: the ray's next mesh, or the ray is done
                        ++item_k;
                        if (!start_item()) {
                            s_best_id[sl] = best.id;
                            busy = false;
                        }
                    }
                }
            }
        };
        // ---- phase A: top level only ---------------------------------------------------------------
        // (PT_K2_PREFETCH: the ray of the NEXT chunk requested before this chunk's traversal starts)
#if PT_K2_PREFETCH
        uint32_t state_next = pool.bounce[wbase + (uint32_t)j_lo * KB + threadIdx.x];
        RayD r_next{};
        if (state_next < SLOT_IDLE) r_next = load_ray(pool, wbase + (uint32_t)j_lo * KB + threadIdx.x);
#endif
        for (int j = j_lo; j < j_hi; ++j) {
            const uint32_t sl = (uint32_t)j * KB + threadIdx.x;
#if PT_K2_PREFETCH
            const uint32_t state = state_next;
            const bool alive = state < SLOT_IDLE;
            const RayD r = r_next;
            if (j + 1 < j_hi) {
                state_next = pool.bounce[wbase + sl + KB];
                if (state_next < SLOT_IDLE) r_next = load_ray(pool, wbase + sl + KB);
            }
#else
            const uint32_t state = pool.bounce[wbase + sl];
            const bool alive = state < SLOT_IDLE;
            RayD r{};
            if (alive) r = load_ray(pool, wbase + sl);
#endif
            uint32_t n_my = 0, items = 0xFFFFFFFFu;
            RayF f{};
            Closest best{D_INF, HIT_NONE};
            float t_max_f = t_max_f32(best.t);
            if (alive) {
                ++nseg;
                f = make_rayf(r.o, r.d, sc.tlas_extent);
            }
            // one world entry whose box the ray enters: meshes are recorded, everything else is tested on the spot
            auto visit_entry = [&](auto uniform, uint32_t ei, const Entry& e, int sp) {   // uniform: ei is the same in every lane
                constexpr bool U = decltype(uniform)::value;
                if (e.kind == ENTRY_MESH) {
                    if (n_my < 4u && ei < 0xFFu) {
                        items = (items & ~(0xFFu << (8u * n_my))) | (ei << (8u * n_my));   // defer to phase B
                        ++n_my;
                    } else {
                        blas_pass<KB, MOT>(sc, r, e, t_min, t_min_f, stk + (size_t)sp * KB, EXT_STACK - sp, best);   // a fifth mesh / a wide index: walk it now
                        t_max_f = t_max_f32(best.t);
                    }
                } else {
                    const RayD lr = ray_to_local_chain<U, MOT>(sc, e.inst, r);
                    const uint32_t n = e.kind == ENTRY_CUBOID ? 6u : 1u;       // cuboid.rs: six quads, linear
                    for (uint32_t i = 0; i < n; ++i) test_world_prim<U>(sc, lr, t_min, e.first_prim + i, best);
                    t_max_f = t_max_f32(best.t);
                }
            };
            if (sc.tlas_flat) {
                // Small top level: the wave walks the ENTRY LIST together instead of each lane walking the tree
                // (flat_top_level; the pair passes are left to the batch kernel: measured slower here, scene 6).
                best = flat_top_level<false, true, MOT>(sc, alive, r, f, t_min, t_min_f, lane, PairLds{}, [&](uint32_t ei, const Entry& e, Closest& b) {
                    best = b;                                       // visit_entry works on this frame's `best`
                    visit_entry(std::true_type{}, ei, e, 0);
                    b = best;
                });
            } else if (alive) {
                int sp = 0;
                uint32_t cur = sc.tlas_root;
                for (;;) {
                    if ((cur & REF_TYPE_MASK) == REF_NODE) {
                        uint32_t c0, c1;
                        const int n = visit_node(&sc.nodes[cur], f, t_min_f, t_max_f, c0, c1);
                        if (n == 2 && sp < EXT_STACK) stk[(sp++) * KB] = c1;
                        if (n > 0) {
                            cur = c0;
                            continue;
                        }
                    } else if ((cur & REF_TYPE_MASK) == REF_ENTRY) {
                        const uint32_t ei = cur & 0x3FFFFFFFu;
                        visit_entry(std::false_type{}, ei, sc.entries[ei], sp);
                    }
                    if (sp == 0) break;
                    cur = stk[(--sp) * KB];
                }
            }
            // append the rays that recorded meshes to the window's candidate list (one LDS atomic per wave, slot
            // order kept inside the wave); when the list is full — a window that is nearly all mesh — walk them now
            const unsigned long long m = __ballot(n_my > 0);
            if (m) {
                const int leader = __ffsll((long long)m) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(&s_seg[seg], (uint32_t)__popcll(m));
                base = n_list + (uint32_t)__shfl((int)base, leader);
#ifdef PT_STAMPS
                const bool walks = __ballot(n_my > 0 && base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) >= (uint32_t)CAND) != 0ull;
                const unsigned long long t_walk = walks ? stamp() : 0ull;
#endif
                if (n_my > 0) {
                    const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (pos < (uint32_t)CAND) {
                        s_cand_t[pos] = best.t;
                        s_cand_items[pos] = items;
                        s_cand_sl[pos] = (uint16_t)sl;
                    } else {
                        for (uint32_t k = 0; k < n_my; ++k) blas_pass<KB, MOT>(sc, r, sc.entries[(items >> (8u * k)) & 0xFFu], t_min, t_min_f, stk, EXT_STACK, best);
                    }
                }
#ifdef PT_STAMPS
                if (walks) p_over += stamp() - t_walk;
#endif
            }
            s_best_id[sl] = alive ? best.id : dead_or_idle(state);
            // ---- the segment's end: the window's last chunk, or a chunk boundary at which the rule is applied (see "rounds of a window")
            const int jn = j + 1;
            const bool last = jn == j_hi;
            if (!last && !(split == K2_SPLIT_DRAIN ? jn >= j_rule : jn == j_rule)) continue;
            K2_LAP(p_a);
            __syncthreads();
            K2_LAP(p_wa);
            n_list += (uint32_t)__builtin_amdgcn_readfirstlane((int)s_seg[seg]);
            ++seg;
            if (!last && n_list <= n_rule) continue;             // the window goes on unsplit: one barrier was all it cost
            const uint32_t n_over = n_list > (uint32_t)CAND ? n_list - (uint32_t)CAND : 0u;   // the rays phase A walked for want of room
            if (threadIdx.x == 0) { s_stat[0] += last ? 0u : 1u; s_stat[1] += n_over; }
#ifdef PT_STAMPS
            n_walked += n_over;
            n_window += n_list;
#endif
            phase_b(n_list - n_over);
            K2_LAP(p_b);
            if (last) break;
            __syncthreads();                                       // every wave has left this round's list
            K2_LAP(p_wb);
            if (threadIdx.x == 0) s_next = 0;                      // (read again behind the barrier that ends the next segment)
            n_list = 0;
        }
        __syncthreads();
        K2_LAP(p_wb);
#ifdef PT_STAMPS
        // K2's row of the profile: CLASS_DEAD (k_shade never runs a group of that class). Per wave: [0] windows, [1] phase A, [2] its barriers,
        // [3] phase B, [4] its barriers, [5] rays phase B walked, [7] cycles of the chunks' ends in which a lane walked for want of room
        // (inside [1]). Per block: [6] the rays walked so, [8 + b / 2] the full windows whose candidates fill b eighths of the window
        // (b = 0 .. 8; even b in the low 32 bits, odd b in the high)
        if (lane == 0) {
            atomicAdd(&g_prof[CLASS_DEAD][0], 1ull);
            atomicAdd(&g_prof[CLASS_DEAD][1], p_a);
            atomicAdd(&g_prof[CLASS_DEAD][2], p_wa);
            atomicAdd(&g_prof[CLASS_DEAD][3], p_b);
            atomicAdd(&g_prof[CLASS_DEAD][4], p_wb);
            atomicAdd(&g_prof[CLASS_DEAD][5], (unsigned long long)(n_window - n_walked));
            atomicAdd(&g_prof[CLASS_DEAD][7], p_over);
        }
        if (threadIdx.x == 0) {
            atomicAdd(&g_prof[CLASS_DEAD][6], (unsigned long long)n_walked);
            const uint32_t bin = n_window * 8u / (uint32_t)WIN;
            if (q < n_full) atomicAdd(&g_prof[CLASS_DEAD][8 + bin / 2u], 1ull << (32u * (bin & 1u)));
        }
#endif
        {   // the window's result: one coalesced 4-byte store per slot; the eight PrimRef gathers (material class) go out together
            uint32_t word[WIN / KB];
#pragma unroll
            for (int j = 0; j < WIN / KB; ++j) word[j] = (j >= j_lo && j < j_hi) ? hit_word(sc, s_best_id[(uint32_t)j * KB + threadIdx.x]) : 0u;
#pragma unroll
            for (int j = 0; j < WIN / KB; ++j) if (j >= j_lo && j < j_hi) stnt(&pool.hit_prim[wbase + (uint32_t)j * KB + threadIdx.x], word[j]);
        }
        if (threadIdx.x == 0) { s_win = (uint32_t)atomicAdd(&cnt->win_extend, 1ull); s_next = 0; }   // all of this window's uses are behind the barrier above
        if (threadIdx.x < (uint32_t)NSEG) s_seg[threadIdx.x] = 0;
        __syncthreads();   // LDS lists are reused by the next window
    }
    nseg = wave_sum(nseg);
    if (nseg && (threadIdx.x & 63u) == 0u) atomicAdd(&cnt->segments, nseg);
    if (threadIdx.x == 0) {                                         // pt_render_stats::k2_split_windows, k2_overflow_rays
        if (s_stat[0]) atomicAdd(&cnt->k2_split_windows, (unsigned long long)s_stat[0]);
        if (s_stat[1]) atomicAdd(&cnt->k2_overflow_rays, (unsigned long long)s_stat[1]);
    }
#ifdef PT_STAMPS
    __syncthreads();
    if (threadIdx.x < PROF_COLS && g_prof[CLASS_DEAD][threadIdx.x]) atomicAdd(&cnt->prof[CLASS_DEAD][threadIdx.x], g_prof[CLASS_DEAD][threadIdx.x]);
#endif
}

}  // namespace pt
