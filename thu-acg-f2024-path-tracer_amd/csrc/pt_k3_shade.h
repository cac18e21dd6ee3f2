// K1: k_init, the raygen kernel that fills the pool with the first sample of every slot.
// K3: k_shade — one bounce of every path of the pool (shade_slot), its windowed class sort and the LDS staging of the next group's records.
#pragma once
#include "pt_k_common.h"
#include "pt_dev_lights.h"
#include "pt_dev_dispersion.h"
#include "pt_dev_punctual.h"

namespace pt {

// ---------------------------------------------------------------------------------------
// LIST: pixel-list render (PoolD::list)
// QMC: the Sobol sampler (pt_scene_set_sampler; RngQ in pt_dev_math.h) — forms of their own, compiled in pt_k3_qmc.hip
// MED: participating media are in effect — a camera ray's bounce word carries the camera medium (pt_types.h MEDIUM_SHIFT);
// forms of their own, compiled in pt_k3_med.hip
// MOT: motion is in effect — generate_ray applies the shutter; forms of their own, compiled in pt_k3_mot.hip
template <bool LIST = false, bool QMC = false, bool MED = false, bool MOT = false>
__global__ __launch_bounds__(BLOCK) void k_init(CamD cam, PoolD pool, uint64_t seed) {
    const uint32_t bounce0 = MED ? cam.medium << MEDIUM_SHIFT : 0u;   // the bounce word of a camera ray
    for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < pool.n_alloc; s += gridDim.x * BLOCK) {
        uint32_t pixel, sample, row = 0, col = 0;
        bool has_work;
        bool idle = false;
        if (pool.dynamic) {   // initial work items 0 .. n_slots-1 (the host starts the shard counters there)
            // experiment (PT_INIT_SHUFFLE): inside every whole 8192-slot granule below n_slots, slot s takes item
            // granule + (s * init_perm mod 8192) — an odd multiplier permutes the granule, so the same items are handed out
            uint32_t item = s;
            if (pool.init_perm != 0u && s < (pool.n_slots & ~8191u)) item = (s & ~8191u) | ((s * pool.init_perm) & 8191u);
            has_work = s < pool.n_slots && (unsigned long long)item < pool.total_work;
            idle = has_work && !work_item<LIST, sky_pass_form(LIST, MED ? MODE_MED : MODE_PLAIN, QMC, MOT)>(pool, item, pixel, sample, row, col);
            if (!has_work || idle) { pixel = 0; sample = 0; }
        } else {
            pixel = slot_pixel<LIST>(pool, s);
            sample = pool.spp_begin + s / (LIST ? pool.n_list : pool.n_pixels);
            divmod_u31(pixel, cam.width, row, col);
            has_work = s < pool.n_slots && sample < pool.spp_end;
            pool.ax[s] = 0.0; pool.ay[s] = 0.0; pool.az[s] = 0.0;
            pool.rx[s] = 0.0; pool.ry[s] = 0.0; pool.rz[s] = 0.0;
        }
        pool.hit_prim[s] = (CLASS_DEAD << HIT_CLASS_SHIFT) | HIT_ID_MASK;   // overwritten by the first K2 launch
        if (!pool.compact) store_path(pool.path, s, V3{1.0, 1.0, 1.0}, pixel, bounce0);
        if (!has_work || idle) {
            pool.bounce[s] = idle ? SLOT_IDLE : SLOT_DEAD;
            store_ray(pool, pool.ray, s, RayD{}, sample, 0u, pixel, 0u);
            continue;
        }
        std::conditional_t<QMC, RngQ, Rng> rng{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample, 0u};
        RayD r = generate_ray<MOT>(cam, row, col, rng);
        store_ray(pool, pool.ray, s, r, sample, rng.draw, pixel, bounce0);
        pool.bounce[s] = 0;
    }
}

// K3: the body of camera.rs:177-226 for the path in slot `s`, executed by all 64 lanes of a wave
// together (it contains wave-level ballots for the work-counter dequeue, K5).
// color += throughput * emitted (camera.rs:182,187). Static mode: into the sample's own sum, which reaches
// the pixel when the sample ends (the reference's order of additions). Dynamic mode: straight into the
// frame accumulator — exact zeros are skipped, NaN/inf are not (they poison the pixel like they do there).
PT_DEV void add_radiance(const PoolD& pool, uint32_t pixel, V3& rad, V3 c) {
    if (!pool.dynamic) {
        rad = rad + c;
    } else if (!(c.x == 0.0 && c.y == 0.0 && c.z == 0.0)) {
        if (pool.accum_tiled) {
            double* a = pool.accum + tiled_index(pool, pixel);
            unsafeAtomicAdd(a, c.x);
            unsafeAtomicAdd(a + pool.n_tile_pixels, c.y);
            unsafeAtomicAdd(a + 2 * (size_t)pool.n_tile_pixels, c.z);
        } else {
            unsafeAtomicAdd(&pool.accum[3 * (size_t)pixel], c.x);
            unsafeAtomicAdd(&pool.accum[3 * (size_t)pixel + 1], c.y);
            unsafeAtomicAdd(&pool.accum[3 * (size_t)pixel + 2], c.z);
        }
    }
}

// ---- path records of one slot as k_shade consumes them -------------------------------------------------------------
struct SlotIn {
    uint32_t bounce, hw, pixel, sample, draw;   // state, K2's result word, pixel (dynamic mode), sample index, RNG draw counter
    V3 thr;
    RayD ray;
};
// straight from the pool (first group of a window, static mode, unsorted K3). `enable` = false: bystander lane.
// `hw_known`: the caller has the slot's result word already (k_shade's sort keeps the window's words in LDS).
// Whether a slot is alive, idle or dead is in the class of K2's result word (K2 read PoolD::bounce, the slots' STATE array,
// coalesced); the bounce NUMBER of a live path travels in its PathRec. k_shade therefore never reads the state array and, in
// place, writes it only when a slot changes state (parked, regenerated from idle, dead) — it used to gather 4 bytes per lane from
// it and scatter 4 bytes per lane back on every bounce of every path. (In shading order, PoolD::reorder, every position gets its
// state: 4 bytes per lane at consecutive addresses.)
PT_DEV uint32_t state_of_class(uint32_t hw) {
    const uint32_t cls = hw >> HIT_CLASS_SHIFT;
    return cls == CLASS_IDLE ? SLOT_IDLE : cls == CLASS_DEAD ? SLOT_DEAD : 0u;
}
PT_DEV SlotIn load_slot_global(const PoolD& pool, uint32_t s, bool enable, const uint32_t* hw_known = nullptr) {
    SlotIn in{};
    in.hw = hw_known ? *hw_known : pool.hit_prim[s];
    in.bounce = enable ? state_of_class(in.hw) : SLOT_DEAD;
    if (in.bounce < SLOT_IDLE) {
        uint32_t tail[2];
        in.ray = load_ray(pool, s, in.sample, in.draw, tail);
        if (pool.compact) {
            in.pixel = tail[0];
            in.bounce = tail[1];
            in.thr = V3{1.0, 1.0, 1.0};
            uint32_t p2, b2;
            if (in.bounce != 0u) in.thr = load_path(pool, s, p2, b2);      // a path at bounce 0 has no PathRec
        } else {
            in.thr = load_path(pool, s, in.pixel, in.bounce);
        }
    }
    return in;
}
// Asynchronous fetch of a group's records into the wave's LDS staging area: `global_load_lds` (LDS-DMA) — the data goes
// from HBM to LDS without passing through (or occupying) a single vector register, which is the only way this kernel, at its
// 256-register limit, can have the NEXT group's 6 KB in flight while it computes on the current one.
// [r3] WHOLE SECTORS per instruction. A lane used to fetch the six 16-byte pieces of ITS OWN records, so every wave-instruction
// touched 64 different 64-byte sectors for 16 bytes each and every sector was requested by four instructions (the L2 saw 4x the
// transactions, and a streaming cache policy could not be used: the pieces of a record must find the sector their sibling
// fetched). Now instruction k serves the records of lanes 16k .. 16k+15 with FOUR lanes per RayRec (two per PathRec), each
// fetching a different piece: 16 (32) whole sectors per instruction, every byte requested exactly once. The LDS image —
// wave-uniform base + lane * 16, as the instruction writes — is then simply the records in lane order: RayRec of lane l at
// stage[4 l .. 4 l + 3], PathRec at stage[256 + 2 l ..]. The slots of the other lanes come by ds_bpermute.
// Must be executed by ALL 64 lanes (wave-uniform control flow).
#ifndef PT_UNIFORM_GROUPS
#define PT_UNIFORM_GROUPS 3         // bit 0: the hit of a single-primitive group by scalar loads, bit 1: its material fields and texture descriptor too; 0: every group per lane (for A/B)
#endif
#ifndef PT_STAGE_AUX
#define PT_STAGE_AUX 0             // cache policy of the record stream: 0 default, 2 = nt (MI355X_MICROARCH.md row "nt-weights")
#endif
constexpr int STAGE_CHUNKS = 6;     // 16-byte pieces per lane: the staging area of a wave is uint4[STAGE_CHUNKS * 64]
PT_DEV void stage_fetch(const PoolD& pool, uint32_t s, uint4* stage, int lane) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t sk = (uint32_t)__shfl((int)s, (lane >> 2) + 16 * k);
        const char* g = reinterpret_cast<const char*>(&pool.ray[sk]) + 16 * (lane & 3);
        __builtin_amdgcn_global_load_lds((glb_ptr)g, (lds_ptr)(stage + 64 * k), 16, 0, PT_STAGE_AUX);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const uint32_t sm = (uint32_t)__shfl((int)s, (lane >> 1) + 32 * m);
        const char* g = reinterpret_cast<const char*>(&pool.path[sm]) + 16 * (lane & 1);
        __builtin_amdgcn_global_load_lds((glb_ptr)g, (lds_ptr)(stage + 256 + 64 * m), 16, 0, PT_STAGE_AUX);
    }
}
// the staged records of this lane (after the issuing wave's s_waitcnt vmcnt(0): nothing else orders an LDS read behind an LDS-DMA)
PT_DEV SlotIn load_slot_stage(const PoolD& pool, const uint4* stage, int lane, bool enable, uint32_t hw) {
    SlotIn in{};
    in.hw = hw;
    const uint4* rr = stage + 4 * lane;
    const uint4* pr = stage + 256 + 2 * lane;
    const uint4 a = rr[0], b = rr[1], c = rr[2], d = rr[3], e = pr[0], f = pr[1];
    auto f64 = [](uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); };
    in.ray = RayD{V3{f64(a.x, a.y), f64(a.z, a.w), f64(b.x, b.y)}, V3{f64(b.z, b.w), f64(c.x, c.y), f64(c.z, c.w)}, pool.compact ? 0.0 : f64(d.x, d.y)};
    in.sample = d.z;
    in.draw = d.w;
    in.thr = V3{f64(e.x, e.y), f64(e.z, e.w), f64(f.x, f.y)};
    in.pixel = f.z;
    const uint32_t state = state_of_class(hw);
    uint32_t bounce = f.w;                                               // the bounce number rides in the PathRec ...
    if (pool.compact) {                                                  // ... or, with the pixel, in the ray record's time slot
        in.pixel = d.x;
        bounce = d.y;
        if (bounce == 0u) in.thr = V3{1.0, 1.0, 1.0};                    // (the staged PathRec of a fresh path is stale)
    }
    in.bounce = !enable ? SLOT_DEAD : state < SLOT_IDLE ? bounce : state;
    return in;
}
struct NoPrefetch {
    PT_DEV void operator()() const {}
};

// K3: the body of camera.rs:177-226 for the path in slot `s`, executed by all 64 lanes of a wave together (it contains
// wave-level ballots for the work-counter dequeue, K5). `in` = the slot's records; in.bounce == SLOT_DEAD makes the lane
// a bystander that only takes part in the ballots.
// Phases, separated by WAVE-UNIFORM points at which `prefetch()` — the asynchronous fetch of the wave's next group of
// records — may be issued exactly once:
//   A  everything that reads global memory: hit reconstruction, environment lookup, material record, texture values
//   -- P1 (a lane of the wave hit a surface, scene without lights): the arithmetic of B hides the fetch
//   B1 roulette, direction (lights.sample reads the lights' records: scenes with lights prefetch at P1b, after it)
//   B2 pdf, eval, throughput, next ray — pure arithmetic
//   C  work dequeue (a RETURNING atomic: its wait would also wait for a fetch issued before it) -- P2 (nothing hit)
//   D  regeneration (arithmetic), stores
// vmcnt counts loads, stores, atomics and LDS-DMA in issue order, so a fetch can only hide behind a stretch in which no
// younger load is waited for — hence the phase discipline (tex values fetched up front, pt_dev_bsdf.h fetch_tex).
// The template arguments. M is the shading mode (pt_types.h ShadeMode, which says what combines with what); ENV / MED / HET / INT / LSE / DSP
// below are the constants the body derives from it, and "the X forms" the modes that have X.
// LIGHTS: the scene has a lights list (World::lights non-empty). The instantiation without compiles lights.sample / lights.pdf, the
// selector draw and the later prefetch point out: p_light = 0 there (camera.rs:199-200), so no result changes.
// ENV: environment importance sampling is in effect (the rule in pt_amd.h; `env` holds the tables). At a hit in the env
// set E the bounce draws its direction from the one-sample mixture {lights, environment, BSDF}; everywhere else it is the bounce above
// bit for bit. The tables are read in B1 (the env sample; env_pdf's texel gather for a BSDF or light direction), so the ENV forms
// prefetch at P1b like the LIGHTS forms and B2 stays arithmetic.
// QMC: the path's draws come from the Sobol sampler (RngQ); nothing else differs.
// MED: participating media are in effect (the rule in pt_amd.h). The path's medium rides in the upper bits of its bounce
// word. Phase A makes the free-flight draw of a path inside a medium: a lane whose distance falls short of the hit (or whose ray left
// the scene) is at a MEDIUM VERTEX — no surface code runs for it; B1 draws roulette, selector and a light or Henyey-Greenstein
// direction, B2 the phase function, the MIS density and the next ray. A lane that reached a medium's BOUNDARY toggles its medium and
// continues straight on. Every other lane is the bounce above bit for bit.
// HET: a grid-density medium is in effect (the rule in pt_amd.h). A path whose medium has a grid makes
// phase A's free flight by delta tracking (grid_track: a lane-divergent loop, nothing sorts around it); a homogeneous medium and every
// other lane are the MED form bit for bit.
// INT: interior media or chromatic absorption are in effect (the rule in pt_amd.h). Phase A
// attenuates the throughput of a path inside a tinted medium over the segment it has just travelled, and makes no free-flight draw in a
// medium of density 0; B2 sets the medium of a bounce that crossed a glass surface with an interior. Every other lane is the HET form bit
// for bit.
// LSE (only with LIGHTS): exact light sampling is in effect (the rule in pt_amd.h). B1's light direction
// and B2's light density come from pt_dev_lights.h: area-weighted mesh lights whose pdf walks the mesh's BVH with the lane's stack in LDS
// (lstk = &stack[0][thread] of k_shade's LSE_KB-lane stack), cone-sampled sphere lights. Everything else is the bounce above bit for bit.
// DSP: spectral dispersion is in effect (the rule in pt_amd.h). The path's MONO flag rides in bit 31 of its
// bounce word. Phase A: a lane at a dispersive glass computes its path's wavelength — a function of (seed, pixel, sample), no draw — the Cauchy
// index n(lambda) and reads its row of the weight table (`env->col`: these forms have no environment tables); B1 / B2 hand n(lambda) to the glass
// case of mat_sample / mat_pdf_eval; a continued bounce of a path whose flag is clear multiplies the new throughput by the row and sets the flag.
// Every other lane is the bounce above bit for bit.
constexpr int LSE_KB = 512;                                            // threads per block of every shape that has LSE forms (pt_forms.h)
// MOT: motion is in effect (the rule in pt_amd.h): the hit is rebuilt, and lights.sample / lights.pdf are evaluated, with every
// instance posed at the path's time (inst_at); a regenerated camera ray takes its time through the shutter. Plain mode only.
// PLT: punctual lights are in effect (the rule in pt_amd.h): the scene's list of point, spot and directional lights is not empty. The
// selector gives the punctual branch the share SceneD::punctual_f: it draws one light, weights the throughput by the material's eval and what the
// light sends, and continues the path as a SHADOW segment — flag and light index ride in the upper bits of the bounce word (pt_types.h). The next visit
// resolves the segment right after the hit is rebuilt: the throughput is added when nothing lies in front of the light, and the path ends either
// way. Every other lane is the plain bounce under the reduced weights. Plain mode, or:
// SHF = PLT in a media mode (MED or HET): light shafts (the rule in pt_amd.h; pt_scene_set_punctual_media). Medium and shadow segment share
// the bounce word (pt_types.h SHF_*). A medium vertex reads its selector and may take the punctual branch, weighted by the phase function. Phase A's
// free flight of a SHADOW segment runs to min(hit, light): a collision blocks the light; a segment that reaches a medium's boundary in front of
// the light crosses it (B2's boundary code) and stays a SHADOW segment; otherwise it is resolved as in the plain mode. Every other lane is the
// MED / HET form's bounce under PLT's weights.
// The light grid (pt_scene_set_punctual_selection): SceneD::punctual_cdf is set — a RUN-TIME branch of the PLT and SHF forms, no form
// of its own. B1 picks the light by one draw and a binary search in the row of the vertex's cell instead of the index draw and hands its
// probability p to B2, where pm = f * p. The search is a real function (PT_GRID_CALL, as grid_track is): inlined at both sites of a
// light-shaft form its loop's registers came on top of B1's (the register table: DESIGN.md §26).
struct GridPick {
    uint32_t k;
    double p;
};
#ifndef PT_GRID_PICK_INLINE
#define PT_GRID_CALL static __device__ __noinline__   // (static: a unit without PLT forms holds no copy)
#else
#define PT_GRID_CALL static __device__ __forceinline__
#endif
PT_GRID_CALL GridPick punctual_grid_search(const double* row, uint32_t n, double u) {
    GridPick r;
    r.k = punctual_select(row, n, u, r.p);
    return r;
}
PT_DEV uint32_t punctual_grid_pick(const SceneD& sc, const double x[3], double u, double& p) {
    const uint32_t cell = punctual_grid_cell(sc.punctual_grid, x);
    const GridPick r = punctual_grid_search(sc.punctual_cdf + (size_t)cell * sc.punctual_grid.stride, sc.n_punctual, u);
    p = r.p;
    return r.k;
}
template <bool LIGHTS, bool LIST, class Prefetch, ShadeMode M = MODE_PLAIN, bool QMC = false, bool UNI = true, bool MOT = false, bool MAP = false, bool PLT = false>
// UNI: the form may take the single-primitive path of phase A (k_shade: every two-wave shape).
// MAP: the form reads the sky pass's tile map when it draws a work item (k_shade: sky_pass_form of its own arguments, pt_types.h).
// pre_mask / pre_base: the work items of this group's certain-to-end lanes were requested one group AHEAD (k_shade's prefetch point,
// [r3]): pre_mask = those lanes, pre_base = the returning atomic's value in the mask's first lane. 0 = not requested: ask here.
// o_base (PoolD::reorder): the wave-uniform output position of lane 0 — the slot's records and state go to PoolD::ray_out / path_out /
// bounce_out at o_base + lane, its position in the window's sorted order; without reorder they are written in place, at `s`.
PT_DEV void shade_slot(const SceneD& sc, const CamD& cam, const PoolD& pool, CountersD* cnt, uint64_t seed, uint32_t s, uint32_t o_base, int lane, const SlotIn& in,
                       uint32_t& shard, uint32_t& n_done, uint32_t& n_died, Prefetch&& prefetch, unsigned long long pre_mask = 0ull,
                       unsigned long long pre_base = 0ull, uint32_t pre_shard = 0u, const EnvTabD* env = nullptr, uint32_t* lstk = nullptr) {
    constexpr bool ENV = M == MODE_ENV, MED = mode_has_media(M), HET = mode_has_grid(M), INT = M == MODE_INT, LSE = M == MODE_LSE, DSP = M == MODE_DSP;
    constexpr bool SHF = PLT && MED;
    PT_STAMP(1);
    uint32_t bounce = in.bounce;
    uint32_t med = 0u;                                                 // MED: the path's medium (material index + 1), 0 = none
    if constexpr (MED) {
        if (bounce < SLOT_IDLE) {
            med = bounce >> MEDIUM_SHIFT;
            bounce &= MEDIUM_BOUNCE_MASK;
        }
    }
    bool mono = false;                                                 // DSP: the path has been weighted by its wavelength
    if constexpr (DSP) {
        if (bounce < SLOT_IDLE) {
            mono = (bounce & DSP_MONO_BIT) != 0u;
            bounce &= DSP_BOUNCE_MASK;
        }
    }
    bool shadow = false;                                               // PLT: the path is on its SHADOW segment towards light plk
    uint32_t plk = 0u;
    if constexpr (PLT) {
        if (bounce < SLOT_IDLE) {
            if constexpr (SHF) {                                       // (the medium is out of the word already)
                shadow = (bounce & SHF_SHADOW_BIT) != 0u;
                plk = (bounce >> SHF_INDEX_SHIFT) & PLT_INDEX_MASK;
                bounce &= SHF_BOUNCE_MASK;
            } else {
            shadow = (bounce & PLT_SHADOW_BIT) != 0u;
            plk = (bounce >> PLT_INDEX_SHIFT) & PLT_INDEX_MASK;
            bounce &= PLT_BOUNCE_MASK;
            }
        }
    }
    const bool alive = bounce != SLOT_DEAD;
    const bool was_idle = bounce == SLOT_IDLE;
    const bool live = alive && !was_idle;
    bool finished = was_idle;
    // A path that ends on a surface (roulette, sampler returned None, depth bound) would make its whole wave run the
    // regeneration code — dequeue, camera ray: ~400 instructions — for one or two lanes: with 64 lanes and a few per cent
    // of such endings per bounce, most surface groups paid for it. Instead the slot is parked as SLOT_IDLE and refilled
    // next iteration together with the other idle slots, where every lane regenerates (class sort: CLASS_IDLE).
    bool parked = false;
    uint32_t pixel = in.pixel, sample = in.sample;
    RayD ray = in.ray;
    V3 thr = in.thr, rad{};
    if constexpr (MED) {
        // compact layout: the loaders take "bounce word != 0" for "has a PathRec" — a camera ray inside the camera medium has none
        if (pool.compact && bounce == 0u) thr = V3{1.0, 1.0, 1.0};
    }
    typedef std::conditional_t<QMC, RngQ, Rng> RngT;
    RngT rng{};
#ifdef PT_STAMPS
    uint32_t prof_class = was_idle ? CLASS_IDLE : CLASS_DEAD;
    if (live) prof_class = in.hw >> HIT_CLASS_SHIFT;
    prof_class = (uint32_t)__builtin_amdgcn_readfirstlane((int)prof_class);
#endif
    // Lanes that are certain to end here — the ray left the scene (class in K2's result word) or the slot is idle — are known
    // before anything is computed: their work items are requested NOW, so that the returning atomic's round trip to the work
    // counter (~3 k cycles, which only the SIMD's other wave could cover) runs under the environment lookup instead of in
    // front of the regeneration. Phase C consumes the answer; paths that end on a surface ask there, as before.
    // [r3] One step further: the class of a wave's NEXT group is known a whole group ahead (the window's sorted result words), so
    // k_shade requests these items at the previous group's prefetch point and hands the pending answer in (pre_mask, pre_base):
    // the round trip — 3-4 us with every CU dequeuing — then runs under a whole group's work instead of under one environment lookup.
    unsigned long long early = 0ull, early_base = 0ull;
    uint32_t early_shard = shard;
    if (pool.dynamic) {
        // (MED: a ray that left the scene inside an unbounded medium scatters instead of ending)
        early = __ballot(alive && (was_idle || ((in.hw >> HIT_CLASS_SHIFT) == CLASS_MISS && (!MED || med == 0u))));
        early_shard = shard;
        if (pre_mask != 0ull) { early_base = pre_base; early_shard = pre_shard; }   // (the same lanes by construction: both come from the slots' result words;
                                                                                    //  the wave may have moved on to another shard since it asked)
        else if (early && lane == __ffsll((long long)early) - 1) early_base = atomicAdd(&cnt->work[shard].next, (unsigned long long)__popcll(early));
    }
    // ---- phase A: all global-memory reads of the bounce -------------------------------------------------------------
    bool is_hit = false;
    bool scatter = false, boundary = false;                            // MED: the lane is at a medium vertex (hit.point) / at a medium's boundary
    bool blocked = false;                                              // SHF: the SHADOW segment collided in front of its end
    double shadow_dl = D_INF;                                          // SHF: D' of the lane's SHADOW segment
    MediumD medium{};
    uint32_t interior = 0u;                                            // INT: the hit is on a glass with an interior: that medium (material index + 1)
    HitD hit{};
    double ior_l = 0.0;                                                // DSP: the hit is on a dispersive glass: n(lambda) of the path's wavelength, else 0
    V3 w_l{1.0, 1.0, 1.0};                                             // ... and the wavelength's row of the weight table
    const MatD* mp = nullptr;
    TexVals tv{};
    LocalFrame lf{};
    PT_STAMP_VAR(a1);
    // A group whose surface lanes all hit ONE primitive, a sphere or a quad (k_shade's sort makes groups of one class, and a class is
    // often dominated by one primitive: a ground quad, a big sphere): every lane would gather the same PrimRef, instance chain,
    // sphere / quad record, material fields and texture descriptor, each gather waiting for the one before. Decided here, at a
    // wave-uniform point; such a group reads them through the scalar cache (reconstruct_hit_prim<.., true>, fetch_tex<true>). Any
    // other group runs the per-lane code. The operands are the same bytes either way: no result changes.
    // Forms whose register allocation pays for the second copy of phase A with more scratch than they had (tools/regs.sh against the
    // same form without it: the MED forms with lights, the pixel-list ENV forms with lights, the three-wave shapes) keep the per-lane path.
    constexpr int UG = UNI && !(MED && LIGHTS) && !(LIGHTS && LIST && ENV) ? PT_UNIFORM_GROUPS : 0;
    bool uni = false;                                                  // wave-uniform
    PrimRef pr0{};
    {
        const uint32_t id = in.hw & HIT_ID_MASK;
        const bool on_surface = live && (in.hw >> HIT_CLASS_SHIFT) != CLASS_MISS;
        const unsigned long long sm = __ballot(on_surface);
        if (UG != 0 && sm != 0ull) {
            const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane((int)id, __ffsll((long long)sm) - 1);
            if (__ballot(on_surface && id != g0) == 0ull) {
                pr0 = ldu(&sc.prims[g0]);
                uni = (pr0.kind & 0xFFu) != PRIM_TRI;
#ifdef PT_STAMPS
                if (lane == 0) {
                    atomicAdd(&g_prof[prof_class][12], 1ull);          // groups of one primitive ...
                    if (uni) atomicAdd(&g_prof[prof_class][13], 1ull); // ... that is no triangle
                }
#endif
            }
        }
    }
    if (live) {
        if (!pool.dynamic) {
            pixel = slot_pixel<LIST>(pool, s);
            rad = V3{pool.rx[s], pool.ry[s], pool.rz[s]};
        }
        rng = RngT{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample, in.draw};
        const uint32_t gid = in.hw & HIT_ID_MASK;
        const bool surface = (in.hw >> HIT_CLASS_SHIFT) != CLASS_MISS &&
                             (uni ? reconstruct_hit_prim<false, true, MOT>(sc, ray, pr0, 1e-3, hit) : reconstruct_hit<false, MOT>(sc, ray, gid, 1e-3, hit));
        PT_STAMP_SET(a1);
        if constexpr (SHF) {
            if (shadow) {
                const double o[3] = {ray.o.x, ray.o.y, ray.o.z};
                shadow_dl = punctual_shadow_distance(sc.punctual[plk], o);
            }
        }
        if constexpr (MED) {
            if (med != 0u) {                                           // free flight: one draw, d = -log(1 - u) / density
                medium = load_medium(sc, med);
                if (!surface && medium.bounded) {
                    // the ray left the scene, so it is not inside a medium that an object bounds: the path lost a crossing (an exit closer
                    // than t_min to an offset entry point, at an edge of a cuboid or mesh). No draw; the miss is processed.
                    med = 0u;
                } else {
                    double d = D_INF;                                  // the distance to the medium vertex, +inf: none
                    bool tracked = false;
                    if constexpr (HET) {
                        const uint32_t grid = (uint32_t)sc.mats[med - 1u].p[6];   // the medium's row of SceneD::grids + 1, 0 = homogeneous
                        if (grid != 0u) {                              // delta tracking through the grid, clipped to its box
                            double t_trk = surface ? hit.dist : D_INF;
                            if constexpr (SHF) { if (shadow && !(t_trk < shadow_dl)) t_trk = shadow_dl; }   // a SHADOW segment ends at min(t, D')
                            const GridTrack tr = grid_track(sc.grids + (grid - 1u), sc.grid_vals, ray.o, ray.d, t_trk, rng);
                            rng.draw = tr.draw;
                            if (tr.collided) d = tr.s;
                            tracked = true;
                        }
                    }
                    if (!tracked && (!INT || medium.density > 0.0)) d = medium_free_flight(rng_f64(rng), medium.density);   // (INT: density 0 makes no draw)
                    const double t_seg = surface ? hit.dist : D_INF;
                    if (SHF && shadow) {
                        blocked = d < (t_seg < shadow_dl ? t_seg : shadow_dl);   // a collision in front of min(t, D'): the light is blocked
                    } else
                    if (d < t_seg) {
                        scatter = true;
                        hit.point = ray.o + ray.d * d;
                    }
                    // absorption over the segment travelled, before anything at this visit uses the throughput
                    if constexpr (INT) thr = medium_absorb(load_absorption(sc, med), thr, scatter ? d : t_seg);
                }
            }
        }
        if (PLT && shadow) {
            // a SHADOW segment is resolved before anything else — no emission, no roulette, no draw: the light is visible when the ray missed
            // or its hit lies at or beyond the light; the environment is not added. The path ends either way: a lane that missed is in the
            // `early` ballot already, one that hit ends like a roulette death.
            if constexpr (SHF) {
                // the free flight above ran over [0, min(t, D')). Not blocked: a medium's boundary in front of the light is crossed (B2's boundary
                // code: toggle, offset, ++bounce, the depth bound) and the path stays a SHADOW segment; anything else resolves the segment. A lane
                // that missed with no medium is in the `early` ballot and ends here; one that ends otherwise asks for work in phase C.
                if (!blocked && surface && hit.dist < shadow_dl && sc.mats[hit.mat].kind == MAT_MEDIUM) {
                    boundary = true;
                } else {
                    if (!blocked && (!surface || hit.dist >= shadow_dl)) add_radiance(pool, pixel, rad, thr);
                    finished = true;
                    parked = (in.hw >> HIT_CLASS_SHIFT) != CLASS_MISS;
                }
            } else if constexpr (PLT) {
                const double o[3] = {ray.o.x, ray.o.y, ray.o.z};
                const double dl = punctual_shadow_distance(sc.punctual[plk], o);
                if (!surface || hit.dist >= dl) add_radiance(pool, pixel, rad, thr);
                finished = true;
                parked = (in.hw >> HIT_CLASS_SHIFT) != CLASS_MISS;
            }
        } else if (MED && scatter) {
            // a medium vertex: no emission, no surface
        } else if (!surface) {
            add_radiance(pool, pixel, rad, thr * sample_environment(sc, cam, ray.d));   // camera.rs:180-183
            finished = true;
        } else {
            // the material fields phase A reads: of the group's one material by scalar loads, else per lane (B1 / B2 read *mp as before)
            mp = &sc.mats[hit.mat];
            uint32_t mkind;
            double m_p0 = 0.0, m_p1 = 0.0, m_p2 = 0.0, m_p3 = 0.0, m_ior = 0.0;   // INT: p[0]; DSP: p[1..3], ior
            if ((UG & 2) != 0 && uni) {
                const MatD* um = &sc.mats[pr0.mat];
                mkind = ldu(&um->kind);
                if (!MED || mkind != MAT_MEDIUM) tv = fetch_tex<true>(sc, *um, hit);
                if constexpr (INT) m_p0 = ldu(&um->p[0]);
                if constexpr (DSP) { m_p1 = ldu(&um->p[1]); m_p2 = ldu(&um->p[2]); m_p3 = ldu(&um->p[3]); m_ior = ldu(&um->ior); }
            } else {
                mkind = mp->kind;
                if (!MED || mkind != MAT_MEDIUM) tv = fetch_tex(sc, *mp, hit);
                if constexpr (INT) m_p0 = mp->p[0];
                if constexpr (DSP) { m_p1 = mp->p[1]; m_p2 = mp->p[2]; m_p3 = mp->p[3]; m_ior = mp->ior; }
            }
            if (MED && mkind == MAT_MEDIUM) {
                boundary = true;                                       // a medium's boundary: invisible, no emission
                mp = nullptr;
            } else {
            is_hit = true;
            lf = make_local_frame(mkind, hit, -ray.d);
            if constexpr (INT) interior = mkind == MAT_GLASS ? (uint32_t)m_p0 : 0u;   // (read here: B2 stays arithmetic)
            if constexpr (DSP) {
                if (mkind == MAT_GLASS && m_p3 != 0.0) {               // dsp_is_dispersive
                    const WavelengthD wl = dsp_wavelength<QMC>((uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample);
                    ior_l = dsp_ior(m_ior, m_p1, m_p2, wl.lambda);
                    const double* row = env->col + 3u * wl.bin;
                    w_l = V3{row[0], row[1], row[2]};
                }
            }
            // camera.rs:186-187 — added for every material (zero unless emissive) so that a
            // non-finite throughput poisons the sample exactly as it does in the reference
            V3 emission = mkind == MAT_LIGHT ? tv.color : V3{0.0, 0.0, 0.0};
            add_radiance(pool, pixel, rad, thr * emission);
            }
        }
    }
    PT_STAMP(a2);
    const bool any_hit = __ballot(is_hit || (MED && (scatter || boundary))) != 0ull;
    bool fetched = false;                                              // wave-uniform
    if (any_hit && !LIGHTS && !ENV && !PLT) { prefetch(); fetched = true; }    // P1 (PLT: B1 reads the light's record)
    // ---- phase B1: roulette and the next direction ------------------------------------------------------------------------
    double p_punct = 0.0;                                              // PLT: the punctual branch's share f of the selector
    if constexpr (PLT) p_punct = sc.punctual_f;
    const double p_light = PLT ? (LIGHTS ? (1.0 - p_punct) / 2.0 : 0.0) : LIGHTS ? 0.5 : 0.0;   // :199-200 (the host picks the instantiation by World::lights)
    const double p_bsdf = PLT ? 1.0 - p_light - p_punct : 1.0 - p_light;
    const V3 wo = -ray.d;
    V3 dir{};
    bool have_dir = false;
    bool punct_dir = false;                                            // PLT: the bounce took the punctual branch (dir = w, towards light plk)
    V3 punct_e{};                                                      // ... E, what the light sends to the hit point
    bool punct_ok = false;                                             // ... d2 is finite and not 0
    double punct_p = 0.0;                                              // ... the light grid's probability of plk in the vertex's cell (read when sc.punctual_cdf is set)
    bool env_lane = false, env_dir = false;                            // ENV: the bounce takes the mixture / its direction is an env sample
    double q_env = 0.0;                                                // ENV: q_env(dir) (pt_amd.h)
    if (is_hit) {
        if (bounce > 5) {                                              // russian roulette :190-196
            double p = clampd(luminance(thr), 0.01, 1.0);
            if (rng_f64(rng) > p) finished = parked = true;
            else thr = thr / p;
        }
        if (!finished) {
            // :201 draws the selector even when there are no lights (p_light = 0: never below it) — then only the counter moves
            double rsel = 1.0;
            bool ok = true;
            if constexpr (ENV) env_lane = env_in_set(*mp, tv, lf);
            if (ENV && env_lane) {
                // one selector draw: lights below p_light, the environment below p_light + p_env, the BSDF above (pt_amd.h)
                const double p_env = env->f, p_l = LIGHTS ? (1.0 - p_env) / 2.0 : 0.0;
                rsel = rng_f64(rng);
                if (LIGHTS && rsel < p_l) {
                    dir = lights_sample<MOT>(sc, hit.point, ray.time, rng);
                } else if (rsel < p_l + p_env) {
                    uint64_t a, b;
                    rng_u64x2(rng, a, b);
                    dir = env_sample(sc, ldu(&sc.tex[cam.env_tex]), *env, u64_to_unit(a), u64_to_unit(b), q_env);
                    env_dir = true;
                } else {
                    ok = mat_sample(sc, *mp, hit, wo, rng, cam.two_pi_scale, tv, lf, dir);
                }
                if (ok) {
                    // support: q_env is zero below the material's local frame; an env direction there ends the path
                    const bool above = to_local(lf.f, dir).z > 0.0;
                    if (!env_dir) q_env = above ? env_pdf(sc, ldu(&sc.tex[cam.env_tex]), *env, dir) : 0.0;
                    else if (!above) ok = false;
                }
            } else if constexpr (PLT) {
                // one selector draw: lights below p_light, the punctual list below p_light + f, the BSDF above — the order of the ENV mixture
                rsel = rng_f64(rng);
                if (LIGHTS && rsel < p_light) {
                    dir = lights_sample<MOT>(sc, hit.point, ray.time, rng);
                } else if (rsel < p_light + p_punct) {
                    const double x[3] = {hit.point.x, hit.point.y, hit.point.z};
                    if (sc.punctual_cdf) plk = punctual_grid_pick(sc, x, rng_f64(rng), punct_p) & PLT_INDEX_MASK;   // the light grid: one draw (§26)
                    else plk = rng_index(rng, sc.n_punctual) & PLT_INDEX_MASK;   // one index draw, as the lights list's
                    const PunctualEval pe = punctual_eval(sc.punctual[plk], x);
                    dir = V3{pe.w[0], pe.w[1], pe.w[2]};
                    punct_e = V3{pe.E[0], pe.E[1], pe.E[2]};
                    punct_ok = pe.d2 != 0.0 && pe.d2 - pe.d2 == 0.0;     // (neither 0 nor inf nor NaN)
                    punct_dir = true;
                } else {
                    ok = mat_sample<RngT, DSP>(sc, *mp, hit, wo, rng, cam.two_pi_scale, tv, lf, dir, ior_l);
                }
            } else if constexpr (LIGHTS) {
                rsel = rng_f64(rng);
                if (rsel < p_light) {
                    if constexpr (LSE) dir = lights_sample_exact(sc, hit.point, ray.time, rng);
                    else dir = lights_sample<MOT>(sc, hit.point, ray.time, rng);
                } else ok = mat_sample<RngT, DSP>(sc, *mp, hit, wo, rng, cam.two_pi_scale, tv, lf, dir, ior_l);
            } else {
                ++rng.draw;
                ok = mat_sample<RngT, DSP>(sc, *mp, hit, wo, rng, cam.two_pi_scale, tv, lf, dir, ior_l);
            }
            if (!ok) finished = parked = true;                         // :209-211
            else have_dir = true;
        }
    }
    bool have_mdir = false;                                            // MED: a medium vertex with a next direction (in `dir`)
    if constexpr (MED) {
        if (scatter) {
            if (bounce > 5) {                                          // roulette exactly as at a surface
                double p = clampd(luminance(thr), 0.01, 1.0);
                if (rng_f64(rng) > p) finished = parked = true;
                else thr = thr / p;
            }
            if (!finished) {
                bool from_light = false;
                double rsel = 1.0;                                     // SHF: the selector is read — lights below p_light, the punctual list below p_light + f
                if constexpr (SHF) { rsel = rng_f64(rng); from_light = LIGHTS && rsel < p_light; }
                else if constexpr (LIGHTS) from_light = rng_f64(rng) < p_light;
                else ++rng.draw;                                       // the selector is drawn even without lights
                if (from_light) {
                    dir = lights_sample<MOT>(sc, hit.point, ray.time, rng);
                } else if (SHF && rsel < p_light + p_punct) {
                    if constexpr (SHF) {                               // the surface bounce's punctual branch at the vertex x = hit.point
                        const double x[3] = {hit.point.x, hit.point.y, hit.point.z};
                        if (sc.punctual_cdf) plk = punctual_grid_pick(sc, x, rng_f64(rng), punct_p) & PLT_INDEX_MASK;
                        else plk = rng_index(rng, sc.n_punctual) & PLT_INDEX_MASK;
                        const PunctualEval pe = punctual_eval(sc.punctual[plk], x);
                        dir = V3{pe.w[0], pe.w[1], pe.w[2]};
                        punct_e = V3{pe.E[0], pe.E[1], pe.E[2]};
                        punct_ok = pe.d2 != 0.0 && pe.d2 - pe.d2 == 0.0;
                        punct_dir = true;
                    }
                } else {
                    uint64_t a, b;
                    rng_u64x2(rng, a, b);
                    dir = hg_sample(medium.g, u64_to_unit(a), u64_to_unit(b), ray.d);
                }
                have_mdir = true;
            }
        }
    }
    PT_STAMP(b1);
    if (any_hit && !fetched) { prefetch(); fetched = true; }           // P1b
    // ---- phase B2: pdf, eval, throughput, next ray (arithmetic only; lights.pdf reads through the scalar cache) -----------------
    if (have_dir) {
        double bsdf_pdf;
        V3 brdf;
        mat_pdf_eval<DSP>(sc, *mp, hit, wo, dir, tv, lf, bsdf_pdf, brdf, ior_l);
        double light_pdf = 0.0;
        if constexpr (LSE) light_pdf = lights_pdf_exact<LSE_KB>(sc, hit.point, dir, ray.time, lstk);
        else if constexpr (LIGHTS) light_pdf = lights_pdf<MOT>(sc, hit.point, dir, ray.time);
        double pdf = p_bsdf * bsdf_pdf + p_light * light_pdf;
        V3 attenuation = brdf / pdf;
        bool env_end = false;
        if constexpr (PLT) {
            if (punct_dir) {
                // thr' = ((thr * e) * E) / pm with pm = f / n: the branch's own probability, no density (the direction has measure zero under the others)
                const double pm = sc.punctual_cdf ? p_punct * punct_p : p_punct / (double)sc.n_punctual;   // (the light grid: pm = f * p)
                const V3 t = ((thr * brdf) * punct_e) / pm;
                env_end = !punct_ok || (t.x == 0.0 && t.y == 0.0 && t.z == 0.0);
                if (!env_end) {
                    ray = make_ray(hit.point + (1e-3 * signum(dot(dir, hit.gn))) * hit.gn, dir, ray.time);
                    thr = t;
                    shadow = true;
                    ++bounce;
                    if (bounce >= cam.max_depth) finished = parked = true;   // a shadow segment that would be the max_depth-th ray is never resolved
                }
            }
        }
        if constexpr (ENV) {
            if (env_lane) {
                // the mixture's density: p_bsdf * s_b + p_light * light_pdf + p_env * q_env, with s_b the BSDF sampler's density. Diffuse:
                // s_b = bsdf_pdf. Metal (Q2): s_b = metal_sample_density, and the integrand keeps today's weight (today's density / pdf),
                // so that the expectation is today's (pt_amd.h).
                const double pe = env->f, pl = LIGHTS ? (1.0 - pe) / 2.0 : 0.0, pb = 1.0 - pl - pe;
                double s_b = bsdf_pdf, w = 1.0;
                if (mp->kind == MAT_METAL) {
                    s_b = metal_sample_density(lf.v, to_local(lf.f, dir), tv.rough);
                    w = (p_bsdf * s_b + p_light * light_pdf) / pdf;
                    env_end = !(pdf > 0.0);
                }
                const double pm = pb * s_b + pl * light_pdf + pe * q_env;
                attenuation = brdf * w / pm;
                const V3 t = thr * attenuation;
                env_end = env_end || !(pm > 0.0) || (t.x == 0.0 && t.y == 0.0 && t.z == 0.0);
            }
        }
        if (env_end) {
            finished = parked = true;                                  // (ENV: a zero-density or zero-throughput bounce ends the path; PLT: the punctual branch's endings)
        } else if (PLT && punct_dir) {
            // (continued above, as a SHADOW segment)
        } else {
            double e = 1e-3 * signum(dot(dir, hit.gn));                // :217-222
            if constexpr (INT) {
                // a glass with an interior: the bounce crossed the surface when the continued ray starts on the side the incoming ray was
                // heading to — into the interior at a front-face hit, out of it at a back-face hit; a reflection keeps the medium
                if (interior != 0u && signum(dot(dir, hit.gn)) == signum(dot(ray.d, hit.gn))) med = hit.front ? interior : 0u;
            }
            ray = make_ray(hit.point + e * hit.gn, dir, ray.time);
            thr = thr * attenuation;
            if constexpr (DSP) {
                if (ior_l > 0.0 && !mono) {                            // the path's first continued bounce at a dispersive glass: weighted once
                    thr = thr * w_l;
                    mono = true;
                }
            }
            ++bounce;
            if (bounce >= cam.max_depth) finished = parked = true;     // loop bound :177
        }
    }
    if constexpr (MED) {
        if (have_mdir) {
            const double ph = hg_phase(medium.g, dot(ray.d, dir));
            if (SHF && punct_dir) {
                // thr' = ((thr * (albedo * ph)) * E) / pm, pm = f / n: the phase function where the surface has its eval, no cosine
                const double pm = sc.punctual_cdf ? p_punct * punct_p : p_punct / (double)sc.n_punctual;
                const V3 t = ((thr * (medium.albedo * ph)) * punct_e) / pm;
                if (!punct_ok || (t.x == 0.0 && t.y == 0.0 && t.z == 0.0)) {
                    finished = parked = true;
                } else {
                    ray = make_ray(hit.point, dir, ray.time);          // no offset, as for a scattered ray
                    thr = t;
                    shadow = true;
                    ++bounce;
                    if (bounce >= cam.max_depth) finished = parked = true;
                }
            } else {
            double light_pdf = 0.0;
            if constexpr (LIGHTS) light_pdf = lights_pdf<MOT>(sc, hit.point, dir, ray.time);
            const double pdf = p_bsdf * ph + p_light * light_pdf;
            if (!(pdf > 0.0) || !(pdf < D_INF)) {
                finished = parked = true;                              // a zero or non-finite density ends the path
            } else {
                thr = thr * (medium.albedo * ph / pdf);
                ray = make_ray(hit.point, dir, ray.time);              // no offset: nothing to leave
                ++bounce;
                if (bounce >= cam.max_depth) finished = parked = true;
            }
            }
        } else if (boundary) {
            // no draw, no roulette, no emission: the path changes medium and goes straight on, offset like every continued ray
            med = med == hit.mat + 1u ? 0u : hit.mat + 1u;
            const double e = 1e-3 * signum(dot(ray.d, hit.gn));
            ray.o = hit.point + e * hit.gn;
            ++bounce;
            if (bounce >= cam.max_depth) finished = parked = true;
        }
    }
#ifdef PT_STAMPS
    const unsigned long long prof_live = __ballot(live), prof_hit = __ballot(is_hit), prof_dir = __ballot(have_dir);
#endif
    PT_STAMP(2);
    // ---- phase C: finished paths accumulate (camera.rs:107) and draw their next work item ------------------------------------
    uint32_t next_pixel = pixel, next_sample = 0, next_row = 0, next_col = 0;
    bool more = false, next_idle = false;
    if (pool.dynamic) {
        // K5: wave ballot + prefix popcount, ONE atomic per wave on the wave's shard of the work counter. When the
        // shard has run dry the wave looks at all shards at once (lane i reads shard i) and moves on to the next one
        // that still has items — without this, slots died while other shards still held work and the frame ended
        // on a long, thin tail.
        parked = parked && pool.defer_regen != 0u;
        // first round: the early request's answer (its lanes are a subset of the finished ones); then whoever is still without
        unsigned long long need = early ? early : __ballot(alive && finished && !parked);
        bool have_base = early != 0ull;
        while (need) {
            const int leader = __ffsll((long long)need) - 1;
            const bool asking = (need >> lane) & 1ull;
            unsigned long long base = early_base;
            uint32_t from = early_shard;                                              // the shard the answer in hand came from
            if (!have_base) {
                base = 0;
                from = shard;
                if (lane == leader) base = atomicAdd(&cnt->work[shard].next, (unsigned long long)__popcll(need));
            }
            have_base = false;
            base = __shfl(base, leader);
            if (asking) {
                const unsigned long long w = shard_item(base + (unsigned long long)__popcll(need & ((1ull << lane) - 1ull)), from);
                if (w < pool.total_work) {
                    more = true;
                    next_idle = !work_item<LIST, MAP>(pool, w, next_pixel, next_sample, next_row, next_col);
                }
            }
            if (__ballot(asking && !more)) {
                static_assert(WORK_SHARDS == 64, "one lane per shard");
                const unsigned long long live_shards = __ballot(shard_item(cnt->work[lane].next, (uint32_t)lane) < pool.total_work);
                if (live_shards == 0ull) break;                                       // the frame's sample budget is handed out
                const unsigned long long above = live_shards & ~((2ull << shard) - 1ull);   // next live shard after this one, cyclically
                shard = (uint32_t)(__ffsll((long long)(above ? above : live_shards)) - 1);
            }
            need = __ballot(alive && finished && !parked && !more);
        }
    } else if (alive && finished) {
        pool.ax[s] += rad.x; pool.ay[s] += rad.y; pool.az[s] += rad.z;
        next_sample = sample + pool.k;
        more = next_sample < pool.spp_end;
    }
    if (!fetched) prefetch();                                          // P2: behind the dequeue, in front of the regeneration arithmetic
#ifdef PT_STAMPS
    const unsigned long long prof_regen = __ballot(alive && finished && more && !next_idle && !(parked && pool.dynamic));
#endif
    PT_STAMP(3);
    // ---- phase D: regeneration, stores (in place, or at the slot's sorted position in the output area: PoolD::reorder) ---------
    if (alive && finished) {
        if (!was_idle) ++n_done;
        if (parked && pool.dynamic) {
            bounce = SLOT_IDLE;
        } else if (more && next_idle) {
            bounce = SLOT_IDLE;
        } else if (more) {
            rng = RngT{(uint32_t)seed, (uint32_t)(seed >> 32), next_pixel, next_sample, 0u};
            if (!pool.dynamic) divmod_u31(next_pixel, cam.width, next_row, next_col);
            ray = generate_ray<MOT>(cam, next_row, next_col, rng);
            thr = V3{1.0, 1.0, 1.0};
            rad = V3{0.0, 0.0, 0.0};
            bounce = 0;
            if constexpr (DSP) mono = false;
            if constexpr (PLT) shadow = false;
            if constexpr (MED) med = cam.medium;
            sample = next_sample;
            pixel = next_pixel;
        } else {
            bounce = SLOT_DEAD;
            ++n_died;
        }
    }
    if (alive) {
        // in place the state array changes only with the slot's state; in shading order every position gets its state written
        const bool reorder = !LIST && pool.reorder != 0u;
        const uint32_t o = reorder ? o_base + (uint32_t)lane : s;
        const uint32_t state_new = bounce < SLOT_IDLE ? 0u : bounce, state_old = was_idle ? SLOT_IDLE : 0u;
        if (reorder || state_new != state_old) pool.bounce_out[o] = state_new;
        if (bounce < SLOT_IDLE) {
            const uint32_t bounce_word = SHF ? bounce | (med << MEDIUM_SHIFT) | (shadow ? SHF_SHADOW_BIT | (plk << SHF_INDEX_SHIFT) : 0u) :
                                         MED ? bounce | (med << MEDIUM_SHIFT) : DSP && mono ? bounce | DSP_MONO_BIT : PLT && shadow ? bounce | PLT_SHADOW_BIT | (plk << PLT_INDEX_SHIFT) : bounce;
            store_ray(pool, pool.ray_out, o, ray, sample, rng.draw, pixel, bounce_word);
            if (!pool.compact || bounce != 0u) store_path(pool.path_out, o, thr, pixel, bounce_word);
            if (!pool.dynamic) { pool.rx[s] = rad.x; pool.ry[s] = rad.y; pool.rz[s] = rad.z; }
        }
    }
#ifdef PT_STAMPS
    PT_STAMP(4);
    if (lane == 0) {   // block-local sums in LDS (global atomics here would themselves be what the next group waits for)
        atomicAdd(&g_prof[prof_class][0], 1ull);
        atomicAdd(&g_prof[prof_class][8], (unsigned long long)__popcll(prof_live));
        atomicAdd(&g_prof[prof_class][9], (unsigned long long)__popcll(prof_hit));
        atomicAdd(&g_prof[prof_class][10], (unsigned long long)__popcll(prof_dir));
        atomicAdd(&g_prof[prof_class][11], (unsigned long long)__popcll(prof_regen));
        atomicAdd(&g_prof[prof_class][1], (t_a1 ? t_a1 : t_a2) - t_1);   // records unpacked, hit reconstructed
        atomicAdd(&g_prof[prof_class][6], t_a2 - (t_a1 ? t_a1 : t_a2));  // environment / textures
        atomicAdd(&g_prof[prof_class][7], t_b1 - t_a2);                  // roulette + direction
        atomicAdd(&g_prof[prof_class][2], t_2 - t_1);
        atomicAdd(&g_prof[prof_class][3], t_3 - t_2);
        atomicAdd(&g_prof[prof_class][4], t_4 - t_3);
        atomicAdd(&g_prof[prof_class][5], t_4 - t_1);
    }
#endif
}

constexpr int SORT_WINDOW = SORT_WINDOW_SLOTS;   // slots sorted together by k_shade<true, *>
// Every thread packs the class keys of its SORT_WINDOW / BLOCK slots into ONE 32-bit word, 4 bits each. A 4096-slot window
// (16 keys) overflowed that word in round 2 and the kernel hung: the bound is a compile error now, not a comment.
static_assert((SORT_WINDOW / BLOCK) * 4 <= 32, "k_shade: the per-thread `keys` word holds at most eight 4-bit class keys — widen it before enlarging SORT_WINDOW");
static_assert(N_CLASSES <= 16, "k_shade: a class key is 4 bits wide (and the class field of K2's result word is bits 28..31)");
static_assert(SORT_WINDOW % BLOCK == 0 && SORT_WINDOW / 64 == 32, "k_shade: one half-wave scans the 32 group counts of a class");
static_assert(SORT_WINDOW <= 65536, "k_shade: s_perm holds 16-bit slot offsets");
#ifndef PT_DEQUEUE_AHEAD
#define PT_DEQUEUE_AHEAD 1          // 0: certain-to-end lanes request their work items at the start of their own group (the round-2 form)
#endif
#ifndef PT_K3_PREFETCH
#define PT_K3_PREFETCH 1            // 0: every group's records straight from the pool (the round-1 form), for A/B
#endif

// K3 launcher kernel. SORT = false: blocks walk the pool in 256-slot chunks, lane i shades slot i.
// SORT = true (default): a block draws a WINDOW of 2048 slots from a queue, counting-sorts their indices
// by class in LDS (miss, one class per material kind, idle, dead), then its four waves pull groups of 64
// same-class slots from an LDS cursor until the window is done — waves execute one material's code
// instead of serialising through all of them, the expensive classes go first and are spread over all
// waves of the block (work stealing), and every slot's records are moved whole by its own lane.
// KB: threads per block (256, or [r3] 512 with a 4096-slot window: the sort's barriers and the window's end are paid once per twice
// as many slots and eight waves level a window's end better than four; one block per CU then).
// M: the shading mode (pt_types.h ShadeMode; shade_slot says what each of the constants derived from it changes). Of `env`, the ENV
// forms read the tables and the DSP forms `col`, their weight table; no other form reads it.
// QMC: the Sobol sampler (shade_slot)
// MED: participating media (shade_slot). A slot's class says nothing certain about a path inside a medium — it may scatter before the
// hit, or instead of leaving — so these forms do not request work items a group ahead.
// LSE: these forms hold the per-lane stack of the light meshes' all-hits walk, LIGHT_STACK levels x KB lanes in LDS
// MOT: motion (shade_slot)
// PLT: punctual lights (shade_slot); in the modes MED and HET: light shafts
template <bool SORT, int MINW, bool LIGHTS, int KB = BLOCK, int PER = SORT_WINDOW / BLOCK, bool LIST = false, ShadeMode M = MODE_PLAIN, bool QMC = false, bool MOT = false, bool PLT = false>
__global__ __launch_bounds__(KB, KB == BLOCK ? MINW : 1) void k_shade(SceneD sc, CamD cam, PoolD pool, CountersD* cnt, uint64_t seed, EnvTabD env) {
    constexpr bool ENV = M == MODE_ENV, MED = mode_has_media(M), LSE = M == MODE_LSE, DSP = M == MODE_DSP;   // (HET and INT change nothing here)
    static_assert(sizeof(SceneD) + sizeof(CamD) + sizeof(PoolD) + sizeof(CountersD*) + sizeof(uint64_t) + sizeof(EnvTabD) + 64 <= 4096, "k_shade: the arguments fit the 4 KiB of kernel arguments");
    static_assert(!MOT || M == MODE_PLAIN, "k_shade: the MOT forms are plain-mode forms");
    static_assert(!PLT || ((M == MODE_PLAIN || M == MODE_MED || M == MODE_HET) && !MOT), "k_shade: the PLT forms are plain-mode forms, or MED / HET forms (light shafts), without motion");
    static_assert((!LSE || LIGHTS) && (!(LSE || DSP) || (SORT && KB == LSE_KB)), "k_shade: the LSE forms need a lights list; the LSE and DSP forms are sorted 512-thread forms");
    __shared__ uint32_t s_lstack[LSE ? LIGHT_STACK * KB : 1];   // 48 KB: stack[level][thread] of lights_pdf_exact's mesh walk
    uint32_t* const lstk = LSE ? &s_lstack[threadIdx.x] : nullptr;
    uint32_t n_done = 0, n_died = 0;   // per thread and launch: far below 2^32 (64-bit counters here were the kernel's only spills)
    const int lane = (int)(threadIdx.x & 63u);
#ifdef PT_STAMPS
    for (uint32_t i = threadIdx.x; i < (N_CLASSES + 1) * PROF_COLS; i += KB) (&g_prof[0][0])[i] = 0ull;
    __syncthreads();
#endif
    uint32_t shard = blockIdx.x % WORK_SHARDS;   // work-counter shard this wave draws from (wave-uniform; moves on when it runs dry)
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->win_extend = 0;
    if (ldu(&cnt->alive) == 0ull) return;   // (see k_extend; a block subtracts its dead slots when it has run out of windows: zero means every window of the pool has been shaded)
    if (!SORT) {
        // n_alloc is a multiple of 256: whole waves run every chunk (wave ballots inside shade_slot)
        for (uint32_t base = blockIdx.x * KB; base < pool.n_alloc; base += gridDim.x * KB) {
            const uint32_t s = base + threadIdx.x;
            const SlotIn in = load_slot_global(pool, s, true);
            shade_slot<LIGHTS, LIST, NoPrefetch, M, QMC, MINW == 2, MOT, sky_pass_form(LIST, M, QMC, MOT || PLT, MINW == 2), PLT>(sc, cam, pool, cnt, seed, s, s - (uint32_t)lane, lane, in, shard, n_done, n_died, NoPrefetch{}, 0ull, 0ull, 0u, &env, lstk);
        }
    } else {
        constexpr int WIN = KB * PER;                           // slots per window: eight (or sixteen) per thread
        static_assert(PER * 4 <= 64 && WIN <= 65536 && WIN % 64 == 0, "sixteen 4-bit keys per thread at most, 16-bit slot offsets");
        __shared__ uint16_t s_perm[WIN];
        __shared__ uint32_t s_hw[WIN];                          //  8 KB: K2's result words of the window
        constexpr uint32_t NCLASS = N_CLASSES, K_DEAD = CLASS_DEAD;   // miss, one per material kind, idle, dead
        __shared__ uint32_t s_cnt[NCLASS][WIN / 64];   // [class][64-slot group of the window, in slot order]
        __shared__ uint32_t s_hist[NCLASS], s_next;
        __shared__ uint4 s_stage[KB / 64][STAGE_CHUNKS * 64];   // 24 KB: one staging area per wave (stage_fetch)
        constexpr int NGRP = WIN / 64;
        const int wave = (int)(threadIdx.x >> 6);
        __shared__ uint32_t s_win;
        const uint32_t n_windows = pool.n_alloc / WIN;
        // (Handing the queue's END out in half windows, as k_extend2 does, was measured here too — the other half's slots counted as
        // dead in the sort —: K3 +-0 on the 33.6 M-slot pool, +1.7 % on a 16.8 M-slot one (+2.4 % with the window's loads predicated): a half
        // window pays the whole window's sort and barriers and levels its eight waves' end worse.)
        // The window index of the NEXT round is drawn by thread 0 when its wave has run out of groups and published by the
        // barrier that ends the window anyway: no barrier of its own, and the atomic's round trip (2-3 k cycles the whole
        // block used to sit out at the top of every window) runs while the other waves finish their groups.
        if (threadIdx.x == 0) s_win = (uint32_t)atomicAdd(&cnt->win_shade, 1ull);
        __syncthreads();
        for (;;) {
            PT_STAMP(w0);
            const uint32_t win = s_win;
            if (win >= n_windows) break;
            if (threadIdx.x == 0) s_next = 0;      // (every wave is past the previous window's last grab; the first one of this window comes three barriers later)
            const uint32_t wbase = win * WIN;
            // classify; STABLE counting sort (slot order is kept inside a class, so the work items a
            // wave dequeues — consecutive pixels of one tile — stay together in a group).
            typename std::conditional<(PER > 8), uint64_t, uint32_t>::type keys = 0;   // PER x 4-bit class keys: K2 left the class in the top bits of its result word
            uint32_t rank[PER];
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                // the window's result words stay in LDS: the groups take theirs from here instead of gathering 4 bytes per lane
                // from the pool a second time (a 32-byte sector each)
                const uint32_t hw = pool.hit_prim[wbase + (uint32_t)j * KB + threadIdx.x];
                s_hw[(uint32_t)j * KB + threadIdx.x] = hw;
                keys |= (decltype(keys))(hw >> HIT_CLASS_SHIFT) << (4 * j);
            }
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const uint32_t key = (uint32_t)(keys >> (4 * j)) & 15u;
                rank[j] = 0;
                // only the classes present among the wave's 64 slots cost a ballot (typically two to four); lane k keeps class k's
                // count and stores it — one LDS store per wave and chunk ([r3]; lane 0 used to zero eleven words and write the rest)
                uint32_t mine = 0;
                unsigned long long todo = ~0ull;
                while (todo) {
                    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)key, __ffsll((long long)todo) - 1));
                    const unsigned long long m = __ballot(key == k);
                    if (key == k) rank[j] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if ((uint32_t)lane == k) mine = (uint32_t)__popcll(m);
                    todo &= ~m;
                }
                if ((uint32_t)lane < NCLASS) s_cnt[lane][j * (KB / 64) + wave] = mine;
            }
            __syncthreads();
            // exclusive prefix over the groups in slot order, per class: NGRP = 32 lanes scan one class with five shuffles (the
            // round-1 form — one thread per class walking its 32 counts through LDS, a chain of 32 dependent reads the other
            // 245 threads waited for at the barrier — was a fifth of the sort's time); the block's waves share the classes
            static_assert(NGRP == 32 || NGRP == 64 || NGRP == 128, "one half-wave or one wave per class (two counts per lane for 128)");
            if constexpr (NGRP <= 64) {
            constexpr uint32_t PER_PASS = 64u / (uint32_t)NGRP;          // classes a wave scans at once
            for (uint32_t k = (uint32_t)wave * PER_PASS + (uint32_t)lane / (uint32_t)NGRP; k < NCLASS; k += (KB / 64) * PER_PASS) {
                const int g = lane % NGRP;
                const uint32_t c = s_cnt[k][g];
                uint32_t incl = c;
#pragma unroll
                for (int d = 1; d < NGRP; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, NGRP);
                    if (g >= d) incl += up;
                }
                s_cnt[k][g] = incl - c;
                if (g == NGRP - 1) s_hist[k] = incl;
            }
            } else {
            for (uint32_t k = (uint32_t)wave; k < NCLASS; k += KB / 64) {
                const uint32_t c0 = s_cnt[k][2 * lane], c1 = s_cnt[k][2 * lane + 1];
                uint32_t incl = c0 + c1;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                    if (lane >= d) incl += up;
                }
                s_cnt[k][2 * lane] = incl - c0 - c1;
                s_cnt[k][2 * lane + 1] = incl - c1;
                if (lane == 63) s_hist[k] = incl;
            }
            }
            __syncthreads();
            // first position of every class: lane k of each wave sums the histogram below k (eleven LDS reads by eleven lanes)
            // and the slots fetch theirs by a lane shuffle ([r3]; every thread used to build the table and select from it with
            // eleven compares per slot)
            uint32_t my_base = 0;
            if ((uint32_t)lane < NCLASS)
                for (uint32_t k = 0; k < (uint32_t)lane; ++k) my_base += s_hist[k];
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const uint32_t key = (uint32_t)(keys >> (4 * j)) & 15u;
                const uint32_t cb = (uint32_t)__shfl((int)my_base, (int)key);
                const uint32_t pos = cb + s_cnt[key][j * (KB / 64) + wave] + rank[j];
                s_perm[pos] = (uint16_t)(j * KB + threadIdx.x);
            }
            __syncthreads();
            const uint32_t n_live = (uint32_t)WIN - s_hist[K_DEAD];
            if (!LIST && pool.reorder)                               // shading order: the dead slots sort last, their positions are the window's tail
                for (uint32_t q = n_live + threadIdx.x; q < (uint32_t)WIN; q += KB) pool.bounce_out[wbase + q] = SLOT_DEAD;
            PT_STAMP(w1);
            // groups are taken from the END of the sorted order: the expensive classes (principled, glass) sort
            // last, and starting with them keeps the four waves level when the window runs out (the cheap
            // misses fill the gaps). Lanes past n_live in the top group are bystanders.
            const uint32_t n_groups = (n_live + 63u) / 64u;
            auto grab = [&]() -> uint32_t {                          // this wave's next group of the window (wave-uniform)
                uint32_t g = 0;
                if (lane == 0) g = atomicAdd(&s_next, 1u);
                return (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
            };
            auto slot_of = [&](uint32_t g, bool& enable) -> uint32_t {
                const uint32_t q = (n_groups - 1u - g) * 64u + (uint32_t)lane;
                enable = q < n_live;
                return wbase + s_perm[enable ? q : 0u];
            };
            // The wave's next group is reserved and its records requested (LDS-DMA, stage_fetch) from inside shade_slot, at the
            // point where the current group's arithmetic can hide the fetch; the first group of a window comes straight from
            // the pool. Dynamic mode only (the static mode's extra per-slot arrays are not staged).
            const bool use_stage = PT_K3_PREFETCH && pool.dynamic != 0u;
            uint4* stage = s_stage[wave];
            uint32_t g = grab();
            bool staged = false;
            unsigned long long pre_mask = 0ull, pre_base = 0ull;      // work items requested a group ahead (shade_slot)
            uint32_t pre_shard = 0u;
            while (g < n_groups) {
                PT_STAMP(0);
                bool enable;
                const uint32_t s = slot_of(g, enable);
                SlotIn in;
                const uint32_t hw = s_hw[s - wbase];
                if (staged) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA has landed (and this wave's older stores with it)
                    in = load_slot_stage(pool, stage, lane, enable, hw);
                } else {
                    in = load_slot_global(pool, s, enable, &hw);
                }
                PT_DRAIN();
#ifdef PT_STAMPS
                PT_STAMP(ld);
                if (lane == 0) atomicAdd(&g_prof[N_CLASSES][5], t_ld - t_0);   // record wait (load or staged), all classes
#endif
                uint32_t g_next = n_groups;
                bool staged_next = false;
                unsigned long long pre_mask_next = 0ull, pre_base_next = 0ull;
                uint32_t pre_shard_next = 0u;
                auto prefetch = [&]() {
                    g_next = grab();
                    if (use_stage && g_next < n_groups) {
                        bool en;
                        const uint32_t sn = slot_of(g_next, en);
                        __builtin_amdgcn_sched_barrier(0);            // nothing of the current group's loads may sink below the DMA
                        stage_fetch(pool, sn, stage, lane);
                        __builtin_amdgcn_sched_barrier(0);
                        staged_next = true;
#if PT_DEQUEUE_AHEAD
                        // the next group's lanes that are certain to end there (ray left the scene / idle slot): their work items now.
                        // Scenes without a lights list only: K3 -1.2 % (scene 6), -0.7 % (scene 5); the lights instantiation, three
                        // registers from the limit, got 0.9 % SLOWER with it (closed scenes have next to no leaving rays anyway).
                        if constexpr (!LIGHTS && !ENV && !MED && !PLT) {
                        const uint32_t cn = s_hw[sn - wbase] >> HIT_CLASS_SHIFT;
                        pre_mask_next = __ballot(en && (cn == CLASS_MISS || cn == CLASS_IDLE));
                        pre_shard_next = shard;
                        if (pre_mask_next && lane == __ffsll((long long)pre_mask_next) - 1)
                            pre_base_next = atomicAdd(&cnt->work[shard].next, (unsigned long long)__popcll(pre_mask_next));
                        }
#endif
                    }
                };
                shade_slot<LIGHTS, LIST, decltype(prefetch)&, M, QMC, MINW == 2, MOT, sky_pass_form(LIST, M, QMC, MOT || PLT, MINW == 2), PLT>(sc, cam, pool, cnt, seed, s, wbase + (n_groups - 1u - g) * 64u, lane, in, shard, n_done,
                                                             n_died, prefetch, pre_mask, pre_base, pre_shard, &env, lstk);
                pre_mask = pre_mask_next;
                pre_base = pre_base_next;
                pre_shard = pre_shard_next;
#ifdef PT_STAMPS
                if (lane == 0) atomicAdd(&g_prof[N_CLASSES][4], 1ull);
#endif
                g = g_next;
                staged = staged_next;
            }
            PT_STAMP(w2);
            if (threadIdx.x == 0) s_win = (uint32_t)atomicAdd(&cnt->win_shade, 1ull);   // everybody read s_win before this window's first barrier
            __syncthreads();   // LDS is reused by the next window
#ifdef PT_STAMPS
            PT_STAMP(w3);
            if (lane == 0) {
                atomicAdd(&g_prof[N_CLASSES][0], 1ull);
                atomicAdd(&g_prof[N_CLASSES][1], t_w1 - t_w0);     // window draw + classification + sort
                atomicAdd(&g_prof[N_CLASSES][2], t_w2 - t_w1);     // shading groups
                atomicAdd(&g_prof[N_CLASSES][3], t_w3 - t_w2);     // waiting for the block's other waves
            }
#endif
        }
    }
    const unsigned long long w_done = wave_sum(n_done), w_died = wave_sum(n_died);
    if (lane == 0) {
        if (w_done) atomicAdd(&cnt->samples, w_done);
        if (w_died) atomicSub(&cnt->alive, w_died);
    }
#ifdef PT_STAMPS
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (N_CLASSES + 1) * PROF_COLS; i += KB)
        if ((&g_prof[0][0])[i]) atomicAdd(&cnt->prof[0][0] + i, (&g_prof[0][0])[i]);
#endif
}

}  // namespace pt
