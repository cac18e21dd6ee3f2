// Which forms of k_shade and k_init exist, which translation unit compiles them, and how a run-time ShadeForm (pt_kernels.h) becomes a
// kernel pointer. A form is a shape (SHADE_SHAPES), five bools (lights, list, qmc, motion, punctual — the last two exclude each other) and the shading mode (pt_types.h ShadeMode,
// which says what the modes are and how they nest). A new exclusive feature is one more ShadeMode and, if its forms want a unit of their
// own, one more FormUnit with its accessor.
#pragma once
#include <utility>

#include "pt_k3_shade.h"

namespace pt {

typedef void (*shade_fn)(SceneD, CamD, PoolD, CountersD*, uint64_t, EnvTabD);
typedef void (*init_fn)(CamD, PoolD, uint64_t);
typedef void (*aov_fn)(SceneD, CamD, uint64_t, uint32_t, uint32_t, double*, uint32_t);

// THE list of k_shade's shapes: variant code = sort * 10 + min waves per SIMD -> k_shade<SORT, MINW, LIGHTS, KB, PER, ...>
struct ShadeShape { int variant; bool sort; int minw, kb, per; };   // KB threads per block; a sorted block takes windows of KB * PER slots
constexpr ShadeShape SHADE_SHAPES[] = {
    {2, false, 2, BLOCK, 8},                                  // unsorted — row 0 is also what an unknown code given through PT_SHADE_VARIANT gets
    {3, false, 3, BLOCK, 8},
    {12, true, 2, BLOCK, 8},                                  // sorted, 2048-slot windows
    {13, true, 3, BLOCK, 8},
    {22, true, 2, 512, 8},                                    // sorted, 512 threads / 4096-slot windows
    {32, true, 2, 512, 16},                                   // the same over 8192-slot windows
    {42, true, 2, 512, 16},                                   // 32 or 22 per launch (launch_shade); its occupancy is asked on the 8192-slot shape
    {52, true, 2, BLOCK, 16},                                 // A/B: 256 threads over 4096-slot windows (window size vs block size)
};
constexpr int N_SHADE_SHAPES = sizeof(SHADE_SHAPES) / sizeof(SHADE_SHAPES[0]);
constexpr int shade_row(int variant, int i = N_SHADE_SHAPES - 1) { return i == 0 || SHADE_SHAPES[i].variant == variant ? i : shade_row(variant, i - 1); }
// Which forms exist: a shape other than the default variant's three has the plain mode only, without pixel list and Sobol sampler; the
// LSE forms need a lights list. The MOT forms (motion in effect) are plain-mode forms of the default variant's shapes.
constexpr bool shade_form_exists(const ShadeShape& s, bool lights, bool list, bool qmc, ShadeMode mode, bool motion = false) {
    return (s.variant == 22 || s.variant == 32 || s.variant == 42 || !(list || qmc || motion || mode != MODE_PLAIN)) && (mode != MODE_LSE || lights) &&
           (!motion || mode == MODE_PLAIN);
}
// ... and with the fifth bool: the PLT forms (punctual lights in effect) are plain-mode forms of the default variant's shapes
// too, without motion — and, for light shafts, MED and HET forms of the same shapes; every other form is what it is above.
constexpr bool shade_form_exists(const ShadeShape& s, bool lights, bool list, bool qmc, ShadeMode mode, bool motion, bool punctual) {
    return punctual ? (s.variant == 22 || s.variant == 32 || s.variant == 42) && (mode == MODE_PLAIN || mode == MODE_MED || mode == MODE_HET) && !motion
                    : shade_form_exists(s, lights, list, qmc, mode, motion);
}
// the unit that compiles a form: pt_k3.hip, pt_k3_qmc.hip, or the mode's own — pt_k3_med.hip (§12), pt_k3_het.hip (§13),
// pt_k3_int.hip (§14), pt_k3_lse.hip (§15), pt_k3_dsp.hip (§16), each with and without QMC. K1 has a plain and a MED form only — a camera
// ray's bounce word is the MED forms', or 0 — so a render's k_init comes from the unit of (its mode has media ? MED : PLAIN, qmc).
// The MOT forms of K1 / K3 (plain mode, with and without QMC) are pt_k3_mot.hip's (§19). The PLT forms of K3 (plain mode, with and without
// QMC) are pt_k3_plt.hip's (§21); K1 has none — a camera ray's bounce word is 0 — so such a render's k_init is the plain or QMC unit's.
// The light-shaft forms of K3 (PLT in the modes MED and HET, with and without QMC) are pt_k3_shf.hip's (§22); a camera ray's bounce word is
// the MED forms', so such a render's k_init is pt_k3_med.hip's.
enum FormUnit { UNIT_PLAIN, UNIT_QMC, UNIT_MED, UNIT_HET, UNIT_INT, UNIT_LSE, UNIT_DSP, UNIT_MOT, UNIT_PLT, UNIT_SHF };
constexpr FormUnit form_unit(ShadeMode mode, bool qmc, bool motion = false, bool punctual = false) {
    if (punctual) return mode == MODE_MED || mode == MODE_HET ? UNIT_SHF : UNIT_PLT;
    if (motion) return UNIT_MOT;
    switch (mode) {
    case MODE_MED: return UNIT_MED; case MODE_HET: return UNIT_HET; case MODE_INT: return UNIT_INT; case MODE_LSE: return UNIT_LSE; case MODE_DSP: return UNIT_DSP;
    default: return qmc ? UNIT_QMC : UNIT_PLAIN;   // PLAIN, ENV
    }
}

// run-time bools -> template arguments: f is called with one std::bool_constant per bool
template <class F> auto expand_bools(F&& f) { return f(); }
template <class F, class... Rest> auto expand_bools(F&& f, bool b, Rest... rest) {
    return b ? expand_bools([&](auto... tail) { return f(std::true_type{}, tail...); }, rest...)
             : expand_bools([&](auto... tail) { return f(std::false_type{}, tail...); }, rest...);
}

// The kernels of unit U for a form; null where the form does not exist or belongs to another unit. Every unit instantiates exactly the
// forms it owns by compiling unit_forms<its U>.
struct FormKernels { shade_fn shade; init_fn init; aov_fn aov; };   // (k_aov / k_aov_qmc are not templates: the unit's accessor names its own)
template <FormUnit U, int ROW, ShadeMode M, bool LIGHTS, bool LIST, bool QMC, bool MOT, bool PLT> shade_fn shade_kernel() {
    constexpr ShadeShape S = SHADE_SHAPES[ROW];
    if constexpr (shade_form_exists(S, LIGHTS, LIST, QMC, M, MOT, PLT) && form_unit(M, QMC, MOT, PLT) == U) return k_shade<S.sort, S.minw, LIGHTS, S.kb, S.per, LIST, M, QMC, MOT, PLT>;
    else return nullptr;
}
template <FormUnit U, size_t... I> shade_fn shade_of(const ShadeForm& f, std::index_sequence<I...>) {   // I = shape row * N_SHADE_MODES + mode
    shade_fn k = nullptr;
    ((shade_row(f.variant) * N_SHADE_MODES + f.mode == (int)I ? k = expand_bools([](auto... b) { return shade_kernel<U, (int)I / N_SHADE_MODES, (ShadeMode)(I % N_SHADE_MODES), decltype(b)::value...>(); }, f.lights, f.list, f.qmc, f.motion, f.punctual) : k), ...);
    return k;
}
template <FormUnit U> FormKernels unit_forms(const ShadeForm& f, aov_fn aov) {
    return FormKernels{shade_of<U>(f, std::make_index_sequence<N_SHADE_SHAPES * N_SHADE_MODES>{}),
                       expand_bools([](auto list, auto qmc, auto med, auto mot) -> init_fn {
                                        if constexpr (!(med && mot) && form_unit(med ? MODE_MED : MODE_PLAIN, qmc, mot) == U) return k_init<list, qmc, med, mot>; else return nullptr; },
                                    f.list, f.qmc, mode_has_media(f.mode), f.motion), aov};
}
// the units' accessors (pt_k3.hip, pt_k3_qmc.hip, pt_k3_med.hip, pt_k3_het.hip, pt_k3_int.hip, pt_k3_lse.hip, pt_k3_dsp.hip, pt_k3_mot.hip, pt_k3_plt.hip, pt_k3_shf.hip) — the only calls from one kernel unit into another
FormKernels forms_plain(const ShadeForm& f), forms_qmc(const ShadeForm& f), forms_med(const ShadeForm& f), forms_het(const ShadeForm& f), forms_int(const ShadeForm& f),
    forms_lse(const ShadeForm& f), forms_dsp(const ShadeForm& f), forms_mot(const ShadeForm& f), forms_plt(const ShadeForm& f), forms_shf(const ShadeForm& f);

}  // namespace pt
