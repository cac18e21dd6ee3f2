// Spectral dispersion of glass (pt_mat_glass_set_dispersion; the rule is in include/pt_amd.h): the wavelength of a path, its
// bin of the weight table and the two-term Cauchy index of refraction, as k_shade's DSP forms and the dispersion probe call them.
#pragma once
#include "pt_dev_math.h"
#include "pt_types.h"

namespace pt {

// The 64 bits the wavelength of sample `sample` of `pixel` is made of: a Philox stream of its own (counter word 3 = 2; 0 and 1 are the
// two samplers'), so no draw of the path's stream is made. Independent sampler: one block per sample, through philox_block — the body the
// kernel holds anyway. Sobol sampler: one block of keys per pixel, the sample index Owen-scrambled (owen(sobol0(s), K[0]) = rev(lk(s, K[0])):
// the reversals telescope as in sobol_pair) — a real function, like sobol_pair, which inlines the rounds (a QMC kernel has no philox_block).
template <int = 0>
PT_PHILOX_CALL uint64_t dsp_bits_sobol(uint32_t seed_lo, uint32_t seed_hi, uint32_t pixel, uint32_t sample) {
    const PhiloxOut key = philox_rounds(0u, 0u, seed_hi, 2u, seed_lo, pixel);
    const uint32_t x = __brev(lk_hash(sample, key.x));
    return ((uint64_t)x << 32) | lk_hash(x, key.y);
}
template <bool QMC>
PT_DEV uint64_t dsp_bits(uint32_t seed_lo, uint32_t seed_hi, uint32_t pixel, uint32_t sample) {
    if constexpr (QMC) {
        return dsp_bits_sobol(seed_lo, seed_hi, pixel, sample);
    } else {
        const PhiloxOut o = philox_block(0u, sample, seed_hi, 2u, seed_lo, pixel);
        return ((uint64_t)o.x << 32) | o.y;
    }
}
struct WavelengthD {
    double u, lambda;   // u in [0, 1), lambda = 380 + u * 350 (nm)
    uint32_t bin;       // min(floor(u * DSP_BINS), DSP_BINS - 1): the row of the weight table
};
template <bool QMC>
PT_DEV WavelengthD dsp_wavelength(uint32_t seed_lo, uint32_t seed_hi, uint32_t pixel, uint32_t sample) {
    WavelengthD w;
    w.u = u64_to_unit(dsp_bits<QMC>(seed_lo, seed_hi, pixel, sample));
    w.lambda = 380.0 + w.u * 350.0;
    const uint32_t j = (uint32_t)(w.u * (double)DSP_BINS);
    w.bin = j < (uint32_t)DSP_BINS - 1u ? j : (uint32_t)DSP_BINS - 1u;
    return w;
}
// n(lambda) = n_d + b * (inv2(lambda_nm * 1e-3) - inv2_d), inv2(l) = 1 / (l * l); b and inv2_d = inv2(0.58756) come from the host (MatD::p[1], p[2])
PT_DEV double dsp_inv2(double l) { return 1.0 / (l * l); }
PT_DEV double dsp_ior(double n_d, double b, double inv2_d, double lambda_nm) { return n_d + b * (dsp_inv2(lambda_nm * 1e-3) - inv2_d); }
PT_DEV bool dsp_is_dispersive(const MatD& m) { return m.kind == MAT_GLASS && m.p[3] != 0.0; }

}  // namespace pt
