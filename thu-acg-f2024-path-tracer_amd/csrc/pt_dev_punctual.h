// Punctual lights (the rule: include/pt_amd.h): what a light of the list sends to a point, and how far a shadow ray's
// origin is from it. Plain f64 on arrays of doubles, one rounding per written operation, compiled for the device (k_shade's PLT forms,
// k_punctual_probe) and for the host (pt_punctual_eval): the same function on both sides, so a CPU test holds what the kernels run.
#pragma once
#include "pt_detmath.h"
#include "pt_types.h"

#define PT_PL PT_DM   // host and device under hipcc, host elsewhere

namespace pt {

// w: the unit direction from the point to the light; D: the distance (+inf for a directional light); d2 = D * D before the root (1 for a
// directional light: never an ending); E: what arrives per unit area facing the light.
struct PunctualEval {
    double w[3], D, d2, E[3];
};
PT_PL PunctualEval punctual_eval(const PunctualD& L, const double x[3]) {
    PunctualEval r;
    if (L.kind == 2u) {
        r.w[0] = -L.axis[0]; r.w[1] = -L.axis[1]; r.w[2] = -L.axis[2];
        r.D = __builtin_huge_val();
        r.d2 = 1.0;
        r.E[0] = L.I[0]; r.E[1] = L.I[1]; r.E[2] = L.I[2];
        return r;
    }
    const double lx = L.pos[0] - x[0], ly = L.pos[1] - x[1], lz = L.pos[2] - x[2];
    const double d2 = (lx * lx) + (ly * ly) + (lz * lz);
    const double D = __builtin_sqrt(d2);
    r.w[0] = lx / D; r.w[1] = ly / D; r.w[2] = lz / D;
    r.D = D;
    r.d2 = d2;
    if (L.kind == 1u) {
        const double c = -((r.w[0] * L.axis[0]) + (r.w[1] * L.axis[1]) + (r.w[2] * L.axis[2]));
        double s;
        if (L.cos_i > L.cos_o) {
            s = (c - L.cos_o) / (L.cos_i - L.cos_o);
            if (s < 0.0) s = 0.0;
            if (s > 1.0) s = 1.0;
        } else {
            s = c >= L.cos_o ? 1.0 : 0.0;
        }
        const double fall = (s * s) * (3.0 - 2.0 * s);
        r.E[0] = (L.I[0] * fall) / d2; r.E[1] = (L.I[1] * fall) / d2; r.E[2] = (L.I[2] * fall) / d2;
    } else {
        r.E[0] = L.I[0] / d2; r.E[1] = L.I[1] / d2; r.E[2] = L.I[2] / d2;
    }
    return r;
}
// D' of a SHADOW segment: from the stored ray origin o to the light; +inf for a directional light
PT_PL double punctual_shadow_distance(const PunctualD& L, const double o[3]) {
    if (L.kind == 2u) return __builtin_huge_val();
    const double lx = L.pos[0] - o[0], ly = L.pos[1] - o[1], lz = L.pos[2] - o[2];
    return __builtin_sqrt((lx * lx) + (ly * ly) + (lz * lz));
}

}  // namespace pt
