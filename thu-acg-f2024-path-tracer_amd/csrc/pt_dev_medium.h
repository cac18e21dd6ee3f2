// Device-side homogeneous participating media (pt_mat_medium; the rule is in include/pt_amd.h): the free-flight
// distance and the Henyey-Greenstein phase function. Called by k_shade's MED forms and by the probe behind pt_medium_probe — the
// same functions, so what the probe returns is what a path computes.
#pragma once
#include "pt_dev_math.h"
#include "pt_types.h"

namespace pt {

// a real function like dev_log2 (pt_dev_math.h): k_shade's MED forms hold the logarithm once
PT_DM_CALL double dev_log(double x) { return detmath::log(x); }

// the medium record of a path's medium word (PoolD bounce word >> MEDIUM_SHIFT = material index + 1)
struct MediumD {
    double density, g;
    V3 albedo;
    bool bounded;   // some world object carries this material: a ray that left the scene cannot be inside it
};
PT_DEV MediumD load_medium(const SceneD& sc, uint32_t med) {
    const MatD& m = sc.mats[med - 1u];
    return MediumD{m.p[0], m.p[1], V3{m.p[2], m.p[3], m.p[4]}, m.p[5] != 0.0};
}

// d = -log(1 - u) / density, u in [0, 1)
PT_DEV double medium_free_flight(double u, double density) { return -dev_log(1.0 - u) / density; }

// ph(c) = (1 - g^2) / (4 pi s sqrt(s)), s = 1 + g^2 - 2 g c, c = the cosine between the propagation direction and the new one
PT_DEV double hg_phase(double g, double c) {
    const double s = 1.0 + g * g - 2.0 * g * c;
    return (1.0 - g * g) / (4.0 * D_PI * s * sqrt(s));
}
// The direction two unit draws give: cos_t by the inverse of HG's CDF (isotropic below |g| = 1e-3), phi = 2 pi u2, expressed in the
// shading frame built around `axis` (frame_to_z) — `axis` is the propagation direction, g > 0 scatters forward.
PT_DEV V3 hg_sample(double g, double u1, double u2, V3 axis) {
    double cos_t;
    if (fabs(g) < 1e-3) {
        cos_t = 1.0 - 2.0 * u1;
    } else {
        const double q = (1.0 - g * g) / (1.0 - g + 2.0 * g * u1);
        cos_t = (1.0 + g * g - q * q) / (2.0 * g);
    }
    cos_t = clampd(cos_t, -1.0, 1.0);
    const double sin_t = sqrt(fmax(0.0, 1.0 - cos_t * cos_t));
    const double phi = 2.0 * D_PI * u2;
    const SinCos sc_phi = dev_sincos(phi);
    const Frame f = frame_to_z(axis);
    return to_world(f, V3{sin_t * sc_phi.c, sin_t * sc_phi.s, cos_t});
}

}  // namespace pt
