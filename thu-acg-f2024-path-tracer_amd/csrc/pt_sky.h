// The physical sky (the rule in include/pt_amd.h): Preetham-Shirley-Smits daylight above the horizon, a Lambertian
// ground below it. This header is the per-direction part of the rule, written once for host and device: pt_sky_eval runs it on the
// host, the bake kernel and pt_sky_probe on the GPU (pt_sky.hip), and the unit is built with -ffp-contract=off on both sides, so the
// two execute the same sequence of IEEE operations and agree bit for bit. Everything that does not depend on the direction — the
// coefficients, the zenith values, F(0, theta_s), the ground's radiance, the disc's radiance — is formed once on the host
// (sky_setup, pt_sky.hip) and travels in SkyParams, a by-value kernel argument: it sits in SGPRs for the whole launch.
#pragma once
#include <stdint.h>

#include "pt_detmath.h"

#if defined(__HIPCC__)
#define PT_SKY_HD __host__ __device__ inline
#else
#define PT_SKY_HD inline
#endif

namespace pt {

constexpr double SKY_PI = 3.14159265358979323846264338327950288;

struct SkyParams {
    double s[3];          // the normalised sun direction
    double coef[3][5];    // A..E of Y, x, y
    double zen[3];        // Yz, xz, yz
    double den[3];        // F(0, theta_s) of Y, x, y
    double scale;
    double ground[3];     // G: the radiance of every direction with d.y <= 0
    double l_sun[3];      // the disc's radiance L_sun (bake only; 0 without a disc)
    double cos_alpha;     // cos of the disc's angular radius
};

// Perez's F without its first factor's argument fixed: (1 + A exp(B / cos_theta)) (1 + C exp(D gamma) + E cos_gamma^2)
PT_SKY_HD double sky_perez(const double* k, double cos_theta, double gamma, double cos_gamma) {
    const double a = 1.0 + k[0] * detmath::exp(k[1] / cos_theta);
    const double b = (1.0 + k[2] * detmath::exp(k[3] * gamma)) + k[4] * (cos_gamma * cos_gamma);
    return a * b;
}
PT_SKY_HD double sky_dot(const double* s, double x, double y, double z) { return (x * s[0] + y * s[1]) + z * s[2]; }

// The radiance of direction d (unit length, used as given): the sky for d.y > 0, else the ground. No disc.
PT_SKY_HD void sky_radiance(const SkyParams& P, double dx, double dy, double dz, double out[3]) {
    if (!(dy > 0.0)) {
        out[0] = P.ground[0]; out[1] = P.ground[1]; out[2] = P.ground[2];
        return;
    }
    double cg = sky_dot(P.s, dx, dy, dz);
    if (cg < -1.0) cg = -1.0;
    if (cg > 1.0) cg = 1.0;
    const double gamma = detmath::acos(cg);
    double q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = (P.zen[c] * sky_perez(P.coef[c], dy, gamma, cg)) / P.den[c];
    const double Y = q[0];
    const double X = (q[1] / q[2]) * Y;
    const double Z = (((1.0 - q[1]) - q[2]) / q[2]) * Y;
    const double r = (3.2404542 * X + -1.5371385 * Y) + -0.4985314 * Z;
    const double g = (-0.9692660 * X + 1.8760108 * Y) + 0.0415560 * Z;
    const double b = (0.0556434 * X + -0.2040259 * Y) + 1.0572252 * Z;
    out[0] = (r > 0.0 ? r : 0.0) * P.scale;
    out[1] = (g > 0.0 ? g : 0.0) * P.scale;
    out[2] = (b > 0.0 ? b : 0.0) * P.scale;
}

}  // namespace pt
