"""The spectral-dispersion rule (pt_mat_glass_set_dispersion in include/pt_amd.h) restated in numpy, for the dispersion
tests: the wavelength of a path under both samplers, the weight table, the Cauchy index, the closed form of a dispersive slab between
two environment tones, and a scalar replay of whole paths through a rough dispersive glass sphere (the glass sampler is
interior_rule's; refs_numpy.glass_pdf_eval has pdf and eval)."""
import math

import numpy as np

import interior_rule as IR
import medium_rule as MR
import refs_numpy as R
import sampler_rule as SR

BINS = 64
LAMBDA_MIN, LAMBDA_RANGE = 380.0, 350.0
LAMBDA_D, LAMBDA_F, LAMBDA_C = 587.56, 486.13, 656.27


# ---- the wavelength of a path ----------------------------------------------------------------------------------------------------
def wavelength_u64(seed, pixel, s, sobol=False):
    """The 64 bits behind the wavelength of sample s of `pixel` under `seed`: Philox counter word 3 = 2, a stream of its own."""
    seed = int(seed)
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    if sobol:
        K = SR.philox4x32_10(0, 0, hi, 2, lo, pixel)
        x = SR.owen(SR.sobol0(s), K[0])
        return (x << np.uint64(32)) | SR.lk(x, K[1])
    K = SR.philox4x32_10(0, s, hi, 2, lo, pixel)
    return (K[0] << np.uint64(32)) | K[1]


def wavelength(seed, pixel, s, sobol=False):
    """(u, lambda in nm, bin) of sample s of `pixel` under `seed`."""
    u = SR.unit(wavelength_u64(seed, pixel, s, sobol))
    return u, LAMBDA_MIN + u * LAMBDA_RANGE, np.minimum(np.floor(u * BINS).astype(np.int64), BINS - 1)


# ---- the weight table --------------------------------------------------------------------------------------------------------------
def _g(l, mu, s1, s2):
    t = (l - mu) / np.where(l < mu, s1, s2)
    return np.exp(-0.5 * (t * t))


def weight_table():
    """W[64][3]: linear-sRGB weights of the bins, each channel's mean over the bins exactly 1 (to rounding)."""
    l = LAMBDA_MIN + (np.arange(BINS) + 0.5) * (LAMBDA_RANGE / BINS)
    x = 1.056 * _g(l, 599.8, 37.9, 31.0) + 0.362 * _g(l, 442.0, 16.0, 26.7) - 0.065 * _g(l, 501.1, 20.4, 26.2)
    y = 0.821 * _g(l, 568.8, 46.9, 40.5) + 0.286 * _g(l, 530.9, 16.3, 31.1)
    z = 1.217 * _g(l, 437.0, 11.8, 36.0) + 0.681 * _g(l, 459.0, 26.0, 13.8)
    rgb = np.stack([3.2404542 * x - 1.5371385 * y - 0.4985314 * z, -0.9692660 * x + 1.8760108 * y + 0.0415560 * z,
                    0.0556434 * x - 0.2040259 * y + 1.0572252 * z], axis=1)
    raw = np.maximum(0.0, rgb)
    total = np.zeros(3)
    for k in range(BINS):                                # summed in order
        total = total + raw[k]
    return raw * BINS / total


# ---- the Cauchy index ---------------------------------------------------------------------------------------------------------------
def inv2(l):
    return 1.0 / (l * l)


def cauchy_b(n_d, abbe):
    return (n_d - 1.0) / (abbe * (inv2(0.48613) - inv2(0.65627)))


def ior(n_d, abbe, lambda_nm):
    """n(lambda), the operations in the rule's order."""
    lam = np.asarray(lambda_nm, dtype=np.float64)
    return n_d + cauchy_b(n_d, abbe) * (inv2(lam * 1e-3) - inv2(0.58756))


# ---- the slab between two tones: closed form by quadrature ----------------------------------------------------------------------------
def fresnel_flat(cos_i, n):
    """interior_rule.slab_angles' reflectance (glass.rs:51-62 at a flat interface met from outside at cos_i), elementwise over arrays."""
    c = np.abs(np.asarray(cos_i, dtype=np.float64))
    g = np.sqrt(n * n - 1.0 + c * c)                     # n > 1: never negative
    gmc, gpc = g - c, g + c
    x = (c * gpc - 1.0) / (c * gmc + 1.0)
    return 0.5 * (gmc * gmc) / (gpc * gpc) * (1.0 + x * x)


def slab_two_tone(cos_i, n_d, abbe, upper, lower, order=8):
    """A smooth dispersive slab seen from above at cos_i per pixel (any shape), the environment `upper` where reflected paths leave and
    `lower` where transmitted ones do: every sample is W_c[j] * upper with probability R_tot(lambda) = 2R / (1 + R), else W_c[j] * lower
    (T_tot = (1 - R) / (1 + R)), R the Fresnel reflectance at n(lambda), lambda uniform in [380, 730). Returns (mean, second moment)
    of the sample, shape cos_i.shape + (3,): Gauss-Legendre of `order` points inside each bin. abbe = None: n == n_d."""
    cos_i = np.asarray(cos_i, dtype=np.float64)
    W = weight_table()
    x, w = np.polynomial.legendre.leggauss(order)
    width = LAMBDA_RANGE / BINS
    mean = np.zeros(cos_i.shape + (3,))
    second = np.zeros(cos_i.shape + (3,))
    for j in range(BINS):
        for xi, wi in zip(x, w):
            lam = LAMBDA_MIN + (j + 0.5 + 0.5 * xi) * width
            n = n_d if abbe is None else float(ior(n_d, abbe, lam))
            Rf = fresnel_flat(cos_i, n)
            r_tot, t_tot = 2.0 * Rf / (1.0 + Rf), (1.0 - Rf) / (1.0 + Rf)
            share = 0.5 * wi / BINS                      # of the whole range
            mean += share * W[j] * (r_tot * upper + t_tot * lower)[..., None]
            second += share * W[j] ** 2 * (r_tot * upper ** 2 + t_tot * lower ** 2)[..., None]
    return mean, second


def accept(z, zg):
    """The z-test acceptance of the estimator tests (test_medium_gpu.py, test_interior_gpu.py): per pixel and channel, and the frame mean."""
    assert np.isfinite(z).all()
    print(f"z: std {z.std():.3f}, max |z| {np.abs(z).max():.2f}, share |z| > 4: {(np.abs(z) > 4).mean():.4f}, image mean z {zg}")
    assert np.abs(zg).max() < 4.0, zg
    assert (np.abs(z) > 4.0).mean() < 0.01
    assert 0.85 < z.std() < 1.3, z.std()


# ---- the replay: a rough dispersive glass sphere under a two-tone environment ----------------------------------------------------------
def two_tone_env(d, upper, lower):
    """sample_environment on a map of two rows: the upper row for directions above the horizon (acos(d.y) < pi / 2)."""
    return np.asarray(upper if d[1] > 0.0 else lower, dtype=np.float64)


def replay_dispersive_path(center, radius, roughness, n_d, abbe, frame, cam, seed, pixel, sample, upper, lower, sobol=False):
    """The radiance (3,) of sample `sample` of `pixel` by the rule, in scalar numpy: one glass sphere with an Abbe number, no lights, the
    two-tone environment. Returns (radiance, number of glass hits)."""
    f64 = SR.sobol_u64 if sobol else SR.independent_u64

    def U(d):
        return float(SR.unit(f64(seed, pixel, sample, d)))

    _, lam, j = wavelength(seed, pixel, sample, sobol)
    n_l = float(ior(n_d, abbe, lam))
    w_l = weight_table()[int(j)]
    ly, lx = SR.camera_locations(frame, cam["blur_strength"], cam["width"], seed, [pixel], [sample], sobol=sobol)
    loc = frame["pixel00"] + frame["dv"] * ly[0, 0] + frame["du"] * lx[0, 0]
    o = np.asarray(frame["center"], dtype=np.float64)
    d = IR._norm(loc - o)
    draw = 5                       # pixel offsets (2), lens offsets (2), time (1)
    c = np.asarray(center, dtype=np.float64)
    bounce, thr, mono, hits = 0, np.ones(3), False, 0
    while True:
        hit = MR._hit_sphere(o, d, c, radius)
        if hit is None:
            return thr * two_tone_env(d, upper, lower), hits
        hits += 1
        _, p, n = hit
        front = float(d @ n) < 0.0
        gn = n if front else -n
        if bounce > 5:             # roulette
            pr = min(max(MR.luminance(thr), 0.01), 1.0)
            r = U(draw)
            draw += 1
            if r > pr:
                return np.zeros(3), hits
            thr = thr / pr
        draw += 1                  # the selector: drawn, never below p_light = 0
        q = MR.frame_to_z(gn)
        v = IR.to_local(q, -d)
        if sobol:
            draw = (draw + 1) & ~1
        e1, e2 = U(draw), U(draw + 1)
        draw += 2
        h = IR.ggx_sample_microfacet_normal(v, roughness, e1, e2)
        eta_i, eta_o = (1.0, n_l) if front else (n_l, 1.0)            # every read of the glass's ior takes n(lambda)
        uf = U(draw)
        draw += 1
        wi = IR.to_world(q, IR.sample_dielectric(v, h, eta_i, eta_o, uf))
        pdf, brdf = R.glass_pdf_eval(roughness, n_l, v, IR.to_local(q, wi), front)
        thr = thr * (brdf / pdf)
        if not mono:               # weighted once, at the path's first continued bounce on the dispersive glass
            thr = thr * w_l
            mono = True
        side = float(wi @ gn)
        o = p + (-IR.T_OFFSET if np.signbit(side) else IR.T_OFFSET) * gn
        d = IR._norm(wi)
        bounce += 1
        if bounce >= cam["max_depth"]:
            return np.zeros(3), hits
