"""The film stage's rule (pt_film_develop, include/pt_amd.h) restated in numpy: exposure, the bright part, separable Gaussian glare by
direct convolution (np.convolve per row and per column, zero outside the image, weights not renormalised), the tone curves.

film_np returns (hdr, v): the scene-linear image and the PRE-quantisation value of the display image; quantise(v) is the rule's last
step. The sums of a convolution are taken in numpy's order, the kernels take them in theirs: every term is non-negative, so the two
agree to about (2 r + 1) * 2^-53 relative."""
import numpy as np

TONEMAPS = {"reference": 0, "srgb": 1, "reinhard": 2, "aces": 3}
DEFAULTS = dict(exposure_ev=0.0, tonemap=0, white=4.0, bloom_strength=0.0, bloom_threshold=1.0, bloom_sigma=2.0, bloom_levels=5)


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def exposed(sums, n_or_counts, exposure_ev=0.0):
    """Step 1: x = fmax(sum * (1 / n) * 2^ev, 0): NaN and negatives become 0, +inf stays."""
    sums = np.asarray(sums, dtype=np.float64)
    n = np.asarray(n_or_counts, dtype=np.float64)
    scale = 1.0 / n
    if scale.ndim:
        scale = scale.reshape(sums.shape[0], sums.shape[1], 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.fmax((sums * scale) * np.exp2(np.float64(exposure_ev)), 0.0)


def bright_part(x, threshold):
    """Step 2: B = x * w, w = (Y - T) / Y where Y = lum(x) is finite and above T, else 0."""
    y = lum(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where((y > threshold) & np.isfinite(y), (y - threshold) / y, 0.0)
        return x * w[..., None]


def gauss_taps(sigma):
    r = int(np.ceil(3.0 * sigma))
    k = np.array([np.exp(-(float(i) * float(i)) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)])
    s = 0.0
    for v in k:
        s += v
    return k / s, r


def radii(bloom_sigma=2.0, bloom_levels=5):
    return [int(np.ceil(3.0 * bloom_sigma * 2.0 ** l)) for l in range(bloom_levels)]


def glare(b, bloom_sigma=2.0, bloom_levels=5):
    """Step 3's G = sum_l (1 / L) V_l of the bright part b (H, W, 3)."""
    h, w = b.shape[:2]
    g = np.zeros_like(b)
    for l in range(bloom_levels):
        k, r = gauss_taps(bloom_sigma * 2.0 ** l)
        hor = np.empty_like(b)
        ver = np.empty_like(b)
        for c in range(3):
            for y in range(h):
                hor[y, :, c] = np.convolve(b[y, :, c], k, mode="full")[r:r + w]   # (the taps are symmetric: correlation = convolution)
            for x in range(w):
                ver[:, x, c] = np.convolve(hor[:, x, c], k, mode="full")[r:r + h]
        g = g + (1.0 / bloom_levels) * ver
    return g


def oetf(t):
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0.0031308, 12.92 * t, 1.055 * np.power(t, 1.0 / 2.4) - 0.055)


def tone(o, tonemap=0, white=4.0):
    """Step 5: the pre-quantisation value v of the scene-linear image o."""
    tonemap = TONEMAPS.get(tonemap, tonemap)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if tonemap == 0:
            return np.sqrt(o)
        o = np.fmin(o, 1e150)
        if tonemap == 1:
            return oetf(np.fmin(o, 1.0))
        if tonemap == 2:
            y = lum(o)
            sc = (1.0 + y / (white * white)) / (1.0 + y)
            return oetf(np.fmin(o * sc[..., None], 1.0))
        t = (o * (2.51 * o + 0.03)) / (o * (2.43 * o + 0.59) + 0.14)
        return oetf(np.clip(t, 0.0, 1.0))


def quantise(v):
    """Step 6: (uint8)(clamp(v, 0, 0.999) * 256), NaN -> 0."""
    q = np.clip(v, 0.0, 0.999) * 256.0
    return np.where(np.isnan(q), 0.0, q).astype(np.uint8)


def film_np(sums, n_or_counts, glare_of=None, **opts):
    """(hdr, v) of the rule. glare_of: an optional function (b, sigma, levels) -> G standing in for glare(), so that callers can share
    one G among calls that differ only in what follows it."""
    o = dict(DEFAULTS)
    o.update(opts)
    x = exposed(sums, n_or_counts, o["exposure_ev"])
    s = o["bloom_strength"]
    if s > 0.0:
        b = bright_part(x, o["bloom_threshold"])
        g = (glare_of or glare)(b, o["bloom_sigma"], o["bloom_levels"])
        with np.errstate(invalid="ignore"):
            hdr = (x - s * b) + s * g
    else:
        hdr = x
    return hdr, tone(hdr, o["tonemap"], o["white"])
