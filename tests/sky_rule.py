"""The physical sky's rule (include/pt_amd.h, "the physical sky") restated in numpy from the printed formulas. Reads nothing of the
product: libm's functions, numpy's order of operations. Directions are unit vectors, arrays of shape (..., 3)."""
import numpy as np

DEFAULTS = dict(sun_dir=(0.0, 1.0, 0.0), turbidity=3.0, ground_albedo=(0.3, 0.3, 0.3), sun_radius_deg=0.2665, sun_scale=1.0, scale=0.04)

COEF = {   # (a, b) of A..E = a T + b
    "Y": ((0.1787, -1.4630), (-0.3554, 0.4275), (-0.0227, 5.3251), (0.1206, -2.5771), (-0.0670, 0.3703)),
    "x": ((-0.0193, -0.2592), (-0.0665, 0.0008), (-0.0004, 0.2125), (-0.0641, -0.8989), (-0.0033, 0.0452)),
    "y": ((-0.0167, -0.2608), (-0.0950, 0.0092), (-0.0079, 0.2102), (-0.0441, -1.6537), (-0.0109, 0.0529)),
}
MX = np.array([[0.00166, -0.00375, 0.00209, 0.0], [-0.02903, 0.06377, -0.03202, 0.00394], [0.11693, -0.21196, 0.06052, 0.25886]])
MY = np.array([[0.00275, -0.00610, 0.00317, 0.0], [-0.04214, 0.08970, -0.04153, 0.00516], [0.15346, -0.26756, 0.06670, 0.26688]])
XYZ_TO_RGB = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]])
LAMBDA = np.array([0.610, 0.550, 0.465])


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    if np.ndim(o["ground_albedo"]) == 0:
        o["ground_albedo"] = (o["ground_albedo"],) * 3
    return o


def sun_unit(o):
    s = np.asarray(o["sun_dir"], dtype=np.float64)
    return s / np.linalg.norm(s)


def perez(T, which, cos_theta, gamma):
    A, B, C, D, E = (a * T + b for a, b in COEF[which])
    return (1.0 + A * np.exp(B / cos_theta)) * (1.0 + C * np.exp(D * gamma) + E * np.cos(gamma) ** 2)


def zenith(T, theta_s):
    chi = (4.0 / 9.0 - T / 120.0) * (np.pi - 2.0 * theta_s)
    Yz = (4.0453 * T - 4.9710) * np.tan(chi) - 0.2155 * T + 2.4192
    tv = np.array([T * T, T, 1.0])
    th = np.array([theta_s ** 3, theta_s ** 2, theta_s, 1.0])
    return Yz, tv @ MX @ th, tv @ MY @ th


def sky_unscaled(o, d):
    """The sky's linear sRGB before `scale`, for directions with d.y > 0 (others: garbage, mask them)."""
    d = np.asarray(d, dtype=np.float64)
    T = float(o["turbidity"])
    s = sun_unit(o)
    theta_s = np.arccos(np.clip(s[1], 0.0, 1.0))
    with np.errstate(all="ignore"):
        cos_t = np.where(d[..., 1] > 0.0, d[..., 1], 1.0)
        gamma = np.arccos(np.clip(d @ s, -1.0, 1.0))
        zen = zenith(T, theta_s)
        Y, x, y = (z * perez(T, k, cos_t, gamma) / perez(T, k, 1.0, theta_s) for z, k in zip(zen, "Yxy"))
        XYZ = np.stack([(x / y) * Y, Y, ((1.0 - x - y) / y) * Y], axis=-1)
    return np.maximum(XYZ @ XYZ_TO_RGB.T, 0.0)


def sun_irradiance_unscaled(o):
    """E_sun (klx) before sun_scale and scale."""
    s = sun_unit(o)
    if not s[1] > 0.0:
        return np.zeros(3)
    T = float(o["turbidity"])
    theta_s = np.arccos(min(s[1], 1.0))
    m = 1.0 / (s[1] + 0.15 * (93.885 - theta_s * 180.0 / np.pi) ** -1.253)
    beta = 0.04608 * T - 0.04586
    tau = 0.008735 * LAMBDA ** -4.08 + beta * LAMBDA ** -1.3
    return 127.5 * np.exp(-(tau * m))


def sun_irradiance(o):
    return o["scale"] * o["sun_scale"] * sun_irradiance_unscaled(o)


def sky_irradiance_unscaled(o, na=16, nb=64):
    """E_sky: the midpoint quadrature of the unscaled sky over the upper hemisphere, na x nb cells."""
    a = np.arange(na, dtype=np.float64)
    b = np.arange(nb, dtype=np.float64)
    theta = ((a + 0.5) * (np.pi / 2.0)) / na
    phi = -np.pi + ((2.0 * np.pi) * (b + 0.5)) / nb
    w = np.cos(theta) * (np.cos((a * (np.pi / 2.0)) / na) - np.cos(((a + 1.0) * (np.pi / 2.0)) / na)) * ((2.0 * np.pi) / nb)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    d = np.stack([st * np.cos(phi)[None, :], ct + 0.0 * phi[None, :], st * np.sin(phi)[None, :]], axis=-1)
    return (sky_unscaled(o, d) * w[:, None, None]).sum(axis=(0, 1))


def ground(o):
    s = sun_unit(o)
    e = sky_irradiance_unscaled(o) + o["sun_scale"] * sun_irradiance_unscaled(o) * max(0.0, s[1])
    return o["scale"] * np.asarray(o["ground_albedo"], dtype=np.float64) * e / np.pi


def sky_eval(o, d):
    """pt_sky_eval: the sky above, the ground below, no disc."""
    d = np.asarray(d, dtype=np.float64)
    up = d[..., 1] > 0.0
    return np.where(up[..., None], o["scale"] * sky_unscaled(o, d), ground(o))


def texel_dirs(W, H, sub=1):
    """Directions of the sub x sub sub-cells' midpoints of every texel: (H, W, sub, sub, 3); sub = 1: the texel centres."""
    j = np.arange(H, dtype=np.float64)[:, None, None, None]
    i = np.arange(W, dtype=np.float64)[None, :, None, None]
    a = ((np.arange(sub, dtype=np.float64) + 0.5) / sub)[None, None, :, None]
    b = ((np.arange(sub, dtype=np.float64) + 0.5) / sub)[None, None, None, :]
    theta = ((j + a) * np.pi) / H + 0.0 * b + 0.0 * i
    phi = -np.pi + ((2.0 * np.pi) * (i + b)) / W + 0.0 * a + 0.0 * j
    return np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)


def solid_angles(W, H):
    """w_ij, (H, W)."""
    j = np.arange(H, dtype=np.float64)
    row = (np.cos((j * np.pi) / H) - np.cos(((j + 1.0) * np.pi) / H)) * ((2.0 * np.pi) / W)
    return np.repeat(row[:, None], W, axis=1)


def texel_of(W, H, d):
    """(i, j) of the texel sample_environment reads for direction d."""
    theta = np.arccos(np.clip(d[1], -1.0, 1.0))
    phi = np.arctan2(d[2], d[0])
    u = np.clip((phi + np.pi) / (2.0 * np.pi), 0.0, 1.0)
    v = 1.0 - np.clip(1.0 - theta / np.pi, 0.0, 1.0)
    return min(int(u * W), W - 1), min(int(v * H), H - 1)


def disc_counts(o, W, H):
    """n_ij (H, W) int: the sub-directions of each texel inside the disc; the fallback texel gets 64 when all are 0."""
    s = sun_unit(o)
    cos_a = np.cos((o["sun_radius_deg"] * np.pi) / 180.0)
    n = np.zeros((H, W), dtype=np.int64)
    rows = max(1, (1 << 18) // (W * 64))
    for j0 in range(0, H, rows):      # in slabs of rows: the (H, W, 8, 8, 3) array of a large map would not fit
        j1 = min(H, j0 + rows)
        jj = np.arange(j0, j1, dtype=np.float64)[:, None, None, None]
        i = np.arange(W, dtype=np.float64)[None, :, None, None]
        a = ((np.arange(8.0) + 0.5) / 8.0)[None, None, :, None]
        b = ((np.arange(8.0) + 0.5) / 8.0)[None, None, None, :]
        theta = ((jj + a) * np.pi) / H
        phi = -np.pi + ((2.0 * np.pi) * (i + b)) / W
        dot = (np.sin(theta) * np.cos(phi)) * s[0] + np.cos(theta) * s[1] + (np.sin(theta) * np.sin(phi)) * s[2]
        n[j0:j1] = (dot >= cos_a).sum(axis=(2, 3))
    if n.sum() == 0:
        i, j = texel_of(W, H, s)
        n[j, i] = 64
    return n


def bake(o, W, H):
    """pt_sky_bake in f64 (before the narrowing to f32): (H, W, 3), and n_ij."""
    base = sky_eval(o, texel_dirs(W, H)[:, :, 0, 0, :])
    irr = sun_irradiance(o)
    n = np.zeros((H, W), dtype=np.int64)
    if o["sun_scale"] > 0.0 and irr.max() > 0.0:
        n = disc_counts(o, W, H)
        omega = ((n.sum(axis=1) / 64.0) * solid_angles(W, H)[:, 0]).sum()
        base = base + (irr / omega)[None, None, :] * (n / 64.0)[:, :, None]
    return base, n
