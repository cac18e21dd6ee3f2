"""The participating-media rule (pt_mat_medium in include/pt_amd.h) restated in numpy, for the medium tests:
the Henyey-Greenstein sampler and phase function, the free-flight distance, a scalar replay of whole paths through scenes made
of media only, and the single-scattering quadrature of a quad light seen through an unbounded medium."""
import numpy as np

import sampler_rule as SR

PI = np.pi


# ---- the device functions -------------------------------------------------------------------------------------------------
def free_flight(u, density):
    return -np.log(1.0 - np.asarray(u, dtype=np.float64)) / density


def hg_cos(g, u1):
    """cos_t of the rule: the inverse of HG's CDF in cos_t (isotropic below |g| = 1e-3), clamped to [-1, 1]."""
    u1 = np.asarray(u1, dtype=np.float64)
    if abs(g) < 1e-3:
        c = 1.0 - 2.0 * u1
    else:
        q = (1.0 - g * g) / (1.0 - g + 2.0 * g * u1)
        c = (1.0 + g * g - q * q) / (2.0 * g)
    return np.clip(c, -1.0, 1.0)


def hg_phase(g, c):
    s = 1.0 + g * g - 2.0 * g * np.asarray(c, dtype=np.float64)
    return (1.0 - g * g) / (4.0 * PI * s * np.sqrt(s))


def hg_cdf(g, c):
    """The analytic CDF of cos_t under HG: F(c) = int_-1^c 2 pi ph(c') dc' = (1 - g^2) / (2 g) * (1 / sqrt(1 + g^2 - 2 g c) - 1 / (1 + g)),
    and (1 + c) / 2 in the isotropic limit. The rule's cos_t satisfies F(cos_t) = u1 (and 1 - u1 on the isotropic branch, which
    runs the other way)."""
    c = np.asarray(c, dtype=np.float64)
    if abs(g) < 1e-3:
        return (1.0 + c) / 2.0
    return (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * c) - 1.0 / (1.0 + g))


def cos_quadrature(panels=32, n=48):
    """Composite Gauss-Legendre nodes and weights on cos_t in [-1, 1] (HG with g = 0.9 is too peaked for one panel at 1e-12)."""
    x, w = np.polynomial.legendre.leggauss(n)
    edges = np.linspace(-1.0, 1.0, panels + 1)
    h = np.diff(edges) / 2.0
    return ((edges[:-1] + h)[:, None] + h[:, None] * x[None, :]).reshape(-1), (h[:, None] * w[None, :]).reshape(-1)


def hg_cos_moments(g):
    """(sum ph dOmega, E[cos_t], E[cos_t^2]) under 2 pi ph(c) dc by Gauss-Legendre."""
    x, w = cos_quadrature()
    p = 2.0 * PI * hg_phase(g, x)
    return float((w * p).sum()), float((w * p * x).sum()), float((w * p * x * x).sum())


def _quat_mul(q, v):
    """glam DQuat * DVec3 (pt_dev_math.h quat_mul); q = (x, y, z, w) arrays, v = (..., 3)."""
    b = np.stack([q[0], q[1], q[2]], axis=-1)
    w = q[3]
    b2 = (b * b).sum(axis=-1)
    return v * (w * w - b2)[..., None] + b * ((v * b).sum(axis=-1) * 2.0)[..., None] + np.cross(b, v) * (w * 2.0)[..., None]


def frame_to_z(n):
    """The shortest-arc quaternion taking n onto +z (vec3.rs:23-29)."""
    n = np.asarray(n, dtype=np.float64)
    qx, qy, qz, qw = n[..., 1], -n[..., 0], np.zeros_like(n[..., 0]), 1.0 + n[..., 2]
    flip = n[..., 2] < -0.99999
    r = 1.0 / np.where(flip, 1.0, np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw))
    return (np.where(flip, 1.0, qx * r), np.where(flip, 0.0, qy * r), np.where(flip, 0.0, qz * r), np.where(flip, 0.0, qw * r))


def hg_dir(g, u1, u2, axis):
    """The rule's new direction for draws (u1, u2) around the propagation direction `axis` ((n, 3) or (3,))."""
    c = hg_cos(g, u1)
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    phi = 2.0 * PI * np.asarray(u2, dtype=np.float64)
    local = np.stack([s * np.cos(phi), s * np.sin(phi), c], axis=-1)
    q = frame_to_z(np.broadcast_to(np.asarray(axis, dtype=np.float64), local.shape))
    return _quat_mul((-q[0], -q[1], -q[2], q[3]), local)


# ---- geometry of the replay scenes: spheres, axis-aligned boxes, rigidly placed triangle meshes --------------------------------
T_MIN = 1e-3


def _hit_sphere(o, d, c, r):
    l = c - o
    sd, l2, r2 = l @ d, l @ l, r * r
    if sd < 0.0 and l2 > r2:
        return None
    d2 = l2 - sd * sd
    if d2 > r2:
        return None
    q = np.sqrt(r2 - d2)
    t = sd - q if l2 > r2 else sd + q
    if t <= T_MIN or not np.isfinite(t):
        return None
    p = o + d * t
    return t, p, (p - c) / np.linalg.norm(p - c)


def _hit_box(o, d, lo, hi):
    """Closest face hit of the six quads of a cuboid, t >= T_MIN (quad.rs:40-59 on each face)."""
    best = None
    for a in range(3):
        if abs(d[a]) < 1e-8:
            continue
        for plane, sign in ((lo[a], -1.0), (hi[a], 1.0)):
            t = (plane - o[a]) / d[a]
            if not (t >= T_MIN) or (best is not None and t >= best[0]):
                continue
            p = o + d * t
            b, c = (a + 1) % 3, (a + 2) % 3
            if lo[b] <= p[b] <= hi[b] and lo[c] <= p[c] <= hi[c]:
                n = np.zeros(3)
                n[a] = sign
                best = (t, p, n)
    return best


def _hit_tris(o, d, v0, e1, e2):
    """Moeller-Trumbore over all triangles (mesh.rs:50-82), closest with t >= T_MIN; returns (t, point, unit normal)."""
    h = np.cross(d, e2)
    a = (e1 * h).sum(axis=1)
    ok = np.abs(a) >= 1e-8
    f = 1.0 / np.where(ok, a, 1.0)
    s = o - v0
    u = f * (s * h).sum(axis=1)
    q = np.cross(s, e1)
    v = f * (q @ d)
    t = f * (e2 * q).sum(axis=1)
    ok &= (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= T_MIN)
    if not ok.any():
        return None
    t = np.where(ok, t, np.inf)
    i = int(np.argmin(t))
    n = np.cross(e1[i], e2[i])
    return float(t[i]), o + d * t[i], n / np.linalg.norm(n)


def rigid(axis, angle, translation):
    """Instance::new's matrix (DQuat::from_axis_angle, rotate then translate): returns (R, t)."""
    ax = np.asarray(axis, dtype=np.float64)
    s, c = np.sin(angle * 0.5), np.cos(angle * 0.5)
    x, y, z, w = ax[0] * s, ax[1] * s, ax[2] * s, c
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, np.asarray(translation, dtype=np.float64)


class Media:
    """A scene of media only. add_*: boundary objects with a medium (density, albedo (3,), g); index = order of addition."""

    def __init__(self):
        self.objs, self.media = [], []

    def _medium(self, density, albedo, g):
        self.media.append((float(density), np.asarray(albedo, dtype=np.float64), float(g)))
        return len(self.media) - 1

    def add_sphere(self, c, r, density, albedo, g):
        self.objs.append(("sphere", np.asarray(c, dtype=np.float64), float(r), self._medium(density, albedo, g)))

    def add_box(self, lo, hi, density, albedo, g):
        self.objs.append(("box", np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), self._medium(density, albedo, g)))

    def add_mesh(self, scale, P, I, axis, angle, translation, density, albedo, g):
        R, t = rigid(axis, angle, translation)
        V = (np.asarray(P, dtype=np.float32).astype(np.float64) * scale) @ R.T + t
        F = np.asarray(I, dtype=np.int64).reshape(-1, 3)
        v0 = V[F[:, 0]]
        self.objs.append(("mesh", v0, V[F[:, 1]] - v0, V[F[:, 2]] - v0, self._medium(density, albedo, g)))

    def closest(self, o, d):
        best = None
        for ob in self.objs:
            if ob[0] == "sphere":
                h = _hit_sphere(o, d, ob[1], ob[2])
            elif ob[0] == "box":
                h = _hit_box(o, d, ob[1], ob[2])
            else:
                h = _hit_tris(o, d, ob[1], ob[2], ob[3])
            if h is not None and (best is None or h[0] < best[0]):
                best = (h[0], h[1], h[2], ob[-1])
        return best


def luminance(c):
    return 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]


def replay_path(media, frame, cam, seed, pixel, sample, env, camera_medium=None, sobol=False, perturb=None):
    """The radiance (3,) of sample `sample` of `pixel` by the rule, in scalar numpy. frame: refs_numpy.camera_frame's dict; cam:
    dict with width, blur_strength, max_depth (pinhole: defocus_angle 0, nothing moves). No lights, constant environment `env`.
    perturb: None, or a function x -> x applied to every unit draw and hit distance (the 1-ulp robustness check)."""
    f64 = SR.sobol_u64 if sobol else SR.independent_u64
    nudge = perturb if perturb is not None else (lambda x: x)

    def U(d):
        return nudge(float(SR.unit(f64(seed, pixel, sample, d))))

    ly, lx = SR.camera_locations(frame, cam["blur_strength"], cam["width"], seed, [pixel], [sample], sobol=sobol)
    loc = frame["pixel00"] + frame["dv"] * ly[0, 0] + frame["du"] * lx[0, 0]
    o = np.asarray(frame["center"], dtype=np.float64)
    d = loc - o
    d = d / np.linalg.norm(d)
    draw = 5                       # pixel offsets (2), lens offsets (2, made and not used), time (1): the same count under both samplers
    m, bounce, thr = camera_medium, 0, np.ones(3)
    env = np.asarray(env, dtype=np.float64)
    while True:
        hit = media.closest(o, d)
        t = nudge(hit[0]) if hit is not None else np.inf
        if m is not None and hit is None:
            m = None               # every medium of these scenes bounds an object: a ray that left the scene is not inside one
        if m is not None:
            dens, alb, g = media.media[m]
            dist = free_flight(U(draw), dens)
            draw += 1
            if dist < t:
                x = o + d * dist
                if bounce > 5:
                    p = min(max(luminance(thr), 0.01), 1.0)
                    r = U(draw)
                    draw += 1
                    if r > p:
                        return np.zeros(3)
                    thr = thr / p
                draw += 1          # the selector: drawn, never below p_light = 0
                if sobol:
                    draw = (draw + 1) & ~1
                u1, u2 = U(draw), U(draw + 1)
                draw += 2
                w = hg_dir(g, u1, u2, d)
                ph = hg_phase(g, d @ w)
                pdf = ph
                if not (pdf > 0.0) or not np.isfinite(pdf):
                    return np.zeros(3)
                thr = thr * (alb * ph / pdf)
                o, d = x, w / np.linalg.norm(w)
                bounce += 1
                if bounce >= cam["max_depth"]:
                    return np.zeros(3)
                continue
        if hit is None:
            return thr * env
        _, p, n, k = hit
        m = None if m == k else k
        o = p + (1e-3 if d @ n >= 0.0 else -1e-3) * n
        bounce += 1
        if bounce >= cam["max_depth"]:
            return np.zeros(3)


# ---- single scattering of a quad light through an unbounded medium, by quadrature ----------------------------------------
def single_scatter_quad(origins, dirs, density, g, quad, n_v, n_a):
    """For rays (origins, dirs) that do NOT hit the quad: the scalar S with radiance = albedo * emission * S per channel,
       S = int_0^inf density e^(-density d) int_quad ph(dir . w) e^(-density r) |n . w| / r^2 dA dd,   x = o + d dir, w = (y - x) / r,
    with d = -log(1 - v) / density (the free-flight density becomes dv on [0, 1)): Gauss-Legendre, n_v nodes in v, n_a x n_a on the quad."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in quad)
    nrm = np.cross(u, v)
    area = np.linalg.norm(nrm)
    nrm = nrm / area
    gx, gw = np.polynomial.legendre.leggauss(n_v)
    vv, wv = 0.5 * (gx + 1.0), 0.5 * gw
    ax, aw = np.polynomial.legendre.leggauss(n_a)
    aa, wa = 0.5 * (ax + 1.0), 0.5 * aw
    Y = (q + aa[:, None, None] * u + aa[None, :, None] * v).reshape(-1, 3)                      # (A, 3)
    WY = (wa[:, None] * wa[None, :]).reshape(-1) * area
    dist = -np.log(1.0 - vv) / density                                                           # (V,)
    out = np.zeros(len(origins))
    for i, (o, d) in enumerate(zip(np.asarray(origins, dtype=np.float64), np.asarray(dirs, dtype=np.float64))):
        X = o + dist[:, None] * d                                                                # (V, 3)
        R = Y[None, :, :] - X[:, None, :]                                                        # (V, A, 3)
        r = np.linalg.norm(R, axis=2)
        W = R / r[..., None]
        f = hg_phase(g, W @ d) * np.exp(-density * r) * np.abs(W @ nrm) / (r * r)
        out[i] = (wv[:, None] * WY[None, :] * f).sum()
    return out
