"""Punctual lights (pt_light_point / pt_light_spot / pt_light_directional) restated in numpy from the rule in include/pt_amd.h: what a
light sends to a point, the selector's branch, the SHADOW segment and its resolution, Lambert's eval, and an independent ray / quad test
for occlusion. f64, one rounding per written operation. Nothing here reads the product."""
from __future__ import annotations

import math

import numpy as np

import light_rule as LR

PI = math.pi
MASK64 = (1 << 64) - 1


def dot(a, b):
    return (a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1]) + (a[..., 2] * b[..., 2])


def unit(v):
    """rand Standard f64 of a 64-bit draw"""
    return (np.asarray(v, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def index_of_draws(v, n):
    """gen_range(0..n) from the single draws v[0], v[1], ...: (index, draws consumed) — widening multiply, rejection above the zone"""
    zone = ((n << (64 - n.bit_length())) - 1) & MASK64
    for used, x in enumerate(v, 1):
        m = int(x) * n
        if (m & MASK64) <= zone:
            return m >> 64, used
    return 0, len(v)


# ---- the records ---------------------------------------------------------------------------------------------------------------------
def record(rec16):
    r = np.asarray(rec16, dtype=np.float64)
    return dict(kind=int(r[0]), pos=r[1:4].copy(), axis=r[4:7].copy(), I=r[7:10].copy(), cos_i=float(r[10]), cos_o=float(r[11]))


def point_intensity(power):
    return np.asarray(power, dtype=np.float64) / (4.0 * PI)


def light_eval(rec, x):
    """(w, D, d2, E) for points x (m, 3): the light evaluation of the punctual branch. rec: record() of the STORED numbers."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    m = len(x)
    if rec["kind"] == 2:
        return (np.broadcast_to(-rec["axis"], (m, 3)).copy(), np.full(m, np.inf), np.ones(m), np.broadcast_to(rec["I"], (m, 3)).copy())
    with np.errstate(divide="ignore", invalid="ignore"):
        L = rec["pos"][None, :] - x
        d2 = dot(L, L)
        D = np.sqrt(d2)
        w = L / D[:, None]
        if rec["kind"] == 1:
            c = -dot(w, rec["axis"][None, :])
            ci, co = rec["cos_i"], rec["cos_o"]
            if ci > co:
                s = (c - co) / (ci - co)
                s = np.where(s < 0.0, 0.0, s)
                s = np.where(s > 1.0, 1.0, s)
            else:
                s = np.where(c >= co, 1.0, 0.0)
            fall = (s * s) * (3.0 - 2.0 * s)
            E = (rec["I"][None, :] * fall[:, None]) / d2[:, None]
        else:
            E = rec["I"][None, :] / d2[:, None]
    return w, D, d2, E


def eval7(rec, x):
    """pt_punctual_eval's seven numbers per point: w.xyz, D, E.rgb"""
    w, D, _, E = light_eval(rec, x)
    return np.concatenate([w, D[:, None], E], axis=1)


# ---- the branch --------------------------------------------------------------------------------------------------------------------------
def probabilities(f, lights):
    p_punct = f
    p_light = (1.0 - f) / 2.0 if lights else 0.0
    p_bsdf = 1.0 - p_light - p_punct
    return p_light, p_punct, p_bsdf


def branch_of(r, f, lights):
    """0 lights.sample, 1 the punctual branch, 2 mat.sample — for selector draws r"""
    p_light, p_punct, _ = probabilities(f, lights)
    r = np.asarray(r, dtype=np.float64)
    return np.where(r < p_light, 0, np.where(r < p_light + p_punct, 1, 2))


def lambert_eval(albedo, sn, w):
    """diffuse eval(wo, w) with its cosine: |l.z| * (a / pi), l = w in the frame of the shading normal sn"""
    sn = np.broadcast_to(np.asarray(sn, dtype=np.float64), w.shape)
    lz = LR.quat_mul(LR.frame_to_z(sn), w)[..., 2]
    return np.abs(lz)[..., None] * (np.asarray(albedo, dtype=np.float64) / PI)[None, :]


def branch_throughput(thr, e, E, f, n):
    """thr' = ((thr * e) * E) / pm with pm = f / n"""
    pm = f / float(n)
    return ((thr * e) * E) / pm


def branch_ends(d2, thr2):
    return (d2 == 0.0) | ~np.isfinite(d2) | np.all(thr2 == 0.0, axis=-1)


def signum(x):
    return np.where(np.signbit(x), -1.0, 1.0)


def shadow_origin(point, gn, w):
    """the offset of every continued ray: point + (1e-3 * signum(dot(w, gn))) * gn"""
    gn = np.broadcast_to(np.asarray(gn, dtype=np.float64), w.shape)
    return point + (1e-3 * signum(dot(w, gn)))[..., None] * gn


def shadow_distance(rec, o):
    """D' of the resolution: length(pos - o), +inf for a directional light"""
    if rec["kind"] == 2:
        return np.full(len(o), np.inf)
    L = rec["pos"][None, :] - o
    return np.sqrt(dot(L, L))


def visible(t_hit, d_light):
    """the light is visible iff the ray missed (t_hit = +inf) or hit.dist >= D'"""
    return t_hit >= d_light


# ---- an independent ray / quad test ---------------------------------------------------------------------------------------------------------
def ray_quad(o, d, q, u, v, t_min=1e-3):
    """(t, margin) of rays (o, d) against the quad q + a u + b v, 0 <= a, b <= 1: t = +inf on a miss; margin = the distance of (a, b) to the
    nearest edge of the unit square, in the quad's parameters (+inf for rays that do not reach the plane)."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in (q, u, v))
    n = np.cross(u, v)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((q - o) @ n) / (d @ n)
    ok = np.isfinite(t) & (t > t_min)
    p = o + d * np.where(ok, t, 0.0)[:, None] - q
    a = (p @ u) / (u @ u)                              # (u and v are orthogonal in every scene of these tests)
    b = (p @ v) / (v @ v)
    margin = np.where(ok, np.minimum(np.minimum(np.abs(a), np.abs(a - 1.0)), np.minimum(np.abs(b), np.abs(b - 1.0))), np.inf)
    inside = ok & (a >= 0.0) & (a <= 1.0) & (b >= 0.0) & (b <= 1.0)
    return np.where(inside, t, np.inf), margin


def first_hit(o, d, quads):
    """closest t over the quads (+inf: none), and the smallest edge margin over them"""
    t = np.full(len(o), np.inf)
    margin = np.full(len(o), np.inf)
    for q, u, v in quads:
        tq, mq = ray_quad(o, d, q, u, v)
        t = np.minimum(t, tq)
        margin = np.minimum(margin, mq)
    return t, margin
