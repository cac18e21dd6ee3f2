"""The interior-media rule (pt_mat_glass_set_interior / pt_mat_medium_tinted in include/pt_amd.h) restated in numpy,
for the interior tests: the closed forms of a glass slab with an interior, a vectorised Monte Carlo of the rule's state machine on
that slab with ideal Fresnel interfaces, and a scalar replay of whole paths through a rough glass sphere with a scattering interior
(the glass sampler is written from the reference's glass.rs:66-90 and bsdf/sampling.rs:57-94; refs_numpy.glass_pdf_eval has pdf and
eval)."""
import math

import numpy as np

import medium_rule as MR
import refs_numpy as R
import sampler_rule as SR

T_OFFSET = 1e-3          # the offset of every continued ray (camera.rs:217-222)


# ---- the slab: closed forms ---------------------------------------------------------------------------------------------------
def slab_angles(cos_i, ior):
    """For a ray that meets a flat interface at cos_i from outside: (R, cos_t) with R the Fresnel reflectance (glass.rs:51-62) —
    the same at every later internal hit, by symmetry — and cos_t the cosine of the refracted ray."""
    cos_i = np.asarray(cos_i, dtype=np.float64)
    sin_i = np.sqrt(np.maximum(0.0, 1.0 - cos_i * cos_i))
    Rf = np.array([R.dielectric_fresnel((s, 0.0, c), (0.0, 0.0, 1.0), 1.0, ior) for s, c in zip(sin_i.reshape(-1), cos_i.reshape(-1))]).reshape(cos_i.shape)
    cos_t = np.sqrt(1.0 - (sin_i / ior) ** 2)
    return Rf, cos_t


def traverse_length(thickness, cos_t):
    """One traversal of the slab by the rule: from the OFFSET point — after entry and after every internal reflection — to the far face."""
    return (thickness - T_OFFSET) / cos_t


def slab_mean(Rf, x):
    """E[sample] / E_env when each traversal multiplies the sample by x (or survives with probability x): the path leaves after k
    traversals with probability (1 - R)^2 R^(k-1), or is reflected at once with probability R."""
    return Rf + (1.0 - Rf) ** 2 * x / (1.0 - Rf * x)


def slab_second_moment(Rf, x):
    """E[sample^2] / E_env^2 for a deterministic factor x per traversal."""
    return Rf + (1.0 - Rf) ** 2 * x * x / (1.0 - Rf * x * x)


def slab_mean_medium_dropped(Rf, x):
    """What the common mistake gives — the medium dropped at an internal reflection, so only the first traversal attenuates."""
    return Rf + (1.0 - Rf) * x


# ---- the slab: a Monte Carlo of the rule ------------------------------------------------------------------------------------
def slab_walk(rng, n, Rf, length, density, absorption, keep_medium=True, max_events=10000):
    """n samples of the rule on a slab seen under one angle: ideal Fresnel interfaces of reflectance Rf, a traversal of `length` per
    crossing of the body, interior = a medium of `density` with albedo 0 (a collision ends the sample's contribution) and absorption
    coefficients `absorption` (3,). Returns the samples' throughput (n, 3) on leaving (environment 1).
    The state is the rule's: m is set by a crossing at a front-face hit, cleared by a crossing at a back-face hit, kept by a
    reflection (keep_medium=False: dropped by an internal reflection, the mistake the tests must catch)."""
    a = np.asarray(absorption, dtype=np.float64)
    thr = np.ones((n, 3))
    inside = rng.random(n) >= Rf                     # the first hit: front face; reflection leaves at once, m none
    m = inside.copy()                                # crossing at a front face: m = k
    for _ in range(max_events):
        idx = np.flatnonzero(inside)
        if idx.size == 0:
            break
        med = m[idx]
        # step 1 with m set: free flight (no draw when density == 0), then absorption over the segment travelled
        if density > 0.0:
            d = np.where(med, -np.log(1.0 - rng.random(idx.size)) / density, np.inf)
        else:
            d = np.full(idx.size, np.inf)
        collided = d < length
        seg = np.where(collided, d, length)
        att = np.where((a > 0.0)[None, :], np.exp(-(a[None, :] * seg[:, None])), 1.0)
        thr[idx] = np.where(med[:, None], thr[idx] * att, thr[idx])
        thr[idx[collided]] = 0.0                     # albedo 0
        inside[idx[collided]] = False
        idx = idx[~collided]
        # the back-face hit: internal reflection keeps m, a crossing clears it and the path leaves
        refl = rng.random(idx.size) < Rf
        if not keep_medium:
            m[idx[refl]] = False
        out = idx[~refl]
        m[out] = False
        inside[out] = False
    return thr


# ---- the replay: a rough glass sphere with a scattering interior ------------------------------------------------------------------
def _norm(v):
    return v * (1.0 / math.sqrt(float(v @ v)))       # glam: v * length_recip


def to_local(q, w):
    return MR._quat_mul(q, np.asarray(w, dtype=np.float64))


def to_world(q, w):
    return MR._quat_mul((-q[0], -q[1], -q[2], q[3]), np.asarray(w, dtype=np.float64))


def ggx_sample_microfacet_normal(v, roughness, e1, e2):
    """sampling.rs:57-94: a visible normal of GGX with alpha = roughness^2 for the local view vector v."""
    a2 = roughness * roughness
    vv = _norm(np.array([v[0] * a2, v[1] * a2, v[2]]))
    t1 = _norm(np.cross(vv, np.array([0.0, 0.0, 1.0]))) if vv[2] < 0.9999 else np.array([1.0, 0.0, 0.0])
    t2 = np.cross(t1, vv)
    a = 1.0 / (1.0 + vv[2])
    r = math.sqrt(e1)
    phi = e2 / a * math.pi if e2 < a else math.pi + (e2 - a) / (1.0 - a) * math.pi
    p1 = r * math.cos(phi)
    p2 = r * math.sin(phi) * (1.0 if e2 < a else vv[2])
    n = p1 * t1 + p2 * t2 + math.sqrt(max(1.0 - p1 * p1 - p2 * p2, 0.0)) * vv
    h = _norm(np.array([a2 * n[0], a2 * n[1], max(n[2], 0.0)]))
    return -h if h[2] < 0.0 else h


def reflect(i, n):
    return i - n * (2.0 * float(i @ n))


def refract(i, n, eta):
    ndi = float(n @ i)
    k = 1.0 - eta * eta * (1.0 - ndi * ndi)
    if k >= 0.0:
        return eta * i - (eta * ndi + math.sqrt(k)) * n
    return np.zeros(3)


def sample_dielectric(v, h, eta_i, eta_o, u):
    """glass.rs:79-89: reflect below the Fresnel reflectance, else refract (total internal reflection reflects)."""
    f = R.dielectric_fresnel(v, h, eta_i, eta_o)
    if u < f:
        return reflect(-v, h)
    t = refract(-v, h, eta_i / eta_o)
    if not t.any():
        t = reflect(-v, h)
    return t


def replay_glass_path(center, radius, roughness, ior, interior, frame, cam, seed, pixel, sample, env, sobol=False):
    """The radiance (3,) of sample `sample` of `pixel` by the rule, in scalar numpy: one glass sphere whose interior is the medium
    (density, albedo (3,), g), no absorption, no lights, constant environment. Returns (radiance, events) with events a dict of
    counts (crossings in / out, internal reflections, medium vertices)."""
    f64 = SR.sobol_u64 if sobol else SR.independent_u64

    def U(d):
        return float(SR.unit(f64(seed, pixel, sample, d)))

    ly, lx = SR.camera_locations(frame, cam["blur_strength"], cam["width"], seed, [pixel], [sample], sobol=sobol)
    loc = frame["pixel00"] + frame["dv"] * ly[0, 0] + frame["du"] * lx[0, 0]
    o = np.asarray(frame["center"], dtype=np.float64)
    d = _norm(loc - o)
    draw = 5                       # pixel offsets (2), lens offsets (2), time (1)
    dens, alb, g = interior
    alb = np.asarray(alb, dtype=np.float64)
    c = np.asarray(center, dtype=np.float64)
    inside, bounce, thr = False, 0, np.ones(3)
    env = np.asarray(env, dtype=np.float64)
    ev = dict(entered=0, left=0, internal=0, vertices=0)

    def roulette():
        nonlocal draw, thr
        if bounce > 5:
            p = min(max(MR.luminance(thr), 0.01), 1.0)
            r = U(draw)
            draw += 1
            if r > p:
                return False
            thr = thr / p
        return True

    while True:
        hit = MR._hit_sphere(o, d, c, radius)
        t = hit[0] if hit is not None else np.inf
        if inside and hit is None:
            inside = False         # the interior is bounded: a ray that left the scene is not in it
        if inside:
            dist = MR.free_flight(U(draw), dens)
            draw += 1
            if dist < t:
                ev["vertices"] += 1
                x = o + d * dist
                if not roulette():
                    return np.zeros(3), ev
                draw += 1          # the selector
                if sobol:
                    draw = (draw + 1) & ~1
                u1, u2 = U(draw), U(draw + 1)
                draw += 2
                w = MR.hg_dir(g, u1, u2, d)
                ph = MR.hg_phase(g, d @ w)
                if not (ph > 0.0) or not np.isfinite(ph):
                    return np.zeros(3), ev
                thr = thr * (alb * ph / ph)
                o, d = x, _norm(w)
                bounce += 1
                if bounce >= cam["max_depth"]:
                    return np.zeros(3), ev
                continue
        if hit is None:
            return thr * env, ev
        _, p, n = hit
        front = float(d @ n) < 0.0
        gn = n if front else -n
        if not roulette():
            return np.zeros(3), ev
        draw += 1                  # the selector: drawn, never below p_light = 0
        q = MR.frame_to_z(gn)
        v = to_local(q, -d)
        if sobol:
            draw = (draw + 1) & ~1
        e1, e2 = U(draw), U(draw + 1)
        draw += 2
        h = ggx_sample_microfacet_normal(v, roughness, e1, e2)
        eta_i, eta_o = (1.0, ior) if front else (ior, 1.0)
        uf = U(draw)
        draw += 1
        wi = to_world(q, sample_dielectric(v, h, eta_i, eta_o, uf))
        pdf, brdf = R.glass_pdf_eval(roughness, ior, v, to_local(q, wi), front)
        thr = thr * (brdf / pdf)
        side = float(wi @ gn)
        crossed = bool(np.signbit(side)) == bool(np.signbit(float(d @ gn)))
        if crossed:
            ev["entered" if front else "left"] += 1
            inside = front
        elif not front:
            ev["internal"] += 1
        o = p + (-T_OFFSET if np.signbit(side) else T_OFFSET) * gn
        d = _norm(wi)
        bounce += 1
        if bounce >= cam["max_depth"]:
            return np.zeros(3), ev
