"""Exact light sampling (pt_scene_set_light_sampling kind 1) restated in numpy from the rule in include/pt_amd.h: the area table, the
mesh and sphere samplers, brute-force all-triangle pdfs, the light-index draw, an irregular tessellation helper, the fixed-seed ray
sets of the GPU probe test and a scalar replay of the two-light MIS scene. Nothing here reads the product."""
from __future__ import annotations

import functools
import math

import numpy as np

import refs_numpy as R
import sampler_rule as SR
from common import MIS_ALBEDO, MIS_CAM, MIS_EMISSION, MIS_QUAD2, MIS_TRI, MIS_TRI_EMISSION, icosphere

PI = math.pi
MASK64 = (1 << 64) - 1


# ---- vectors, rigid placements ---------------------------------------------------------------------------------------------------
def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def normalize(v):
    return v * (1.0 / np.sqrt(dot(v, v)))[..., None]          # glam: v * length_recip


def rigid(axis, angle, translation):
    """Instance::new's forward matrix (DQuat::from_axis_angle, rotate then translate): (M with columns c0 c1 c2, t)."""
    ax = np.asarray(axis, dtype=np.float64)
    sn, cs = math.sin(angle * 0.5), math.cos(angle * 0.5)
    qx, qy, qz, qw = ax[0] * sn, ax[1] * sn, ax[2] * sn, cs
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz, yy, yz, zz, wx, wy, wz = qx * x2, qx * y2, qx * z2, qy * y2, qy * z2, qz * z2, qw * x2, qw * y2, qw * z2
    M = np.array([[1.0 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1.0 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1.0 - (xx + yy)]])
    return M, np.asarray(translation, dtype=np.float64)


class Chain:
    """An instance chain, outermost first: world = M_0 (M_1 (... local) + t_1) + t_0."""

    def __init__(self, *placements):
        self.p = [rigid(*pl) for pl in placements]

    def point_to_local(self, x):
        for M, t in self.p:
            x = x @ M - (t @ M)                                # R^T x + (-(R^T t)), the analytic rigid inverse
        return x

    def vector_to_local(self, v):
        for M, _ in self.p:
            v = v @ M
        return v

    def vector_to_world(self, v):
        for M, _ in reversed(self.p):
            v = v @ M.T
        return v

    def point_to_world(self, x):
        for M, t in reversed(self.p):
            x = x @ M.T + t
        return x


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def mesh_tris(P, I, scale=1.0):
    """(n, 3, 3) f64 vertices of pt_mesh's faces: f32 positions widened, times scale."""
    P = np.asarray(P, dtype=np.float32).reshape(-1, 3).astype(np.float64) * scale
    return P[np.asarray(I, dtype=np.int64).reshape(-1, 3)]


def tessellate_quad(q, u, v, n=8):
    """An irregular tessellation of the quad q + a u + b v: n x n cells whose edges sit at (i / n)^2, two triangles a cell
    (areas differ by more than 10x). Returns (f32 positions, u32 indices)."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in (q, u, v))
    s = (np.arange(n + 1) / n) ** 2
    P = np.array([q + u * s[i] + v * s[j] for j in range(n + 1) for i in range(n + 1)], dtype=np.float32)
    I = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i
            I += [a, b, c, a, c, d]
    return P, np.array(I, dtype=np.uint32)


def tessellate_box(lo, hi, n=4):
    """The closed surface of the box [lo, hi], every face tessellated n x n x 2 like tessellate_quad."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d = hi - lo
    ex, ey, ez = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    faces = [(lo, ex, ey), (lo, ey, ez), (lo, ez, ex), (hi, -ey, -ex), (hi, -ez, -ey), (hi, -ex, -ez)]
    Ps, Is, base = [], [], 0
    for q, u, v in faces:
        P, I = tessellate_quad(q, u, v, n)
        Ps.append(P)
        Is.append(I + base)
        base += len(P)
    return np.concatenate(Ps), np.concatenate(Is).astype(np.uint32)


def area_table(tris):
    """C[0] = 0, C[i + 1] = C[i] + A_i in face order, A_i = 0.5 |cross(v1 - v0, v2 - v0)|."""
    c = cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    a = 0.5 * np.sqrt(dot(c, c))
    C = np.zeros(len(tris) + 1)
    acc = 0.0
    for i, x in enumerate(a):                                   # summed in order
        acc = acc + x
        C[i + 1] = acc
    return C


# ---- draws -------------------------------------------------------------------------------------------------------------------------
class Draws:
    """The draws of (seed, pixel, sample) for arrays of pixels / samples, with a per-row draw counter."""

    def __init__(self, seed, pixels, samples, sobol=False, draw=0):
        self.seed, self.sobol = seed, sobol
        self.pixels = np.atleast_1d(np.asarray(pixels, dtype=np.uint64))
        self.samples = np.broadcast_to(np.asarray(samples, dtype=np.uint64), self.pixels.shape)
        self.draw = np.full(self.pixels.shape, draw, dtype=np.uint64)

    def u64_at(self, d):
        f = SR.sobol_u64 if self.sobol else SR.independent_u64
        return f(self.seed, self.pixels, self.samples, d)

    def single(self, active=None):
        """one single draw per (active) row: the 64-bit values"""
        v = self.u64_at(self.draw)
        self.draw = self.draw + (np.uint64(1) if active is None else active.astype(np.uint64))
        return v

    def unit(self, active=None):
        return SR.unit(self.single(active))

    def pair(self, active=None):
        """one two-value draw: pair-aligned under the Sobol sampler"""
        act = np.ones(self.draw.shape, bool) if active is None else active
        if self.sobol:
            self.draw = np.where(act, (self.draw + np.uint64(1)) & ~np.uint64(1), self.draw)
        a, b = SR.unit(self.u64_at(self.draw)), SR.unit(self.u64_at(self.draw + np.uint64(1)))
        self.draw = self.draw + np.uint64(2) * act.astype(np.uint64)
        return a, b

    def index(self, n, active=None):
        """gen_range(0..n): widening multiply with rejection above the zone (rand 0.8.5 UniformInt)"""
        zone = ((n << (64 - n.bit_length())) - 1) & MASK64
        pending = np.ones(self.draw.shape, bool) if active is None else active.copy()
        out = np.zeros(self.draw.shape, dtype=np.int64)
        for _ in range(64):
            if not pending.any():
                break
            v = self.single(pending)
            for i in np.nonzero(pending)[0]:
                m = int(v[i]) * n
                if (m & MASK64) <= zone:
                    out[i] = m >> 64
                    pending[i] = False
        return out


# ---- the samplers --------------------------------------------------------------------------------------------------------------------
def choose_face(C, u0):
    A = C[-1]
    x = u0 * A
    x = np.where(x >= A, np.nextafter(A, 0.0), x)
    return np.searchsorted(C[1:], x, side="right")             # the smallest j with x < C[j + 1]


def sample_mesh(C, tris, origin, u0, u1, u2):
    """kind 1, mesh entry: (face, unit direction) for local-space origins (m, 3)."""
    j = choose_face(C, u0)
    s = np.sqrt(u1)
    b0, b1, b2 = 1.0 - s, s * (1.0 - u2), s * u2
    t = tris[j]
    point = t[:, 0] * b0[:, None] + t[:, 1] * b1[:, None] + t[:, 2] * b2[:, None]
    return j, normalize(point - origin), point


def frame_to_z(n):
    """the shortest-arc quaternion taking n onto +z (vec3.rs:23-29), as (x, y, z, w) arrays"""
    qx, qy, qz, qw = n[..., 1], -n[..., 0], np.zeros_like(n[..., 0]), 1.0 + n[..., 2]
    flip = n[..., 2] < -0.99999
    r = 1.0 / np.where(flip, 1.0, np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw))
    return np.where(flip, 1.0, qx * r), np.where(flip, 0.0, qy * r), np.where(flip, 0.0, qz * r), np.where(flip, 0.0, qw * r)


def quat_mul(q, v):
    b = np.stack([q[0], q[1], q[2]], axis=-1)
    w = q[3]
    return v * (w * w - dot(b, b))[..., None] + b * (dot(v, b) * 2.0)[..., None] + cross(b, v) * (w * 2.0)[..., None]


def cone_k(r2, d2):
    x = r2 / d2
    return x / (1.0 + np.sqrt(1.0 - x))


def sample_sphere(center, radius, origin, u1, u2):
    """kind 1, sphere entry: unit directions for origins (m, 3)."""
    L = np.asarray(center, dtype=np.float64) - origin
    d2, r2 = dot(L, L), radius * radius
    inside = d2 <= r2
    k = cone_k(r2, np.where(inside, 2.0 * r2, d2))
    cos_t = np.where(inside, 1.0 - 2.0 * u1, 1.0 - u1 * k)
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    phi = 2.0 * PI * u2
    local = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], axis=-1)
    q = frame_to_z(normalize(L))
    return np.where(inside[:, None], local, quat_mul((-q[0], -q[1], -q[2], q[3]), local))


def pdf_sphere(center, radius, origin, direction):
    L = np.asarray(center, dtype=np.float64) - origin
    d = normalize(direction)
    l2, r2 = dot(L, L), radius * radius
    inside = l2 <= r2
    sd = dot(L, d)
    dd = l2 - sd * sd
    ok = ~((sd < 0.0) & (l2 > r2)) & (dd <= r2)                 # sphere.rs:64-87 with t_min = 0 for an origin outside: t = sd - q
    t = sd - np.sqrt(np.maximum(r2 - dd, 0.0))
    ok &= (t > 0.0) & np.isfinite(t)
    return np.where(inside, 1.0 / (4.0 * PI), np.where(ok, 1.0 / (2.0 * PI * cone_k(r2, np.where(inside, 2.0 * r2, l2))), 0.0))


# ---- brute-force pdfs ------------------------------------------------------------------------------------------------------------
EDGE_EPS, COS_EPS = 1e-9, 1e-6


def pdf_mesh_brute(tris, A, origin, direction, pairs=1 << 21, first_hit_only=False):
    """The rule's mesh pdf by testing EVERY triangle (mesh.rs:50-82, t_min = 0) for local-space rays (m, 3): returns (pdf, number of
    hits, risky) — risky marks rows with a hit (or a near miss) whose |dot(d, n)| < COS_EPS or with a barycentric coordinate within
    EDGE_EPS of an edge, where the last bits of the ray decide what is hit."""
    d_all = normalize(np.asarray(direction, dtype=np.float64))
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    c = cross(e1, e2)
    nrm = normalize(c)
    m = len(origin)
    pdf, hits, risky = np.zeros(m), np.zeros(m, dtype=np.int64), np.zeros(m, bool)
    step = max(1, pairs // len(tris))
    for lo in range(0, m, step):
        o, d = origin[lo:lo + step, None, :], d_all[lo:lo + step, None, :]
        h = cross(d, e2[None])
        a = dot(e1[None], h)
        big = np.abs(a) >= 1e-8
        f = 1.0 / np.where(big, a, 1.0)
        s = o - v0[None]
        u = f * dot(s, h)
        q = cross(s, e1[None])
        v = f * dot(d, q)
        t = f * dot(e2[None], q)
        ok = big & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= 0.0) & (t <= np.inf)
        cosn = np.abs(dot(d, nrm[None]))
        term = np.where(ok, (t * t) / (np.where(ok, cosn, 1.0) * A), 0.0)
        if first_hit_only:
            tt = np.where(ok, t, np.inf)
            only = tt == tt.min(axis=1, keepdims=True)
            term = np.where(only, term, 0.0)
        pdf[lo:lo + step] = term.sum(axis=1)
        hits[lo:lo + step] = ok.sum(axis=1)
        w = 1.0 - u - v
        near = big & (u >= -EDGE_EPS) & (v >= -EDGE_EPS) & (w >= -EDGE_EPS) & (t >= -EDGE_EPS)
        edge = near & ((np.abs(u) < EDGE_EPS) | (np.abs(v) < EDGE_EPS) | (np.abs(w) < EDGE_EPS) | (np.abs(t) < EDGE_EPS))
        inside_loose = (np.abs(a) > 0.0) & (u >= -EDGE_EPS) & (v >= -EDGE_EPS) & (w >= -EDGE_EPS) & (t >= 0.0)
        graze = inside_loose & (cosn < COS_EPS)
        risky[lo:lo + step] = (edge | graze).any(axis=1)
    return pdf, hits, risky


def pdf_mesh_from_point(tris, A, origin, direction, first_hit_only=False, chunk=40000):
    """pdf_mesh_brute for MANY rays from ONE origin (the quadrature of the CPU test): the same tests with the triple products regrouped
    around the ray direction, so that they are three matrix products — equal to the brute force up to rounding. Returns (pdf, signature),
    the signature a number that identifies the SET of faces hit."""
    d_all = normalize(np.asarray(direction, dtype=np.float64))
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    c = cross(e1, e2)
    nrm = normalize(c)
    s = np.asarray(origin, dtype=np.float64)[None, :] - v0
    q = cross(s, e1)
    tn = dot(e2, q)
    keys = np.random.default_rng(1).integers(1, 1 << 40, len(tris)).astype(np.float64)
    pdf, sig = np.zeros(len(d_all)), np.zeros(len(d_all))
    for lo in range(0, len(d_all), chunk):
        d = d_all[lo:lo + chunk]
        a = -(d @ c.T)                                          # e1 . (d x e2) = -d . (e1 x e2)
        big = np.abs(a) >= 1e-8
        f = 1.0 / np.where(big, a, 1.0)
        u, v, t = f * (d @ cross(e2, s).T), f * (d @ q.T), f * tn[None, :]
        ok = big & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= 0.0)
        term = np.where(ok, (t * t) / (np.where(ok, np.abs(d @ nrm.T), 1.0) * A), 0.0)
        if first_hit_only:
            tt = np.where(ok, t, np.inf)
            term = np.where(tt == tt.min(axis=1, keepdims=True), term, 0.0)
        pdf[lo:lo + chunk] = term.sum(axis=1)
        sig[lo:lo + chunk] = ok @ keys
    return pdf, sig


def pdf_quad(q, u, v, origin, direction):
    """quad.rs:88-98 for a quad without a normal map."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in (q, u, v))
    n0 = np.cross(u, v)
    w = n0 / (n0 @ n0)
    n = n0 / np.sqrt(n0 @ n0)
    d = normalize(direction)
    nd = d @ n
    ok = np.abs(nd) >= 1e-8
    t = ((n @ q) - origin @ n) / np.where(ok, nd, 1.0)
    p = origin + d * t[:, None] - q
    al, be = np.cross(p, v) @ w, np.cross(u, p) @ w
    ok &= (t >= 0.0) & (al >= 0.0) & (al <= 1.0) & (be >= 0.0) & (be <= 1.0)
    area = np.sqrt(n0 @ n0)
    return np.where(ok, (t * t) / (np.abs(nd) * area), 0.0)


# ---- the GPU probe test's meshes, placements and fixed-seed ray sets ------------------------------------------------------------------
PROBE_MESHES = ("ico1", "quad", "ico5")
PROBE_CHAIN = (((0.3, 1.0, 0.2), 0.7, (1.5, -0.5, 2.0)), ((1.0, 0.2, -0.4), -1.1, (0.2, 0.3, -0.4)))   # outermost first; axes normalised below
N_SAMPLE_ROWS, N_PDF_ROWS = 4096, 2048


def probe_chain():
    return Chain(*[(tuple(np.asarray(a) / np.linalg.norm(a)), ang, tr) for a, ang, tr in PROBE_CHAIN])


def probe_chain_spec():
    return [(tuple(float(x) for x in np.asarray(a) / np.linalg.norm(a)), ang, tr) for a, ang, tr in PROBE_CHAIN]


def probe_mesh(name):
    """(f32 positions, u32 indices, scale)"""
    if name == "ico1":
        return (*icosphere(1), 0.8)
    if name == "ico5":
        return (*icosphere(5), 1.1)
    return (*tessellate_quad((-1.0, 0.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), 8), 1.0)


@functools.lru_cache(maxsize=None)
def _probe_local(name):
    """The mesh, its table, and the local-space inputs with the brute-force pdfs: computed once per mesh, shared by both placements
    (a rigid chain moves the rays, not the answers: rows where the ray's last bits could matter are left out anyway)."""
    P, I, scale = probe_mesh(name)
    tris = mesh_tris(P, I, scale)
    C = area_table(tris)
    rng = np.random.default_rng({"ico1": 11, "quad": 12, "ico5": 13}[name])

    def shell(n, lo, hi):
        x = rng.normal(size=(n, 3))
        return x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(lo, hi, size=(n, 1))

    o1, t1 = shell(N_SAMPLE_ROWS, 1.6, 4.0), rng.uniform(0.0, 1.0, size=(N_SAMPLE_ROWS, 1))
    # pdf check: half of the rays aimed at points of the mesh, half random (fewer rows for the large mesh: the brute force is n x rows)
    n_rows = N_PDF_ROWS if len(tris) < 4096 else N_PDF_ROWS // 4
    half = n_rows // 2
    o2 = shell(n_rows, 1.6, 4.0)
    _, _, pts = sample_mesh(C, tris, o2[:half], rng.uniform(size=half), rng.uniform(size=half), rng.uniform(size=half))
    aimed = (pts - o2[:half]) * rng.uniform(0.5, 2.0, size=(half, 1))            # lights.pdf takes any length
    d2 = np.concatenate([aimed, shell(n_rows - half, 1.0, 1.0)])
    t2 = rng.uniform(0.0, 1.0, size=(n_rows, 1))
    pdf, hits, risky = pdf_mesh_brute(tris, C[-1], o2, d2)
    return dict(P=P, I=I, scale=scale, tris=tris, C=C, o1=o1, t1=t1, o2=o2, d2=d2, t2=t2, pdf=pdf, hits=hits, keep=~risky)


@functools.lru_cache(maxsize=None)
def probe_case(name, chained):
    """Everything the probe test compares for one mesh and placement: world-space inputs and the rule's expected outputs."""
    L = _probe_local(name)
    chain = probe_chain() if chained else Chain()
    origins = np.concatenate([chain.point_to_world(L["o1"]), L["t1"]], axis=1)
    dr = Draws(0, np.arange(N_SAMPLE_ROWS), 0)
    light = dr.index(1)
    u0 = dr.unit()
    u1, u2 = dr.pair()
    face, d_loc, _ = sample_mesh(L["C"], L["tris"], chain.point_to_local(origins[:, :3]), u0, u1, u2)
    sample = dict(origins=origins, face=face, light=light, dirs=chain.vector_to_world(d_loc), draws=dr.draw.astype(np.int64))
    rays = np.concatenate([chain.point_to_world(L["o2"]), chain.vector_to_world(L["d2"]), L["t2"]], axis=1)
    return dict(L, sample=sample, rays=rays)


# ---- scalar replay of the two-light MIS scene (common.mis_scene("two")) -------------------------------------------------------------
def replay_two(frame, cam, seed, pixel, sample, sobol=False):
    """The radiance (3,) of (pixel, sample) of mis_scene("two") under kind 1 when the first bounce samples the lights; None when its
    selector draw picks the BSDF. Lambert floor at y = 0, quad light MIS_QUAD2 and the one-triangle mesh MIS_TRI above, max_depth 2."""
    dr = Draws(seed, [pixel], sample, sobol=sobol)
    ly, lx = SR.camera_locations(frame, cam["blur_strength"], cam["width"], seed, [pixel], [sample], sobol=sobol)
    loc = frame["pixel00"] + frame["dv"] * ly[0, 0] + frame["du"] * lx[0, 0]
    o = np.asarray(frame["center"], dtype=np.float64)
    d = normalize(loc - o)
    dr.draw[:] = 5                                              # pixel offsets (2), lens offsets (2), time (1)
    t = (0.0 - o[1]) / d[1]
    p = o + d * t
    gn = np.array([0.0, 1.0, 0.0])
    if not float(dr.unit()[0]) < 0.5:                           # the selector
        return None
    origin = p[None, :]
    q, u, v = (np.asarray(a, dtype=np.float64) for a in MIS_QUAD2)
    tris = mesh_tris(np.array(MIS_TRI, dtype=np.float32), [0, 1, 2])
    C = area_table(tris)
    i = int(dr.index(2)[0])
    if i == 0:
        a, b = dr.pair()
        w = normalize(q + u * a[0] + v * b[0] - p)
    else:
        u0 = dr.unit()
        u1, u2 = dr.pair()
        w = sample_mesh(C, tris, origin, u0, u1, u2)[1][0]
    lz = abs(float(w @ gn))
    bsdf_pdf, brdf = lz / PI, lz * (np.asarray(MIS_ALBEDO) / PI)
    light_pdf = (float(pdf_quad(q, u, v, origin, w[None])[0]) + float(pdf_mesh_brute(tris, C[-1], origin, w[None])[0][0])) / 2.0
    thr = brdf / (0.5 * bsdf_pdf + 0.5 * light_pdf)
    o2 = p + (1e-3 if w @ gn >= 0.0 else -1e-3) * gn
    # the second segment: the closest of the two lights (they never overlap in direction); the floor lies behind
    tq = float(pdf_quad(q, u, v, o2[None], w[None])[0]) > 0.0
    tt = float(pdf_mesh_brute(tris, C[-1], o2[None], w[None])[0][0]) > 0.0
    if tq:
        return thr * np.asarray(MIS_EMISSION)
    if tt:
        return thr * np.asarray(MIS_TRI_EMISSION)
    return np.zeros(3)


def mis_frame(width=None):
    c = MIS_CAM
    return R.camera_frame(width or c["width"], c["aspect"], c["vfov"], c["look_from"], c["look_at"], c["vup"], c["focal_length"])
