"""The grid-density medium rule (pt_mat_medium_grid in include/pt_amd.h) restated in numpy, for the grid-medium tests:
the trilinear density, the clip of a segment to the grid's box, delta tracking (one row at a time and many rows at once), the exact
optical depth of a segment, a scalar replay of whole paths through scenes of homogeneous and grid media, the single-scattering
quadrature of a quad light seen through a grid whose values are a ramp along one axis, and the plume of `pt_render --smoke`."""
import numpy as np

import medium_rule as MR
import sampler_rule as SR


def _lerp(a, b, f):
    return a + f * (b - a)


class Grid:
    """sigma(x) = scale * V(x); values: float32 (nz, ny, nx), samples at the cell centres of the box [lo, hi]."""

    def __init__(self, scale, values, lo, hi):
        self.scale = float(scale)
        self.values = np.ascontiguousarray(values, dtype=np.float32)
        self.v = self.values.astype(np.float64)
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        nz, ny, nx = self.values.shape
        self.n = np.array([nx, ny, nz], dtype=np.int64)
        self.cells = self.n.astype(np.float64) / (self.hi - self.lo)
        self.mu = self.scale * float(self.values.max())

    # ---- density ------------------------------------------------------------------------------------------------------------
    def V(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        inside = ((x >= self.lo) & (x <= self.hi)).all(axis=1)
        xs = np.where(inside[:, None], x, self.lo)
        q = np.clip((xs - self.lo) * self.cells - 0.5, 0.0, (self.n - 1).astype(np.float64))
        i = np.minimum(np.floor(q).astype(np.int64), self.n - 2)
        f = q - i
        at = lambda dx, dy, dz: self.v[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx]
        c00, c10 = _lerp(at(0, 0, 0), at(1, 0, 0), f[:, 0]), _lerp(at(0, 1, 0), at(1, 1, 0), f[:, 0])
        c01, c11 = _lerp(at(0, 0, 1), at(1, 0, 1), f[:, 0]), _lerp(at(0, 1, 1), at(1, 1, 1), f[:, 0])
        c0, c1 = _lerp(c00, c10, f[:, 1]), _lerp(c01, c11, f[:, 1])
        return np.where(inside, _lerp(c0, c1, f[:, 2]), 0.0)

    def sigma(self, x):
        return self.scale * self.V(x)

    # ---- the clip ---------------------------------------------------------------------------------------------------------------
    def clip(self, o, d, t):
        """Rows of (o, d, t) -> (ok, t0, t1): the slab test of the rule."""
        o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (len(o),))
        near, far = np.zeros(len(o)), t.copy()
        ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
        for a in range(3):
            zero = d[:, a] == 0.0
            ok &= ~zero | ((o[:, a] >= self.lo[a]) & (o[:, a] <= self.hi[a]))
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / d[:, a]
                ta, tb = (self.lo[a] - o[:, a]) * inv, (self.hi[a] - o[:, a]) * inv
            lo_t, hi_t = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            near = np.where(~zero & (lo_t > near), lo_t, near)
            far = np.where(~zero & (hi_t < far), hi_t, far)
        with np.errstate(invalid="ignore"):
            ok &= (near < far) & (far < np.inf)
        return ok, near, far

    # ---- the optical depth of a segment, exactly ------------------------------------------------------------------------------
    def tau(self, o, d, t=np.inf):
        """int_0^t sigma(o + s d) ds of ONE ray. Between consecutive cell-centre planes (and the box's faces) V is a product of three
        functions linear in s — a cubic — so the 2-point Gauss-Legendre rule per piece is exact."""
        o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
        ok, t0, t1 = self.clip(o, d, t)
        if not ok[0]:
            return 0.0
        t0, t1 = float(t0[0]), float(t1[0])
        cuts = [t0, t1]
        for a in range(3):
            if d[a] != 0.0:
                planes = self.lo[a] + (np.arange(self.n[a]) + 0.5) / self.cells[a]
                s = (planes - o[a]) / d[a]
                cuts.extend(s[(s > t0) & (s < t1)])
        cuts = np.unique(np.array(cuts))
        mid, h = 0.5 * (cuts[1:] + cuts[:-1]), 0.5 * np.diff(cuts)
        g = h / np.sqrt(3.0)
        s = np.concatenate([mid - g, mid + g])
        sig = self.sigma(o[None, :] + s[:, None] * d[None, :])
        return float((np.concatenate([h, h]) * sig).sum())

    # ---- delta tracking -----------------------------------------------------------------------------------------------------------
    def track(self, o, d, t, U, draw):
        """One row. U(draw) -> the unit value of draw index `draw`. Returns (collided, s, draw after the loop, tentative collisions)."""
        ok, t0, t1 = self.clip(o, d, t)
        if not ok[0]:
            return False, 0.0, draw, 0
        s, t1, trips = float(t0[0]), float(t1[0]), 0
        while True:
            s += -np.log(1.0 - U(draw)) / self.mu
            draw += 1
            if not (s < t1):
                return False, 0.0, draw, trips
            v = U(draw)
            draw += 1
            trips += 1
            if v * self.mu < self.sigma(o + d * s)[0]:
                return True, s, draw, trips

    def track_many(self, o, d, t, units):
        """Many rows at once. units(rows, draws) -> unit values of draw `draws[i]` of row `rows[i]`. Returns (collided, s, draws)."""
        o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
        ok, s, t1 = self.clip(o, d, t)
        n = len(o)
        draws, collided, out_s = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n)
        act = np.flatnonzero(ok)
        s = s.copy()
        while len(act):
            s[act] += -np.log(1.0 - units(act, draws[act])) / self.mu
            draws[act] += 1
            act = act[s[act] < t1[act]]
            v = units(act, draws[act])
            draws[act] += 1
            hit = v * self.mu < self.sigma(o[act] + d[act] * s[act][:, None])
            collided[act[hit]] = True
            out_s[act[hit]] = s[act[hit]]
            act = act[~hit]
        return collided, out_s, draws


def probe_units(rows, draws):
    """The draws pt_medium_probe's which = 3 gives row i: the independent sampler's of (seed 0, pixel i, sample 0)."""
    return SR.unit(SR.independent_u64(0, np.asarray(rows, dtype=np.uint64), 0, np.asarray(draws, dtype=np.uint64)))


# ---- a scalar replay of whole paths -----------------------------------------------------------------------------------------------
class Media(MR.Media):
    """medium_rule.Media whose media may be grids: `density` is a number (homogeneous) or a Grid. add_unbounded: a medium that no
    object bounds (the camera medium), returns its index."""

    def _medium(self, density, albedo, g):
        self.media.append((density if isinstance(density, Grid) else float(density), np.asarray(albedo, dtype=np.float64), float(g)))
        return len(self.media) - 1

    def add_unbounded(self, density, albedo, g):
        return self._medium(density, albedo, g)

    def bounded(self, m):
        return any(ob[-1] == m for ob in self.objs)


def replay_path(media, frame, cam, seed, pixel, sample, env, camera_medium=None, sobol=False, perturb=None):
    """medium_rule.replay_path with step 1 of the rule for grid media (delta tracking) and the unbounded camera medium: the radiance
    (3,) of sample `sample` of `pixel`, and whether the path ever ran a tracking loop or scattered. No lights, constant environment."""
    f64 = SR.sobol_u64 if sobol else SR.independent_u64
    nudge = perturb if perturb is not None else (lambda x: x)

    def U(d):
        return nudge(float(SR.unit(f64(seed, pixel, sample, d))))

    ly, lx = SR.camera_locations(frame, cam["blur_strength"], cam["width"], seed, [pixel], [sample], sobol=sobol)
    loc = frame["pixel00"] + frame["dv"] * ly[0, 0] + frame["du"] * lx[0, 0]
    o = np.asarray(frame["center"], dtype=np.float64)
    d = loc - o
    d = d / np.linalg.norm(d)
    draw = 5
    m, bounce, thr = camera_medium, 0, np.ones(3)
    env = np.asarray(env, dtype=np.float64)
    met = False
    while True:
        hit = media.closest(o, d)
        t = nudge(hit[0]) if hit is not None else np.inf
        if m is not None and hit is None and media.bounded(m):
            m = None
        if m is not None:
            dens, alb, g = media.media[m]
            if isinstance(dens, Grid):
                collided, dist, draw2, trips = dens.track(o, d, t, U, draw)
                met = met or draw2 != draw
                draw = draw2
            else:
                dist = MR.free_flight(U(draw), dens)
                draw += 1
                collided = dist < t
                met = True
            if collided:
                x = o + d * dist
                if bounce > 5:
                    p = min(max(MR.luminance(thr), 0.01), 1.0)
                    r = U(draw)
                    draw += 1
                    if r > p:
                        return np.zeros(3), met
                    thr = thr / p
                draw += 1
                if sobol:
                    draw = (draw + 1) & ~1
                u1, u2 = U(draw), U(draw + 1)
                draw += 2
                w = MR.hg_dir(g, u1, u2, d)
                ph = MR.hg_phase(g, d @ w)
                pdf = ph
                if not (pdf > 0.0) or not np.isfinite(pdf):
                    return np.zeros(3), met
                thr = thr * (alb * ph / pdf)
                o, d = x, w / np.linalg.norm(w)
                bounce += 1
                if bounce >= cam["max_depth"]:
                    return np.zeros(3), met
                continue
        if hit is None:
            return thr * env, met
        _, p, n, k = hit
        m = None if m == k else k
        o = p + (1e-3 if d @ n >= 0.0 else -1e-3) * n
        bounce += 1
        if bounce >= cam["max_depth"]:
            return np.zeros(3), met


# ---- single scattering through a ramp grid, by quadrature -----------------------------------------------------------------------
class Ramp:
    """A grid whose values are a linear ramp v0 .. v1 along `axis`: sigma is a clamped linear function of that coordinate inside the
    box, and the optical depth of any segment has a closed form."""

    def __init__(self, scale, v0, v1, n, axis, lo, hi):
        self.axis = axis
        ramp = np.linspace(v0, v1, n[axis]).astype(np.float32)
        assert (ramp.astype(np.float64) == np.linspace(v0, v1, n[axis])).all(), "the ramp's values must be exact in f32"
        shape = [1, 1, 1]
        shape[2 - axis] = n[axis]                                     # values are (nz, ny, nx)
        self.grid = Grid(scale, np.broadcast_to(ramp.reshape(shape), (n[2], n[1], n[0])).copy(), lo, hi)
        g = self.grid
        self.c0 = g.lo[axis] + 0.5 / g.cells[axis]                    # first and last cell centre: the ramp is flat beyond them
        self.c1 = g.lo[axis] + (n[axis] - 0.5) / g.cells[axis]
        self.s0, self.s1 = g.scale * float(ramp[0]), g.scale * float(ramp[-1])

    def f(self, x):
        """sigma as a function of the ramp coordinate (inside the box)."""
        w = np.clip((x - self.c0) / (self.c1 - self.c0), 0.0, 1.0)
        return self.s0 + w * (self.s1 - self.s0)

    def F(self, x):
        """An antiderivative of f."""
        xc = np.clip(x, self.c0, self.c1)
        k = (self.s1 - self.s0) / (self.c1 - self.c0)
        mid = self.s0 * (xc - self.c0) + 0.5 * k * (xc - self.c0) ** 2
        return mid + self.s0 * np.minimum(x - self.c0, 0.0) + self.s1 * np.maximum(x - self.c1, 0.0)

    def tau(self, P, Q):
        """The optical depth of the segments P -> Q (arrays (..., 3)), vectorised."""
        g, a = self.grid, self.axis
        D = Q - P
        t0, t1 = np.zeros(D.shape[:-1]), np.ones(D.shape[:-1])
        empty = np.zeros(D.shape[:-1], dtype=bool)
        for b in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                ta, tb = (g.lo[b] - P[..., b]) / D[..., b], (g.hi[b] - P[..., b]) / D[..., b]
            zero = D[..., b] == 0.0
            empty |= zero & ((P[..., b] < g.lo[b]) | (P[..., b] > g.hi[b]))
            t0 = np.where(zero, t0, np.maximum(t0, np.minimum(ta, tb)))
            t1 = np.where(zero, t1, np.minimum(t1, np.maximum(ta, tb)))
        empty |= ~(t0 < t1)
        xa, xb = P[..., a] + t0 * D[..., a], P[..., a] + t1 * D[..., a]
        dx = xb - xa
        flat = np.abs(dx) < 1e-9
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(flat, self.f(0.5 * (xa + xb)), (self.F(xb) - self.F(xa)) / np.where(flat, 1.0, dx))
        return np.where(empty, 0.0, np.linalg.norm(D, axis=-1) * (t1 - t0) * mean)


def single_scatter_quad(origins, dirs, ramp, g, quad, n_v, n_a, d_max):
    """medium_rule.single_scatter_quad with sigma_s(x) T for a Ramp medium: for rays that do NOT hit the quad, the scalar S with
    radiance = albedo * emission * S,
       S = int_0^d_max sigma(x) T(o, x) int_quad ph(dir . w) T(x, y) |n . w| / r^2 dA dd,   x = o + d dir, w = (y - x) / r.
    Gauss-Legendre: n_v nodes in d on each of the pieces the ramp's two kinks and the box's faces cut [0, d_max] into, n_a x n_a on the
    quad. d_max must reach past the box along every ray."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in quad)
    nrm = np.cross(u, v)
    area = np.linalg.norm(nrm)
    nrm = nrm / area
    gx, gw = np.polynomial.legendre.leggauss(n_v)
    ax, aw = np.polynomial.legendre.leggauss(n_a)
    aa, wa = 0.5 * (ax + 1.0), 0.5 * aw
    Y = (q + aa[:, None, None] * u + aa[None, :, None] * v).reshape(-1, 3)
    WY = (wa[:, None] * wa[None, :]).reshape(-1) * area
    G, a = ramp.grid, ramp.axis
    out = np.zeros(len(origins))
    for i, (o, d) in enumerate(zip(np.asarray(origins, dtype=np.float64), np.asarray(dirs, dtype=np.float64))):
        ok, t0, t1 = G.clip(o, d, d_max)
        if not ok[0]:
            continue
        cuts = [float(t0[0]), float(t1[0])]
        if d[a] != 0.0:
            cuts += [s for s in ((ramp.c0 - o[a]) / d[a], (ramp.c1 - o[a]) / d[a]) if cuts[0] < s < cuts[1]]
        cuts = np.sort(np.array(cuts))
        mid, h = 0.5 * (cuts[1:] + cuts[:-1]), 0.5 * np.diff(cuts)
        dist = (mid[:, None] + h[:, None] * gx[None, :]).reshape(-1)
        wv = (h[:, None] * gw[None, :]).reshape(-1)
        X = o + dist[:, None] * d
        sig = G.sigma(X)
        T0 = np.exp(-ramp.tau(np.broadcast_to(o, X.shape), X))
        R = Y[None, :, :] - X[:, None, :]
        r = np.linalg.norm(R, axis=2)
        W = R / r[..., None]
        T1 = np.exp(-ramp.tau(np.broadcast_to(X[:, None, :], R.shape), np.broadcast_to(Y[None, :, :], R.shape)))
        f = MR.hg_phase(g, W @ d) * T1 * np.abs(W @ nrm) / (r * r)
        out[i] = ((wv * sig * T0)[:, None] * WY[None, :] * f).sum()
    return out


# ---- the plume of `pt_render --smoke` ------------------------------------------------------------------------------------------------
def smoke_plume(n=64):
    """The values `pt_render --smoke` samples: (nz, ny, nx) float32 at the cell centres of the unit box, y up."""
    c = (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    cx, cz, r = 0.5 + 0.08 * np.sin(3.0 * np.pi * y), 0.5 + 0.08 * np.cos(2.0 * np.pi * y), 0.06 + 0.22 * y
    return ((1.0 - 0.7 * y) * np.exp(-((x - cx) ** 2 + (z - cz) ** 2) / (r * r))).astype(np.float32)
