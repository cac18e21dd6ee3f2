"""The Loop subdivision rule (include/pt_amd.h, "Loop subdivision surfaces") restated in numpy from the printed rule: np.unique on the
edge keys, a stable argsort for the runs, per-vertex sums in ascending order of the neighbour's index. Reads nothing of the product.
float32 arrays in, float32 arrays out; all arithmetic in float64 with one rounding to float32 per written attribute and level. Also
the meshes the tests add to tess_rule's."""
import numpy as np

f32, f64, u64 = np.float32, np.float64, np.uint64


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _runs(group, n_groups):
    """members of each group in stable order: (order, start, count) with group[order] ascending"""
    order = np.argsort(group, kind="stable")
    count = np.bincount(group, minlength=n_groups)
    return order, np.cumsum(count) - count, count


def _run_sum(values, order, start, count):
    """S = 0, then S += values[member] over each group's members in order: one add per member, in that order"""
    S = np.zeros((len(start), values.shape[1]), f64)
    for j in range(int(count.max()) if len(count) else 0):
        sel = np.flatnonzero(count > j)
        S[sel] = S[sel] + values[order[start[sel] + j]]
    return S


class _Edges:
    """The distinct keys of a mesh in ascending order; per key its run (slots ascending), class and opposite vertices"""

    def __init__(self, tri, crease):
        flat = tri.reshape(-1)
        ends = np.stack([tri, np.roll(tri, -1, axis=1)], axis=-1)            # e0 = (a, b), e1 = (b, c), e2 = (c, a)
        keys = ((ends.min(axis=-1).astype(u64) << u64(32)) | ends.max(axis=-1).astype(u64)).reshape(-1)
        uniq, self.rank = np.unique(keys, return_inverse=True)
        self.rank = self.rank.reshape(-1)
        self.E = len(uniq)
        self.A, self.B = (uniq >> u64(32)).astype(np.int64), (uniq & u64(0xFFFFFFFF)).astype(np.int64)
        self.order, self.start, self.count = _runs(self.rank, self.E)
        self.flagged = np.zeros(self.E, bool)
        np.logical_or.at(self.flagged, self.rank, crease != 0)
        self.sharp = (self.count != 2) | (self.A == self.B) | self.flagged
        if self.E:
            self.s0 = self.order[self.start]
            self.s1 = self.order[self.start + (self.count > 1)]
            opposite = lambda s: flat[3 * (s // 3) + (s % 3 + 2) % 3]
            self.C, self.D = opposite(self.s0), opposite(self.s1)


def _crease_by_angle(pos, tri, crease, crease_cos):
    e = _Edges(tri, crease)
    if not e.E:
        return crease
    pick = np.flatnonzero((e.count == 2) & (e.A != e.B))
    p = pos.astype(f64)
    with np.errstate(all="ignore"):
        cross = lambda f: np.cross(p[tri[f, 1]] - p[tri[f, 0]], p[tri[f, 2]] - p[tri[f, 0]])
        c0, c1 = cross(e.s0[pick] // 3), cross(e.s1[pick] // 3)
        fold = _dot(c0, c1) < crease_cos * np.sqrt(_dot(c0, c0) * _dot(c1, c1))
    crease = crease.copy()
    crease[e.s0[pick[fold]]] = 1
    crease[e.s1[pick[fold]]] = 1
    return crease


def _even(attrs, pos, e, corner_cos, limit):
    """The even vertices (or limit positions) of every attribute array in `attrs`; classification from `pos`"""
    n = len(pos)
    real = np.flatnonzero(e.A != e.B) if e.E else np.zeros(0, np.int64)
    v = np.concatenate([e.A[real], e.B[real]]) if e.E else np.zeros(0, np.int64)
    w = np.concatenate([e.B[real], e.A[real]]) if e.E else np.zeros(0, np.int64)
    r = np.concatenate([real, real])
    by = np.lexsort((w, v))                                                  # by v, then by the other endpoint
    v, w, r = v[by], w[by], r[by]
    k = np.bincount(v, minlength=n)
    start = np.cumsum(k) - k
    is_sharp = e.sharp[r] if len(r) else np.zeros(0, bool)
    s = np.bincount(v, weights=is_sharp, minlength=n).astype(np.int64)
    nth = np.cumsum(is_sharp) - np.concatenate([[0], np.cumsum(is_sharp)])[start[v]] if len(v) else np.zeros(0, np.int64)
    w0, w1 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    first, second = is_sharp & (nth == 1), is_sharp & (nth == 2)
    w0[v[first]], w1[v[second]] = w[first], w[second]
    p = pos.astype(f64)
    with np.errstate(all="ignore"):
        d0, d1 = p[w0] - p, p[w1] - p
        corner = _dot(d0, d1) > corner_cos * np.sqrt(_dot(d0, d0) * _dot(d1, d1))
        crease = (k > 0) & (s == 2) & ~corner
        smooth = (k > 0) & (s <= 1)
        kd = np.maximum(k, 1).astype(f64)
        beta = np.where(k == 3, 0.2, 0.5 / kd) if limit else np.where(k == 3, 0.1875, 0.375 / kd)
        own, other = (2.0 / 3.0, 1.0 / 6.0) if limit else (0.75, 0.125)
        out = []
        for a in attrs:
            if a is None:
                out.append(None)
                continue
            x = a.astype(f64)
            S = _run_sum(x[w], np.arange(len(w)), start, k)                  # S += P[w], neighbours ascending
            smooth_v = x * (1.0 - k.astype(f64) * beta)[:, None] + S * beta[:, None]
            crease_v = x * own + (x[w0] + x[w1]) * other
            new = np.where(smooth[:, None], smooth_v, np.where(crease[:, None], crease_v, x)).astype(f32)
            keep = ~(smooth | crease)
            new[keep] = a[keep]                                              # a kept value keeps its bits (a NaN's payload too)
            out.append(new)
    return out


def _level(pos, tri, uv, crease, corner_cos):
    n = len(pos)
    e = _Edges(tri, crease)
    even = _even([pos, uv], pos, e, corner_cos, False)
    if not e.E:
        return even[0], tri.reshape(0, 3), even[1], np.zeros(0, np.uint8)
    with np.errstate(all="ignore"):
        def odd(a):
            x = a.astype(f64)
            sharp = (x[e.A] + x[e.B]) * 0.5
            soft = (x[e.A] + x[e.B]) * 0.375 + (x[e.C] + x[e.D]) * 0.125
            return np.where(e.sharp[:, None], sharp, soft).astype(f32)
        pos2 = np.concatenate([even[0], odd(pos)])
        uv2 = None if uv is None else np.concatenate([even[1], odd(uv)])
    mid = (n + e.rank).reshape(-1, 3)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
    kids = np.stack([a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca], axis=1).reshape(-1, 3)
    fl = e.flagged[e.rank].reshape(-1, 3).astype(np.uint8)
    e0, e1, e2, z = fl[:, 0], fl[:, 1], fl[:, 2], np.zeros(len(tri), np.uint8)
    flags = np.stack([e0, z, e2, e0, e1, z, z, e1, e2, z, z, z], axis=1).reshape(-1)
    return pos2, kids, uv2, flags


def smooth_normals(pos, tri):
    p = pos.astype(f64)
    with np.errstate(all="ignore"):
        cf = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
        order, start, count = _runs(tri.reshape(-1), len(pos))               # corners 3f + k of each vertex, ascending
        total = _run_sum(cf[np.arange(3 * len(tri)) // 3], order, start, count)
        L = np.sqrt((total[:, 0] * total[:, 0] + total[:, 1] * total[:, 1]) + total[:, 2] * total[:, 2])
        ok = np.isfinite(L) & (L > 0.0)
        unit = total / np.where(ok, L, 1.0)[:, None]
    return np.where(ok[:, None], unit.astype(f32), np.array([0, 1, 0], f32))


def subdivide(pos, idx, uv=None, crease=None, levels=1, crease_cos=-2.0, corner_cos=2.0, limit=False, normals="smooth"):
    """-> (pos, idx, nrm | None, uv | None, crease)"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    if uv is not None:
        uv = np.concatenate([np.asarray(uv, f32).reshape(-1, 2), np.zeros((len(pos), 2), f32)])[: len(pos)]
    crease = np.zeros(3 * len(tri), np.uint8) if crease is None else (np.asarray(crease).reshape(-1) != 0).astype(np.uint8)
    crease = _crease_by_angle(pos, tri, crease, crease_cos)
    for _ in range(levels):
        pos, tri, uv, crease = _level(pos, tri, uv, crease, corner_cos)
    if limit:
        pos, uv = _even([pos, uv], pos, _Edges(tri, crease), corner_cos, True)
    nrm = smooth_normals(pos, tri) if normals == "smooth" else None
    return pos, tri.reshape(-1).astype(np.uint32), nrm, uv, crease


# ---- the meshes the tests add to tess_rule.shapes(): (pos, idx, uv | None, crease | None) ----
def cube(flagged=True):
    """The unit cube of 12 triangles, outward winding; flagged: its 12 cube edges sharp (the 6 face diagonals not)"""
    pos = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], f32)          # index = x + 2 y + 4 z
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    idx, crease = [], []
    for a, b, c, d in quads:                                                                   # (a, b, c) and (a, c, d): the diagonal is (a, c)
        idx += [a, b, c, a, c, d]
        crease += [1, 1, 0, 0, 1, 1]
    return pos, np.array(idx, np.uint32), None, (np.array(crease, np.uint8) if flagged else None)


def fan(valence, closed=True):
    """A hub (vertex 0) with `valence` spokes on a bumpy ring; closed: the hub is interior"""
    t = np.arange(valence) * (2 * np.pi / valence)
    ring = np.stack([np.cos(t), 0.2 * np.sin(3 * t), np.sin(t)], axis=1)
    pos = np.concatenate([[[0, 0.5, 0]], ring]).astype(f32)
    k = np.arange(valence if closed else valence - 1)
    idx = np.stack([np.zeros_like(k), 1 + (k + 1) % valence, 1 + k], axis=1).reshape(-1).astype(np.uint32)
    uv = (pos[:, [0, 2]] * 0.5 + 0.5).astype(f32)
    return pos, idx, uv, None
