"""The light grid (pt_scene_set_punctual_selection kind 1) restated in numpy from the rule in include/pt_amd.h: the cells, a light's weight
for a cell, a cell's row of the table, the selection at a vertex, and the per-sample variance the rule predicts. f64, one rounding per
written operation; sums run in ascending k as the rule says. Nothing here reads the product."""
from __future__ import annotations

import numpy as np

FLOOR_SHARE = 0.125                                                        # the uniform floor: every p_k >= 1 / (8 n)
CAP = 1 << 25                                                              # cells * n of the largest table
AUTO_RES = 16


def auto_dims(box, n):
    """the automatic dims for a box and n lights"""
    box = np.asarray(box, dtype=np.float64)
    ext = box[3:] - box[:3]
    ext_max = ext.max()
    R = AUTO_RES
    while True:
        dims = [int(min(max(np.ceil(R * e / ext_max), 1.0), R)) if e > 0.0 else 1 for e in ext]
        if dims[0] * dims[1] * dims[2] * n <= CAP or R == 1:
            return tuple(dims)
        R //= 2


def cell_geometry(box, dims):
    """(a, b, m) of shape (cells, 3) and rc2 (cells,), cell (ix, iy, iz) at index (iz * ny + iy) * nx + ix"""
    box = np.asarray(box, dtype=np.float64)
    nx, ny, nz = (int(d) for d in dims)
    c = np.arange(nx * ny * nz)
    idx = np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], axis=1).astype(np.float64)
    a, b = np.empty_like(idx), np.empty_like(idx)
    for ax, n_axis in enumerate((nx, ny, nz)):
        s = (box[3 + ax] - box[ax]) / float(n_axis)
        a[:, ax] = box[ax] + idx[:, ax] * s
        b[:, ax] = box[ax] + (idx[:, ax] + 1.0) * s
    m = (a + b) * 0.5
    h = (b - a) * 0.5
    rc2 = (h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) + h[:, 2] * h[:, 2]
    return a, b, m, rc2


def weights(recs16, box, dims):
    """w[cell, k]"""
    recs = np.asarray(recs16, dtype=np.float64).reshape(-1, 16)
    a, b, m, rc2 = cell_geometry(box, dims)
    w = np.empty((len(a), len(recs)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k, r in enumerate(recs):
            kind, pos, axis, I, cos_o = int(r[0]), r[1:4], r[4:7], r[7:10], r[11]
            Y = (I[0] + I[1]) + I[2]
            if kind == 2:
                w[:, k] = Y
                continue
            p = pos[None, :]
            t = np.where(p < a, a - p, np.where(p > b, p - b, 0.0))
            dmin2 = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
            wk = Y / (dmin2 + rc2)
            if kind == 1:
                v = m - p
                d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
                d = np.sqrt(d2)
                sa = np.sqrt(rc2) / d
                ca = np.sqrt(1.0 - sa * sa)
                c_m = ((v[:, 0] * axis[0] + v[:, 1] * axis[1]) + v[:, 2] * axis[2]) / d
                so = np.sqrt(max(0.0, 1.0 - cos_o * cos_o))
                c_far = cos_o * ca - so * sa
                cull = (d2 > rc2) & (cos_o > -ca) & (c_m < c_far - 1e-9)
                wk = np.where(cull, 0.0, wk)
            w[:, k] = wk
    return w


def table(recs16, box, dims):
    """C[cell, k]: every cell's CDF over the list"""
    w = weights(recs16, box, dims)
    cells, n = w.shape
    W = np.zeros(cells)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            W = W + w[:, k]
        by_weight = np.isfinite(W) & (W > 0.0)
        C = np.zeros(cells)
        T = np.empty((cells, n))
        for k in range(n):
            p = np.where(by_weight, 0.875 * (w[:, k] / W) + FLOOR_SHARE / float(n), 1.0 / float(n))
            C = C + p
            T[:, k] = C
    T[:, n - 1] = 1.0
    return T


def probabilities(T):
    """p[cell, k] = C[k] - C[k-1], as the selection forms it"""
    return T - np.concatenate([np.zeros((len(T), 1)), T[:, :-1]], axis=1)


def cell_of(box, dims, x):
    box = np.asarray(box, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    i = []
    with np.errstate(invalid="ignore", over="ignore"):
        for ax in range(3):
            n_axis = int(dims[ax])
            lo, hi = box[ax], box[3 + ax]
            inv = float(n_axis) / (hi - lo) if hi > lo else 0.0
            q = (x[:, ax] - lo) * inv
            inside = (q >= 0.0) & (q < float(n_axis))
            i.append(np.where(q >= 0.0, np.where(q < float(n_axis), np.where(inside, q, 0.0).astype(np.int64), n_axis - 1), 0))
    return (i[2] * int(dims[1]) + i[1]) * int(dims[0]) + i[0]


def select(box, dims, T, x, u):
    """(cell, k, p): k the smallest index with u < C[cell, k]"""
    cell = cell_of(box, dims, x)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    k = np.zeros(len(u), dtype=np.int64)
    for c in np.unique(cell):
        sel = cell == c
        k[sel] = np.searchsorted(T[c], u[sel], side="right")              # the number of C <= u (rows are non-decreasing and end at 1 > u)
    ck = T[cell, k]
    prev = np.where(k > 0, T[cell, np.maximum(k - 1, 0)], 0.0)
    return cell, k, ck - prev


def branch_throughput(thr, e, E, f, p):
    """thr' = ((thr * e) * E) / pm with pm = f * p"""
    pm = f * p
    return ((thr * e) * E) / (pm[..., None] if np.ndim(pm) else pm)


def variance(c, p, f):
    """The exact per-sample variance of the punctual estimator at points with contributions c[point, k] (= e * E_k, one channel) under
    probabilities p[point, k] and the branch's share f: sum_k c_k^2 / (f p_k) - S^2 with S = sum_k c_k."""
    S = c.sum(axis=1)
    return (c * c / (f * p)).sum(axis=1) - S * S
