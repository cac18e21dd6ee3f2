"""The tessellation and displacement rule (include/pt_amd.h, "mesh tessellation and displacement mapping") restated in numpy from the
printed rule: np.unique on the edge keys, per-vertex sums in corner order. Reads nothing of the product. float32 arrays in, float32
arrays out; all arithmetic in float64 with one rounding to float32 per written attribute. Also the small meshes the tests share."""
import numpy as np

f32, f64 = np.float32, np.float64


def _norm(s):
    """(ok, s / L) with L = sqrt((x x + y y) + z z), ok where L is finite and > 0"""
    with np.errstate(all="ignore"):
        L = np.sqrt((s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2])
        ok = np.isfinite(L) & (L > 0.0)
        return ok, s / np.where(ok, L, 1.0)[..., None]


def subdivide(pos, idx, nrm, uv):
    tri = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    n = len(pos)
    ends = np.stack([tri, np.roll(tri, -1, axis=1)], axis=-1)            # (F, 3, 2): e0 = (a, b), e1 = (b, c), e2 = (c, a)
    keys = (ends.min(axis=-1).astype(np.uint64) << np.uint64(32)) | ends.max(axis=-1).astype(np.uint64)
    uniq, rank = np.unique(keys.reshape(-1), return_inverse=True)
    mid = (n + rank.reshape(-1, 3)).astype(np.int64)
    lo, hi = (uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64)
    with np.errstate(all="ignore"):
        half = lambda a: ((a[lo].astype(f64) + a[hi].astype(f64)) * 0.5).astype(f32)
        pos2 = np.concatenate([pos, half(pos)])
        uv2 = None if uv is None else np.concatenate([uv, half(uv)])
        nrm2 = None
        if nrm is not None:
            ok, unit = _norm(nrm[lo].astype(f64) + nrm[hi].astype(f64))
            nrm2 = np.concatenate([nrm, np.where(ok[:, None], unit.astype(f32), nrm[lo])])
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
    kids = np.stack([a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca], axis=1)
    return pos2, kids.reshape(-1).astype(np.uint32), nrm2, uv2


def smooth_normals(pos, idx, prev):
    tri = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    p = pos.astype(f64)
    with np.errstate(all="ignore"):
        cf = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
        total = np.zeros((len(pos), 3), f64)
        for f in range(len(tri)):          # corners 3f + k in ascending order: each vertex's sum grows in that order
            for k in range(3):
                total[tri[f, k]] = total[tri[f, k]] + cf[f]
        ok, unit = _norm(total)
    fallback = prev if prev is not None else np.tile(np.array([0, 1, 0], f32), (len(pos), 1))
    return np.where(ok[:, None], unit.astype(f32), fallback)


def _axis(t, n, wrap, flip):
    t = t - np.floor(t) if wrap == "repeat" else np.clip(t, 0.0, 1.0)
    x = ((1.0 - t) if flip else t) * n - 0.5
    i0 = np.floor(x)
    w = x - i0
    i0 = i0.astype(np.int64)
    i1 = i0 + 1
    if wrap == "repeat":
        return np.mod(i0, n), np.mod(i1, n), w
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w


def offsets(uv, height, scale, midlevel, wrap):
    """d per vertex"""
    H, W = height.shape
    u, v = uv[:, 0].astype(f64), uv[:, 1].astype(f64)
    fin = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(fin, u, 0.0), np.where(fin, v, 0.0)
    i0, i1, tx = _axis(u, W, wrap, False)
    j0, j1, ty = _axis(v, H, wrap, True)
    h = height.astype(f64)
    with np.errstate(all="ignore"):
        hh = (h[j0, i0] * (1.0 - tx) + h[j0, i1] * tx) * (1.0 - ty) + (h[j1, i0] * (1.0 - tx) + h[j1, i1] * tx) * ty
        d = scale * (hh - midlevel)
    return np.where(fin & np.isfinite(hh), d, 0.0)


def tessellate(pos, idx, nrm=None, uv=None, levels=1, height=None, scale=1.0, midlevel=0.5, wrap="clamp", normals="auto"):
    pos = np.asarray(pos, f32).reshape(-1, 3)
    idx = np.asarray(idx, np.uint32).reshape(-1)
    fit = lambda a, k: None if a is None else np.concatenate([np.asarray(a, f32).reshape(-1, k), np.zeros((len(pos), k), f32)])[: len(pos)]
    nrm, uv = fit(nrm, 3), fit(uv, 2)
    for _ in range(levels):
        pos, idx, nrm, uv = subdivide(pos, idx, nrm, uv)
    if height is not None:
        if nrm is None:
            nrm = smooth_normals(pos, idx, None)
        d = offsets(uv, np.asarray(height, f32), float(scale), float(midlevel), wrap)
        with np.errstate(all="ignore"):
            pos = (pos.astype(f64) + nrm.astype(f64) * d[:, None]).astype(f32)
    if normals == "auto":
        normals = "smooth" if height is not None else "keep"
    if normals == "smooth":
        nrm = smooth_normals(pos, idx, nrm)
    elif normals == "none":
        nrm = None
    return pos, idx, nrm, uv


def mesh_grid(q, u, v, nu, nv):
    q, u, v = (np.asarray(a, f64) for a in (q, u, v))
    j, i = np.meshgrid(np.arange(nv + 1), np.arange(nu + 1), indexing="ij")
    s, t = (i / nu).reshape(-1), (j / nv).reshape(-1)
    pos = ((q[None, :] + u[None, :] * s[:, None]) + v[None, :] * t[:, None]).astype(f32)
    _, unit = _norm(np.cross(u, v))
    v00 = (j[:-1, :-1] * (nu + 1) + i[:-1, :-1]).reshape(-1)
    v10, v01 = v00 + 1, v00 + nu + 1
    v11 = v01 + 1
    idx = np.stack([v00, v10, v11, v00, v11, v01], axis=1).reshape(-1).astype(np.uint32)
    return pos, idx, np.tile(unit.astype(f32), (len(pos), 1)), np.stack([s, t], axis=1).astype(f32)


# ---- the shapes the CPU and GPU tests share: name -> (pos, idx, nrm | None, uv | None) ----
def _unit(a):
    a = np.asarray(a, f64)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(f32)


def shapes():
    out = {}
    tri = np.array([[0, 0, 0], [1, 0, 0.25], [0.3, 1, 0]], f32)
    out["triangle"] = (tri, [0, 1, 2], _unit([[0, 0, 1], [0.2, 0, 1], [0, 0.3, 1]]), np.array([[0, 0], [1, 0], [0.3, 1]], f32))
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]], f32)
    out["pair_consistent"] = (quad, [0, 1, 2, 0, 2, 3], None, quad[:, :2].copy())
    out["pair_opposed"] = (quad, [0, 1, 2, 3, 2, 0], None, None)
    tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], f32)
    out["tetrahedron"] = (tet, [0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2], _unit(tet), None)
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    out["octahedron"] = (octa, [0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5], None, None)
    fin = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [-1, 0.5, 0], [0, -1, 0]], f32)
    out["three_faces_one_edge"] = (fin, [0, 1, 2, 0, 1, 3, 1, 0, 4], None, fin[:, :2].copy())
    out["face_aab"] = (tri, [0, 0, 1, 0, 1, 2], out["triangle"][2], out["triangle"][3])
    spare = np.concatenate([np.array([[9, 9, 9]], f32), tri, np.array([[7, 7, 7], [5, 5, 5]], f32)])
    out["unreferenced"] = (spare, [1, 2, 3], _unit([[1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 1, 0]]), np.arange(12, dtype=f32).reshape(6, 2) / 12)
    out["opposite_normals"] = (tri, [0, 1, 2], np.array([[0, 0, 1], [0, 0, -1], [0, 1, 0]], f32), None)
    # two coincident faces of opposite winding: every vertex's face normals cancel
    out["cancelling"] = (tri, [0, 1, 2, 0, 2, 1], np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], f32), None)
    for nu, nv in ((1, 1), (3, 2), (8, 4)):
        out[f"grid_{nu}x{nv}"] = mesh_grid((-1.0, 0.25, 2.0), (2.0, 0.0, 0.5), (0.0, 0.1, -3.0), nu, nv)
    return out


def strip(n_faces):
    """A triangle strip of n_faces faces: 3 n_faces edge slots"""
    k = np.arange(n_faces + 2)
    pos = np.stack([k // 2 * 0.5, k % 2 * 1.0, np.sin(k * 0.37) * 0.2], axis=1).astype(f32)
    f = np.arange(n_faces)
    tri = np.where((f % 2 == 0)[:, None], np.stack([f, f + 1, f + 2], axis=1), np.stack([f + 1, f, f + 2], axis=1))
    return pos, tri.reshape(-1).astype(np.uint32), None, np.stack([k / (n_faces + 1), k % 2 * 1.0], axis=1).astype(f32)
