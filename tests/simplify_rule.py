"""The rule of mesh welding and simplification (include/pt_amd.h) restated in numpy from the printed rule: np.unique on
the keys where the product sorts, dictionaries for the face groups, TSUM as reshapes. Reads nothing of the product. float32 arrays in,
float32 arrays out; all arithmetic in float64 with one rounding to float32 per written attribute. Also the meshes the tests share."""
import numpy as np

import tess_rule as R

f32, f64 = np.float32, np.float64
NONE = np.uint32(0xFFFFFFFF)


def tsum(t):
    """TSUM along axis 0 of t [L, ...], L >= 1: tiles of 16 (missing entries +0.0), each a balanced pairwise tree, added in order"""
    t = np.asarray(t, f64)
    L = len(t)
    tiles = -(-L // 16)
    s = np.zeros((tiles * 16,) + t.shape[1:], f64)
    s[:L] = t
    s = s.reshape((tiles, 16) + t.shape[1:])
    for _ in range(4):
        s = s[:, 0::2] + s[:, 1::2]
    acc = s[0, 0]
    for j in range(1, tiles):
        acc = acc + s[j, 0]
    return acc


def solve(q, m, reg, cell):
    """Step 6's regularised minimiser: q = (a00 a01 a02 a11 a12 a22 b0 b1 b2), python floats (IEEE f64, nothing fused) -> (x, used)"""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (float(v) for v in q)
    m = [float(v) for v in m]
    T = (a00 + a11) + a22
    if not (np.isfinite(T) and T > 0.0):
        return m, False
    lam = reg * T
    a00, a11, a22 = a00 + lam, a11 + lam, a22 + lam
    r0, r1, r2 = b0 + lam * m[0], b1 + lam * m[1], b2 + lam * m[2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    if not det > 0.0:
        return m, False
    x = [((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det]
    if not all(np.isfinite(v) and abs(v) <= cell for v in x):
        return m, False
    return x, True


def grid_of(pos, idx, cell=0.0, grid_n=64):
    """(lo, cell) of mode 1"""
    p = np.asarray(pos, f32).astype(f64)[np.unique(np.asarray(idx, np.int64))]
    lo, hi = p.min(axis=0), p.max(axis=0)
    E = float((hi - lo).max())
    return lo, (float(cell) if cell > 0 else E / float(grid_n))


def simplify(pos, idx, uv=None, mode="cluster", cell=0.0, grid_n=64, placement="quadric", reg=1e-3, dedup=True, normals="smooth", stats=None):
    """-> (pos, idx, nrm | None, uv | None, map) as Context.simplify returns them. stats (a dict): the number of clusters and of
    quadric solves that fell back to the mean."""
    P32 = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    P = P32.astype(f64)
    n = len(P)
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    flat = tri.reshape(-1)
    T32 = None
    if uv is not None:
        T32 = np.zeros((n, 2), f32)
        k = min(n, len(uv))
        T32[:k] = np.asarray(uv, f32).reshape(-1, 2)[:k]
    # 1, 2: the referenced vertices and their keys
    rv = np.unique(flat)
    if mode in ("weld", 0):
        rows = (P32[rv] + f32(0.0)).view(np.uint32)                     # -0 + 0 = +0; every other value keeps its bits
        lo = cell_edge = None
    else:
        lo, cell_edge = grid_of(P32, flat, cell, grid_n)
        rows = np.floor((P[rv] - lo) / cell_edge).astype(np.int64)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    # 3: a cluster's id is the rank of its lowest member among the lowest members
    head = np.full(len(uniq), n, np.int64)
    np.minimum.at(head, inv, rv)
    cid = np.empty(len(uniq), np.int64)
    cid[np.argsort(head)] = np.arange(len(uniq))
    C = len(uniq)
    vcl = np.full(n, -1, np.int64)
    vcl[rv] = cid[inv]
    by_cluster = rv[np.argsort(vcl[rv], kind="stable")]                 # members in ascending vertex index within a cluster
    mstart = np.searchsorted(vcl[by_cluster], np.arange(C + 1))
    # 6: placement
    cpos = np.zeros((C, 3), f32)
    cuv = None if T32 is None else np.zeros((C, 2), f32)
    fallbacks = 0
    if mode in ("weld", 0):
        heads = by_cluster[mstart[:-1]]
        cpos[:] = P32[heads]
        if cuv is not None:
            cuv[:] = T32[heads]
    else:
        corner_order = np.argsort(vcl[flat], kind="stable")             # slots ascending within a cluster
        cstart = np.searchsorted(vcl[flat][corner_order], np.arange(C + 1))
        cells = np.empty((C, 3), np.int64)
        cells[cid] = uniq
        for c in range(C):
            mem = by_cluster[mstart[c]:mstart[c + 1]]
            count = float(len(mem))
            o = lo + (cells[c].astype(f64) + 0.5) * cell_edge
            m = tsum((P[mem] - o) / count)
            if cuv is not None:
                cuv[c] = (tsum(T32[mem].astype(f64)) / count).astype(f32)
            x = m
            if placement in ("quadric", 0):
                f = corner_order[cstart[c]:cstart[c + 1]] // 3
                p0, p1, p2 = P[tri[f, 0]] - o, P[tri[f, 1]] - o, P[tri[f, 2]] - o
                e1, e2 = p1 - p0, p2 - p0
                nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
                ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
                nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
                d = (nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2]
                q = tsum(np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d], axis=1))
                x, used = solve(q, m, float(reg), cell_edge)
                fallbacks += 0 if used else 1
            cpos[c] = (o + np.asarray(x, f64)).astype(f32)
    if stats is not None:
        stats.update(clusters=C, fallbacks=fallbacks)
    # 4: the faces
    ids = vcl[tri]
    live = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 2] != ids[:, 0])
    keep = live.copy()
    if dedup:
        keep[:] = False
        groups = {}
        for f in np.flatnonzero(live):
            a, b, c = (int(v) for v in ids[f])
            l, m_, h = sorted((a, b, c))
            even = (a, b, c) in ((l, m_, h), (m_, h, l), (h, l, m_))
            groups.setdefault((l, m_, h), ([], []))[0 if even else 1].append(f)
        for ev, od in groups.values():
            if len(ev) > len(od):
                keep[ev[:len(ev) - len(od)]] = True
            elif len(od) > len(ev):
                keep[od[:len(od) - len(ev)]] = True
    # 5: the output
    used = np.zeros(C, bool)
    used[ids[keep].reshape(-1)] = True
    new = np.cumsum(used) - used
    out_pos = cpos[used]
    out_uv = None if cuv is None else cuv[used]
    out_idx = new[ids[keep]].reshape(-1).astype(np.uint32)
    vmap = np.full(n, NONE, np.uint32)
    ok = (vcl >= 0) & used[np.maximum(vcl, 0)]
    vmap[ok] = new[vcl[ok]].astype(np.uint32)
    nrm = R.smooth_normals(out_pos, out_idx, None) if normals in ("smooth", 0) else None
    return out_pos, out_idx, nrm, out_uv, vmap


# ---- properties --------------------------------------------------------------------------------------------------------------------
def directed_edges(idx):
    use = {}
    for a, b, c in np.asarray(idx, np.int64).reshape(-1, 3):
        for e in ((a, b), (b, c), (c, a)):
            use[e] = use.get(e, 0) + 1
    return use


def assert_balanced(idx):
    """Every directed edge occurs as often as its reverse"""
    use = directed_edges(idx)
    for (a, b), k in use.items():
        assert use.get((b, a), 0) == k, f"edge ({a}, {b}): {k} times, reversed {use.get((b, a), 0)} times"


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def rotation(ax, az):
    """About x by ax, then about z by az"""
    cx, sx, cz, sz = np.cos(ax), np.sin(ax), np.cos(az), np.sin(az)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def grid_cube(k, rot=None):
    """The cube [0, 1]^3 with k x k cells a face, vertices shared across the edges, outward winding -> (pos f32, idx, the rotation)"""
    index, pos, idx = {}, [], []

    def vid(i, j, l):
        if (i, j, l) not in index:
            index[(i, j, l)] = len(pos)
            pos.append((i / k, j / k, l / k))
        return index[(i, j, l)]

    for axis in range(3):
        for side in (0, 1):
            for u in range(k):
                for v in range(k):
                    def at(du, dv):
                        c = [0, 0, 0]
                        c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = side * k, u + du, v + dv
                        return vid(*c)
                    q = (at(0, 0), at(1, 0), at(1, 1), at(0, 1))          # counter-clockwise seen from +axis
                    if side == 0:
                        q = q[::-1]
                    idx += [q[0], q[1], q[2], q[0], q[2], q[3]]
    P = np.array(pos, f64)
    rot = np.eye(3) if rot is None else rot
    return (P @ rot.T).astype(f32), np.array(idx, np.uint32), rot


def cube_surface_distance(points, rot):
    """The distance of points to the surface of the cube [0, 1]^3 rotated by rot"""
    p = np.asarray(points, f64) @ rot                                    # back into the cube's frame (rot is orthogonal)
    q = np.maximum(np.maximum(-p, p - 1.0), 0.0)
    outside = np.sqrt((q * q).sum(axis=1))
    inside = np.minimum(p, 1.0 - p).min(axis=1)
    return np.where(outside > 0, outside, inside)


def exploded(pos, idx, uv=None):
    """Every face with three vertices of its own"""
    flat = np.asarray(idx, np.int64)
    return pos[flat].copy(), np.arange(len(flat), dtype=np.uint32), None if uv is None else uv[flat].copy()


def fan(corners, members=1, cell=0.25):
    """`members` vertices in one cell (the cell at the lower corner of the bounds) and max(corners, members) triangles, triangle i
    from member i % members to the rim vertices i and i + 1, each of which has a cell of its own; one more triangle from a vertex alone
    in a neighbouring cell -> (pos, idx, cell). The first cluster has `members` members and max(corners, members) corners."""
    k = np.arange(members, dtype=f64)
    blob = np.stack([0.1 + 0.8 * ((k * 7) % 13) / 13.0, 0.1 + 0.8 * ((k * 5) % 11) / 11.0, 0.1 + 0.8 * ((k * 3) % 7) / 7.0], axis=1)
    blob[0] = 0.1                                                         # the lower corner of the bounds
    faces = max(corners, members)
    i = np.arange(faces + 1, dtype=f64)
    rim = np.stack([2.0 + 1.5 * i, 1.0 + 0.5 * np.sin(0.37 * i), 0.5 + 0.0 * i], axis=1)
    lone = np.array([[1.5, 0.5, 1.5]])
    pos = (np.concatenate([blob, rim, lone]) * cell).astype(f32)
    r0, l0 = members, members + faces + 1
    f = np.arange(faces)
    idx = np.stack([f % members, r0 + f, r0 + f + 1], axis=1).reshape(-1)
    return pos, np.concatenate([idx, [l0, r0, r0 + 1]]).astype(np.uint32), cell
