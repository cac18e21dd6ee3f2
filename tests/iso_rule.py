"""The isosurface rule of include/pt_amd.h restated in numpy, for the byte-for-byte tests of pt_mesh_isosurface_host.
Marching tetrahedra on the lattice of sample centres: f64 arithmetic on the f32 samples, in the header's order, one rounding to f32 per
written attribute. The case table is not copied from the header: it is derived here from the construction the header states (which edges,
in which order, which diagonal) and the winding property, so a wrong row in either place shows as a difference."""
import numpy as np

import tess_rule as R

# the six tetrahedra of the Kuhn split around the diagonal 0-7, cube corners numbered x + 2y + 4z
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
LOCAL_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)


def tet_positive(t):
    p = [corner_xyz(c) for c in TETS[t]]
    return int(round(np.linalg.det(np.array([p[1] - p[0], p[2] - p[0], p[3] - p[0]], dtype=np.float64)))) > 0


def _edge(a, b):
    return LOCAL_EDGES.index((min(a, b), max(a, b)))


def _derive_table():
    """Rows for a tetrahedron whose corners (v0, v1, v2, v3) have det(v1 - v0, v2 - v0, v3 - v0) > 0; bit l of the row number is set when
    corner l is inside. A tetrahedron of the other orientation swaps the second and third vertex of every triangle."""
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], dtype=np.float64)   # tetrahedron 0 itself
    mid = lambda e: 0.5 * (P[LOCAL_EDGES[e][0]] + P[LOCAL_EDGES[e][1]])
    table = []
    for m in range(16):
        ins = [l for l in range(4) if m >> l & 1]
        out = [l for l in range(4) if not m >> l & 1]
        tris = []
        if len(ins) in (1, 3):
            a = ins[0] if len(ins) == 1 else out[0]
            b, c, d = [l for l in range(4) if l != a]
            tris = [[_edge(a, b), _edge(a, c), _edge(a, d)]]
        elif len(ins) == 2:
            (a, b), (c, d) = ins, out
            tris = [[_edge(a, c), _edge(a, d), _edge(b, d)], [_edge(a, c), _edge(b, d), _edge(b, c)]]
        rows = []
        for t in tris:
            want = P[out].mean(axis=0) - P[ins].mean(axis=0)
            if np.dot(np.cross(mid(t[1]) - mid(t[0]), mid(t[2]) - mid(t[0])), want) < 0:
                t = [t[0], t[2], t[1]]
            assert np.dot(np.cross(mid(t[1]) - mid(t[0]), mid(t[2]) - mid(t[0])), want) > 0
            rows.append(tuple(t))
        table.append(tuple(rows))
    return tuple(table)


TABLE = _derive_table()
TET_POSITIVE = tuple(tet_positive(t) for t in range(6))


def lattice(values, closed, outside):
    v = np.ascontiguousarray(values, dtype=np.float32)
    assert v.ndim == 3                      # indexed [k, j, i]
    if closed:
        v = np.pad(v, 1, constant_values=np.float32(outside))
    return v, (1 if closed else 0)


def axis_positions(n, lo, hi, N, pad):
    h = (np.float64(hi) - np.float64(lo)) / np.float64(n)
    return np.float64(lo) + ((np.arange(N, dtype=np.int64) - pad).astype(np.float64) + 0.5) * h, h


def _normalise(N):
    with np.errstate(all="ignore"):
        L = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        ok = np.isfinite(L) & (L > 0)
        out = np.zeros((len(N), 3), dtype=np.float32)
        out[:, 1] = 1.0
        out[ok] = (N[ok] / L[ok, None]).astype(np.float32)
    return out


def gradient(V, h):
    """Per lattice point and axis: central difference over 2h where both neighbours exist, one-sided over h at the lattice's ends"""
    V = V.astype(np.float64)
    g = []
    for axis, ha in ((2, h[0]), (1, h[1]), (0, h[2])):
        W = np.moveaxis(V, axis, 0)
        G = np.empty_like(W)
        G[1:-1] = (W[2:] - W[:-2]) / (2.0 * ha)
        G[0] = (W[1] - W[0]) / ha
        G[-1] = (W[-1] - W[-2]) / ha
        g.append(np.moveaxis(G, 0, axis))
    return np.stack(g, axis=-1)            # [k, j, i, axis x y z]


def isosurface(values, box_lo, box_hi, iso=0.5, closed=False, outside=0.0, normals="gradient"):
    """-> (pos (n, 3) f32, idx (3F,) u32, nrm (n, 3) f32 or None)"""
    nz, ny, nx = np.shape(values)
    V, pad = lattice(values, closed, outside)
    NZ, NY, NX = V.shape
    iso = np.float64(iso)
    X, hx = axis_positions(nx, box_lo[0], box_hi[0], NX, pad)
    Y, hy = axis_positions(ny, box_lo[1], box_hi[1], NY, pad)
    Z, hz = axis_positions(nz, box_lo[2], box_hi[2], NZ, pad)
    inside = V.astype(np.float64) >= iso
    lin = np.arange(NX * NY * NZ, dtype=np.int64).reshape(NZ, NY, NX)

    # crossing edges, in ascending (A, kind) order: kind d = dx + 2 dy + 4 dz, which is ascending B for a fixed A
    As, Bs, kinds = [], [], []
    for d in range(1, 8):
        dx, dy, dz = d & 1, (d >> 1) & 1, (d >> 2) & 1
        a = (slice(0, NZ - dz), slice(0, NY - dy), slice(0, NX - dx))
        b = (slice(dz, NZ), slice(dy, NY), slice(dx, NX))
        cross = inside[a] != inside[b]
        As.append(lin[a][cross])
        Bs.append(lin[b][cross])
        kinds.append(np.full(int(cross.sum()), d, dtype=np.int64))
    A, B, kind = np.concatenate(As), np.concatenate(Bs), np.concatenate(kinds)
    order = np.lexsort((B, A))
    A, B, kind = A[order], B[order], kind[order]
    assert np.all(np.diff(A * 8 + kind) > 0)          # (A, B) order is (A, kind) order
    n = len(A)
    vertex_of = {(int(a), int(k)): r for r, (a, k) in enumerate(zip(A, kind))}

    def coords(p):
        return p % NX, (p // NX) % NY, p // (NX * NY)

    ai, aj, ak = coords(A)
    bi, bj, bk = coords(B)
    Vf = V.astype(np.float64).reshape(-1)
    va, vb = Vf[A], Vf[B]
    t = (iso - va) / (vb - va)
    PA = np.stack([X[ai], Y[aj], Z[ak]], axis=1)
    PB = np.stack([X[bi], Y[bj], Z[bk]], axis=1)
    pos = (PA + (PB - PA) * t[:, None]).astype(np.float32)

    # triangles: cubes in ascending order of their anchor's linear index, tetrahedra 0..5, triangles 0..1
    idx = []
    offs = [int(c & 1) + int((c >> 1) & 1) * NX + int((c >> 2) & 1) * NX * NY for c in range(8)]
    ins_flat = inside.reshape(-1)
    anchors = lin[:NZ - 1, :NY - 1, :NX - 1].reshape(-1)
    corner_in = np.stack([ins_flat[anchors + o] for o in offs], axis=1)
    mixed = np.flatnonzero(corner_in.any(axis=1) & ~corner_in.all(axis=1))
    for row in mixed:
        p = int(anchors[row])
        for ti, tet in enumerate(TETS):
            m = sum(int(corner_in[row, c]) << l for l, c in enumerate(tet))
            for tri in TABLE[m]:
                vs = []
                for e in tri:
                    la, lb = LOCAL_EDGES[e]
                    ca, cb = tet[la], tet[lb]                   # ca < cb, and ca's bits are among cb's
                    vs.append(vertex_of[(p + offs[ca], cb - ca)])
                if not TET_POSITIVE[ti]:
                    vs = [vs[0], vs[2], vs[1]]
                idx.extend(vs)
    idx = np.array(idx, dtype=np.uint32)

    if normals in ("none", 2):
        nrm = None
    elif normals in ("gradient", 0):
        g = gradient(V, (hx, hy, hz)).reshape(-1, 3)
        G = g[A] + (g[B] - g[A]) * t[:, None]
        nrm = _normalise(-G)
    else:
        nrm = R.smooth_normals(pos, idx, None) if n else np.zeros((0, 3), np.float32)
    return pos, idx, nrm


# ---- test fields ------------------------------------------------------------------------------------------------------------------------
def centres(n, lo, hi):
    """The sample positions of an (nx, ny, nz) grid over the box, as [k, j, i, 3] f64"""
    ax = [np.float64(lo[a]) + (np.arange(n[a], dtype=np.float64) + 0.5) * ((np.float64(hi[a]) - np.float64(lo[a])) / n[a]) for a in range(3)]
    Zs, Ys, Xs = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([Xs, Ys, Zs], axis=-1)


def sphere_field(n, lo, hi, centre, r):
    return (r - np.linalg.norm(centres(n, lo, hi) - np.asarray(centre, np.float64), axis=-1)).astype(np.float32)


def torus_field(n, lo, hi, centre, R0, r0):
    d = centres(n, lo, hi) - np.asarray(centre, np.float64)
    q = np.sqrt(d[..., 0] ** 2 + d[..., 2] ** 2) - R0
    return (r0 - np.sqrt(q * q + d[..., 1] ** 2)).astype(np.float32)
