"""The rule of mesh voxelisation (include/pt_amd.h) restated in numpy.

winding(): the sign rule exactly as the header writes it, every triangle against every column at once (f64, the header's operation
order), so the integers must match the product's exactly.

distance(): NOT a transcription of the header's walk through the Voronoi regions. The distance from a point to a triangle is the
minimum of (a) the distance to the triangle's plane, where the point's projection falls inside the triangle, and (b) the distances to
its three segments. Both are f64 evaluations of the same exact quantity, so the product, rounded to f32, may differ from this by
ulp_f32(ref) + 1e-12 * |box diagonal| (tolerance()): an f32 rounding boundary plus an absolute f64 cancellation error."""
import numpy as np


def coords(n, lo, hi):
    """The sample centres along one axis: lo + ((double)i + 0.5) * h"""
    h = (np.float64(hi) - np.float64(lo)) / np.float64(n)
    return np.float64(lo) + (np.arange(n, dtype=np.float64) + 0.5) * h


def _edge(Uy, Uz, Vy, Vz, Py, Pz):
    """Steps 1-4 for arrays of edges [T, 1] against columns [1, C] -> (side, value)"""
    swapped = (Vy < Uy) | ((Vy == Uy) & (Vz < Uz))
    Uy2, Vy2 = np.where(swapped, Vy, Uy), np.where(swapped, Uy, Vy)
    Uz2, Vz2 = np.where(swapped, Vz, Uz), np.where(swapped, Uz, Vz)
    dy, dz = Vy2 - Uy2, Vz2 - Uz2
    e = dy * (Pz - Uz2) - dz * (Py - Uy2)
    s = np.where((e > 0) | ((e == 0) & ((dz < 0) | ((dz == 0) & (dy > 0)))), 1, -1)
    return np.where(swapped, -s, s), np.where(swapped, -e, e)


def winding(pos, idx, dims, lo, hi):
    """-> int32 [nz, ny, nx]: the winding number of every sample"""
    nx, ny, nz = dims
    P = np.asarray(pos, np.float32).astype(np.float64)
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    x, y, z = coords(nx, lo[0], hi[0]), coords(ny, lo[1], hi[1]), coords(nz, lo[2], hi[2])
    Pz, Py = (a.reshape(1, -1) for a in np.meshgrid(z, y, indexing="ij"))           # columns in (k, j) order
    out = np.zeros((nz * ny, nx), np.int32)
    for t0 in range(0, len(tri), 64):                                               # (blocks of triangles keep the arrays small)
        A, B, Cc = (P[tri[t0:t0 + 64, c]][:, :, None] for c in range(3))            # [T, 3, 1]
        ylo, yhi = np.minimum(np.minimum(A[:, 1], B[:, 1]), Cc[:, 1]), np.maximum(np.maximum(A[:, 1], B[:, 1]), Cc[:, 1])
        zlo, zhi = np.minimum(np.minimum(A[:, 2], B[:, 2]), Cc[:, 2]), np.maximum(np.maximum(A[:, 2], B[:, 2]), Cc[:, 2])
        in_box = (Py >= ylo) & (Py <= yhi) & (Pz >= zlo) & (Pz <= zhi)
        sc, wc = _edge(A[:, 1], A[:, 2], B[:, 1], B[:, 2], Py, Pz)
        sa, wa = _edge(B[:, 1], B[:, 2], Cc[:, 1], Cc[:, 2], Py, Pz)
        sb, wb = _edge(Cc[:, 1], Cc[:, 2], A[:, 1], A[:, 2], Py, Pz)
        den = (wa + wb) + wc
        with np.errstate(all="ignore"):
            xs = ((wa * A[:, 0] + wb * B[:, 0]) + wc * Cc[:, 0]) / den
        cross = in_box & (sa == sb) & (sb == sc) & (den != 0) & np.isfinite(xs)
        for t, c in zip(*np.nonzero(cross)):
            m = int(np.count_nonzero(x < xs[t, c]))
            out[c, :m] += sa[t, c]
    return out.reshape(nz, ny, nx)


def inside(w, fill="nonzero"):
    return (w != 0) if fill in ("nonzero", 0) else (w % 2 != 0)


def kept(pos, idx):
    """The triangles the distance pass keeps: no repeated index, n.n != 0"""
    P = np.asarray(pos, np.float32).astype(np.float64)
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    n = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
    ok = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0]) & ((n * n).sum(axis=1) != 0)
    return tri[ok]


def _segment(Q, U, V):
    """Distances from points Q [S, 1, 3] to segments U V [1, T, 3]"""
    d = V - U
    L = (d * d).sum(axis=2)
    with np.errstate(all="ignore"):
        t = np.clip(((Q - U) * d).sum(axis=2) / L, 0.0, 1.0)
    t = np.where(L > 0, t, 0.0)
    r = Q - (U + d * t[:, :, None])
    return np.sqrt((r * r).sum(axis=2))


def point_distance(points, pos, idx):
    """The distance from each of `points` [S, 3] to the mesh: plane where the projection is inside, else the three segments"""
    P = np.asarray(pos, np.float32).astype(np.float64)
    tri = kept(pos, idx)
    A, B, Cc = P[tri[:, 0]][None], P[tri[:, 1]][None], P[tri[:, 2]][None]          # [1, T, 3]
    n = np.cross(B - A, Cc - A)
    nn = (n * n).sum(axis=2)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.empty(len(points))
    step = max(1, 400000 // max(1, len(tri)))
    for s0 in range(0, len(points), step):
        Q = points[s0:s0 + step, None, :]                                           # [S, 1, 3]
        best = np.minimum(np.minimum(_segment(Q, A, B), _segment(Q, B, Cc)), _segment(Q, Cc, A))
        # the projection is inside when it lies on the inner side of all three edges: n . ((V - U) x (Q - U)) >= 0
        within = np.ones(best.shape, bool)
        for U, V in ((A, B), (B, Cc), (Cc, A)):
            within &= (np.cross(V - U, Q - U) * n).sum(axis=2) >= 0
        plane = np.abs(((Q - A) * n).sum(axis=2)) / np.sqrt(nn)
        best = np.where(within, np.minimum(best, plane), best)
        out[s0:s0 + step] = best.min(axis=1)
    return out


def point_distance_within(points, pos, idx, reach, blocks=5):
    """point_distance where it is at most `reach`, some value above `reach` elsewhere: the points are taken block by block of their
    bounding box, each against the triangles whose own box comes within `reach` of the block (a triangle that holds a point within
    `reach` of a sample is among them)."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    P = np.asarray(pos, np.float32).astype(np.float64)
    tri = kept(pos, idx)
    tlo, thi = P[tri].min(axis=1), P[tri].max(axis=1)
    lo, hi = points.min(axis=0), points.max(axis=0)
    cell = np.floor((points - lo) / np.where(hi > lo, hi - lo, 1.0) * blocks).clip(0, blocks - 1).astype(np.int64)
    key = (cell[:, 2] * blocks + cell[:, 1]) * blocks + cell[:, 0]
    out = np.full(len(points), np.inf)
    for b in np.unique(key):
        mine = np.flatnonzero(key == b)
        blo, bhi = points[mine].min(axis=0) - reach, points[mine].max(axis=0) + reach
        near = np.all((thi >= blo) & (tlo <= bhi), axis=1)
        if near.any():
            out[mine] = point_distance(points[mine], pos, tri[near].reshape(-1))
    return out


def grid_points(dims, lo, hi):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(coords(nz, lo[2], hi[2]), coords(ny, lo[1], hi[1]), coords(nx, lo[0], hi[0]), indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3)


def distance(pos, idx, dims, lo, hi):
    """-> f64 [nz, ny, nx]: the distance of every sample centre to the mesh"""
    nx, ny, nz = dims
    return point_distance(grid_points(dims, lo, hi), pos, idx).reshape(nz, ny, nx)


def ulp_f32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def tolerance(ref, lo, hi):
    diag = float(np.linalg.norm(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    return ulp_f32(ref) + 1e-12 * diag


def depth(pos, idx, dims, lo, hi, fill="nonzero"):
    """-> (f64 depth, positive inside; the winding numbers)"""
    w = winding(pos, idx, dims, lo, hi)
    d = distance(pos, idx, dims, lo, hi)
    return np.where(inside(w, fill), d, -d), w


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------------
def cube(c0, c1):
    """The 12-triangle box [c0, c1], outward normals"""
    c0, c1 = np.asarray(c0, np.float64), np.asarray(c1, np.float64)
    pos = np.array([[(c1 if b & 1 else c0)[0], (c1 if b & 2 else c0)[1], (c1 if b & 4 else c0)[2]] for b in range(8)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # -z +z -y +y -x +x
    idx = np.array([[q[0], q[1], q[2], q[0], q[2], q[3]] for q in quads], np.uint32).reshape(-1)
    return pos, idx


def tetrahedron():
    pos = np.array([[0.1, 0.2, 0.15], [1.3, 0.25, 0.3], [0.4, 1.4, 0.2], [0.5, 0.6, 1.2]], np.float32)
    idx = np.array([0, 2, 1, 0, 1, 3, 1, 2, 3, 2, 0, 3], np.uint32)
    return pos, idx


def octahedron(c=(0.0, 0.0, 0.0), r=1.0):
    c = np.asarray(c, np.float64)
    pos = np.array([c + r * np.array(v) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))], np.float32)
    idx = np.array([0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5], np.uint32)
    return pos, idx


def flipped(idx):
    return np.asarray(idx, np.uint32).reshape(-1, 3)[:, ::-1].reshape(-1).copy()


def merged(*meshes):
    pos, idx, base = [], [], 0
    for p, i in meshes:
        pos.append(np.asarray(p, np.float32))
        idx.append(np.asarray(i, np.uint32) + np.uint32(base))
        base += len(p)
    return np.concatenate(pos), np.concatenate(idx)


def signed_volume(pos, idx):
    p = np.asarray(pos, np.float32).astype(np.float64)[np.asarray(idx, np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
