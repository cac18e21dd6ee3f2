"""The motion rule (pt_instance_moving / pt_scene_set_shutter in include/pt_amd.h) restated in numpy, for the motion tests:
the two lerps as the rule writes them, the pose (pt_instance's operation sequence, with libm's sin / cos), the ray-versus-parallelogram
test of a quad under one instance, and the box rule."""
import numpy as np


def lerp_keys(angle0, angle1, tr0, tr1, time):
    """angle = angle0 + (angle1 - angle0) * time; tr = tr0 + (tr1 - tr0) * time, componentwise; the differences are formed first."""
    da = np.float64(angle1) - np.float64(angle0)
    dtr = np.asarray(tr1, dtype=np.float64) - np.asarray(tr0, dtype=np.float64)
    return np.float64(angle0) + da * np.float64(time), np.asarray(tr0, dtype=np.float64) + dtr * np.float64(time)


def xform_vector(c0, c1, c2, v):
    r = c0 * v[0]
    r = c1 * v[1] + r
    return c2 * v[2] + r


def pose(axis, angle, tr):
    """Instance::new(axis, angle, tr): rows c0, c1, c2, t, i0, i1, i2, it (InstD's order), shape (8, 3)."""
    axis, tr = np.asarray(axis, dtype=np.float64), np.asarray(tr, dtype=np.float64)
    sn, cs = np.sin(angle * 0.5), np.cos(angle * 0.5)
    qx, qy, qz = axis * sn
    qw = cs
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz = qx * x2, qx * y2, qx * z2
    yy, yz, zz = qy * y2, qy * z2, qz * z2
    wx, wy, wz = qw * x2, qw * y2, qw * z2
    c0 = np.array([1.0 - (yy + zz), xy + wz, xz - wy])
    c1 = np.array([xy - wz, 1.0 - (xx + zz), yz + wx])
    c2 = np.array([xz + wy, yz - wx, 1.0 - (xx + yy)])
    i0, i1, i2 = np.array([c0[0], c1[0], c2[0]]), np.array([c0[1], c1[1], c2[1]]), np.array([c0[2], c1[2], c2[2]])
    it = -xform_vector(i0, i1, i2, tr)
    return np.stack([c0, c1, c2, tr, i0, i1, i2, it])


def pose_at(axis, angle0, angle1, tr0, tr1, time):
    angle, tr = lerp_keys(angle0, angle1, tr0, tr1, time)
    return pose(axis, angle, tr)


def to_world(P, p):
    """points (n, 3) of the instance's object space -> world"""
    p = np.asarray(p, dtype=np.float64)
    r = P[0] * p[..., 0:1]                     # glam's transform_point3, column by column: t + (c2 * z + (c1 * y + c0 * x))
    r = P[1] * p[..., 1:2] + r
    r = P[2] * p[..., 2:3] + r
    return P[3] + r


def hit_parallelogram(q, u, v, P, origin, direction, t_min=1e-3):
    """A quad (q, u, v) under ONE instance of pose P against a world ray, as the kernels do it (instance.rs:36-38, quad.rs:40-59):
    returns (hit, margin): margin = how far the decisive quantities are from the test's edges — alpha, beta from 0 and 1, |n . d| from
    1e-8, t from t_min — so that a caller can leave out the samples rounding could decide."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in (q, u, v))
    o = P[7] + xform_vector(P[4], P[5], P[6], np.asarray(origin, dtype=np.float64))
    d = xform_vector(P[4], P[5], P[6], np.asarray(direction, dtype=np.float64))
    d = d * (1.0 / np.sqrt(d @ d))
    n = np.cross(u, v)
    normal = n * (1.0 / np.sqrt(n @ n))
    w = n / (n @ n)
    nd = normal @ d
    if abs(nd) < 1e-8:
        return False, abs(abs(nd) - 1e-8)
    t = (normal @ q - normal @ o) / nd
    p = o + d * t - q
    alpha, beta = w @ np.cross(p, v), w @ np.cross(u, p)
    margin = min(abs(alpha), abs(alpha - 1.0), abs(beta), abs(beta - 1.0), abs(t - t_min), abs(abs(nd) - 1e-8))
    return bool(t >= t_min and 0.0 <= alpha <= 1.0 and 0.0 <= beta <= 1.0), margin


def corners(box):
    box = np.asarray(box, dtype=np.float64)
    return np.array([[box[3 if i & 1 else 0], box[4 if i & 2 else 1], box[5 if i & 4 else 2]] for i in range(8)])


def xform_box(box, P):
    w = to_world(P, corners(box))
    return np.concatenate([w.min(axis=0), w.max(axis=0)])


def union(a, b):
    return np.concatenate([np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])])


def swept_box(box, axis, angle0, angle1, tr0, tr1):
    """One level of the box rule. Translates only: the union of the transformed box at times 0 and 1. Spins: rho = the largest corner
    norm (widened by 1e-14 relative), the union of tr(0) +- rho and tr(1) +- rho, widened by four ulps of its largest coordinate."""
    if angle0 == angle1:
        return union(xform_box(box, pose_at(axis, angle0, angle1, tr0, tr1, 0.0)), xform_box(box, pose_at(axis, angle0, angle1, tr0, tr1, 1.0)))
    rho = np.sqrt((corners(box) ** 2).sum(axis=1)).max() * (1.0 + 1e-14)
    t0, t1 = lerp_keys(angle0, angle1, tr0, tr1, 0.0)[1], lerp_keys(angle0, angle1, tr0, tr1, 1.0)[1]
    r = np.concatenate([np.minimum(t0, t1) - rho, np.maximum(t0, t1) + rho])
    pad = np.abs(r).max() * (4.0 * np.finfo(np.float64).eps)
    return np.concatenate([r[:3] - pad, r[3:] + pad])


# ---- the same, over arrays of times (the blur test decides hundreds of thousands of samples) ------------------------------------------
def poses_at(axis, angle0, angle1, tr0, tr1, times):
    """pose_at for an array of n times: (n, 8, 3), entry for entry the same operations."""
    axis = np.asarray(axis, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    da = np.float64(angle1) - np.float64(angle0)
    dtr = np.asarray(tr1, dtype=np.float64) - np.asarray(tr0, dtype=np.float64)
    angle = np.float64(angle0) + da * times
    tr = np.asarray(tr0, dtype=np.float64)[None, :] + dtr[None, :] * times[:, None]
    sn, cs = np.sin(angle * 0.5), np.cos(angle * 0.5)
    qx, qy, qz, qw = axis[0] * sn, axis[1] * sn, axis[2] * sn, cs
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz = qx * x2, qx * y2, qx * z2
    yy, yz, zz = qy * y2, qy * z2, qz * z2
    wx, wy, wz = qw * x2, qw * y2, qw * z2
    c0 = np.stack([1.0 - (yy + zz), xy + wz, xz - wy], axis=1)
    c1 = np.stack([xy - wz, 1.0 - (xx + zz), yz + wx], axis=1)
    c2 = np.stack([xz + wy, yz - wx, 1.0 - (xx + yy)], axis=1)
    i0, i1, i2 = np.stack([c0[:, 0], c1[:, 0], c2[:, 0]], axis=1), np.stack([c0[:, 1], c1[:, 1], c2[:, 1]], axis=1), np.stack([c0[:, 2], c1[:, 2], c2[:, 2]], axis=1)
    it = -xform_vectors(i0, i1, i2, tr)
    return np.stack([c0, c1, c2, tr, i0, i1, i2, it], axis=1)


def xform_vectors(c0, c1, c2, v):
    r = c0 * v[:, 0:1]
    r = c1 * v[:, 1:2] + r
    return c2 * v[:, 2:3] + r


def hit_parallelogram_many(q, u, v, P, origins, directions, t_min=1e-3):
    """hit_parallelogram for n rays, ray i under the pose P[i]: (hit (n,) bool, margin (n,))."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in (q, u, v))
    o = P[:, 7] + xform_vectors(P[:, 4], P[:, 5], P[:, 6], np.asarray(origins, dtype=np.float64))
    d = xform_vectors(P[:, 4], P[:, 5], P[:, 6], np.asarray(directions, dtype=np.float64))
    d = d * (1.0 / np.sqrt((d * d).sum(axis=1)))[:, None]
    n = np.cross(u, v)
    normal = n * (1.0 / np.sqrt(n @ n))
    w = n / (n @ n)
    nd = d @ normal
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (normal @ q - o @ normal) / nd
        p = o + d * t[:, None] - q
        alpha, beta = np.cross(p, v) @ w, np.cross(u, p) @ w
        margin = np.minimum.reduce([np.abs(alpha), np.abs(alpha - 1.0), np.abs(beta), np.abs(beta - 1.0), np.abs(t - t_min)])
        hit = (np.abs(nd) >= 1e-8) & (t >= t_min) & (alpha >= 0.0) & (alpha <= 1.0) & (beta >= 0.0) & (beta <= 1.0)
    margin = np.where(np.isfinite(margin), np.minimum(margin, np.abs(np.abs(nd) - 1e-8)), 0.0)
    return hit, margin
