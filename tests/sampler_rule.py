"""The Sobol sampler's rule (pt_scene_set_sampler in include/pt_amd.h) restated in numpy, for the sampler tests.
Everything is elementwise over arrays; 32-bit words are carried in uint64 and masked."""
import numpy as np

M = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x, dtype=np.uint64)


def rev(x):
    x = _u(x)
    x = ((x >> np.uint64(1)) & np.uint64(0x55555555)) | ((x & np.uint64(0x55555555)) << np.uint64(1))
    x = ((x >> np.uint64(2)) & np.uint64(0x33333333)) | ((x & np.uint64(0x33333333)) << np.uint64(2))
    x = ((x >> np.uint64(4)) & np.uint64(0x0F0F0F0F)) | ((x & np.uint64(0x0F0F0F0F)) << np.uint64(4))
    x = ((x >> np.uint64(8)) & np.uint64(0x00FF00FF)) | ((x & np.uint64(0x00FF00FF)) << np.uint64(8))
    return ((x >> np.uint64(16)) | (x << np.uint64(16))) & M


def lk(x, k):
    x = (_u(x) + _u(k)) & M
    for c in (0x6C50B47C, 0xB82F1E52, 0xC7AFE638, 0x8D22F6E6):
        x = x ^ ((x * np.uint64(c)) & M)
    return x


def owen(x, k):
    return rev(lk(rev(x), k))


def sobol0(i):
    return rev(i)


def sobol1_loop(i):
    """Sobol's second dimension by its direction numbers: v_0 = 1 << 31, v_{b+1} = v_b ^ (v_b >> 1)."""
    i = _u(i).copy()
    x = np.zeros_like(i)
    v = np.uint64(1 << 31)
    for _ in range(32):
        x = x ^ np.where(i & np.uint64(1), v, np.uint64(0))
        i = i >> np.uint64(1)
        v = v ^ (v >> np.uint64(1))
    return x


def sobol1(i):
    """The same map in five steps (the matrix is Pascal's triangle mod 2: the substitution t -> t + 1)."""
    y = _u(i).copy()
    for m, s in ((0xAAAAAAAA, 1), (0xCCCCCCCC, 2), (0xF0F0F0F0, 4), (0xFF00FF00, 8), (0xFFFF0000, 16)):
        y = y ^ ((y & np.uint64(m)) >> np.uint64(s))
    return rev(y)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u(v) & M for v in (c0, c1, c2, c3, k0, k1)))
    M0, M1, W0, W1 = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M, n2, p0 & M
        k0, k1 = (k0 + W0) & M, (k1 + W1) & M
    return c0, c1, c2, c3


def pair_points(s, k0, k1, k2):
    """The two 32-bit coordinates of sample index s under the three keys of one pair."""
    j = owen(s, k0)
    return owen(sobol0(j), k1), owen(sobol1(j), k2)


def sobol_u64(seed, pixel, s, d):
    """The 64-bit value of draw d of sample s of `pixel` under `seed` (kind 1)."""
    s, d = _u(s), _u(d)
    k, c = d >> np.uint64(1), d & np.uint64(1)
    K = philox4x32_10(k, 0, seed >> 32, 1, seed & 0xFFFFFFFF, pixel)
    j = owen(s, K[0])
    x = np.where(c == 0, owen(sobol0(j), K[1]), owen(sobol1(j), K[2]))
    return (x << np.uint64(32)) | lk(x, (K[3] + c) & M)


def independent_u64(seed, pixel, s, d):
    """kind 0: half of the Philox block (d >> 1, s, seed_hi, 0) under the key (seed_lo, pixel)."""
    s, d = _u(s), _u(d)
    o = philox4x32_10(d >> np.uint64(1), s, seed >> 32, 0, seed & 0xFFFFFFFF, pixel)
    odd = (d & np.uint64(1)) == 1
    return np.where(odd, (o[3] << np.uint64(32)) | o[2], (o[1] << np.uint64(32)) | o[0])


def unit(v):
    """u64_to_unit: the top 53 bits as a double in [0, 1)."""
    return (_u(v) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def elementary_interval_violations(x, y, m):
    """Of the 2^m points (x, y) (32-bit coordinates): how many of the m + 1 shapes 2^-p x 2^-(m-p) do NOT hold exactly one point a cell."""
    bad = 0
    for p in range(m + 1):
        q = m - p
        cx = (x >> np.uint64(32 - p)) if p else np.zeros_like(x)
        cy = (y >> np.uint64(32 - q)) if q else np.zeros_like(y)
        if len(np.unique(cx * np.uint64(1 << q) + cy)) != (1 << m):
            bad += 1
    return bad


def camera_locations(frame, blur_strength, width, seed, pixels, samples, sobol=True):
    """generate_ray's sample locations on the image plane for a pinhole camera (defocus_angle 0), in PIXEL coordinates
    (row + bx, col + by): draws 0 and 1 of every (pixel, sample) -> radius = sqrt(u0), angle = 2 pi u1 (camera.rs:133-157).
    Returns two arrays of shape (len(pixels), len(samples))."""
    p = _u(pixels)[:, None]
    s = _u(samples)[None, :]
    f = sobol_u64 if sobol else independent_u64
    u0, u1 = unit(f(seed, p, s, 0)), unit(f(seed, p, s, 1))
    radius, angle = np.sqrt(u0), u1 * 2.0 * np.pi
    bx, by = radius * np.cos(angle) * blur_strength, radius * np.sin(angle) * blur_strength
    rows, cols = np.divmod(np.asarray(pixels, dtype=np.int64), width)
    return rows[:, None] + bx, cols[:, None] + by
