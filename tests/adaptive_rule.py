"""The rule of adaptive sampling (include/pt_amd.h, csrc/pt_adaptive.hip) restated in numpy, and the small helpers the pixel-list and
adaptive tests share. adaptive_replay is the yardstick of tests/test_adaptive_gpu.py and tests/test_adaptive_shapes_gpu.py: in the static
mode every round of pt_render_adaptive is the per-pixel sum over a sample range, so the replay over renders of the same ranges gives the
sample counts and the sums bit for bit. tests/test_adaptive_cpu.py checks the replay itself against hand-written outcomes."""
import ctypes as C

import numpy as np


def schedule(m, n):
    b = [0, m // 2, m]
    while b[-1] < n:
        b.append(min(n, b[-1] + max(m // 2, b[-1] // 2)))
    return b


def dilate(bad):
    h, w = bad.shape
    p = np.zeros((h + 2, w + 2), dtype=bool)
    p[1:-1, 1:-1] = bad
    out = np.zeros_like(bad)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def error_estimate(E, O, ne, no):
    """k_adapt_error for every pixel: the two-set error of the sums E over ne samples and O over no samples."""
    with np.errstate(invalid="ignore", divide="ignore"):
        A, B = E / float(ne), O / float(no)
        d = np.abs(A[..., 0] - B[..., 0]) + np.abs(A[..., 1] - B[..., 1]) + np.abs(A[..., 2] - B[..., 2])
        M = (E[..., 0] + O[..., 0] + E[..., 1] + O[..., 1] + E[..., 2] + O[..., 2]) / float(ne + no)
        return d / (1e-4 + np.sqrt(M))


def adaptive_replay(render_range, h, w, m, n, threshold):
    """render_range(lo, hi) -> (h, w, 3) sums of samples [lo, hi) of every pixel. Returns (E + O, counts, stop rounds)."""
    b = schedule(m, n)
    E, O = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    active = np.ones((h, w), dtype=bool)
    stop = np.zeros((h, w), dtype=np.uint32)
    rounds = np.full((h, w), -1)
    ne = no = 0
    for i in range(len(b) - 1):
        if not active.any():
            break
        lo, hi = b[i], b[i + 1]
        r = render_range(lo, hi)
        tgt = E if i % 2 == 0 else O
        tgt[active] += r[active]
        if i % 2 == 0:
            ne += hi - lo
        else:
            no += hi - lo
        if i >= 1 and hi < n:
            err = np.where(active, error_estimate(E, O, ne, no), 0.0)
            keep = active & dilate(~(err < threshold))
            stopping = active & ~keep
            stop[stopping] = hi
            rounds[stopping] = i
            active = keep
    return E + O, np.where(stop > 0, stop, n).astype(np.uint32), rounds


def quantise_counts_np(accum, counts):
    c = accum * (1.0 / counts.astype(np.float64))[..., None]
    g = np.sqrt(np.fmax(c, 0.0))
    g = np.where(g < 0.0, 0.0, g)
    g = np.where(g > 0.999, 0.999, g)
    q = g * 256.0
    return np.where(q != q, 0.0, q).astype(np.uint8)


def tiled_index(h, w):
    """(h, w) array: each pixel's index in the tiled order (8x8 tiles row by row, row-major inside a tile) the select kernels walk."""
    y, x = np.mgrid[0:h, 0:w]
    return ((y >> 3) * ((w + 7) // 8) + (x >> 3)) * 64 + ((y & 7) << 3) + (x & 7)


class DeviceBuffer:
    hip = None

    def __init__(self, host):
        if DeviceBuffer.hip is None:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            DeviceBuffer.hip = hip
        self.nbytes, self.shape, self.dtype = host.nbytes, host.shape, host.dtype
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), host.nbytes) == 0
        assert self.hip.hipMemcpy(self.ptr, host.ctypes.data, host.nbytes, 1) == 0

    def get(self):
        out = np.empty(self.shape, self.dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.ptr)


def sentinel_frame(shape, rng):
    s = rng.uniform(-3.0, 3.0, size=shape)
    flat = s.reshape(-1)
    flat[::7] = -0.0
    flat[3::11] = np.nan
    flat[5::13] = np.inf
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)
