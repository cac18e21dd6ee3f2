"""Cost of the film stage (pt_film_develop) on one GPU, on device buffers (on_device = 1).

A --width x --height frame of random sums (15 % of the pixels four times brighter, so a real share lies above the glare threshold) is
developed with each configuration --repeat times after --warmup calls; the wall time of the call (it returns when the work is done,
and allocates and frees its scratch inside) is reported as median and minimum, next to the algorithmic counts the time is bounded by
(DESIGN.md §17): multiply-add pairs, LDS bytes read by the convolution's sliding windows and the HBM bytes of all kernels.
Prints one JSON line per configuration and, with --out, writes them all to a file."""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")

CONFIGS = {
    "no_glare": dict(tonemap="aces"),
    "defaults_s0.2": dict(bloom_strength=0.2, tonemap="aces"),
    "sigma4_L6": dict(bloom_strength=0.2, bloom_sigma=4.0, bloom_levels=6, tonemap="aces"),
}
CONV_TX, CONV_TY = 256, 8   # the convolution's tile (csrc/pt_film.hip)


class DeviceBuffer:
    def __init__(self, hip, host):
        self.hip, self.ptr = hip, C.c_void_p()
        assert hip.hipMalloc(C.byref(self.ptr), host.nbytes) == 0
        assert hip.hipMemcpy(self.ptr, host.ctypes.data, host.nbytes, 1) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def counts_of(w, h, opts):
    """Algorithmic work of one call: multiply-add pairs, LDS bytes the sliding windows read, bytes to and from global memory."""
    n = w * h
    hbm = n * (24 + 24 + 3)                                  # develop: sums in, hdr and rgb8 out
    pairs = lds = 0
    if opts.get("bloom_strength", 0.0) > 0.0:
        hbm += n * (24 + 24) + n * 24                        # prepare: sums in, B out; develop: G in
        for l in range(opts.get("bloom_levels", 5)):
            taps = 2 * math.ceil(3.0 * opts.get("bloom_sigma", 2.0) * 2.0 ** l) + 1
            pairs += 2 * 3 * n * taps                        # two passes, three channels
            lds += 2 * 3 * n * taps * 8 // 4                 # one 8-byte read feeds four outputs
            for rows, cols in ((h, w), (w, h)):              # a tile reads its columns plus both halos, writes its outputs (the second pass also reads G)
                tiles = math.ceil(cols / CONV_TX)
                hbm += 3 * 8 * rows * (tiles * (CONV_TX + taps - 1) + cols)
            hbm += n * 24 if l else 0
    return {"mul_add_pairs": pairs, "lds_read_bytes": lds, "global_bytes": hbm}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = pt.Context(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    w, h, n = args.width, args.height, 64
    rng = np.random.default_rng(1)
    sums = rng.uniform(0.0, 1.5, (h, w, 3)) * np.where(rng.random((h, w, 1)) < 0.15, 4.0, 1.0) * n
    d_sums = DeviceBuffer(hip, sums)
    d_hdr = DeviceBuffer(hip, np.zeros((h, w, 3)))
    d_rgb = DeviceBuffer(hip, np.zeros((h, w, 3), dtype=np.uint8))
    ptrs = (w, h, d_sums.ptr.value, None, d_hdr.ptr.value, d_rgb.ptr.value)
    rows = []
    for name, opts in CONFIGS.items():
        ms = []
        for i in range(args.warmup + args.repeat):
            t = time.perf_counter()
            ctx.film(None, n, device_ptrs=ptrs, **opts)
            if i >= args.warmup:
                ms.append((time.perf_counter() - t) * 1e3)
        row = {"config": name, "width": w, "height": h, "device": ctx.name(), "opts": opts, "calls": len(ms),
               "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
        row.update(counts_of(w, h, opts))
        rows.append(row)
        print(json.dumps(row), flush=True)
    for b in (d_sums, d_hdr, d_rgb):
        b.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
