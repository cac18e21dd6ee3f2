#!/usr/bin/env python3
"""What isosurface extraction costs on the GPU, against its host twin. Needs the GPU.
  Context.isosurface against isosurface_host in the same run at 64^3, 128^3 and 256^3 samples: the plume of pt_render --smoke at level
  0.3 (closed), and a sphere open and closed. Host wall clock around the synchronous call (upload of the samples, the counting pass, the
  two scans, both emit kernels, download, the allocations): the best and the median of --repeats calls after one warm-up; the twin once
  (twice up to 128^3). The two results are compared byte for byte. Each row also carries the bytes the rule implies for the count and
  the emit kernels (13 B a lattice point for the count; 5 B a point and 24 B a vertex, 8 B a point and 12 B a triangle for the two
  emits), to set beside the per-kernel times of a run of its own: rocprofv3 --kernel-trace --stats around
  tools/iso_eval.py --only plume:256 --repeats 3.
  tools/iso_eval.py --out profiles/iso_eval.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def centres(n):
    t = (np.arange(n, dtype=np.float64) + 0.5) / n
    return np.meshgrid(t, t, t, indexing="ij")          # z, y, x at [k, j, i]


def plume(n):
    """smoke_plume of host/main.cpp at the cell centres of the unit box"""
    z, y, x = centres(n)
    cx, cz, r = 0.5 + 0.08 * np.sin(3.0 * np.pi * y), 0.5 + 0.08 * np.cos(2.0 * np.pi * y), 0.06 + 0.22 * y
    return ((1.0 - 0.7 * y) * np.exp(-((x - cx) ** 2 + (z - cz) ** 2) / (r * r))).astype(np.float32)


def sphere(n):
    z, y, x = centres(n)
    return (0.55 - np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)).astype(np.float32)      # leaves the box through all six faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case, e.g. plume:256 or sphere_open:128")
    a = ap.parse_args()
    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    ctx = pt.Context(0)
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    cases = []
    for n in (64, 128, 256):
        cases += [("plume", n, plume, dict(iso=0.3, closed=True)), ("sphere_open", n, sphere, dict(iso=0.0)), ("sphere_closed", n, sphere, dict(iso=0.0, closed=True, outside=-1.0))]
    if a.only:
        name, n = a.only.split(":")
        cases = [c for c in cases if c[0] == name and c[1] == int(n)]
    res = {"device": ctx.name(), "timing": "host wall clock around the synchronous call, ms; the GPU call includes upload, download and allocations", "isosurface": []}
    for name, n, field, kw in cases:
        v = field(n)
        ctx.isosurface(v, lo, hi, **kw)                                # warm-up: code objects, hipcub's first launch
        got, gpu_ms = timed(lambda: ctx.isosurface(v, lo, hi, **kw), a.repeats)
        ref, host_ms = timed(lambda: pt.isosurface_host(v, lo, hi, **kw), 2 if n <= 128 else 1)
        same = all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        points = (n + 2) ** 3 if kw.get("closed") else n ** 3
        verts, tris = len(got[0]), len(got[1]) // 3
        row = {"field": name, "n": n, "lattice_points": points, "vertices": verts, "triangles": tris, "gpu_ms_best": min(gpu_ms), "gpu_ms_median": float(np.median(gpu_ms)),
               "host_ms_best": min(host_ms), "host_over_gpu": min(host_ms) / min(gpu_ms), "bytes_equal": same, "bytes_up": int(v.nbytes),
               "bytes_down": int(sum(x.nbytes for x in got)), "count_kernel_bytes": 4 * n ** 3 + 9 * points, "vertex_kernel_bytes": 5 * points + 24 * verts,
               "triangle_kernel_bytes": 8 * points + 12 * tris}
        res["isosurface"].append(row)
        print(row, flush=True)
    ctx.close()
    if not all(r["bytes_equal"] for r in res["isosurface"]):
        raise SystemExit("the GPU stage and the twin differ")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
