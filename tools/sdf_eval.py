#!/usr/bin/env python3
"""What mesh voxelisation costs on the GPU, against its host twin. Needs the GPU.
  Context.mesh_sdf against mesh_sdf_host in the same run: assets/spot.obj and assets/cow.obj through mesh_fit_grid at 32, 64, 128 and 256
  cells along the longest extent (margin 2), band = 0 and band = 4 h, what = depth and what = density (ramp 2 h). Host wall clock around
  the synchronous call (upload of the mesh, the four kernels, download of the grid, the allocations): the best and the median of
  --repeats calls after one warm-up; the twin once, and the two results compared byte for byte. The twin is a single thread that tries
  every triangle its own sample cannot rule out (110 s for spot at 256 cells); --twin-up-to N leaves it out of the rows above
  N cells (their ratio and comparison are null): the traced single-case runs below use --twin-up-to 0.
  A tool build of the library (PT_AMD_LIB; csrc/pt_sdf.hip compiled with -DPT_SDF_COUNT) also counts the point-triangle tests the cull
  left to k_sdf_dist; -DPT_SDF_CULL=0 builds the form without the cull. For per-kernel times run one case alone under
  rocprofv3 --kernel-trace --stats: tools/sdf_eval.py --only spot:128:0:depth --repeats 3 --twin-up-to 0.
  tools/sdf_eval.py --out profiles/sdf_eval.json"""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case: MESH:N:BAND_CELLS:WHAT, e.g. spot:128:0:depth or cow:64:4:density")
    ap.add_argument("--twin-up-to", type=int, default=256, help="the largest N the twin runs at")
    a = ap.parse_args()
    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    ctx = pt.Context(0)
    try:
        counter = C.c_ulonglong.in_dll(pt.lib, "pt_sdf_tests_counted")          # a tool build only
    except ValueError:
        counter = None
    cases = [(m, n, b, w) for m in ("spot", "cow") for n in (32, 64, 128, 256) for b in (0, 4) for w in ("depth", "density")]
    if a.only:
        m, n, b, w = a.only.split(":")
        cases = [(m, int(n), int(b), w)]
    res = {"device": ctx.name(), "timing": "host wall clock around the synchronous call, ms; the GPU call includes upload, download and allocations", "mesh_sdf": []}
    meshes = {}
    for mesh, n, band_cells, what in cases:
        if mesh not in meshes:
            meshes[mesh] = pt.load_obj(os.path.join(pt.ASSET_DIR, mesh + ".obj"))[:2]
        pos, idx = meshes[mesh]
        dims, lo, hi = pt.mesh_fit_grid(pos, n, 2.0)
        h = float(hi[0] - lo[0]) / dims[0]
        kw = dict(what=what, band=band_cells * h, ramp=2.0 * h if what == "density" else None)
        ctx.mesh_sdf(pos, idx, dims, lo, hi, **kw)                             # warm-up: code objects
        got, gpu_ms = timed(lambda: ctx.mesh_sdf(pos, idx, dims, lo, hi, **kw), a.repeats)
        tests = int(counter.value) if counter is not None else None
        row = {"mesh": mesh, "triangles": len(idx) // 3, "n": n, "dims": list(dims), "samples": int(np.prod(dims)), "band_cells": band_cells, "what": what,
               "gpu_ms_best": min(gpu_ms), "gpu_ms_median": float(np.median(gpu_ms)), "host_ms": None, "host_over_gpu": None, "bytes_equal": None,
               "tests_all_pairs": int(np.prod(dims)) * (len(idx) // 3), "tests_after_cull": tests}
        if n <= a.twin_up_to:
            ref, host_ms = timed(lambda: pt.mesh_sdf_host(pos, idx, dims, lo, hi, **kw), 1)
            row.update(host_ms=min(host_ms), host_over_gpu=min(host_ms) / min(gpu_ms), bytes_equal=got.tobytes() == ref.tobytes())
        res["mesh_sdf"].append(row)
        print(row, flush=True)
    ctx.close()
    if any(r["bytes_equal"] is False for r in res["mesh_sdf"]):
        raise SystemExit("the GPU stage and the twin differ")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
