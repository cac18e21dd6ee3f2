#!/usr/bin/env python3
"""What mesh simplification costs on the GPU, against its host twin, and what it saves the BVH build. Needs the GPU.
  Context.simplify against simplify_host in the same run on cow, spot (both as pt_load_obj gives them) and the 128^3 isosurface of the
  plume of pt_render --smoke (level 0.3, closed), at grid_n 32, 64, 128 and 256, quadric placement, and a weld of each. Host wall clock
  around the synchronous call (upload, every kernel, sort and scan, the three counts that come back in between, download, the
  allocations): the best and the median of --repeats calls after one warm-up; the twin once or twice. The two results are compared byte
  for byte every time. Each row carries the faces and vertices in and out, and the wall clock of Scene.mesh + world_build (the BVH over
  the mesh, built where the library builds it for that size) for the input and for the result.
  tools/simplify_eval.py --out profiles/simplify_eval.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def build_ms(pt, ctx, pos, idx, nrm, repeats=2):
    """Scene.mesh + world_build of one mesh, best of `repeats`"""
    best = None
    for _ in range(repeats):
        gs = pt.Scene(ctx)
        grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
        t0 = time.perf_counter()
        gs.world_add_object(gs.mesh(1.0, pos, idx, nrm, None, grey))
        gs.world_build()
        ms = (time.perf_counter() - t0) * 1e3
        gs.close()
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="one input: cow, spot or plume")
    a = ap.parse_args()
    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    from iso_eval import plume
    ctx = pt.Context(0)
    inputs = []
    for name in ("cow", "spot"):
        pos, idx, _ = pt.load_obj(os.path.join(pt.ASSET_DIR, name + ".obj"))
        inputs.append((name, pos, idx))
    ip, ii, _ = ctx.isosurface(plume(128), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), iso=0.3, closed=True, normals="none")
    inputs.append(("plume", ip, ii))
    if a.only:
        inputs = [i for i in inputs if i[0] == a.only]
    res = {"device": ctx.name(), "timing": "host wall clock around the synchronous call, ms; the GPU call includes upload, download and allocations", "simplify": []}
    for name, pos, idx in inputs:
        before = build_ms(pt, ctx, pos, idx, None)
        for kw in [dict(mode="weld")] + [dict(grid_n=g) for g in (32, 64, 128, 256)]:
            ctx.simplify(pos, idx, **kw)                                   # warm-up: code objects, hipcub's first launch
            got, gpu_ms = timed(lambda: ctx.simplify(pos, idx, **kw), a.repeats)
            ref, host_ms = timed(lambda: pt.simplify_host(pos, idx, **kw), 2 if len(idx) < 300000 else 1)
            same = all((g is None and r is None) or g.tobytes() == r.tobytes() for g, r in zip(got, ref))
            row = {"mesh": name, "mode": kw.get("mode", "cluster"), "grid_n": kw.get("grid_n"), "faces_in": len(idx) // 3, "vertices_in": len(pos),
                   "faces_out": len(got[1]) // 3, "vertices_out": len(got[0]), "gpu_ms_best": min(gpu_ms), "gpu_ms_median": float(np.median(gpu_ms)),
                   "host_ms_best": min(host_ms), "host_over_gpu": min(host_ms) / min(gpu_ms), "bytes_equal": same,
                   "world_build_ms_before": before, "world_build_ms_after": build_ms(pt, ctx, got[0], got[1], got[2]) if len(got[1]) else None}
            res["simplify"].append(row)
            print(row, flush=True)
    ctx.close()
    if not all(r["bytes_equal"] for r in res["simplify"]):
        raise SystemExit("the GPU stage and the twin differ")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
