#!/usr/bin/env python3
"""What Loop subdivision costs on the GPU, against its host twin and against tessellation. Needs the GPU.
  Context.subdivide (limit projection, smooth normals) against subdivide_host in the same run: assets/cow.obj at levels 1..4 and a
  64 x 64 grid at levels 2..4. Host wall clock around the synchronous call (upload, every level, the projection, the normals, download,
  the allocations): the best and the median of --repeats calls after one warm-up; the twin once (twice up to a million triangles). The
  two results are compared byte for byte. Context.tessellate of the same mesh to the same levels (smooth normals, no displacement) is
  timed the same way: the ratio at equal output size.
  Where the time goes is taken in a run of its own: rocprofv3 --kernel-trace --stats around
  tools/subdiv_eval.py --only cow:3 --repeats 3.
  tools/subdiv_eval.py --out profiles/subdiv_eval.json"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case, e.g. cow:3 or grid:4")
    a = ap.parse_args()
    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    ctx = pt.Context(0)
    gp, gi, _, gt = pt.mesh_grid((0.0, 0.0, 0.0), (0.0, 0.0, 4.0), (4.0, 0.0, 0.0), 64, 64)
    gp = gp.copy()
    gp[:, 1] = (0.1 * np.sin(3.0 * gp[:, 0]) * np.cos(2.0 * gp[:, 2])).astype(np.float32)
    cp, ci, _ = pt.load_obj(os.path.join(pt.ASSET_DIR, "cow.obj"))
    cases = [("cow", lv, (cp, ci, None)) for lv in (1, 2, 3, 4)] + [("grid", lv, (gp, gi, gt)) for lv in (2, 3, 4)]
    if a.only:
        name, lv = a.only.split(":")
        cases = [c for c in cases if c[0] == name and c[1] == int(lv)]
    res = {"device": ctx.name(), "timing": "host wall clock around the synchronous call, ms; the GPU call includes upload, download and allocations", "subdivide": []}
    for name, lv, (pos, idx, uv) in cases:
        kw = dict(levels=lv, limit=True)
        ctx.subdivide(pos, idx, uv, **kw)                              # warm-up: code objects, hipcub's first launch
        got, gpu_ms = timed(lambda: ctx.subdivide(pos, idx, uv, **kw), a.repeats)
        tris = len(got[1]) // 3
        ref, host_ms = timed(lambda: pt.subdivide_host(pos, idx, uv, **kw), 2 if tris <= 1000000 else 1)
        same = all((g is None and r is None) or g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        ctx.tessellate(pos, idx, None, uv, levels=lv, normals="smooth")
        _, tess_ms = timed(lambda: ctx.tessellate(pos, idx, None, uv, levels=lv, normals="smooth"), a.repeats)
        row = {"mesh": name, "levels": lv, "triangles_in": len(idx) // 3, "triangles_out": tris, "vertices_out": len(got[0]), "gpu_ms_best": min(gpu_ms),
               "gpu_ms_median": float(np.median(gpu_ms)), "host_ms_best": min(host_ms), "host_over_gpu": min(host_ms) / min(gpu_ms), "bytes_equal": same,
               "tessellate_gpu_ms_best": min(tess_ms), "subdivide_over_tessellate": min(gpu_ms) / min(tess_ms),
               "bytes_up": int(sum(x.nbytes for x in (pos, idx, uv) if x is not None)), "bytes_down": int(sum(x.nbytes for x in got if x is not None))}
        res["subdivide"].append(row)
        print(row, flush=True)
    ctx.close()
    if not all(r["bytes_equal"] for r in res["subdivide"]):
        raise SystemExit("the GPU stage and the twin differ")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
