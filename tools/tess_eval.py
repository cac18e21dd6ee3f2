#!/usr/bin/env python3
"""What mesh tessellation and displacement cost on the GPU and against the host twin. Needs the GPU.
  1. Context.tessellate against tessellate_host in the same run: a 64 x 64 grid displaced by a 256 x 256 image at levels 2..5 and
     assets/bunny.obj at levels 1..3 (smooth normals). Host wall clock around the synchronous call (upload, every level, download, the
     allocations): the best and the median of --repeats calls after one warm-up; the twin once (twice up to a million triangles). The two
     results are compared byte for byte.
  2. pt_world_build of the results up to --build-max triangles, on the host's binned-SAH builder (device BVH threshold 0) and on the
     device's LBVH builder (threshold 1): wall clock, and the depth the device builder reports.
  3. pt_render -s 7 --stats at --width / --spp, plain and with --displace assets/bricks/color.png,8,3: K2's milliseconds per launch.
  The split of a call into copies and kernels is taken in a run of its own: rocprofv3 --kernel-trace --memory-copy-trace --stats around
  tools/tess_eval.py --only grid:4 --repeats 3 --no-build --no-render.
  tools/tess_eval.py --out profiles/tess_eval.json"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def smooth_image(n):
    y, x = np.meshgrid((np.arange(n) + 0.5) / n, (np.arange(n) + 0.5) / n, indexing="ij")
    return (0.5 + 0.25 * np.sin(4 * np.pi * x) * np.cos(3 * np.pi * y) + 0.2 * np.sin(2 * np.pi * (x + y))).astype(np.float32)


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
    ap.add_argument("--only", default=None, help="one case, e.g. grid:4 or bunny:2")
    ap.add_argument("--build-max", type=int, default=2200000)
    ap.add_argument("--no-build", action="store_true")
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    ctx = pt.Context(0)
    grid = pt.mesh_grid((0.0, 0.0, 0.0), (0.0, 0.0, 4.0), (4.0, 0.0, 0.0), 64, 64)
    bp, bi, _ = pt.load_obj(os.path.join(pt.ASSET_DIR, "bunny.obj"))
    img = smooth_image(256)
    cases = [("grid", lv, grid, dict(levels=lv, height=img, scale=0.05)) for lv in (2, 3, 4, 5)]
    cases += [("bunny", lv, (bp, bi, None, None), dict(levels=lv, normals="smooth")) for lv in (1, 2, 3)]
    if a.only:
        name, lv = a.only.split(":")
        cases = [c for c in cases if c[0] == name and c[1] == int(lv)]
    res = {"device": ctx.name(), "timing": "host wall clock around the synchronous call, ms; the GPU call includes upload, download and allocations", "tessellate": [], "world_build": []}
    for name, lv, mesh, kw in cases:
        ctx.tessellate(*mesh, **kw)                                   # warm-up: code objects, hipcub's first launch
        got, gpu_ms = timed(lambda: ctx.tessellate(*mesh, **kw), a.repeats)
        tris = len(got[1]) // 3
        ref, host_ms = timed(lambda: pt.tessellate_host(*mesh, **kw), 2 if tris <= 1000000 else 1)
        same = all((g is None and r is None) or g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        row = {"mesh": name, "levels": lv, "triangles_in": len(mesh[1]) // 3, "triangles_out": tris, "vertices_out": len(got[0]), "gpu_ms_best": min(gpu_ms),
               "gpu_ms_median": float(np.median(gpu_ms)), "host_ms_best": min(host_ms), "host_over_gpu": min(host_ms) / min(gpu_ms), "bytes_equal": same,
               "bytes_up": int(sum(x.nbytes for x in mesh if x is not None) + (img.nbytes if "height" in kw else 0)),
               "bytes_down": int(sum(x.nbytes for x in got if x is not None))}
        res["tessellate"].append(row)
        print(row, flush=True)
        if a.no_build or tris > a.build_max:
            continue
        for builder, threshold in (("host binned SAH", 0), ("device LBVH", 1)):
            gs = pt.Scene(ctx)
            gs.set_device_bvh_threshold(threshold)
            gs.world_add_object(gs.mesh(1.0, *got, gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)))
            t0 = time.perf_counter()
            try:
                gs.world_build()
                err = None
            except pt.PtError as e:
                err = str(e)
            wall = (time.perf_counter() - t0) * 1e3
            n_dev, depth = gs.device_bvh_info() if err is None else (0, 0)
            gs.close()
            row = {"mesh": name, "levels": lv, "triangles": tris, "builder": builder, "ms": wall, "device_built_meshes": n_dev, "device_depth": depth, "error": err}
            res["world_build"].append(row)
            print(row, flush=True)
    ctx.close()
    if not a.no_render:
        exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
        res["scene7"] = []
        with tempfile.TemporaryDirectory() as tmp:
            for label, extra in (("plain", []), ("--displace assets/bricks/color.png,8,3", ["--displace", "assets/bricks/color.png,8,3"])):
                cmd = [exe, "-s", "7", "--width", str(a.width), "--spp", str(a.spp), "--assets", pt.ASSET_DIR, "--stats", "--out", os.path.join(tmp, "x.png")] + extra
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise SystemExit(f"{' '.join(cmd)} failed: {r.stderr}")
                st = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                st.update({"case": label, "width": a.width, "spp": a.spp, "wall_s": time.perf_counter() - t0, "ms_extend_per_launch": st["ms_extend"] / max(1, st["launches_extend"])})
                res["scene7"].append(st)
                print(st, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
