"""Participating media (pt_mat_medium): what the fog costs (GPU).

Scene 3 at --width x --width (default 1920) and --spp (default 256): without media, and wrapped in a box of fog — the world's bounds
grown by 1 %, what `pt_render --fog` builds — at each of --densities, albedo 0.9, g 0.4. Per configuration: Msamples/s of three plain
renders (median), segments per sample, K2 and K3 ms per launch of one profiled render. Writes profiles/r08_medium_scene3.json (--out-dir).

  python tools/medium_eval.py [--width 1920] [--spp 256] [--densities 0.001,0.004]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")

BOX_LO, BOX_HI = 0.0, 555.0     # scene 3's bounds on every axis (main.rs cornell_box)


def measure(gs, cam, spp, runs):
    gs.render(cam, 7, 0, 4)                                                   # warm the pool and the code objects
    rates, st = [], None
    for k in range(runs):
        t = time.perf_counter()
        acc, st = gs.render(cam, 1 + k, 0, spp)
        rates.append(st.samples / (time.perf_counter() - t) / 1e6)
    _, sp = gs.render(cam, 1, 0, spp, profile=True)
    return {"msamples_per_s": [round(r, 1) for r in rates], "msamples_per_s_median": round(float(np.median(rates)), 1),
            "segments_per_sample": round(st.segments / st.samples, 3), "iterations": int(st.iterations),
            "k3_ms_per_launch": round(sp.ms_shade / max(1, sp.launches_shade), 4), "k2_ms_per_launch": round(sp.ms_extend / max(1, sp.launches_extend), 4),
            "ms_shade": round(sp.ms_shade, 1), "ms_extend": round(sp.ms_extend, 1), "mean_radiance": [round(float(x), 5) for x in (acc / spp).mean(axis=(0, 1))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--densities", default="0.001,0.004")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ctx = pt.Context(0)
    rec = {"scene": 3, "width": args.width, "spp": args.spp, "device": ctx.name(), "albedo": 0.9, "g": 0.4, "configs": {}}
    for density in [None] + [float(d) for d in args.densities.split(",")]:
        gs = pt.Scene(ctx)
        cam = gs.build_scene(3, args.width, args.spp)
        if density is not None:
            grow = 0.005 * (BOX_HI - BOX_LO)
            fog = gs.mat_medium(density, (0.9, 0.9, 0.9), 0.4)
            gs.world_add_object(gs.cuboid((BOX_LO - grow,) * 3, (BOX_HI + grow,) * 3, fog))
            gs.world_build()
        name = "no media" if density is None else f"fog {density:g}"
        rec["configs"][name] = measure(gs, cam, args.spp, args.runs)
        print(json.dumps({name: rec["configs"][name]}), flush=True)
        gs.close()
    with open(os.path.join(args.out_dir, "r08_medium_scene3.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
