"""Interior media and chromatic absorption (pt_mat_glass_set_interior, pt_mat_medium_tinted): what a filled glass costs (GPU).

Scene 6 at --width (default 1920, the script's 16:9 frame) and --spp (default 256) in three forms: plain; every glass material of the
scene script filled with a clear tinted medium (what `pt_render --interior 0,1,1,1,0,0.2,0.7,1.5` builds); and with a scattering one
(`--interior 2,0.9,0.9,0.9,0.3`). Per configuration: Msamples/s of three plain renders (median), segments per sample, K2 and K3 ms per
launch of one profiled render. Writes profiles/r11_interior_scene6.json (--out-dir).

  python tools/interior_eval.py [--width 1920] [--spp 256]
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

CONFIGS = [("plain", None),
           ("tinted 0,1,1,1,0,0.2,0.7,1.5", (0.0, (1.0, 1.0, 1.0), 0.0, (0.2, 0.7, 1.5))),
           ("scattering 2,0.9,0.9,0.9,0.3", (2.0, (0.9, 0.9, 0.9), 0.3, (0.0, 0.0, 0.0)))]


def fill_glass(gs, interior, max_handles=4094):
    """Gives every glass material of the scene the interior (density, albedo, g, absorption); returns how many there were."""
    med = gs.mat_medium_tinted(*interior)
    n = 0
    for h in range(min(med, max_handles)):
        try:
            gs.mat_glass_set_interior(h, med)                                 # refused for everything that is not a glass material
            n += 1
        except pt.PtError:
            pass
    gs.world_build()
    return n


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
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ctx = pt.Context(0)
    rec = {"scene": 6, "width": args.width, "spp": args.spp, "device": ctx.name(), "configs": {}}
    for name, interior in CONFIGS:
        gs = pt.Scene(ctx)
        cam = gs.build_scene(6, args.width, args.spp)
        n_glass = fill_glass(gs, interior) if interior is not None else 0
        rec["configs"][name] = dict(measure(gs, cam, args.spp, args.runs), glass_materials_filled=n_glass)
        print(json.dumps({name: rec["configs"][name]}), flush=True)
        gs.close()
    with open(os.path.join(args.out_dir, "r11_interior_scene6.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
