"""Quality and cost of the a-trous denoiser (pt_denoise) on one GPU.

Default: for each spp in --spp, the frame is rendered as two halves [0, s/2) and [s/2, s), the first-hit AOVs over
[0, min(--aov-spp, s)), and denoised with the default options; relMSE of the raw and the denoised frame against a --ref-spp render
(over all pixels and over all but the 0.1 % of pixels with the largest error, "trimmed", as tools/adaptive_eval.py), and the wall
time of each step against one plain render of s samples.
--calibrate: relMSE ratio (denoised / raw) at --cal-spp over a grid of (K, sigma_l, sigma_z) on the given scenes at --cal-width."""
import argparse
import importlib
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")


def rel_mse(x, ref):
    e = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(axis=2).reshape(-1)
    keep = np.sort(e)[: int(len(e) * 0.999)]
    return {"all": float(e.mean()), "trimmed": float(keep.mean())}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def table(args):
    ctx = pt.Context(0)
    gs = pt.Scene(ctx)
    cam = gs.build_scene(args.scene, args.width, max(args.spp))
    gs.render(cam, 99, 0, 4)   # warm-up (pool allocation, code load)
    gs.render_aovs(cam, 99, 0, 1)
    ref, ref_ms = timed(lambda: gs.render(cam, 7777, 0, args.ref_spp)[0] / float(args.ref_spp))
    gs.set_sampler(args.sampler)   # (after the reference render)
    out = {"scene": args.scene, "width": args.width, "ref_spp": args.ref_spp, "aov_spp": args.aov_spp, "device": ctx.name(), "sampler": args.sampler,
           "relmse": "mean((x - ref)^2 / (ref^2 + 1e-2)); trimmed: without the 0.1 % of pixels with the largest error", "rows": []}
    for s in args.spp:
        half, n_aov = s // 2, min(args.aov_spp, s)
        (plain, _), plain_ms = timed(lambda: gs.render(cam, args.seed, 0, s))
        (a, _), a_ms = timed(lambda: gs.render(cam, args.seed, 0, half))
        (b, _), b_ms = timed(lambda: gs.render(cam, args.seed, half, s))
        aov, aov_ms = timed(lambda: gs.render_aovs(cam, args.seed, 0, n_aov))
        dn, dn_ms = timed(lambda: ctx.denoise(a, half, b, s - half, aov, n_aov))
        row = {"spp": s, "plain_ms": round(plain_ms, 1), "halves_ms": round(a_ms + b_ms, 1), "aov_ms": round(aov_ms, 1),
               "denoise_ms": round(dn_ms, 1), "relmse_raw": rel_mse(plain / float(s), ref), "relmse_denoised": rel_mse(dn, ref)}
        row["ratio_trimmed"] = round(row["relmse_denoised"]["trimmed"] / row["relmse_raw"]["trimmed"], 4)
        row["ratio_all"] = round(row["relmse_denoised"]["all"] / row["relmse_raw"]["all"], 4)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    return out


def calibrate(args):
    ctx = pt.Context(0)
    res = []
    for scene in args.cal_scenes:
        gs = pt.Scene(ctx)
        cam = gs.build_scene(scene, args.cal_width, args.cal_spp)
        ref = gs.render(cam, 7777, 0, args.ref_spp)[0] / float(args.ref_spp)
        frames = []
        for seed in (1, 2, 3):
            a, _ = gs.render(cam, seed, 0, args.cal_spp // 2)
            b, _ = gs.render(cam, seed, args.cal_spp // 2, args.cal_spp)
            aov = gs.render_aovs(cam, seed, 0, min(args.aov_spp, args.cal_spp))
            frames.append((a, b, aov, rel_mse((a + b) / float(args.cal_spp), ref)))
        for K, sl, sz in itertools.product(args.cal_k, args.cal_sigma_l, args.cal_sigma_z):
            r = []
            for a, b, aov, raw in frames:
                dn = ctx.denoise(a, args.cal_spp // 2, b, args.cal_spp - args.cal_spp // 2, aov, min(args.aov_spp, args.cal_spp), K, sl, sz)
                r.append(rel_mse(dn, ref)["trimmed"] / raw["trimmed"])
            row = {"scene": scene, "K": K, "sigma_l": sl, "sigma_z": sz, "ratio_trimmed": round(float(np.mean(r)), 4)}
            res.append(row)
            print(json.dumps(row), flush=True)
        gs.close()
    return {"calibration": res, "width": args.cal_width, "spp": args.cal_spp, "ref_spp": args.ref_spp}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=6)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--aov-spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=16000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calibrate", action="store_true")
    ap.add_argument("--cal-scenes", type=int, nargs="+", default=[3, 6])
    ap.add_argument("--cal-width", type=int, default=320)
    ap.add_argument("--cal-spp", type=int, default=64)
    ap.add_argument("--cal-k", type=int, nargs="+", default=[3, 4, 5, 6])
    ap.add_argument("--cal-sigma-l", type=float, nargs="+", default=[2.0, 4.0, 8.0])
    ap.add_argument("--cal-sigma-z", type=float, nargs="+", default=[0.05, 0.1, 0.3])
    ap.add_argument("--sampler", default="independent", choices=["independent", "sobol"],
                    help="sampler of the renders under test (the reference render always uses the independent one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = calibrate(args) if args.calibrate else table(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
