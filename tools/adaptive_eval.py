"""Adaptive sampling on the headline frame: what pt_render_adaptive saves and what it costs (GPU).

Default run (scene 6, 1920x1080, min_spp 16, max_spp 4000): for each threshold, the wall time and mean spp of the adaptive render
and its relMSE against a 16000-spp uniform reference, next to a uniform render with the same total sample count; and the
overhead of threshold 0 (every round of the schedule renders every pixel: 16 passes plus the per-round tests) against one
pt_render of 4000 spp. Writes one JSON record (--out).

  python tools/adaptive_eval.py --out profiles/r04_adaptive_scene6.json
  python tools/adaptive_eval.py --calibrate      # the constants of tests/test_adaptive_gpu.py's accuracy test, over five seeds

relMSE = mean over pixels and channels of (x - ref)^2 / (ref^2 + 1e-2), x = sum / samples of the pixel; reported over all
pixels and over all but the 0.1 % of pixels with the largest error ("trimmed").
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


def rel_mse(x, ref):
    """(all pixels, without the 0.1 % of pixels with the largest error): scene 6's rare fireflies in the reference dominate the
    plain mean (every estimate then shows the same figure), the trimmed one shows the noise that sampling leaves."""
    e = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(axis=2).reshape(-1)
    keep = np.sort(e)[: int(len(e) * 0.999)]
    return {"all": float(e.mean()), "trimmed": float(keep.mean())}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def headline(args):
    ctx = pt.Context(0)
    gs = pt.Scene(ctx)
    cam = gs.build_scene(args.scene, args.width, args.max_spp)
    h, w = pt.image_height(cam), args.width
    out = {"scene": args.scene, "width": w, "height": h, "min_spp": args.min_spp, "max_spp": args.max_spp, "seed": args.seed,
           "device": ctx.name(), "relmse": "mean((x - ref)^2 / (ref^2 + 1e-2)) over pixels and channels; trimmed: without the 0.1 % of pixels with the largest error",
           "reference": {"spp": args.ref_spp, "seed": args.seed + 1000}}
    gs.render(cam, args.seed, 0, 64)                                       # warm-up: pool allocation, code objects
    ref, ref_ms = timed(lambda: gs.render(cam, args.seed + 1000, 0, args.ref_spp)[0])
    ref /= float(args.ref_spp)
    out["reference"]["ms"] = round(ref_ms, 1)
    gs.set_sampler(args.sampler)   # (after the reference render)
    out["sampler"] = args.sampler
    uni, uni_ms = timed(lambda: gs.render(cam, args.seed, 0, args.max_spp)[0])
    out["uniform_max_spp"] = {"spp": args.max_spp, "ms": round(uni_ms, 1), "relmse": rel_mse(uni / args.max_spp, ref)}
    # threshold 0: nothing stops, every pass renders the whole frame
    (acc0, cnt0, st0), ms0 = timed(lambda: gs.render_adaptive(cam, args.seed, args.min_spp, args.max_spp, 0.0))
    assert (cnt0 == args.max_spp).all()
    out["threshold_0"] = {"ms": round(ms0, 1), "passes": len(pt.adaptive_schedule(args.min_spp, args.max_spp)) - 1,
                          "overhead_vs_one_render": round(ms0 / uni_ms - 1.0, 4), "relmse": rel_mse(acc0 / args.max_spp, ref)}
    runs = []
    for thr in args.thresholds:
        (acc, cnt, st), ms = timed(lambda: gs.render_adaptive(cam, args.seed, args.min_spp, args.max_spp, thr))
        mean_spp = float(cnt.mean())
        eq_spp = max(1, int(round(mean_spp)))
        eq, eq_ms = timed(lambda: gs.render(cam, args.seed, 0, eq_spp)[0])
        r = {"threshold": thr, "ms": round(ms, 1), "mean_spp": round(mean_spp, 2), "samples": int(st.samples),
             "stopped_before_max": round(float((cnt < args.max_spp).mean()), 4),
             "spp_percentiles_10_50_90": [int(x) for x in np.percentile(cnt, [10, 50, 90])],
             "relmse": rel_mse(acc / cnt[..., None].astype(np.float64), ref),
             "uniform_same_samples": {"spp": eq_spp, "ms": round(eq_ms, 1), "relmse": rel_mse(eq / eq_spp, ref)}}
        r["relmse_ratio_adaptive_over_uniform"] = {k: round(r["relmse"][k] / r["uniform_same_samples"]["relmse"][k], 4) for k in ("all", "trimmed")}
        runs.append(r)
        print(json.dumps(r), flush=True)
    out["adaptive"] = runs
    print(json.dumps({k: v for k, v in out.items() if k != "adaptive"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    gs.close(); ctx.close()


def calibrate(args):
    """tests/test_adaptive_gpu.py::test_adaptive_saves_samples_and_keeps_accuracy over several seeds and thresholds."""
    ctx = pt.Context(0)
    gs = pt.Scene(ctx)
    m, n = 16, 1024
    cam = gs.build_scene(3, 128, n)
    ref = gs.render(cam, 99, 0, 8192)[0] / 8192.0
    res = {}
    for thr in (0.01, 0.02, 0.05, 0.1):
        fr, ra = [], []
        for seed in range(1, 6):
            acc, cnt, _ = gs.render_adaptive(cam, seed, m, n, thr)
            mean = acc / cnt[..., None].astype(np.float64)
            stopped = cnt < n
            err = np.abs(mean - ref).sum(axis=2) / (1e-4 + np.sqrt(ref.sum(axis=2)))
            fr.append(cnt.mean() / n)
            ra.append(err[stopped].mean() / thr if stopped.any() else float("nan"))
        res[thr] = {"frac": fr, "ratio": ra, "frac_mean": float(np.mean(fr)), "frac_std": float(np.std(fr, ddof=1)),
                    "ratio_mean": float(np.mean(ra)), "ratio_std": float(np.std(ra, ddof=1))}
        print(thr, json.dumps(res[thr]), flush=True)
    gs.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=6)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=4000)
    ap.add_argument("--ref-spp", type=int, default=16000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.02, 0.01, 0.005])
    ap.add_argument("--sampler", default="independent", choices=["independent", "sobol"],
                    help="sampler of the renders under test (the reference render always uses the independent one)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calibrate", action="store_true")
    args = ap.parse_args()
    calibrate(args) if args.calibrate else headline(args)


if __name__ == "__main__":
    main()
