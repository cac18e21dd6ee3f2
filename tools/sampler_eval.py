"""The Sobol sampler (pt_scene_set_sampler): what it gains and costs per scene (GPU).

For scenes 3 and 6 at --width (default 240) — scene 6 also in float-HDR mode with environment sampling 0.5 — the trimmed and
untrimmed relMSE (tools/adaptive_eval.py's definition) and the wall ms of the independent and the Sobol sampler at 16 / 64 / 256 /
1024 spp, three seeds each, against a --ref-spp render made with the INDEPENDENT sampler; K3 ms per launch and the whole render's
wall ms of both samplers (profiled 1024-spp renders) at that width and, with --headline, on the 1920-wide frame.
Writes profiles/r07_sampler_scene{3,6}.json (--out-dir).

  python tools/sampler_eval.py [--headline]
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

SPPS = (16, 64, 256, 1024)
SEEDS = (1, 2, 3)
KINDS = ("independent", "sobol")


def rel_mse(x, ref):
    e = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(axis=2).reshape(-1)
    keep = np.sort(e)[: int(len(e) * 0.999)]
    return {"all": float(e.mean()), "trimmed": float(keep.mean())}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def k3_cost(gs, cam, spp):
    """K3 ms per launch and the wall ms of one profiled render, per sampler."""
    out = {}
    for kind in KINDS:
        gs.set_sampler(kind)
        gs.render(cam, 7, 0, 4)                                                               # warm the pool and the code objects
        (_, st), ms = timed(lambda: gs.render(cam, 2, 0, spp, profile=True))
        (_, _), plain_ms = timed(lambda: gs.render(cam, 2, 0, spp))
        out[kind] = {"k3_ms_per_launch": round(st.ms_shade / max(1, st.launches_shade), 4), "launches": int(st.launches_shade),
                     "ms_shade": round(st.ms_shade, 2), "ms_extend": round(st.ms_extend, 2), "profiled_wall_ms": round(ms, 2), "wall_ms": round(plain_ms, 2)}
    out["k3_ratio_sobol_over_independent"] = round(out["sobol"]["k3_ms_per_launch"] / out["independent"]["k3_ms_per_launch"], 4)
    out["wall_ratio_sobol_over_independent"] = round(out["sobol"]["wall_ms"] / out["independent"]["wall_ms"], 4)
    return out


def mode_record(ctx, sid, mode, args):
    gs = pt.Scene(ctx)
    if mode == "float_hdr_env0.5":
        gs.set_float_hdr(True)
    cam = gs.build_scene(sid, args.width, 16)
    if mode == "float_hdr_env0.5":
        gs.set_env_sampling(0.5)
    gs.set_sampler("independent")
    chunk = 512
    ref = sum(gs.render(cam, 1000 + k, 0, chunk)[0] for k in range(args.ref_spp // chunk)) / float(args.ref_spp // chunk * chunk)
    r = {"by_sampler": {}}
    for kind in KINDS:
        gs.set_sampler(kind)
        gs.render(cam, 7, 0, 4)
        per = {}
        for spp in SPPS:
            runs = []
            for seed in SEEDS:
                (acc, _), ms = timed(lambda: gs.render(cam, seed, 0, spp))
                runs.append({"seed": seed, "ms": round(ms, 2), "relmse": rel_mse(acc / spp, ref)})
            per[str(spp)] = {"runs": runs, "trimmed_mean": float(np.mean([x["relmse"]["trimmed"] for x in runs])),
                             "all_mean": float(np.mean([x["relmse"]["all"] for x in runs])), "ms_mean": round(float(np.mean([x["ms"] for x in runs])), 2)}
        r["by_sampler"][kind] = per
    ind, sob = r["by_sampler"]["independent"], r["by_sampler"]["sobol"]
    r["trimmed_ratio_sobol_over_independent"] = {str(s): round(sob[str(s)]["trimmed_mean"] / ind[str(s)]["trimmed_mean"], 4) for s in SPPS}
    r["trimmed_ratio_per_seed"] = {str(s): [round(a["relmse"]["trimmed"] / b["relmse"]["trimmed"], 4) for a, b in zip(sob[str(s)]["runs"], ind[str(s)]["runs"])]
                                   for s in SPPS}
    r["k3_1024spp"] = k3_cost(gs, cam, 1024)
    gs.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--scenes", default="3,6")
    ap.add_argument("--headline", action="store_true", help="also K3 and wall time of both samplers on the 1920-wide frame (scene 6, 256 spp)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ctx = pt.Context(0)
    for sid in (int(s) for s in args.scenes.split(",")):
        rec = {"scene": sid, "width": args.width, "ref_spp": args.ref_spp, "reference_sampler": "independent", "seeds": list(SEEDS), "device": ctx.name(),
               "relmse": "mean((x - ref)^2 / (ref^2 + 1e-2)) over pixels and channels; trimmed: without the 0.1 % of pixels with the largest error",
               "modes": {}}
        for mode in (("rgb8", "float_hdr_env0.5") if sid == 6 else ("rgb8",)):
            rec["modes"][mode] = mode_record(ctx, sid, mode, args)
        if args.headline and sid == 6:
            gs = pt.Scene(ctx)
            cam = gs.build_scene(6, 1920, 256)
            rec["headline_1920_256spp"] = k3_cost(gs, cam, 256)
            gs.close()
        with open(os.path.join(args.out_dir, f"r07_sampler_scene{sid}.json"), "w") as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps({"scene": sid, "ratio": {m: rec["modes"][m]["trimmed_ratio_sobol_over_independent"] for m in rec["modes"]},
                          "k3": {m: rec["modes"][m]["k3_1024spp"] for m in rec["modes"]}, "headline": rec.get("headline_1920_256spp")}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
