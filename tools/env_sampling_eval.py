"""Environment importance sampling (pt_scene_set_env_sampling): what it gains and costs per image-lit scene (GPU).

For scenes 4, 5 and 6 at --width (default 240), in RGB8 and float-HDR mode: the trimmed and untrimmed relMSE (tools/adaptive_eval.py's
definition) and the wall ms of today's estimator (f = 0) and of f in {0.25, 0.5, 0.75} at 16 / 64 / 256 / 1024 spp, against a
--ref-spp env-on (f = 0.5) render; K3 ms per launch of the ENV form against the default form (profiled 1024-spp renders); and the
table build's ms and bytes. Writes profiles/r06_env_sampling_scene{4,5,6}.json (--out-dir).

  python tools/env_sampling_eval.py
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
    e = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(axis=2).reshape(-1)
    keep = np.sort(e)[: int(len(e) * 0.999)]
    return {"all": float(e.mean()), "trimmed": float(keep.mean())}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def scene_record(ctx, sid, args):
    rec = {"scene": sid, "width": args.width, "ref_spp": args.ref_spp, "device": ctx.name(),
           "relmse": "mean((x - ref)^2 / (ref^2 + 1e-2)) over pixels and channels; trimmed: without the 0.1 % of pixels with the largest error",
           "modes": {}}
    for mode in ("rgb8", "float_hdr"):
        gs = pt.Scene(ctx)
        if mode == "float_hdr":
            gs.set_float_hdr(True)
        cam = gs.build_scene(sid, args.width, 16)
        tex = cam.env_tex
        h = pt.image_height(cam)
        gs.set_env_sampling(0.5)
        _, build_ms = timed(lambda: gs.env_probe(cam, 1, np.array([[0.0, 1.0, 0.0]])))   # the first call builds the tables
        _, probe_ms = timed(lambda: gs.env_probe(cam, 1, np.array([[0.0, 1.0, 0.0]])))
        r = {"table_build_ms": round(build_ms - probe_ms, 2), "env_tex": int(tex)}
        ref = gs.render(cam, 1000, 0, args.ref_spp)[0] / args.ref_spp
        rows = {}
        for f in (0.0, 0.25, 0.5, 0.75):
            gs.set_env_sampling(f)
            gs.render(cam, 7, 0, 4)                                                           # warm the pool
            per = {}
            for spp in (16, 64, 256, 1024):
                (acc, _), ms = timed(lambda: gs.render(cam, 1, 0, spp))
                per[str(spp)] = {"ms": round(ms, 2), "relmse": rel_mse(acc / spp, ref)}
            _, st = gs.render(cam, 2, 0, 1024, profile=True)
            per["k3_ms_per_launch_1024spp"] = round(st.ms_shade / max(1, st.launches_shade), 4)
            rows[str(f)] = per
        r["by_f"] = rows
        r["relmse_ratio_vs_off"] = {f: {s: round(rows[f][s]["relmse"]["trimmed"] / rows["0.0"][s]["relmse"]["trimmed"], 4)
                                        for s in ("16", "64", "256", "1024")} for f in ("0.25", "0.5", "0.75")}
        rec["modes"][mode] = r
        gs.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--scenes", default="4,5,6")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ctx = pt.Context(0)
    for sid in (int(s) for s in args.scenes.split(",")):
        rec = scene_record(ctx, sid, args)
        path = os.path.join(args.out_dir, f"r06_env_sampling_scene{sid}.json")
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps({"scene": sid, "ratio_vs_off": {m: rec["modes"][m]["relmse_ratio_vs_off"] for m in rec["modes"]},
                          "table_build_ms": {m: rec["modes"][m]["table_build_ms"] for m in rec["modes"]}}))
    ctx.close()


if __name__ == "__main__":
    main()
