#!/usr/bin/env python3
"""What the physical sky costs and what its disc-in-the-map design buys. Needs the GPU.
  1. pt_sky_bake into a device buffer at 2048x1024 and 8192x4096, with the disc (count launch, row counters to the host, bake launch) and
     with sun_scale = 0 (the bake launch alone): host wall clock around the synchronous call, the best and the median of --repeats calls.
  2. pt_render -s 6 --sky EL,AZ at --width / --spp with --env-sampling 0 and 0.5: relMSE against a --ref-spp render (env sampling 0.5,
     another seed) of the same scene, read from the f32 .pfm files the CLI writes. relMSE = mean over pixels and channels of
     (x - ref)^2 / (ref^2 + 1e-4).
  tools/sky_eval.py --out profiles/r24_sky.json [--strip FILE.pfm: also a strip of 256x128 maps over the day, elevations 2..80 degrees]"""
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


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(x) for x in f.readline().split())
        assert float(f.readline()) < 0.0                       # little-endian
        return np.frombuffer(f.read(), dtype="<f4").reshape(h, w, 3)[::-1].astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--sky", default="40,60")
    ap.add_argument("--strip", default=None)
    a = ap.parse_args()
    import torch

    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    ctx = pt.Context(0)
    res = {"device": ctx.name(), "timing": "host wall clock around the synchronous pt_sky_bake call, output in a device buffer, ms", "bake": []}
    sun = (0.5, 0.6, 0.62)
    for w, h in ((2048, 1024), (8192, 4096)):
        buf = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
        for label, kw in (("disc", dict(sun_dir=sun)), ("no disc (sun_scale 0)", dict(sun_dir=sun, sun_scale=0.0)), ("disc, radius 10 deg", dict(sun_dir=sun, sun_radius_deg=10.0))):
            ctx.sky_bake(w, h, device_ptr=buf.data_ptr(), **kw)
            ms = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                ctx.sky_bake(w, h, device_ptr=buf.data_ptr(), **kw)
                ms.append((time.perf_counter() - t0) * 1e3)
            res["bake"].append({"width": w, "height": h, "case": label, "ms_best": min(ms), "ms_median": float(np.median(ms))})
            print(res["bake"][-1], flush=True)
        del buf
    if a.strip:
        els = (2.0, 5.0, 10.0, 20.0, 40.0, 60.0, 80.0)
        maps = [ctx.sky_bake(256, 128, sun_dir=(np.cos(np.radians(e)), np.sin(np.radians(e)), 0.0)) for e in els]
        pt.save_pfm(a.strip, np.concatenate(maps, axis=1))
    ctx.close()
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    with tempfile.TemporaryDirectory() as tmp:
        def render(name, spp, f, seed):
            pfm = os.path.join(tmp, name + ".pfm")
            cmd = [exe, "-s", "6", "--width", str(a.width), "--spp", str(spp), "--seed", str(seed), "--sky", a.sky, "--assets", pt.ASSET_DIR,
                   "--out", os.path.join(tmp, name + ".png"), "--out-hdr", pfm]
            if f > 0.0:
                cmd += ["--env-sampling", str(f)]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{' '.join(cmd)} failed: {r.stderr}")
            return read_pfm(pfm), time.perf_counter() - t0
        ref, t_ref = render("ref", a.ref_spp, 0.5, 2)
        rel = lambda x: float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-4)))
        res["scene6"] = {"sky": a.sky, "width": a.width, "spp": a.spp, "ref_spp": a.ref_spp, "ref_env_sampling": 0.5, "ref_seed": 2, "ref_wall_s": t_ref, "runs": []}
        for f in (0.0, 0.5):
            img, t = render(f"f{f}", a.spp, f, 1)
            res["scene6"]["runs"].append({"env_sampling": f, "relmse": rel(img), "mean": float(img.mean()), "ref_mean": float(ref.mean()), "wall_s": t})
            print(res["scene6"]["runs"][-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
