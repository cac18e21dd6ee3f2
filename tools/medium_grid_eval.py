"""Grid-density participating media (pt_mat_medium_grid): what the smoke costs (GPU).

Scene 3 at --width x --width (default 1920) and --spp (default 256): without media; with the plume of `pt_render --smoke` (64^3 values
over the world's bounds grown by 1 %, an unbounded camera medium) at each of --scales, albedo 0.9, g 0.4; and wrapped in `--fog` of the
plume's mean density at each scale. Per configuration: Msamples/s of three plain renders (median), segments per sample, K2 and K3 ms per
launch of one profiled render. For the plume also the tracking loop's trips, counted by the probe (pt_medium_probe, which = 3) on the
frame's camera rays up to their first hit: tentative collisions per ray (mean, maximum) and, per 64 consecutive rays of an 8 x 8 pixel
tile — one wave's visit —, the trips of the lane that loops longest (mean, maximum). Writes profiles/r10_medium_grid_scene3.json (--out-dir).

  python tools/medium_grid_eval.py [--width 1920] [--spp 256] [--scales 0.02,0.08]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
from medium_eval import BOX_HI, BOX_LO, measure          # noqa: E402
from medium_grid_rule import smoke_plume                 # noqa: E402
import refs_numpy as R                                   # noqa: E402


def camera_ray_trips(gs, cam, smoke, width):
    """Tentative collisions of the frame's pixel-centre camera rays (seed 0, pixel = row of the probe), each up to its first hit."""
    fr = R.camera_frame(width, cam.aspect_ratio, cam.vfov, tuple(cam.look_from), tuple(cam.look_at), tuple(cam.vup), cam.focal_length)
    H = fr["height"]
    ty, tx = np.meshgrid(np.arange(0, H - 7, 8), np.arange(0, width - 7, 8), indexing="ij")          # whole 8 x 8 tiles, tile after tile
    iy, ix = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    rows = (ty.reshape(-1, 1) + iy.reshape(1, -1)).reshape(-1)
    cols = (tx.reshape(-1, 1) + ix.reshape(1, -1)).reshape(-1)
    d = fr["pixel00"] + rows[:, None] * fr["dv"] + cols[:, None] * fr["du"] - fr["center"]
    d /= np.linalg.norm(d, axis=1)[:, None]
    d = np.nextafter(d, 0.0)
    o = np.broadcast_to(fr["center"], d.shape)
    hits = gs.intersect(np.concatenate([o, d, np.zeros((len(d), 1))], axis=1))
    t = np.where(hits[:, 0] == 1.0, hits[:, 1], np.inf)
    out = gs.medium_probe(smoke, 3, np.concatenate([o, d, t[:, None]], axis=1))
    trips = ((out[:, 2] - (1.0 - out[:, 0]) * (out[:, 2] > 0)) / 2.0).astype(np.int64)           # draws = 2 trips + 1 for the step out
    wave = trips.reshape(-1, 64).max(axis=1)
    return {"rays": int(len(trips)), "collided_share": round(float(out[:, 0].mean()), 4), "trips_per_ray_mean": round(float(trips.mean()), 3),
            "trips_per_ray_max": int(trips.max()), "trips_per_wave_visit_mean": round(float(wave.mean()), 3), "trips_per_wave_visit_max": int(wave.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scales", default="0.02,0.08")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ctx = pt.Context(0)
    plume = smoke_plume()
    mean_v = float(plume.astype(np.float64).mean())
    grow = 0.005 * (BOX_HI - BOX_LO)
    lo, hi = (BOX_LO - grow,) * 3, (BOX_HI + grow,) * 3
    rec = {"scene": 3, "width": args.width, "spp": args.spp, "device": ctx.name(), "albedo": 0.9, "g": 0.4, "plume_mean_value": round(mean_v, 5), "configs": {}}
    configs = [("no media", None, None)]
    for s in [float(x) for x in args.scales.split(",")]:
        configs += [(f"smoke {s:g}", "smoke", s), (f"fog {s * mean_v:.3g} (the mean density of smoke {s:g})", "fog", s * mean_v)]
    for name, kind, strength in configs:
        gs = pt.Scene(ctx)
        cam = gs.build_scene(3, args.width, args.spp)
        smoke = None
        if kind == "smoke":
            smoke = gs.mat_medium_grid(strength, (0.9, 0.9, 0.9), 0.4, plume, lo, hi)
            gs.set_camera_medium(smoke)
            gs.world_build()
        elif kind == "fog":
            fog = gs.mat_medium(strength, (0.9, 0.9, 0.9), 0.4)
            gs.world_add_object(gs.cuboid(lo, hi, fog))
            gs.world_build()
        rec["configs"][name] = measure(gs, cam, args.spp, args.runs)
        if smoke is not None:
            rec["configs"][name]["camera_rays"] = camera_ray_trips(gs, cam, smoke, args.width)
        print(json.dumps({name: rec["configs"][name]}), flush=True)
        gs.close()
    with open(os.path.join(args.out_dir, "r10_medium_grid_scene3.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
