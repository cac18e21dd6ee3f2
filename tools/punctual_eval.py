"""Punctual lights (pt_light_point ...): what they are for, and what they cost (GPU).

1. A point light against the emissive sphere a user had to build before: a Lambert floor under an occluder, lit by a point light of power P,
   or by a sphere light of radius r and radiance P / (4 pi^2 r^2) — the same power — in the lights list, at shrinking r. relMSE of the mean
   image at equal spp against a point-light render with 64 times the samples (the sphere light's image converges to it as r -> 0).
   (Under the default light sampling the reference's Sphere::pdf yields NaN for most origins: the share of non-finite pixels is recorded
   beside each figure, and a sphere's relMSE covers the finite pixels only.)
2. The cost of the feature: scene 3 (the Cornell box) at --width x --width, --spp samples, with one point light under its ceiling against the
   same scene without: milliseconds per frame, nanoseconds per sample, segments per sample; the median of --runs renders, alternating.

Writes profiles/r21_punctual.json (--out-dir, --tag).

  python tools/punctual_eval.py [--runs 3] [--width 512] [--spp 256]
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POS, POWER = (0.3, 1.7, -0.2), 40.0


def floor_scene(pt, ctx, radius):
    """radius None: the point light; else the sphere light of the same power"""
    gs = pt.Scene(ctx)
    diffuse = lambda c: gs.mat_diffuse(gs.tex_solid_rgb(*c), -1)
    gs.world_add_object(gs.quad((-2.0, 0.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), diffuse((0.8, 0.6, 0.4))))
    gs.world_add_object(gs.quad((-0.35, 0.9, -0.45), (0.6, 0.0, 0.0), (0.0, 0.0, 0.7), diffuse((0.5, 0.5, 0.5))))
    if radius is None:
        gs.light_point(POS, (POWER,) * 3)
    else:
        le = POWER / (4.0 * math.pi ** 2 * radius ** 2)
        gs.world_add_light(gs.sphere(radius, POS, POS, gs.mat_light(gs.tex_solid_rgb(le, le, le))))
    gs.world_build()
    cam = pt.Camera()
    cam.aspect_ratio, cam.image_width, cam.samples_per_pixel, cam.max_depth, cam.vfov = 1.0, 128, 1, 4, 64.0
    for k, v in (("look_from", (0.0, 2.9, 0.0)), ("look_at", (0.0, 0.0, 0.0)), ("vup", (0.0, 0.0, -1.0)), ("env_color", (0.0, 0.0, 0.0))):
        for i, x in enumerate(v):
            getattr(cam, k)[i] = x
    cam.blur_strength, cam.focal_length, cam.defocus_angle, cam.env_is_map, cam.env_tex = 0.5, 1.0, 0.0, 0, -1
    return gs, cam


def rel_mse(img, ref):
    fin = np.isfinite(img).all(axis=2)
    return float(np.mean(((img - ref) ** 2).sum(axis=2)[fin] / ((ref ** 2).sum(axis=2)[fin] + 1e-4))), float(1.0 - fin.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--eq-spp", type=int, default=64)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="r21_punctual")
    args = ap.parse_args()
    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    ctx = pt.Context(0)
    out = {"equal_spp": {"spp": args.eq_spp, "rows": []}, "cost": {"scene": 3, "width": args.width, "spp": args.spp, "runs": args.runs}}

    gs, cam = floor_scene(pt, ctx, None)
    ref = gs.render(cam, 99, 0, 64 * args.eq_spp)[0] / (64 * args.eq_spp)
    img = gs.render(cam, 1, 0, args.eq_spp)[0] / args.eq_spp
    e, bad = rel_mse(img, ref)
    out["equal_spp"]["rows"].append({"light": "point", "radius": 0.0, "rel_mse": e, "non_finite_pixels": bad})
    gs.close()
    for radius in (0.2, 0.05, 0.0125, 0.003):
        gs, cam = floor_scene(pt, ctx, radius)
        img = gs.render(cam, 1, 0, args.eq_spp)[0] / args.eq_spp
        e, bad = rel_mse(img, ref)
        out["equal_spp"]["rows"].append({"light": "sphere", "radius": radius, "rel_mse": e, "non_finite_pixels": bad})
        gs.close()
    for row in out["equal_spp"]["rows"]:
        print(json.dumps(row), flush=True)

    rows = {"without": [], "with": []}
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, args.width, args.spp)
    gs.render(cam, 1, 0, args.spp)                                          # warm-up
    for _ in range(args.runs):
        for name in ("without", "with"):
            gs.clear_punctual_lights()
            if name == "with":
                gs.light_point((278.0, 500.0, 278.0), (3e6, 3e6, 3e6))
            gs.world_build()
            _, st = gs.render(cam, 1, 0, args.spp)
            rows[name].append({"ms_total": st.ms_total, "samples": st.samples, "segments": st.segments, "ns_per_sample": st.ms_total * 1e6 / st.samples,
                               "segments_per_sample": st.segments / st.samples})
    for name, r in rows.items():
        out["cost"][name] = {k: statistics.median(x[k] for x in r) for k in r[0]}
        print(name, json.dumps(out["cost"][name]), flush=True)
    out["cost"]["raw"] = rows
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"{args.tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    gs.close()
    ctx.close()


if __name__ == "__main__":
    main()
