"""Camera projections (pt_scene_set_projection): what the new kinds cost, and the demonstration image (GPU).

Scene 6 as the perspective camera renders it (1920x1080), as a fisheye (1920x1080, the scene's vfov across the height) and as a panorama
(1920x960), same spp: Msamples/s and segments per sample, best of --runs. Then scene 3 as a panorama (a light probe of the box, taken
inside it) and a second scene lit by nothing but that probe as its float environment map: a mirror ball, a diffuse ball
and a floor. Writes profiles/r16_projection.json and profiles/images/projection_probe_demo.png (--out-dir); git ignores the image.

  python tools/projection_eval.py [--spp 256] [--runs 3] [--demo-spp 256]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")


def cost(ctx, spp, runs):
    rows = []
    for kind, width, aspect in (("perspective", 1920, None), ("orthographic", 1920, None), ("fisheye", 1920, None), ("panorama", 1920, 2.0)):
        gs = pt.Scene(ctx)
        cam = gs.build_scene(6, width, spp)
        gs.set_projection(kind)
        if kind in ("fisheye", "panorama"):
            cam.defocus_angle = 0.0
        if aspect:
            cam.aspect_ratio = aspect
        h = pt.image_height(cam)
        best = None
        for _ in range(runs + 1):                                     # the first run warms up
            acc, st = gs.render(cam, 1, 0, spp)
            if best is None or st.ms_total < best.ms_total:
                best = st
        rows.append(dict(kind=kind, width=width, height=h, spp=spp, ms=best.ms_total, msamples_per_s=width * h * spp / best.ms_total / 1e3,
                         segments_per_sample=best.segments / best.samples, finite=bool(np.isfinite(acc).all())))
        print(rows[-1], flush=True)
        gs.close()
    return rows


def demo(ctx, spp, out_png, out_hdr):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 512, spp)
    gs.set_projection("panorama")
    cam.aspect_ratio = 2.0
    for i, v in enumerate((278.0, 400.0, 200.0)):                     # inside the box, above its objects (the script's camera stands outside it)
        cam.look_from[i] = v
    acc, _ = gs.render(cam, 1, 0, spp)
    gs.close()
    probe = (acc / spp).astype(np.float32)
    pt.save_hdr(out_hdr, probe)
    back = pt.load_hdr_rgbf32(out_hdr)                                # through the file, as a user would
    lit = pt.Scene(ctx)
    env = lit.tex_image_rgbf32(back)
    floor = lit.mat_diffuse(lit.tex_checker(0.6, lit.tex_solid_rgb(0.8, 0.8, 0.8), lit.tex_solid_rgb(0.3, 0.3, 0.3)))
    lit.world_add_object(lit.quad((-8.0, 0.0, -8.0), (0.0, 0.0, 16.0), (16.0, 0.0, 0.0), floor))
    mirror = lit.mat_metal(lit.tex_solid_rgb(0.95, 0.95, 0.95), lit.tex_solid_f(0.0))
    white = lit.mat_diffuse(lit.tex_solid_rgb(0.8, 0.8, 0.8))
    lit.world_add_object(lit.sphere(1.0, (-1.1, 1.0, 0.0), (-1.1, 1.0, 0.0), mirror))
    lit.world_add_object(lit.sphere(1.0, (1.1, 1.0, 0.0), (1.1, 1.0, 0.0), white))
    lit.world_build()
    c = pt.Camera()
    c.aspect_ratio, c.image_width, c.samples_per_pixel, c.max_depth = 2.0, 512, spp, 50
    c.env_is_map, c.env_tex, c.vfov, c.focal_length = 1, env, 35.0, 6.0
    for i, (a, b, u) in enumerate(zip((0.0, 2.2, -6.0), (0.0, 0.9, 0.0), (0.0, 1.0, 0.0))):
        c.look_from[i], c.look_at[i], c.vup[i] = a, b, u
    img, _ = lit.render(c, 1, 0, spp)
    lit.close()
    top = ctx.resolve_u8(probe.astype(np.float64), 1)
    bottom = ctx.resolve_u8(img, spp)
    pt.save_png(out_png, np.concatenate([top, bottom], axis=0))
    return dict(probe="scene 3 as a 512x256 panorama from (278, 400, 200)", lit="two balls and a floor lit by the probe alone, 512x256", spp=spp,
                probe_mean=float(probe.mean()), lit_mean=float((img / spp).mean()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--demo-spp", type=int, default=256)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ctx = pt.Context(0)
    os.makedirs(os.path.join(args.out_dir, "images"), exist_ok=True)
    result = dict(device=ctx.name(), cost=cost(ctx, args.spp, args.runs),
                  demo=demo(ctx, args.demo_spp, os.path.join(args.out_dir, "images", "projection_probe_demo.png"), os.path.join(args.out_dir, "projection_probe_demo.hdr")))
    with open(os.path.join(args.out_dir, "r16_projection.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    ctx.close()
