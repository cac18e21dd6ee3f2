"""Exact light sampling (pt_scene_set_light_sampling): what a mesh light costs and what the estimator gains (GPU).

1. Time per sample at kind 0 (the reference's lights.sample / lights.pdf: every triangle tested per pdf) and kind 1 (exact: a BVH walk):
   a Lambert floor under an emissive icosphere of 320 / 5120 / 81920 triangles, 480 x 480, 64 spp (--spp; kind 0 on the largest mesh
   renders fewer samples, the figure is per sample). Median of --runs renders, and K3's ms per launch from one profiled render.
2. relMSE at 64 spp against a long kind-1 render (the estimator the quadrature tests show to be unbiased), for kind 0 and kind 1, on the
   irregular 128-triangle mesh light and on the sphere light of the MIS scenes.

--kinds 0 runs kind 0 alone and never touches the setting: with PT_AMD_LIB pointing at an older build that is the parent's own code.
Writes profiles/r12_light_sampling.json (--out-dir, --tag).

  python tools/light_sampling_eval.py [--spp 64] [--runs 3] [--kinds 0,1] [--levels 2,4,6]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
from common import MIS_EMISSION, MIS_QUAD, SceneSpec, default_camera, icosphere, mis_scene   # noqa: E402


def ball_scene(ctx, level, width):
    gs = pt.Scene(ctx)
    floor = gs.mat_diffuse(gs.tex_checker(0.8, gs.tex_solid_rgb(0.2, 0.3, 0.1), gs.tex_solid_rgb(0.9, 0.9, 0.9)), -1)
    gs.world_add_object(gs.quad((-20.0, 0.0, -20.0), (0.0, 0.0, 40.0), (40.0, 0.0, 0.0), floor))
    P, I = icosphere(level)
    P = (np.asarray(P, dtype=np.float64) + np.array([0.0, 1.6, 0.0])).astype(np.float32)
    ball = gs.mesh(1.0, P, I, None, None, gs.mat_light(gs.tex_solid_rgb(6.0, 5.0, 4.0)))
    gs.world_add_object(ball)
    gs.world_add_light(ball)
    gs.world_build()
    cam = pt.Camera()
    for k, v in default_camera(width=width, aspect=1.0, spp=1, look_from=(0.0, 2.0, -7.0), look_at=(0.0, 1.0, 0.0), env_color=(0.02, 0.02, 0.03)).items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(cam, k)[i] = x
        else:
            setattr(cam, k, v)
    return gs, cam, len(I) // 3


def timed(gs, cam, spp, runs):
    gs.render(cam, 7, 0, 1)                                                   # warm the pool and the code objects
    secs, st = [], None
    for k in range(runs):
        t = time.perf_counter()
        _, st = gs.render(cam, 1 + k, 0, spp)
        secs.append(time.perf_counter() - t)
    _, sp = gs.render(cam, 1, 0, spp, profile=True)
    return {"spp": spp, "ns_per_sample": [round(s / st.samples * 1e9, 2) for s in secs], "ns_per_sample_median": round(float(np.median(secs)) / st.samples * 1e9, 2),
            "segments_per_sample": round(st.segments / st.samples, 3), "k3_ms_per_launch": round(sp.ms_shade / max(1, sp.launches_shade), 4),
            "k2_ms_per_launch": round(sp.ms_extend / max(1, sp.launches_extend), 4), "shade_variant": int(st.shade_variant)}


def quad_mesh_scene():
    import light_rule as LR
    s = SceneSpec()
    floor = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.8, 0.6, 0.4), -1)
    s.add("world_add_object", s.add("quad", (-4.0, 0.0, -4.0), (0.0, 0.0, 8.0), (8.0, 0.0, 0.0), floor))
    P, I = LR.tessellate_quad(*MIS_QUAD, 8)
    s.add("world_add_light", s.add("mesh", 1.0, P, I, None, None, s.add("mat_light", s.add("tex_solid_rgb", *MIS_EMISSION))))
    s.add("world_build")
    s.camera = dict(mis_scene("quad").camera)
    return s


def rel_mse(ctx, spec, kinds, spp, n_batches, long_spp):
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    out = {}
    ref = None
    if 1 in kinds:
        gs.set_light_sampling("exact")
        ref = gs.render(cam, 99, 0, long_spp)[0] / long_spp
    for kind in kinds:
        if 1 in kinds:
            gs.set_light_sampling(kind)
        imgs = np.stack([gs.render(cam, 200 + b, 0, spp)[0] / spp for b in range(n_batches)])
        rec = {"mean_radiance": round(float(imgs.mean()), 6)}
        if ref is not None:
            rec["rel_mse"] = round(float(((imgs - ref) ** 2).mean() / (ref ** 2).mean()), 6)
            rec["rel_bias"] = round(float((imgs.mean(axis=0) - ref).mean() / ref.mean()), 5)
        out[f"kind{kind}"] = rec
    gs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--levels", default="2,4,6")
    ap.add_argument("--long-spp", type=int, default=16384)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    kinds = [int(k) for k in args.kinds.split(",")]
    ctx = pt.Context(0)
    rec = {"width": args.width, "device": ctx.name(), "library": "another build (PT_AMD_LIB)" if os.environ.get("PT_AMD_LIB") else "this build", "time": {}, "rel_mse": {}}
    for level in (int(v) for v in args.levels.split(",")):
        gs, cam, n_tris = ball_scene(ctx, level, args.width)
        for kind in kinds:
            if 1 in kinds:
                gs.set_light_sampling(kind)
            spp = args.spp if kind == 1 or n_tris <= 5120 else max(2, args.spp * 5120 // n_tris)   # kind 0 is O(n) per pdf
            rec["time"][f"{n_tris} triangles, kind {kind}"] = timed(gs, cam, spp, args.runs)
            print(json.dumps({f"{n_tris} triangles, kind {kind}": rec["time"][f"{n_tris} triangles, kind {kind}"]}), flush=True)
        gs.close()
    for name, spec in (("irregular 128-triangle mesh light", quad_mesh_scene()), ("sphere light", mis_scene("sphere"))):
        rec["rel_mse"][name] = rel_mse(ctx, spec, kinds, args.spp, 16, args.long_spp)
        print(json.dumps({name: rec["rel_mse"][name]}), flush=True)
    with open(os.path.join(args.out_dir, f"r12_light_sampling{args.tag}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
