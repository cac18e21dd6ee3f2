"""Spectral dispersion of glass (pt_mat_glass_set_dispersion): what it costs and what the stratified wavelengths gain (GPU).

1. --bench-parent LIB: the headline rate (bench.py --gpus 1 --steps 3 --warmup 1) of another build of the library (PT_AMD_LIB) and of this
   one, alternating, --runs times each: dispersion does not touch the benchmark's forms, so the medians should agree.
2. The cost of dispersion: scene 1 at 960 px, 64 spp, every glass of the scene with Abbe number 20 against none: Msamples/s (median of
   --runs renders, the two scenes alternating after a common warm-up), segments per sample and K3's ms per launch from one profiled render.
3. Colour noise: relMSE per channel at 64 spp against a 16384-spp dispersive render (Sobol sampler, its own seed), for the independent and
   the Sobol sampler, 16 seeds each — where one wavelength per stratum should show.

Writes profiles/r13_dispersion.json (--out-dir, --tag).

  python tools/dispersion_eval.py [--bench-parent /path/to/parent/libpt_amd.so] [--runs 3] [--skip-bench] [--skip-noise]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")


def bench_once(lib):
    env = dict(os.environ)
    if lib:
        env["PT_AMD_LIB"] = lib
    else:
        env.pop("PT_AMD_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed ({r.returncode}): {r.stderr[-400:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["value"]


def disperse_every_glass(gs, abbe):
    """Scene scripts hand out no material handles: every handle below a fresh one is asked whether it is a glass."""
    n = gs.mat_clearcoat(0.5)
    glasses = [h for h in range(n) if gs.mat_glass_dispersion(h) >= 0.0]
    done = 0
    for h in glasses:
        try:
            gs.mat_glass_set_dispersion(h, abbe)
            done += 1
        except pt.PtError:
            pass                                                # a mix's child
    gs.world_build()
    return done


def scene1(ctx, width, abbe, sampler="independent"):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(1, width, 64)
    n_glass = disperse_every_glass(gs, abbe) if abbe else 0
    gs.set_sampler(sampler)
    return gs, cam, n_glass


def timed(scenes, spp, runs, warm_s=1.5):
    """scenes: name -> (gs, cam). The renders alternate between the scenes after a common warm-up (device clocks, code objects, pools), so
    that neither pays for going first."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for gs, cam in scenes.values():
            gs.render(cam, 7, 0, spp)
    secs = {name: [] for name in scenes}
    stats = {}
    for k in range(runs):
        for name, (gs, cam) in scenes.items():
            t = time.perf_counter()
            _, stats[name] = gs.render(cam, 1 + k, 0, spp)
            secs[name].append(time.perf_counter() - t)
    out = {}
    for name, (gs, cam) in scenes.items():
        st = stats[name]
        _, sp = gs.render(cam, 1, 0, spp, profile=True)
        out[name] = {"spp": spp, "msamples_per_s": [round(st.samples / s / 1e6, 1) for s in secs[name]],
                     "msamples_per_s_median": round(st.samples / float(np.median(secs[name])) / 1e6, 1), "segments_per_sample": round(st.segments / st.samples, 3),
                     "k3_ms_per_launch": round(sp.ms_shade / max(1, sp.launches_shade), 4), "k2_ms_per_launch": round(sp.ms_extend / max(1, sp.launches_extend), 4),
                     "shade_variant": int(st.shade_variant), "launches_shade": int(sp.launches_shade)}
    return out


def rel_mse(imgs, ref):
    return [round(float(((imgs[..., c] - ref[..., c]) ** 2).mean() / (ref[..., c] ** 2).mean()), 6) for c in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench-parent", default=None, help="libpt_amd.so of the parent commit, for the headline A/B")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--abbe", type=float, default=20.0)
    ap.add_argument("--noise-width", type=int, default=320)
    ap.add_argument("--long-spp", type=int, default=16384)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--skip-noise", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    rec = {"abbe": args.abbe}
    out_path = os.path.join(args.out_dir, f"r13_dispersion{args.tag}.json")

    def save():
        with open(out_path, "w") as fh:
            json.dump(rec, fh, indent=1)

    if args.bench_parent and not args.skip_bench:               # before this process opens the device itself
        a, b = [], []
        for _ in range(args.runs):
            a.append(bench_once(args.bench_parent))
            b.append(bench_once(None))
            print(json.dumps({"bench parent": a[-1], "bench this": b[-1]}), flush=True)
        rec["headline"] = {"parent": a, "this": b, "parent_median": float(np.median(a)), "this_median": float(np.median(b)),
                           "parent_spread": round(max(a) - min(a), 3), "this_spread": round(max(b) - min(b), 3)}
        save()
    ctx = pt.Context(0)
    rec["device"] = ctx.name()
    scenes, n_glass = {}, {}
    for name, abbe in (("plain", 0.0), (f"dispersion {args.abbe:g}", args.abbe)):
        gs, cam, n_glass[name] = scene1(ctx, args.width, abbe)
        scenes[name] = (gs, cam)
    rec["cost"] = timed(scenes, args.spp, args.runs)
    for name, (gs, cam) in scenes.items():
        rec["cost"][name].update(glass_materials_dispersive=n_glass[name], width=args.width)
        print(json.dumps({name: rec["cost"][name]}), flush=True)
        gs.close()
    save()
    if not args.skip_noise:
        gs, cam, _ = scene1(ctx, args.noise_width, args.abbe, "sobol")
        ref = gs.render(cam, 999, 0, args.long_spp)[0] / args.long_spp
        rec["noise"] = {"width": args.noise_width, "spp": args.spp, "long_spp": args.long_spp, "seeds": args.seeds, "reference_mean": [round(float(v), 5) for v in ref.mean(axis=(0, 1))]}
        for sampler in ("independent", "sobol"):
            gs.set_sampler(sampler)
            imgs = np.stack([gs.render(cam, 100 + k, 0, args.spp)[0] / args.spp for k in range(args.seeds)])
            rec["noise"][sampler] = {"rel_mse_rgb": rel_mse(imgs, ref)}
            print(json.dumps({sampler: rec["noise"][sampler]}), flush=True)
        gs.close()
        # the same two samplers without dispersion, against their own long render: what part of the gain is the wavelength's
        gs, cam, _ = scene1(ctx, args.noise_width, 0.0, "sobol")
        ref0 = gs.render(cam, 999, 0, args.long_spp)[0] / args.long_spp
        for sampler in ("independent", "sobol"):
            gs.set_sampler(sampler)
            imgs = np.stack([gs.render(cam, 100 + k, 0, args.spp)[0] / args.spp for k in range(args.seeds)])
            rec["noise"][sampler + ", no dispersion"] = {"rel_mse_rgb": rel_mse(imgs, ref0)}
            print(json.dumps({sampler + ", no dispersion": rec["noise"][sampler + ", no dispersion"]}), flush=True)
        gs.close()
        save()
    ctx.close()


if __name__ == "__main__":
    main()
