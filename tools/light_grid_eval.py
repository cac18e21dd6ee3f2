"""The light grid (pt_scene_set_punctual_selection): what it buys and what it costs (GPU).

1. --bench-parent LIB: the headline rate (bench.py --gpus 1 --steps 3 --warmup 1) of another build of the library (PT_AMD_LIB) and of this
   one, alternating, --runs times each.
2. --cost-parent LIB: §21's cost scene (scene 3 with one point light under its ceiling, tools/punctual_eval.py) at kind 0 under another build
   and under this one, alternating: the price of the run-time branch in the PLT forms. Each render runs in a child process of its own.
3. The many-lights table: scene 3 with 64, 512 and 2048 lamps in a lattice under its ceiling, kinds 0 and 1: ms per frame, relMSE at equal
   spp against a long kind-0 render, and relMSE at equal time (kind 1 gets the samples that fit kind 0's time); each relMSE also
   trimmed of the 2 % of pixels with the largest error.
4. The table's build: time and bytes at the largest size (2^25 entries: 64 x 64 x 32 cells x 256 lights, and 16 x 16 x 64 x 2048), staged
   through LDS and with direct stores (PT_EXPERIMENT=1 PT_GRID_DIRECT=1), as PT_VERBOSE prints them.

Writes profiles/r26_light_grid.json (--out-dir, --tag).

  python tools/light_grid_eval.py [--bench-parent LIB] [--cost-parent LIB] [--runs 3] [--width 256] [--spp 64]
"""
import argparse
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(code, lib=None, extra_env=None, timeout=600):
    env = dict(os.environ)
    env.pop("PT_AMD_LIB", None)
    if lib:
        env["PT_AMD_LIB"] = lib
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    return r


def bench(lib):
    env = dict(os.environ)
    env.pop("PT_AMD_LIB", None)
    if lib:
        env["PT_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    return json.loads(r.stdout.strip().splitlines()[-1])


COST = """
import importlib, json
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
ctx = pt.Context(0)
gs = pt.Scene(ctx)
cam = gs.build_scene(3, {width}, {spp})
gs.light_point((278.0, 500.0, 278.0), (3e6, 3e6, 3e6))
gs.world_build()
gs.render(cam, 1, 0, {spp})
ms = [gs.render(cam, 1, 0, {spp})[1].ms_total for _ in range(3)]
print(json.dumps(ms))
"""

BUILD = """
import importlib
import numpy as np
pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
ctx = pt.Context(0)
gs = pt.Scene(ctx)
gs.world_add_object(gs.quad((-2.0, 0.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)))
rng = np.random.default_rng(1)
for i in range({n}):
    gs.light_point(tuple(rng.uniform(-2.0, 2.0, 3)), (1.0, 1.0, 1.0))
gs.set_punctual_selection("grid")
gs.set_punctual_grid({nx}, {ny}, {nz}, box=(-2.0, 0.0, -2.0, 2.0, 3.0, 2.0))
for _ in range(3):
    gs.world_build()
"""


def lamps(gs, n):
    """n lamps in a lattice under the Cornell box's ceiling (555 wide), each of power 3e7 / n"""
    side = int(np.ceil(np.sqrt(n)))
    for i in range(n):
        x, z = 40.0 + 475.0 * (i % side + 0.5) / side, 40.0 + 475.0 * (i // side + 0.5) / side
        gs.light_point((x, 450.0, z), (3e7 / n,) * 3)                    # 105 under the ceiling, 120 above the tall box: no surface comes near a lamp


def rel_mse(img, ref, trim=0.0):
    """mean over the pixels of |img - ref|^2 / (|ref|^2 + 1e-4); trim: without that share of the pixels, those of the largest error (the
    metal sphere's highlights of single lamps are fireflies under either selection and swamp the plain mean)"""
    e = np.sort((((img - ref) ** 2).sum(axis=2) / ((ref ** 2).sum(axis=2) + 1e-4)).reshape(-1))
    return float(np.mean(e[:len(e) - int(trim * len(e))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench-parent")
    ap.add_argument("--cost-parent")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-factor", type=int, default=32)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="r26_light_grid")
    args = ap.parse_args()
    out = {"width": args.width, "spp": args.spp}

    if args.bench_parent:
        rows = {"parent": [], "this": []}
        for _ in range(args.runs):
            for name, lib in (("parent", args.bench_parent), ("this", None)):
                rows[name].append(bench(lib))
                print(name, json.dumps(rows[name][-1]), flush=True)
        out["headline"] = rows
    if args.cost_parent:
        rows = {"parent": [], "this": []}
        for _ in range(args.runs):
            for name, lib in (("parent", args.cost_parent), ("this", None)):
                rows[name] += json.loads(child(COST.format(width=512, spp=256), lib).stdout.strip().splitlines()[-1])
        out["default_kind_cost_ms"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in rows.items()}
        print("default-kind cost (scene 3 + one point light, 512 x 512, 256 spp), ms:", json.dumps({k: v["median"] for k, v in out["default_kind_cost_ms"].items()}), flush=True)

    out["build"] = []
    for n, dims in ((256, (64, 64, 32)), (2048, (16, 16, 64))):
        for direct in (False, True):
            env = {"PT_EXPERIMENT": "1", "PT_VERBOSE": "1"}
            if direct:
                env["PT_GRID_DIRECT"] = "1"
            err = child(BUILD.format(n=n, nx=dims[0], ny=dims[1], nz=dims[2]), extra_env=env).stderr
            ms = [float(m) for m in re.findall(r"light grid: .* built in ([0-9.]+) ms", err)]
            nbytes = int(re.search(r"light grid: .* lights, (\d+) bytes", err).group(1))
            out["build"].append({"lights": n, "dims": dims, "bytes": nbytes, "stores": "direct" if direct else "lds", "ms": ms})
            print(json.dumps(out["build"][-1]), flush=True)

    pt = importlib.import_module("thu-acg-f2024-path-tracer_amd")
    ctx = pt.Context(0)
    out["many_lights"] = []
    for n in (64, 512, 2048):
        gs = pt.Scene(ctx)
        cam = gs.build_scene(3, args.width, args.spp)
        lamps(gs, n)
        gs.world_build()
        ref = gs.render(cam, 99, 0, args.ref_factor * args.spp)[0] / (args.ref_factor * args.spp)
        row = {"lights": n}
        for kind in (0, 1):
            gs.set_punctual_selection(kind)
            t0 = time.perf_counter()
            gs.world_build()
            row[f"build_s_kind{kind}"] = time.perf_counter() - t0
            gs.render(cam, 1, 0, args.spp)
            ms = statistics.median(gs.render(cam, 1, 0, args.spp)[1].ms_total for _ in range(args.runs))
            img = gs.render(cam, 1, 0, args.spp)[0] / args.spp
            row[f"ms_kind{kind}"] = ms
            row[f"rel_mse_equal_spp_kind{kind}"] = rel_mse(img, ref)
            row[f"rel_mse_trimmed_equal_spp_kind{kind}"] = rel_mse(img, ref, 0.02)
            if kind == 1:
                row["grid"] = gs.punctual_grid()[0]
                spp_t = max(1, int(round(args.spp * row["ms_kind0"] / ms)))
                row["equal_time_spp_kind1"] = spp_t
                img_t = gs.render(cam, 1, 0, spp_t)[0] / spp_t
                row["rel_mse_equal_time_kind1"] = rel_mse(img_t, ref)
                row["rel_mse_trimmed_equal_time_kind1"] = rel_mse(img_t, ref, 0.02)
        out["many_lights"].append(row)
        print(json.dumps(row), flush=True)
        gs.close()
    ctx.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"{args.tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
