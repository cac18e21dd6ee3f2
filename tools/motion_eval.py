"""Motion blur of instances (pt_instance_moving, pt_scene_set_shutter): what the per-lane pose costs (GPU).

Scene 6 at 1920 x 1080 @ 500 spp through the CLI (`pt_render --stats`, which times every launch): still, every instance translating
(--motion 0.3,0,0) and every instance translating and spinning (--motion 0.3,0,0,20). Per case: K2 and K3 milliseconds per launch and
Msamples/s, the median of --runs renders, the cases alternating after one warm-up render.

Writes profiles/r19_motion_scene6.json (--out-dir, --tag).

  python tools/motion_eval.py [--runs 3] [--width 1920] [--spp 500] [--scene 6]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thu-acg-f2024-path-tracer_amd", "pt_render")
CASES = (("still", []), ("translate", ["--motion", "0.3,0,0"]), ("translate+spin", ["--motion", "0.3,0,0,20"]))


def render(args, extra, out_png):
    cmd = [EXE, "-s", str(args.scene), "--width", str(args.width), "--spp", str(args.spp), "--assets", os.path.join(ROOT, "assets"), "--out", out_png, "--stats"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-400:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--scene", type=int, default=6)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="r19_motion")
    args = ap.parse_args()
    rows = {name: [] for name, _ in CASES}
    with tempfile.TemporaryDirectory() as tmp:
        png = os.path.join(tmp, "out.png")
        render(args, [], png)                                   # warm-up
        for _ in range(args.runs):
            for name, extra in CASES:
                st = render(args, extra, png)
                st["k2_ms_per_launch"] = st["ms_extend"] / max(1, st["launches_extend"])
                st["k3_ms_per_launch"] = st["ms_shade"] / max(1, st["launches_shade"])
                st["msamples_per_s"] = st["samples"] / (st["ms_total"] * 1e-3) * 1e-6
                st["segments_per_sample"] = st["segments"] / st["samples"]
                rows[name].append(st)
                print(name, json.dumps(st), flush=True)
    med = lambda name, key: statistics.median(r[key] for r in rows[name])
    summary = {name: {k: med(name, k) for k in ("k2_ms_per_launch", "k3_ms_per_launch", "msamples_per_s", "segments_per_sample", "ms_extend", "ms_shade", "ms_total")}
               for name, _ in CASES}
    for name, _ in CASES:
        summary[name]["motion"] = rows[name][0]["motion"]
    out = {"scene": args.scene, "width": args.width, "spp": args.spp, "runs": args.runs, "median": summary, "raw": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"{args.tag}_scene{args.scene}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary, indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
