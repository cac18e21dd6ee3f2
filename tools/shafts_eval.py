"""Light shafts (pt_scene_set_punctual_media): what the feature costs (GPU), through the CLI.

Scene 3 (the Cornell box) at --width x --width, --spp samples, three ways: with --fog and one spot light under the ceiling (--light-shafts:
the new forms), with the fog alone (the MED forms), with the light alone (the PLT forms). Milliseconds per frame, nanoseconds per sample and
segments per sample from `pt_render --stats`; the median of --runs renders, alternating. --picture also keeps the first way's image.

Writes profiles/r22_shafts.json (--out-dir, --tag); merges into the file when it exists (the headline and build-time records live there too).

  python tools/shafts_eval.py [--runs 3] [--width 512] [--spp 256] [--picture shafts.png]
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
FOG = ["--fog", "0.002,0.9,0.9,0.9,0.3"]
SPOT = ["--spot-light", "278,540,278,278,0,278,15,25,3e6,3e6,3e6"]
WAYS = {"fog_and_light": FOG + SPOT + ["--light-shafts"], "fog_alone": FOG, "light_alone": SPOT}


def render(args, extra, out):
    cmd = [EXE, "-s", "3", "--width", str(args.width), "--spp", str(args.spp), "--stats", "--out", out, "--assets", os.path.join(ROOT, "assets")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)} failed:\n{r.stderr}")
    for line in (r.stdout + r.stderr).splitlines():
        if line.startswith("{") and '"segments"' in line:
            st = json.loads(line)
            return {"ms_total": st["ms_total"], "samples": st["samples"], "segments": st["segments"], "ns_per_sample": st["ms_total"] * 1e6 / st["samples"],
                    "segments_per_sample": st["segments"] / st["samples"]}
    sys.exit("pt_render --stats printed no statistics line")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--picture", default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="r22_shafts")
    args = ap.parse_args()
    rows = {name: [] for name in WAYS}
    with tempfile.TemporaryDirectory() as tmp:
        for run in range(args.runs):
            for name, extra in WAYS.items():
                keep = args.picture if (args.picture and run == 0 and name == "fog_and_light") else os.path.join(tmp, "x.png")
                rows[name].append(render(args, extra, keep))
    cost = {"scene": 3, "width": args.width, "spp": args.spp, "runs": args.runs, "command": {k: " ".join(v) for k, v in WAYS.items()}}
    for name, r in rows.items():
        cost[name] = {k: statistics.median(x[k] for x in r) for k in r[0]}
        print(name, json.dumps(cost[name]), flush=True)
    cost["raw"] = rows
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"{args.tag}.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["cost"] = cost
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
