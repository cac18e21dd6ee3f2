"""tools/scene_host_check.cpp — the scene graph and the flattener (csrc/pt_error.cpp, pt_graph.cpp, pt_flatten.cpp) as a stand-alone host
program — builds with plain g++, without a ROCm include path or library, and passes: the seven built-in scenes and every hand-made graph
flatten into arrays that keep the structural invariants (the program exits non-zero on a breach) and print a checksum each, and the
refusals come with their messages. The sanitizer run of the same program is made by hand (its command is in the program's first lines)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "thu-acg-f2024-path-tracer_amd")
UNITS = ["csrc/pt_error.cpp", "csrc/pt_graph.cpp", "csrc/pt_flatten.cpp", "csrc/pt_assets.cpp", "csrc/pt_jpeg.cpp", "host/scenes.cpp"]
SCENES = [f"builtin-{i}" for i in range(1, 8)] + [
    "one-sphere", "one-triangle", "five-triangles", "shared-mesh", "moving-mesh", "cuboid-instance", "flat-top-level", "tree-top-level", "checkers",
    "mix-of-mixes", "glass-interior", "grid-medium", "light-grid-auto", "light-grid-given", "grid-corrected"]
REFUSALS = {"empty-world": "the world is empty", "empty-mesh": "empty mesh", "deep-chain": "instance chain too deep",
            "grid-infinite-box": "the light grid needs a finite box", "grid-table-too-large": "more than 2^25 entries"}


def test_scene_host_check(tmp_path):
    exe = str(tmp_path / "scene_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tools", "scene_host_check.cpp")] + [os.path.join(PKG, u) for u in UNITS] +
                        ["-lz", "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe, os.path.join(ROOT, "assets")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    sums = dict(re.findall(r"^scene (\S+): .* checksum ([0-9a-f]{16})$", r.stdout, re.M))
    assert sorted(sums) == sorted(SCENES)
    assert len(set(sums.values())) == len(SCENES)          # no two of these scenes flatten alike
    refused = dict(re.findall(r"^refused (\S+): (.*)$", r.stdout, re.M))
    assert sorted(refused) == sorted(REFUSALS)
    for name, text in REFUSALS.items():
        assert refused[name].startswith("pt_world_build: ") and text in refused[name], name
    assert "BREACH" not in r.stdout and r.stdout.rstrip().endswith("scene_host_check: 0 breaches")
