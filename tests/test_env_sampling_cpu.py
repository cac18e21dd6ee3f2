"""Environment importance sampling, host side (no GPU): the library exports its entry points and the CLI refuses a weight
outside [0, 1) before it opens a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thu-acg-f2024-path-tracer_amd", "pt_render")


def test_env_sampling_symbols_exported(pt):
    for name in ("pt_scene_set_env_sampling", "pt_scene_env_sampling", "pt_env_probe"):
        assert name in pt.ABI_SYMBOLS and hasattr(pt.lib, name), name


@pytest.mark.parametrize("bad", ["1", "1.5", "-0.1", "nan", "inf"])
def test_cli_refuses_bad_env_sampling(bad):
    r = subprocess.run([EXE, "-s", "6", "--width", "16", "--spp", "1", "--env-sampling", bad], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (bad, r.returncode, r.stderr)
    assert "--env-sampling" in r.stderr


def test_cli_usage_names_env_sampling():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--env-sampling F" in r.stdout
