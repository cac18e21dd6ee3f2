"""Participating media (pt_mat_medium) without a device: the ABI symbols, the CLI's --fog argument, and the properties
of the numpy restatement of the rule (tests/medium_rule.py) that the GPU tests compare the kernels with."""
import os
import subprocess

import numpy as np
import pytest

import medium_rule as MR

GS = (-0.7, 0.0, 0.3, 0.9)
SYMBOLS = ("pt_mat_medium", "pt_scene_set_camera_medium", "pt_scene_camera_medium", "pt_medium_probe")


def test_symbols_exported(pt):
    for name in SYMBOLS:
        assert name in pt.ABI_SYMBOLS, name
        assert hasattr(pt.lib, name), name
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name


def _exe(pt):
    return os.path.join(os.path.dirname(pt.__file__), "pt_render")


@pytest.mark.parametrize("value", ["", "abc", "0", "-1", "nan", "inf", "0.5,1", "0.5,1,1", "0.5,1,1,2", "0.5,1,1,1,1", "0.5,1,1,1,-1.5",
                                   "0.5,1,1,1,0.3,7", "0.5x", "0.5,,1,1", "0.5,1,1,-0.1"])
def test_cli_refuses_bad_fog(pt, value):
    # status 2 before any device is opened: this runs on a machine without a GPU
    r = subprocess.run([_exe(pt), "-s", "3", "--fog", value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (value, r.returncode, r.stderr)
    assert "--fog" in r.stderr


def test_cli_refuses_fog_with_env_sampling(pt):
    r = subprocess.run([_exe(pt), "-s", "6", "--fog", "0.1", "--env-sampling", "0.5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stderr
    r = subprocess.run([_exe(pt), "--fog"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


def test_cli_help_names_fog(pt):
    r = subprocess.run([_exe(pt), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--fog DENSITY[,R,G,B[,G]]" in r.stdout


@pytest.mark.parametrize("g", GS)
def test_hg_sampler_inverts_the_cdf(g):
    u = np.concatenate([np.linspace(0.0, 1.0, 4001)[:-1], np.random.default_rng(1).random(100000)])
    c = MR.hg_cos(g, u)
    assert (np.abs(c) <= 1.0).all()
    want = 1.0 - u if abs(g) < 1e-3 else u
    assert np.abs(MR.hg_cdf(g, c) - want).max() < 1e-12


@pytest.mark.parametrize("g", GS)
def test_hg_phase_is_normalised_and_has_mean_g(g):
    total, m1, m2 = MR.hg_cos_moments(g)                                  # sum ph dOmega with phi integrated out, E[cos_t], E[cos_t^2]
    assert abs(total - 1.0) < 1e-12, total
    assert abs(m1 - g) < 1e-12, m1
    assert abs(m2 - (1.0 + 2.0 * g * g) / 3.0) < 1e-12, m2                # the second moment the GPU test's standard error uses


@pytest.mark.parametrize("g", GS)
def test_hg_directions_are_unit_and_at_the_right_angle(g):
    rng = np.random.default_rng(5)
    axis = rng.normal(size=(20000, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    axis[:3] = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)]     # the frame's special cases
    u = rng.random((20000, 2))
    w = MR.hg_dir(g, u[:, 0], u[:, 1], axis)
    assert np.abs(np.linalg.norm(w, axis=1) - 1.0).max() < 1e-12
    assert np.abs((w * axis).sum(axis=1) - MR.hg_cos(g, u[:, 0])).max() < 1e-12


def test_free_flight_is_exponential():
    u = (np.arange(200000) + 0.5) / 200000
    d = MR.free_flight(u, 2.5)
    assert abs(d.mean() - 1.0 / 2.5) < 1e-4 and (d >= 0).all()
    assert MR.free_flight(0.0, 3.0) == 0.0


def _replay_scene():
    from common import icosphere
    m = MR.Media()
    m.add_sphere((-1.2, 0.0, 0.0), 0.8, 1.5, (0.5, 0.25, 0.125), 0.0)
    m.add_box((0.2, -0.7, -0.6), (1.6, 0.7, 0.6), 2.0, (0.25, 0.5, 1.0), 0.6)
    P, I = icosphere(1)
    m.add_mesh(0.7, P, I, (0.0, 1.0, 0.0), 0.4, (0.0, 1.6, 0.3), 1.0, (1.0, 0.125, 0.5), -0.4)
    return m


def test_replay_is_stable_under_one_ulp():
    """The GPU replay test allows 1 of its (pixel, sample) pairs to disagree, for a comparison that rounding flips: the replay
    against itself with every unit draw and hit distance moved by one ulp must stay within that."""
    import refs_numpy as R
    media = _replay_scene()
    fr = R.camera_frame(32, 1.0, 40.0, (0.0, 0.4, -5.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 1.0)
    cam = dict(width=32, blur_strength=0.5, max_depth=12)
    rng = np.random.default_rng(2)
    pairs = [(int(rng.integers(0, 32 * fr["height"])), int(rng.integers(0, 8))) for _ in range(400)]
    up = lambda x: np.nextafter(x, np.inf)
    bad = 0
    for sobol in (False, True):
        for p, s in pairs:
            a = MR.replay_path(media, fr, cam, 9, p, s, (1.0, 1.0, 1.0), sobol=sobol)
            b = MR.replay_path(media, fr, cam, 9, p, s, (1.0, 1.0, 1.0), sobol=sobol, perturb=up)
            bad += not np.allclose(a, b, rtol=1e-12, atol=0.0)
    assert bad <= 1, bad
