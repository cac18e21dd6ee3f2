"""Grid-density participating media (pt_mat_medium_grid) without a device: the ABI symbol, the CLI's --smoke argument,
and the properties of the numpy restatement of the rule (tests/medium_grid_rule.py) that the GPU tests compare the kernels with."""
import os
import subprocess

import numpy as np
import pytest

import medium_grid_rule as GR


def test_symbol_exported(pt):
    assert "pt_mat_medium_grid" in pt.ABI_SYMBOLS
    assert hasattr(pt.lib, "pt_mat_medium_grid")
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    assert "pt_mat_medium_grid(" in header
    assert hasattr(pt.Scene, "mat_medium_grid")


def _exe(pt):
    return os.path.join(os.path.dirname(pt.__file__), "pt_render")


@pytest.mark.parametrize("value", ["", "abc", "0", "-1", "nan", "inf", "0.5,1", "0.5,1,1", "0.5,1,1,2", "0.5,1,1,1,1", "0.5,1,1,1,-1.5",
                                   "0.5,1,1,1,0.3,7", "0.5x", "0.5,,1,1", "0.5,1,1,-0.1"])
def test_cli_refuses_bad_smoke(pt, value):
    # status 2 before any device is opened: this runs on a machine without a GPU
    r = subprocess.run([_exe(pt), "-s", "3", "--smoke", value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (value, r.returncode, r.stderr)
    assert "--smoke" in r.stderr


def test_cli_refuses_smoke_with_env_sampling_or_fog(pt):
    r = subprocess.run([_exe(pt), "-s", "6", "--smoke", "0.1", "--env-sampling", "0.5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--smoke" in r.stderr, r.stderr
    for args in (["--smoke", "0.1", "--fog", "0.1"], ["--fog", "0.1", "--smoke", "0.1"]):
        r = subprocess.run([_exe(pt), "-s", "3"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--smoke and --fog" in r.stderr, r.stderr
    r = subprocess.run([_exe(pt), "--smoke"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


def test_cli_help_names_smoke_and_its_formula(pt):
    r = subprocess.run([_exe(pt), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--smoke SCALE[,R,G,B[,G]]" in r.stdout and "--fog DENSITY[,R,G,B[,G]]" in r.stdout
    assert "V = (1 - 0.7 y) exp(-((x - cx)^2 + (z - cz)^2) / r^2)" in r.stdout


# ---- the rule's self-checks -----------------------------------------------------------------------------------------------------
LO, HI = np.array([-0.9, -0.6, -0.5]), np.array([0.8, 0.7, 0.6])


def random_grid(seed=1, scale=2.5):
    rng = np.random.default_rng(seed)
    v = rng.random((7, 5, 6)).astype(np.float32)                       # nx, ny, nz = 6, 5, 7
    v[rng.random(v.shape) < 0.3] = 0.0
    return GR.Grid(scale, v, LO, HI)


def test_density_is_bounded_and_interpolates():
    g = random_grid()
    rng = np.random.default_rng(2)
    x = LO + (HI - LO) * rng.random((200000, 3))
    V = g.V(x)
    assert (V >= 0.0).all() and (V <= float(g.values.max())).all()
    assert (g.sigma(x) <= g.mu).all()
    # the cell centres return the samples; the faces and corners of the box are inside and take the nearest samples; outside is 0
    k, j, i = np.meshgrid(np.arange(7), np.arange(5), np.arange(6), indexing="ij")
    centres = LO + (np.stack([i, j, k], axis=-1).reshape(-1, 3) + 0.5) / g.cells
    np.testing.assert_allclose(g.V(centres), g.v.reshape(-1), rtol=1e-13, atol=1e-15)
    assert (g.V(centres) <= float(g.values.max())).all()
    assert g.V(LO)[0] == g.v[0, 0, 0] and g.V(HI)[0] == g.v[-1, -1, -1]
    eps = 1e-9
    for a in range(3):
        for p in (LO - eps * np.eye(3)[a], HI + eps * np.eye(3)[a]):
            assert g.sigma(p)[0] == 0.0
    assert g.sigma([np.nan, 0.0, 0.0])[0] == 0.0
    # a constant grid is a constant
    c = GR.Grid(1.5, np.full((3, 4, 2), 0.25, dtype=np.float32), LO, HI)
    assert (c.sigma(x[:1000]) == 1.5 * 0.25).all()


def test_clip():
    g = random_grid()
    ok, t0, t1 = g.clip([[0.0, 0.0, -4.0], [0.0, 0.0, -4.0], [0.0, 0.0, 0.0], [0.0, 5.0, -4.0], [0.0, 0.0, -4.0], [np.nan, 0.0, 0.0]],
                        [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]],
                        [np.inf, 3.7, np.inf, np.inf, np.inf, np.inf])
    assert ok.tolist() == [True, True, True, False, False, False]
    np.testing.assert_allclose(t0[:3], [3.5, 3.5, 0.0])
    np.testing.assert_allclose(t1[:3], [4.6, 3.7, 0.6])
    assert not g.clip([0.0, 0.0, -4.0], [0.0, 0.0, 1.0], 3.5)[0][0]            # a surface in front of the box: nothing to track


def test_optical_depth_is_exact():
    """2-point Gauss-Legendre per piece against a 200 001-point trapezoid."""
    g = random_grid()
    rng = np.random.default_rng(3)
    for _ in range(6):
        o = np.array([0.3, 0.4, -4.0]) + 0.2 * rng.normal(size=3)
        d = LO + (HI - LO) * rng.uniform(0.2, 0.8, size=3) - o                 # through a point well inside the box
        d /= np.linalg.norm(d)
        ok, t0, t1 = g.clip(o, d, np.inf)
        assert ok[0]
        s = np.linspace(t0[0], t1[0], 200001)
        sig = g.sigma(np.clip(o + s[:, None] * d, LO, HI))                    # (the end points lie ON the faces: rounding must not put them outside)
        trap = float(((sig[1:] + sig[:-1]) * 0.5 * np.diff(s)).sum())
        tau = g.tau(o, d)
        assert abs(tau - trap) < 1e-9 * max(1.0, trap), (tau, trap)           # (the trapezoid's own error: h^2 at the kinks)
        # additivity: the depth up to a surface at t plus the rest
        t_mid = 0.5 * (t0[0] + t1[0])
        rest = g.tau(o + t_mid * d, d)
        assert abs(g.tau(o, d, t_mid) + rest - tau) < 1e-12
    assert g.tau([0.0, 5.0, -4.0], [0.0, 0.0, 1.0]) == 0.0


def test_tracking_survives_with_exp_minus_tau():
    """Delta tracking is unbiased: a ray crosses the grid without a collision with probability exp(-tau)."""
    g = random_grid()
    n, z = 100000, []
    for k, (o, d) in enumerate([((0.3, 0.4, -4.0), (-0.07, -0.1, 1.0)), ((-3.0, 0.1, 0.05), (1.0, 0.0, 0.02)), ((0.1, 0.0, 0.0), (0.3, 0.5, -0.4))]):
        o, d = np.array(o), np.array(d) / np.linalg.norm(d)
        tau = g.tau(o, d)
        units = lambda rows, draws: GR.probe_units(rows + k * n, draws)
        collided, s, draws = g.track_many(np.broadcast_to(o, (n, 3)), np.broadcast_to(d, (n, 3)), np.inf, units)
        p = np.exp(-tau)
        z.append(((~collided).mean() - p) / np.sqrt(p * (1.0 - p) / n))
        assert (draws[collided] % 2 == 0).all() and (draws[~collided] % 2 == 1).all()      # 2 per tentative collision, 1 for the step out
        ok, t0, t1 = g.clip(o, d, np.inf)
        assert (s[collided] > t0[0]).all() and (s[collided] < t1[0]).all() and (s[~collided] == 0.0).all()
    print("z of the survival frequency:", z)
    assert np.abs(z).max() < 4.0, z


def test_tracking_one_row_equals_many_rows():
    g = random_grid()
    rng = np.random.default_rng(5)
    o = np.array([0.3, 0.4, -4.0]) + 0.1 * rng.normal(size=(64, 3))
    d = -o + 0.4 * rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    t = np.where(rng.random(64) < 0.5, np.inf, 4.0)
    collided, s, draws = g.track_many(o, d, t, GR.probe_units)
    for i in range(64):
        c1, s1, d1, trips = g.track(o[i], d[i], t[i], lambda k: float(GR.probe_units([i], [k])[0]), 0)
        assert (c1, s1, d1) == (bool(collided[i]), s[i], draws[i])
        assert d1 == (2 * trips + (0 if c1 else 1) if d1 else 0)


def test_ramp_closed_form_matches_the_exact_depth():
    ramp = GR.Ramp(1.5, 0.25, 1.0, (4, 3, 7), 2, (-3.0, -2.0, 0.5), (3.0, 2.5, 4.5))
    rng = np.random.default_rng(6)
    P = rng.uniform(-4.0, 5.0, size=(200, 3))
    Q = rng.uniform(-4.0, 5.0, size=(200, 3))
    Q[:20, 2] = P[:20, 2]                                                  # segments along which the ramp coordinate does not change
    tau = ramp.tau(P, Q)
    for i in range(200):
        L = np.linalg.norm(Q[i] - P[i])
        want = ramp.grid.tau(P[i], (Q[i] - P[i]) / L, L)
        assert abs(tau[i] - want) < 1e-12 * max(1.0, want), (i, tau[i], want)
    assert (tau > 0.0).sum() > 100


def test_smoke_plume_is_a_valid_grid():
    v = GR.smoke_plume()
    assert v.shape == (64, 64, 64) and v.dtype == np.float32 and (v >= 0.0).all() and 0.9 < v.max() <= 1.0
    assert 0.02 < v.mean() < 0.2                                         # mostly empty space around a column


def test_replay_is_stable_under_one_ulp():
    """As for §12: the GPU replay allows one (pixel, sample) pair to disagree; the replay against itself with every unit draw and hit
    distance moved by one ulp must stay within that."""
    import refs_numpy as R
    from test_medium_grid_gpu import REPLAY_CAM, replay_media
    media, cm = replay_media()
    c = REPLAY_CAM
    fr = R.camera_frame(c["width"], 1.0, c["vfov"], c["look_from"], c["look_at"], (0.0, 1.0, 0.0), 1.0)
    cam = dict(width=c["width"], blur_strength=c["blur_strength"], max_depth=c["max_depth"])
    rng = np.random.default_rng(2)
    pairs = [(int(rng.integers(0, c["width"] * fr["height"])), int(rng.integers(0, 8))) for _ in range(150)]
    up = lambda x: np.nextafter(x, np.inf)
    bad = 0
    for sobol in (False, True):
        for p, s in pairs:
            a, _ = GR.replay_path(media, fr, cam, 9, p, s, (1.0, 1.0, 1.0), camera_medium=cm, sobol=sobol)
            b, _ = GR.replay_path(media, fr, cam, 9, p, s, (1.0, 1.0, 1.0), camera_medium=cm, sobol=sobol, perturb=up)
            bad += not np.allclose(a, b, rtol=1e-12, atol=0.0)
    assert bad <= 1, bad
