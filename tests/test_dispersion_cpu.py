"""Spectral dispersion of glass (pt_mat_glass_set_dispersion) without a device: the ABI symbols and bindings, the
CLI's --dispersion argument, and the properties of the rule's restatement in tests/dispersion_rule.py — which the GPU tests compare
the kernels with: the weight table, the Cauchy law, the stratified wavelengths of the Sobol sampler and the slab's closed form."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dispersion_rule as DR
import interior_rule as IR

NEW_SYMBOLS = ("pt_mat_glass_set_dispersion", "pt_mat_glass_dispersion", "pt_dispersion_probe")


def test_symbols_and_bindings(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pt.ABI_SYMBOLS and hasattr(pt.lib, sym) and sym + "(" in header, sym
    for method in ("mat_glass_set_dispersion", "mat_glass_dispersion", "dispersion_probe"):
        assert hasattr(pt.Scene, method), method
    assert pt.lib.pt_mat_glass_set_dispersion.argtypes == [C.c_void_p, C.c_int, C.c_double]
    assert pt.lib.pt_mat_glass_dispersion.argtypes == [C.c_void_p, C.c_int] and pt.lib.pt_mat_glass_dispersion.restype == C.c_double
    hpp = open(os.path.join(os.path.dirname(pt.__file__), "host", "pt.hpp")).read()
    assert "with_dispersion(" in hpp and "glass_dispersion" in hpp


def test_null_scene_is_refused(pt):
    assert pt.lib.pt_mat_glass_set_dispersion(None, 0, 20.0) == -1
    assert pt.lib.pt_mat_glass_dispersion(None, 0) == -1.0
    one = (C.c_double * 2)(0.0, 0.0)
    out = (C.c_double * 7)()
    assert pt.lib.pt_dispersion_probe(None, 0, 0, 0, one, 1, out) == -1


# ---- the rule's restatement ----------------------------------------------------------------------------------------------------------
def test_weight_table():
    W = DR.weight_table()
    assert W.shape == (64, 3) and (W >= 0.0).all()
    np.testing.assert_allclose(W.mean(axis=0), 1.0, rtol=0.0, atol=1e-14)
    # red peaks above green above blue in wavelength; the negative lobe of red around 500 nm is clamped to exactly 0
    lam = 380.0 + (np.arange(64) + 0.5) * (350.0 / 64)
    peak = lam[W.argmax(axis=0)]
    assert peak[0] > peak[1] > peak[2] and (W[:, 0] == 0.0).any()


@pytest.mark.parametrize("n_d, abbe", [(1.5, 60.0), (1.5, 20.0), (1.5, 10.0), (1.62, 36.0), (2.417, 55.0), (1.33, 1e30)])
def test_cauchy_law(n_d, abbe):
    assert DR.ior(n_d, abbe, DR.LAMBDA_D) == n_d
    v = (n_d - 1.0) / (DR.ior(n_d, abbe, DR.LAMBDA_F) - DR.ior(n_d, abbe, DR.LAMBDA_C)) if abbe < 1e29 else abbe
    assert abs(v / abbe - 1.0) < 1e-12, v
    lam = np.linspace(380.0, 730.0, 101)
    n = DR.ior(n_d, abbe, lam)
    assert (np.diff(n) <= 0.0).all() and n[-1] > 1.0          # normal dispersion: blue bends more
    if abbe == 1e30:
        assert (n == n_d).all()                               # the GPU test's "no dispersion" glass: n(lambda) == n_d exactly


def test_sobol_wavelengths_are_stratified():
    """Sampler kind 1: the 2^m samples of every aligned block of one pixel put exactly one u into each stratum of width 2^-m."""
    seed = (3 << 32) | 12345
    pixels = np.arange(16, dtype=np.uint64) * np.uint64(977) + np.uint64(5)
    s = np.arange(512, dtype=np.uint64)
    u, lam, j = DR.wavelength(seed, pixels[:, None], s[None, :], sobol=True)
    assert u.shape == (16, 512) and (u >= 0.0).all() and (u < 1.0).all()
    for m in range(9):
        n = 1 << m
        cell = np.floor(u * n).astype(np.int64).reshape(16, 512 // n, n)
        assert (np.sort(cell, axis=2) == np.arange(n)).all(), m
    np.testing.assert_array_equal(lam, 380.0 + u * 350.0)
    np.testing.assert_array_equal(j, np.minimum(np.floor(u * 64), 63))
    # the independent sampler's are not (a check that the test above can fail) but are uniform
    ui, _, _ = DR.wavelength(seed, pixels[:, None], s[None, :], sobol=False)
    cell = np.floor(ui * 512).astype(np.int64)
    assert any(len(np.unique(row)) < 512 for row in cell)
    assert abs(ui.mean() - 0.5) < 4.0 / np.sqrt(12.0 * ui.size)
    # different pixels and seeds get different scrambles
    assert not np.array_equal(u[0], u[1])
    assert not np.array_equal(DR.wavelength(seed + 1, pixels[:1, None], s[None, :], sobol=True)[0], u[:1])


def test_slab_closed_form():
    """The vectorised Fresnel is interior_rule's; with n == n_d every channel has the grey slab's mean (E[W] = 1); dispersion moves blue most."""
    cos_i = np.array([0.3, 0.5736, 0.9, 1.0])
    for n in (1.473, 1.5, 1.6055):
        np.testing.assert_array_equal(DR.fresnel_flat(cos_i, n), IR.slab_angles(cos_i, n)[0])
    A, B = 1.0, 0.2
    flat, _ = DR.slab_two_tone(cos_i, 1.5, None, A, B)
    Rf = DR.fresnel_flat(cos_i, 1.5)
    grey = 2.0 * Rf / (1.0 + Rf) * A + (1.0 - Rf) / (1.0 + Rf) * B
    np.testing.assert_allclose(flat, np.repeat(grey[:, None], 3, axis=1), rtol=1e-13)
    disp, second = DR.slab_two_tone(cos_i, 1.5, 10.0, A, B)
    assert (second > disp ** 2).all()
    d = disp - flat
    assert (d[:, 2] > d[:, 1]).all() and (d[:, 2] > 0.005).all()       # blue sees the higher index: more reflection of the bright half
    coarse, _ = DR.slab_two_tone(cos_i, 1.5, 10.0, A, B, order=4)      # the quadrature has converged
    np.testing.assert_allclose(coarse, disp, rtol=1e-12)


def test_replay_runs_and_meets_the_glass():
    from test_dispersion_gpu import REPLAY, replay_frame
    fr, cam = replay_frame()
    W = REPLAY["width"]
    reached = total = 0
    for p in range(0, W * fr["height"], 5):
        for sobol in (False, True):
            rad, hits = DR.replay_dispersive_path(REPLAY["center"], REPLAY["radius"], REPLAY["roughness"], REPLAY["ior"], REPLAY["abbe"], fr, cam, 9, p, 0,
                                                  REPLAY["upper"], REPLAY["lower"], sobol=sobol)
            assert rad.shape == (3,) and np.isfinite(rad).all() and (rad >= 0.0).all()
            total += 1
            reached += hits > 0
    assert reached > total // 4, (reached, total)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def _exe(pt):
    return os.path.join(os.path.dirname(pt.__file__), "pt_render")


@pytest.mark.parametrize("value", ["", "abc", "0", "-1", "-20", "nan", "inf", "20x", "20,30", "1e999"])
def test_cli_refuses_bad_dispersion(pt, value):
    # status 2 before any device is opened: this runs on a machine without a GPU
    r = subprocess.run([_exe(pt), "-s", "1", "--dispersion", value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (value, r.returncode, r.stderr)
    assert "--dispersion" in r.stderr


def test_cli_refuses_dispersion_with_what_it_cannot_run_with(pt):
    for extra in (["--env-sampling", "0.5"], ["--fog", "0.1"], ["--smoke", "0.1"], ["--interior", "2"], ["--light-sampling", "exact"],
                  ["--mesh-light", "0,2,0,0.5"]):
        for args in (["--dispersion", "20"] + extra, extra + ["--dispersion", "20"]):
            r = subprocess.run([_exe(pt), "-s", "1"] + args, capture_output=True, text=True, timeout=60)
            assert r.returncode == 2 and "--dispersion" in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([_exe(pt), "--dispersion"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    r = subprocess.run([_exe(pt), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--dispersion ABBE" in r.stdout
