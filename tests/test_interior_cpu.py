"""Interior media and chromatic absorption (pt_mat_glass_set_interior, pt_mat_medium_tinted) without a device: the ABI
symbols and bindings, the CLI's --interior argument, and the closed forms of tests/interior_rule.py — which the GPU tests compare the
kernels with — against a seeded Monte Carlo of the rule's state machine with ideal Fresnel interfaces."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import interior_rule as IR
import refs_numpy as R

NEW_SYMBOLS = ("pt_mat_medium_tinted", "pt_mat_glass_set_interior", "pt_mat_glass_interior")


def test_symbols_and_bindings(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pt.ABI_SYMBOLS and hasattr(pt.lib, sym) and sym + "(" in header, sym
    for method in ("mat_medium_tinted", "mat_glass_set_interior", "mat_glass_interior"):
        assert hasattr(pt.Scene, method), method
    # the prototypes the refusals are stated in: doubles for the medium, the absorption by pointer, plain ints for the handles
    assert pt.lib.pt_mat_medium_tinted.argtypes == [C.c_void_p] + [C.c_double] * 5 + [C.POINTER(C.c_double)]
    assert pt.lib.pt_mat_glass_set_interior.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert pt.lib.pt_mat_glass_interior.argtypes == [C.c_void_p, C.c_int]
    assert "which = 4" in header                                           # the probe's new function is documented where the others are
    hpp = open(os.path.join(os.path.dirname(pt.__file__), "host", "pt.hpp")).read()
    assert "with_interior(" in hpp and "tinted(" in hpp


def test_null_scene_is_refused(pt):
    a = (C.c_double * 3)(0.1, 0.2, 0.3)
    assert pt.lib.pt_mat_medium_tinted(None, 1.0, 1.0, 1.0, 1.0, 0.0, a) == -1
    assert pt.lib.pt_mat_glass_set_interior(None, 0, 0) == -1
    assert pt.lib.pt_mat_glass_interior(None, 0) == -1


def _exe(pt):
    return os.path.join(os.path.dirname(pt.__file__), "pt_render")


@pytest.mark.parametrize("value", ["", "abc", "0", "-1", "nan", "inf", "0.5,1", "0.5,1,1", "0.5,1,1,2", "0.5,1,1,1,1", "0.5,1,1,1,-1.5",
                                   "0.5,1,1,1,0.3,7", "0.5,1,1,1,0.3,7,7", "0.5,1,1,1,0.3,1,1,1,1", "0.5x", "0.5,,1,1", "0.5,1,1,-0.1",
                                   "0,1,1,1,0,0,0,0", "0.5,1,1,1,0,-0.1,0,0", "0.5,1,1,1,0,0,inf,0", "0,1,1,1,0"])
def test_cli_refuses_bad_interior(pt, value):
    # status 2 before any device is opened: this runs on a machine without a GPU
    r = subprocess.run([_exe(pt), "-s", "6", "--interior", value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (value, r.returncode, r.stderr)
    assert "--interior" in r.stderr


def test_cli_refuses_interior_with_env_sampling_fog_or_smoke(pt):
    for extra in (["--env-sampling", "0.5"], ["--fog", "0.1"], ["--smoke", "0.1"]):
        for args in (["--interior", "0,1,1,1,0,0.2,0.7,1.5"] + extra, extra + ["--interior", "2,0.9,0.9,0.9,0.3"]):
            r = subprocess.run([_exe(pt), "-s", "6"] + args, capture_output=True, text=True, timeout=60)
            assert r.returncode == 2 and "--interior" in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([_exe(pt), "--interior"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    r = subprocess.run([_exe(pt), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--interior DENSITY[,R,G,B[,G[,AR,AG,AB]]]" in r.stdout


# ---- the closed forms against a Monte Carlo of the rule ---------------------------------------------------------------------------
ABSORB = np.array([0.2, 0.7, 1.5])


@pytest.mark.parametrize("cos_i", [1.0, 0.995, 0.6, 0.25])
@pytest.mark.parametrize("ior", [1.5, 2.0])
def test_slab_closed_forms_match_the_rule(ior, cos_i):
    n = 400000
    Rf, cos_t = IR.slab_angles(np.array([cos_i]), ior)
    Rf, L = float(Rf[0]), float(IR.traverse_length(1.0, cos_t)[0])
    assert Rf == R.dielectric_fresnel((np.sqrt(1 - cos_i ** 2), 0.0, cos_i), (0.0, 0.0, 1.0), 1.0, ior) and 0.0 < Rf < 1.0
    rng = np.random.default_rng(int(ior * 10) * 1000 + int(cos_i * 1000))
    # collisions, albedo 0: every sample is 1 or 0
    x = np.exp(-1.0 * L)
    p = IR.slab_mean(Rf, x)
    s = IR.slab_walk(rng, n, Rf, L, 1.0, np.zeros(3))
    assert np.isin(s, (0.0, 1.0)).all()
    z = (s[:, 0].mean() - p) / np.sqrt(p * (1.0 - p) / n)
    assert abs(z) < 4.0, (z, p)
    # pure absorption: a deterministic factor per traversal, mean and second moment
    xc = np.exp(-(ABSORB * L))
    s = IR.slab_walk(rng, n, Rf, L, 0.0, ABSORB)
    mean, m2 = IR.slab_mean(Rf, xc), IR.slab_second_moment(Rf, xc)
    z = (s.mean(axis=0) - mean) / np.sqrt((m2 - mean ** 2) / n)
    assert np.abs(z).max() < 4.0, z
    # the sample variance agrees with the closed-form second moment (its own standard error from the fourth moment)
    v = s.var(axis=0)
    se_v = np.sqrt(((s - s.mean(axis=0)) ** 4).mean(axis=0) / n)
    assert (np.abs(v - (m2 - mean ** 2)) < 5.0 * se_v).all()
    # both together
    s = IR.slab_walk(rng, n, Rf, L, 0.5, ABSORB)
    xs = np.exp(-0.5 * L)
    mean = Rf + (1.0 - Rf) ** 2 * xs * xc / (1.0 - Rf * xs * xc)
    m2 = Rf + (1.0 - Rf) ** 2 * xs * xc ** 2 / (1.0 - Rf * xs * xc ** 2)
    z = (s.mean(axis=0) - mean) / np.sqrt((m2 - mean ** 2) / n)
    assert np.abs(z).max() < 4.0, z


def test_the_common_mistake_is_far_from_the_rule():
    """Dropping the medium at an internal reflection: the GPU test's slab (ior 2, density 1, head-on) would see it 0.024 too bright."""
    Rf, cos_t = IR.slab_angles(np.array([1.0]), 2.0)
    x = np.exp(-IR.traverse_length(1.0, cos_t))
    right, wrong = IR.slab_mean(Rf, x)[0], IR.slab_mean_medium_dropped(Rf, x)[0]
    assert 0.02 < wrong - right < 0.03, (right, wrong)
    n = 400000
    s = IR.slab_walk(np.random.default_rng(3), n, float(Rf[0]), float(IR.traverse_length(1.0, cos_t)[0]), 1.0, np.zeros(3), keep_medium=False)
    z_wrong = (s[:, 0].mean() - wrong) / np.sqrt(wrong * (1.0 - wrong) / n)
    z_right = (s[:, 0].mean() - right) / np.sqrt(right * (1.0 - right) / n)
    assert abs(z_wrong) < 4.0 and abs(z_right) > 20.0, (z_wrong, z_right)


def test_zero_absorption_channels_are_untouched_and_infinite_segments_give_zero():
    """The rule's two corner cases, on the restatement: a_c == 0 never multiplies (no 0 * inf), a_c > 0 over +inf gives exactly 0."""
    a = np.array([0.0, 0.3, 0.0])
    with np.errstate(invalid="raise"):
        att = np.where(a > 0.0, np.exp(-(np.where(a > 0.0, a, 1.0) * np.inf)), 1.0)
    np.testing.assert_array_equal(att, [1.0, 0.0, 1.0])


# ---- the replay's glass sampler ---------------------------------------------------------------------------------------------------
def test_glass_sampler_is_consistent_with_pdf_and_eval():
    """The sampler written from glass.rs / sampling.rs draws unit directions on the side its Fresnel choice names, and with the visible
    normal it drew the pdf refs_numpy gives is positive and finite — so eval / pdf in the replay is a number."""
    rng = np.random.default_rng(8)
    n_refl = n_refr = 0
    for _ in range(2000):
        v = rng.normal(size=3)
        v[2] = abs(v[2]) + 0.05
        v /= np.linalg.norm(v)
        front = bool(rng.random() < 0.5)
        eta_i, eta_o = (1.0, 1.5) if front else (1.5, 1.0)
        h = IR.ggx_sample_microfacet_normal(v, 0.2, rng.random(), rng.random())
        assert abs(np.linalg.norm(h) - 1.0) < 1e-12 and h[2] >= 0.0
        l = IR.sample_dielectric(v, h, eta_i, eta_o, rng.random())
        assert abs(np.linalg.norm(l) - 1.0) < 1e-9
        if l[2] * v[2] > 0.0:
            n_refl += 1
        else:
            n_refr += 1
        pdf, f = R.glass_pdf_eval(0.2, 1.5, v, l, front)
        assert np.isfinite(pdf) and pdf > 0.0 and np.isfinite(f).all()
    assert n_refl > 100 and n_refr > 1000


def test_replay_runs_and_meets_the_interior():
    from test_interior_gpu import REPLAY, replay_frame
    fr, cam = replay_frame()
    tot = dict(entered=0, left=0, internal=0, vertices=0)
    W = REPLAY["width"]
    for p in range(0, W * fr["height"], 7):
        for sobol in (False, True):
            rad, ev = IR.replay_glass_path(REPLAY["center"], REPLAY["radius"], REPLAY["roughness"], REPLAY["ior"], REPLAY["interior"], fr, cam, 9, p, 0,
                                           (1.0, 1.0, 1.0), sobol=sobol)
            assert rad.shape == (3,) and np.isfinite(rad).all() and (rad >= 0.0).all()
            for k in tot:
                tot[k] += ev[k]
    assert tot["entered"] > 20 and tot["left"] > 10 and tot["vertices"] > 20 and tot["internal"] > 0, tot
