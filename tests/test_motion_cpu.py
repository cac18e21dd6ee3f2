"""Motion blur of instances (pt_instance_moving, pt_scene_set_shutter) without a device: the ABI symbols and bindings,
the refusal of null / bad / non-finite arguments, the host's pose and box functions against the numpy restatement of the rule in
tests/motion_rule.py, the CLI's --shutter / --motion arguments, and the Python mirrors of shade_form_exists and of the refusal table
against the sources' text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_rule as MR

NEW_SYMBOLS = ("pt_instance_moving", "pt_scene_set_shutter", "pt_scene_shutter", "pt_scene_motion", "pt_motion_pose", "pt_motion_swept_box",
               "pt_world_entry_box")
D3 = C.c_double * 3
AXIS, TR0, TR1 = D3(0.0, 1.0, 0.0), D3(0.0, 0.0, 0.0), D3(1.0, 0.0, 0.0)


def test_symbols_and_bindings(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pt.ABI_SYMBOLS and hasattr(pt.lib, sym) and sym + "(" in header, sym
    for method in ("instance_moving", "set_shutter", "shutter", "motion", "entry_box"):
        assert hasattr(pt.Scene, method), method
    assert callable(pt.motion_pose) and callable(pt.motion_swept_box)
    integration = open(os.path.join(pt.REPO_ROOT, "INTEGRATION.md")).read()
    for sym in NEW_SYMBOLS:
        assert sym in integration, sym
    hpp = open(os.path.join(os.path.dirname(pt.__file__), "host", "pt.hpp")).read()
    assert "pt_instance_moving(" in hpp and "new_moving" in hpp and "instance_motion" in hpp and "pt_scene_set_shutter(" in hpp


def test_null_and_non_finite_arguments_are_refused(pt):
    lib = pt.lib
    assert lib.pt_instance_moving(None, 0, AXIS, 0.0, 1.0, TR0, TR1) == -1 and b"null scene" in lib.pt_last_error()
    assert lib.pt_scene_set_shutter(None, 0.0, 1.0) == -1 and b"null scene" in lib.pt_last_error()
    assert lib.pt_scene_shutter(None, (C.c_double * 2)()) == -1
    assert lib.pt_scene_motion(None) == -1 and b"not built" in lib.pt_last_error()
    assert lib.pt_world_entry_box(None, 0, (C.c_double * 6)()) == -1
    out24, out6, box = (C.c_double * 24)(), (C.c_double * 6)(), (C.c_double * 6)(0, 0, 0, 1, 1, 1)
    assert lib.pt_motion_pose(AXIS, 0.0, 1.0, TR0, TR1, 0.5, None) == -1
    assert lib.pt_motion_pose(None, 0.0, 1.0, TR0, TR1, 0.5, out24) == -1
    assert lib.pt_motion_swept_box(None, AXIS, 0.0, 1.0, TR0, TR1, out6) == -1
    assert lib.pt_motion_swept_box(box, AXIS, 0.0, 1.0, TR0, TR1, None) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.pt_motion_pose(AXIS, bad, 1.0, TR0, TR1, 0.5, out24) == -1 and b"finite" in lib.pt_last_error()
        assert lib.pt_motion_pose(AXIS, 0.0, bad, TR0, TR1, 0.5, out24) == -1
        assert lib.pt_motion_pose(AXIS, 0.0, 1.0, TR0, TR1, bad, out24) == -1
        assert lib.pt_motion_pose(D3(0.0, bad, 0.0), 0.0, 1.0, TR0, TR1, 0.5, out24) == -1
        assert lib.pt_motion_pose(AXIS, 0.0, 1.0, D3(bad, 0.0, 0.0), TR1, 0.5, out24) == -1
        assert lib.pt_motion_pose(AXIS, 0.0, 1.0, TR0, D3(0.0, 0.0, bad), 0.5, out24) == -1
        assert lib.pt_motion_swept_box(box, AXIS, 0.0, bad, TR0, TR1, out6) == -1
        assert lib.pt_motion_swept_box((C.c_double * 6)(0, 0, 0, 1, bad, 1), AXIS, 0.0, 1.0, TR0, TR1, out6) == -1
    assert lib.pt_motion_swept_box((C.c_double * 6)(0, 0, 0, 1, -1, 1), AXIS, 0.0, 1.0, TR0, TR1, out6) == -1 and b"lo <= hi" in lib.pt_last_error()
    assert lib.pt_motion_pose(AXIS, 0.0, 1.0, TR0, TR1, 0.5, out24) == 0


def _keys(rng):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a0, a1 = rng.uniform(-3.0, 3.0, size=2)
    return axis, a0, a1, rng.uniform(-4.0, 4.0, size=3), rng.uniform(-4.0, 4.0, size=3)


def test_pose_at_time_0_is_the_static_pose(pt):
    rng = np.random.default_rng(1)
    for _ in range(50):
        axis, a0, a1, tr0, tr1 = _keys(rng)
        np.testing.assert_array_equal(pt.motion_pose(axis, a0, a1, tr0, tr1, 0.0), pt.motion_pose(axis, a0, a0, tr0, tr0, 0.0))
        # ... and at any time a static key pair gives the same record
        np.testing.assert_array_equal(pt.motion_pose(axis, a0, a0, tr0, tr0, 0.73), pt.motion_pose(axis, a0, a0, tr0, tr0, 0.0))
        # a key pair that translates only keeps its rotation columns
        P0, P1 = pt.motion_pose(axis, a0, a0, tr0, tr1, 0.0), pt.motion_pose(axis, a0, a0, tr0, tr1, 0.61)
        np.testing.assert_array_equal(P0[[0, 1, 2, 4, 5, 6]], P1[[0, 1, 2, 4, 5, 6]])
        assert (P1[3] == MR.lerp_keys(a0, a0, tr0, tr1, 0.61)[1]).all()


def test_pose_agrees_with_the_numpy_restatement(pt):
    """1000 random (keys, time) against the numpy quaternion restatement; libm's sin / cos against the deterministic ones is the only
    difference. Plain "4 ulp of the entry" proved too tight, as the issue foresaw: measured over 10^5 draws of these keys the worst entry is
    4096 ulp of itself off and 497 draws (0.5 %) hold an entry more than 4 ulp off — always an entry that cancels: xy - wz and its like
    are differences of two products of magnitude up to 2, `1 - (yy + zz)` is a difference from 1, and `it` is a sum of three products of
    size |tr|, so one ulp of an operand is many ulps of a small result. The bound asserted here is therefore 4 ulp at the magnitude of
    the operands: 4 ulp of max(|entry|, 1) for the rotation entries, of max(|entry|, 3 max|tr|) for `it`; the translation is plain
    arithmetic and must be equal. Over the same 10^5 draws the worst figure on that scale is 3."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(1000):
        axis, a0, a1, tr0, tr1 = _keys(rng)
        t = rng.uniform(0.0, 1.0)
        got, ref = pt.motion_pose(axis, a0, a1, tr0, tr1, t), MR.pose_at(axis, a0, a1, tr0, tr1, t)
        np.testing.assert_array_equal(got[3], ref[3])                       # the translation is plain arithmetic
        scale = np.ones((8, 3))
        scale[7] = np.abs(ref[3]).max() * 3.0                             # it: a sum of three products of entries <= 1 with tr
        err = np.abs(got - ref) / (np.spacing(np.maximum(np.abs(ref), scale)))
        worst = max(worst, err.max())
    assert worst <= 4.0, worst


def test_inverse_is_the_inverse(pt):
    rng = np.random.default_rng(3)
    for _ in range(200):
        axis, a0, a1, tr0, tr1 = _keys(rng)
        P = pt.motion_pose(axis, a0, a1, tr0, tr1, rng.uniform(0.0, 1.0))
        R, Ri = P[0:3].T, P[4:7].T                                          # columns
        assert np.abs(Ri @ R - np.eye(3)).max() < 1e-14
        assert np.abs(Ri @ P[3] + P[7]).max() < 1e-14


def test_swept_box_holds_every_corner_at_every_time(pt):
    rng = np.random.default_rng(4)
    times = np.concatenate([[0.0, 1.0], rng.uniform(0.0, 1.0, size=510)])
    for case in range(200):
        axis, a0, a1, tr0, tr1 = _keys(rng)
        if case % 4 == 0:
            a1 = a0                                                          # translates only
        lo = rng.uniform(-3.0, 3.0, size=3)
        box = np.concatenate([lo, lo + rng.uniform(0.0, 2.0, size=3)])
        got = pt.motion_swept_box(box, axis, a0, a1, tr0, tr1)
        cs = MR.corners(box)
        for t in times:
            w = MR.to_world(pt.motion_pose(axis, a0, a1, tr0, tr1, t), cs)
            assert (w >= got[:3]).all() and (w <= got[3:]).all(), (case, t)
        if a0 == a1:
            P0, P1 = pt.motion_pose(axis, a0, a1, tr0, tr1, 0.0), pt.motion_pose(axis, a0, a1, tr0, tr1, 1.0)
            np.testing.assert_array_equal(got, MR.union(MR.xform_box(box, P0), MR.xform_box(box, P1)))
        else:
            np.testing.assert_allclose(got, MR.swept_box(box, axis, a0, a1, tr0, tr1), rtol=0.0, atol=1e-12)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def _exe(pt):
    return os.path.join(os.path.dirname(pt.__file__), "pt_render")


@pytest.mark.parametrize("value", ["", "0.5", "0.2,0.1", "-0.1,0.5", "0,1.5", "a,b", "0,1,2", "nan,1", "0.1,"])
def test_cli_refuses_bad_shutter(pt, value):
    r = subprocess.run([_exe(pt), "-s", "3", "--shutter", value], capture_output=True, text=True, timeout=60)   # status 2 before any device is opened
    assert r.returncode == 2 and "--shutter must be OPEN,CLOSE with 0 <= OPEN <= CLOSE <= 1" in r.stderr, (value, r.returncode, r.stderr)


@pytest.mark.parametrize("value", ["", "1", "1,2", "1,2,x", "1,2,3,4,5", "inf,0,0", "1,2,3,"])
def test_cli_refuses_bad_motion(pt, value):
    r = subprocess.run([_exe(pt), "-s", "3", "--motion", value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--motion must be DX,DY,DZ[,DEGREES]: finite numbers" in r.stderr, (value, r.returncode, r.stderr)


def test_cli_help_lists_shutter_and_motion(pt):
    r = subprocess.run([_exe(pt), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--shutter OPEN,CLOSE" in r.stdout and "--motion DX,DY,DZ[,DEGREES]" in r.stdout
    assert "--stats" in r.stdout                                           # (tools/motion_eval.py reads the line it prints)


# ---- mirrors of the sources ------------------------------------------------------------------------------------------------------------
def shade_form_exists(variant, lights, pixel_list, qmc, mode, motion=False):
    """csrc/pt_forms.h shade_form_exists, restated."""
    return ((variant in (22, 32, 42) or not (pixel_list or qmc or motion or mode != "PLAIN")) and (mode != "LSE" or lights)
            and (not motion or mode == "PLAIN"))


REFUSED_WITH_MOTION = ("environment importance sampling", "participating media or a glass interior", "exact light sampling", "spectral dispersion")


def test_mirrors_agree_with_the_sources(pt):
    csrc = os.path.join(os.path.dirname(pt.__file__), "csrc")
    forms = open(os.path.join(csrc, "pt_forms.h")).read()
    body = re.search(r"constexpr bool shade_form_exists\(const ShadeShape& s, bool lights, bool list, bool qmc, ShadeMode mode, bool motion = false\) \{(.*?)\n\}", forms, flags=re.S).group(1)
    expr = re.sub(r"\s+", " ", body)
    assert expr.strip() == ("return (s.variant == 22 || s.variant == 32 || s.variant == 42 || !(list || qmc || motion || mode != MODE_PLAIN)) && "
                            "(mode != MODE_LSE || lights) && (!motion || mode == MODE_PLAIN);")
    n = sum(shade_form_exists(v, l, p, q, m, True) for v in (2, 3, 12, 13, 22, 32, 52) for l in (False, True) for p in (False, True) for q in (False, True)
            for m in ("PLAIN", "ENV", "MED", "HET", "INT", "LSE", "DSP"))
    assert n == 16                                                          # shapes 22 / 32 x lights x list x qmc, plain mode
    for v in (2, 22):                                                       # without motion it is the existing predicate
        for m in ("PLAIN", "LSE"):
            assert shade_form_exists(v, True, False, False, m) == shade_form_exists(v, True, False, False, m, False)
    render = open(os.path.join(csrc, "pt_render.cpp")).read()
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for what in REFUSED_WITH_MOTION:
        assert f'"pt_render: motion together with {what} is not supported' in render, what
    rule = re.sub(r"\s*\*\s*", " ", header)
    assert "a render returns -1 when environment importance sampling, any participating or interior medium, exact light sampling or dispersion is in effect too" in rule


def test_the_vectorised_restatement_is_the_scalar_one():
    rng = np.random.default_rng(5)
    axis, a0, a1, tr0, tr1 = _keys(rng)
    times = rng.uniform(0.0, 1.0, size=64)
    P = MR.poses_at(axis, a0, a1, tr0, tr1, times)
    o, d = rng.uniform(-1.0, 1.0, size=(64, 3)) + np.array([0.0, 0.0, -8.0]), rng.normal(size=(64, 3)) * 0.2 + np.array([0.0, 0.0, 1.0])
    quad = ((-2.0, -2.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0))
    hit, margin = MR.hit_parallelogram_many(*quad, P, o, d)
    assert hit.any() and not hit.all()
    for i, t in enumerate(times):
        np.testing.assert_array_equal(P[i], MR.pose_at(axis, a0, a1, tr0, tr1, t))
        h, m = MR.hit_parallelogram(*quad, P[i], o[i], d[i])
        assert h == hit[i] and abs(m - margin[i]) <= 1e-12
