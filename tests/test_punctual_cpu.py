"""Punctual lights (pt_light_point, pt_light_spot, pt_light_directional) without a device: the ABI symbols, bindings and the
header's text, the host mirror of the device's light evaluation against the numpy restatement of the rule (tests/punctual_rule.py) bit for
bit, the expectation of the punctual branch by quadrature, and the CLI's arguments."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import punctual_rule as PR

NEW_SYMBOLS = ("pt_light_point", "pt_light_spot", "pt_light_directional", "pt_scene_clear_punctual_lights", "pt_scene_punctual_count",
               "pt_scene_punctual_light", "pt_scene_set_punctual_fraction", "pt_scene_punctual_fraction", "pt_punctual_probe", "pt_punctual_eval")
D3 = C.c_double * 3


def test_symbols_bindings_and_header(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pt.ABI_SYMBOLS and hasattr(pt.lib, sym) and sym + "(" in header, sym
        assert getattr(pt.lib, sym).argtypes is not None, sym
    assert pt.lib.pt_scene_punctual_fraction.restype is C.c_double
    assert len(pt.lib.pt_light_spot.argtypes) == 6 and len(pt.lib.pt_punctual_probe.argtypes) == 5 and len(pt.lib.pt_punctual_eval.argtypes) == 3
    for method in ("light_point", "light_spot", "light_directional", "clear_punctual_lights", "punctual_light", "punctual_count",
                   "set_punctual_fraction", "punctual_fraction", "punctual_probe"):
        assert hasattr(pt.Scene, method), method
    assert callable(pt.punctual_eval)
    # the rule, as the issue states it
    for text in ("I_c = power_c / (4 * PI)", "axis = normalize(target - position)", "0 <= inner_deg <= outer_deg < 180", "p_light = lights ? (1 - f) / 2 : 0",
                 "p_bsdf = 1 - p_light - p_punct", "fall = (s * s) * (3 - 2 * s)", "pm = f / (double)n", "thr' = ((thr * e) * E) / pm",
                 "hit.dist >= D'", "max_depth >= 2^20", "n <= 2048", "The sky", "Selection is uniform, not by power"):
        assert text in header, text
    hpp = open(os.path.join(os.path.dirname(pt.__file__), "host", "pt.hpp")).read()
    for text in ("struct PointLight", "struct SpotLight", "struct DirectionalLight", "add_punctual", "punctual_fraction", "pt_light_point("):
        assert text in hpp, text
    for doc, texts in (("INTEGRATION.md", ("light.rs", "pt_light_point")), ("README.md", ("pt_light_point", "--point-light")), ("DESIGN.md", ("## 21", "light.rs"))):
        body = open(os.path.join(pt.REPO_ROOT, doc)).read()
        for text in texts:
            assert text in body, (doc, text)


def test_null_arguments_are_refused(pt):
    lib, z = pt.lib, D3(0.0, 0.0, 0.0)
    one = D3(1.0, 1.0, 1.0)
    assert lib.pt_light_point(None, z, one) == -1 and b"null scene" in lib.pt_last_error()
    assert lib.pt_light_spot(None, z, one, 10.0, 20.0, one) == -1
    assert lib.pt_light_directional(None, one, one) == -1
    assert lib.pt_scene_clear_punctual_lights(None) == -1 and lib.pt_scene_punctual_count(None) == -1
    assert lib.pt_scene_punctual_light(None, 0, (C.c_double * 16)()) == -1
    assert lib.pt_scene_set_punctual_fraction(None, 0.5) == -1 and lib.pt_scene_punctual_fraction(None) == -1.0
    assert lib.pt_punctual_probe(None, 0, None, 0, None) == -1 and b"not built" in lib.pt_last_error()
    rec = (C.c_double * 16)()
    assert lib.pt_punctual_eval(None, z, (C.c_double * 7)()) == -1 and lib.pt_punctual_eval(rec, None, (C.c_double * 7)()) == -1
    assert lib.pt_punctual_eval(rec, z, None) == -1
    rec[0] = 3.0
    assert lib.pt_punctual_eval(rec, z, (C.c_double * 7)()) == -1 and b"kind" in lib.pt_last_error()


def records():
    """One stored record per case: (name, rec16). The cosines are any two numbers in order: the rule starts from the stored ones."""
    pos, tgt = np.array([0.3, 1.7, -0.2]), np.array([0.1, 0.0, 0.4])
    axis = PR.LR.normalize(tgt - pos)
    sun = PR.LR.normalize(np.array([0.3, -1.0, 0.2]))
    z4 = [0.0] * 4

    def rec(kind, p, a, I, ci, co):
        return np.array([kind, *p, *a, *I, ci, co, *z4], dtype=np.float64)

    return [("point", rec(0, pos, (0, 0, 0), PR.point_intensity((40.0, 30.0, 20.0)), 0.0, 0.0)),
            ("spot", rec(1, pos, axis, (9.0, 8.0, 7.0), math.cos(math.radians(15.0)), math.cos(math.radians(25.0)))),
            ("spot_hard_edge", rec(1, pos, axis, (9.0, 8.0, 7.0), math.cos(math.radians(20.0)), math.cos(math.radians(20.0)))),
            ("spot_wide", rec(1, pos, axis, (1.0, 2.0, 3.0), math.cos(math.radians(0.0)), math.cos(math.radians(179.0)))),
            ("sun", rec(2, (0, 0, 0), sun, (3.0, 2.5, 2.0), 0.0, 0.0))]


def cone_edge_points(rec, cos_edge, m, rng):
    """points whose direction to the light makes the angle acos(cos_edge) with the axis, up to rounding: on a cone's edge"""
    r = PR.record(rec)
    a = r["axis"]
    t = PR.LR.normalize(np.cross(a, np.array([0.0, 0.0, 1.0])))
    b = np.cross(a, t)
    phi = rng.uniform(0.0, 2.0 * math.pi, m)
    dist = rng.uniform(0.2, 6.0, m)
    sin_e = math.sqrt(max(0.0, 1.0 - cos_edge * cos_edge))
    d = a[None, :] * cos_edge + (t[None, :] * np.cos(phi)[:, None] + b[None, :] * np.sin(phi)[:, None]) * sin_e
    return r["pos"][None, :] + d * dist[:, None]


def test_host_mirror_equals_the_rule_bit_for_bit(pt):
    rng = np.random.default_rng(2106)
    for name, rec in records():
        r = PR.record(rec)
        pts = [rng.uniform(-4.0, 4.0, (4096 - 1024 - 1, 3))]
        if r["kind"] == 1:
            pts += [cone_edge_points(rec, r["cos_i"], 512, rng), cone_edge_points(rec, r["cos_o"], 512, rng)]
        else:
            pts += [rng.normal(0.0, 1e-3, (1024, 3)) + r["pos"]]
        pts += [r["pos"][None, :]]                                         # the light's own position: d2 = 0
        pts = np.concatenate(pts)
        assert len(pts) == 4096
        want = PR.eval7(r, pts)
        got = np.stack([pt.punctual_eval(rec, p) for p in pts])
        assert got.tobytes() == want.tobytes(), (name, np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0][:5])
        if r["kind"] == 1:
            # both sides of both edges occur among the edge points, and inner == outer gives only 0 and 1
            w, _, d2, E = PR.light_eval(r, pts[:-1])
            fall = E[:, 0] * d2 / r["I"][0]
            assert (fall == 0.0).any() and (fall > 0.0).any()
            if name == "spot_hard_edge":
                assert set(np.unique(np.round(fall, 9))) <= {0.0, 1.0}
        if r["kind"] != 2:
            assert got[-1, 3] == 0.0 and np.isnan(got[-1, 0])              # at the light: D = 0, w = 0 / 0 (the branch ends the path there)


def test_branch_expectation_by_quadrature():
    """E[sample's punctual contribution] = sum_k e_k * E_k for n = 1, 3, 7 lights, f = 0.25, 0.5 and with / without a lights list: a midpoint grid
    over the selector draw r and over the index draw's 64-bit value (rejected values are left out: the draws that follow are independent and
    identically distributed, so the accepted values' distribution is the draw's). The selector grid has M = 4096 points, so the branch's share is
    f exactly; of the M2 = 3 * 5 * 7 * 4096 index values at least half are accepted and each light's count is off its share by at most one point
    per end of its interval: relative error <= 4 n / M2 < 7e-5. No random numbers."""
    M, M2 = 4096, 3 * 5 * 7 * 4096
    r = (np.arange(M) + 0.5) / M
    albedo, sn = (0.8, 0.6, 0.4), np.array([0.0, 1.0, 0.0])
    x = np.array([[0.4, 0.0, -0.3]])
    all_recs = [PR.record(rec) for _, rec in records()] + [PR.record(rec) for _, rec in records()[:2]]
    vals = [((2 * j + 1) << 63) // M2 for j in range(M2)]                 # (j + 1/2) * 2^64 / M2
    for n in (1, 3, 7):
        recs = all_recs[:n]
        eE = []
        for rec in recs:
            w, D, d2, E = PR.light_eval(rec, x)
            eE.append((PR.lambert_eval(albedo, sn, w) * E)[0])
        want = np.sum(eE, axis=0)
        zone = ((n << (64 - n.bit_length())) - 1) & PR.MASK64
        ks = np.array([(v * n) >> 64 for v in vals if ((v * n) & PR.MASK64) <= zone])
        assert len(ks) * 2 >= M2
        for f in (0.25, 0.5):
            for lights in (False, True):
                share = np.mean(PR.branch_of(r, f, lights) == 1)
                assert share == f
                contrib = np.stack([PR.branch_throughput(np.ones(3), PR.lambert_eval(albedo, sn, PR.light_eval(rec, x)[0])[0], PR.light_eval(rec, x)[3][0], f, n)
                                    for rec in recs])
                got = share * contrib[ks].mean(axis=0)
                np.testing.assert_allclose(got, want, rtol=4.0 * n / M2, atol=0.0)


def test_cli_arguments(pt):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    run = lambda *a: subprocess.run([exe, *a], capture_output=True, text=True, timeout=60)
    assert "--point-light X,Y,Z,R,G,B" in run("--help").stdout and "--punctual-fraction F" in run("--help").stdout
    for bad in (("--point-light", "1,2,3"), ("--point-light", "1,2,3,4,5,x"), ("--spot-light", "0,1,0,0,0,0,10,20,1,1"), ("--sun", "0,-1,0,1,1,nan"),
                ("--punctual-fraction", "0"), ("--punctual-fraction", "1"), ("--punctual-fraction", "abc"),
                ("--point-light", "0,1,0,1,1,1", "--env-sampling", "0.5"), ("--sun", "0,-1,0,1,1,1", "--motion", "1,0,0")):
        p = run(*bad)
        assert p.returncode == 2 and p.stderr.strip(), bad
