"""Light shafts (pt_scene_set_punctual_media) without a device: the rule's additions (tests/shafts_rule.py) are unbiased —
a Monte Carlo of the rule with numpy's own generator against a quadrature of the single-scattering integral —, the bounce word's layout
round-trips over the corners of its fields, and the ABI: symbols, bindings, the header's text, the null arguments, and (where a device
exists) the setter and getter."""
import itertools
import os

import numpy as np
import pytest

import punctual_rule as PR
import shafts_rule as SH

NEW_SYMBOLS = ("pt_scene_set_punctual_media", "pt_scene_punctual_media")

# ---- the single-scattering configuration shared with tests/test_shafts_gpu.py ------------------------------------------------------------
DENSITY, ALBEDO, T_WALL = 0.45, (0.9, 0.8, 0.7), 4.0
RAY_O, RAY_D = np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
POINT = dict(kind=0, pos=np.array([0.7, 0.3, 1.8]), axis=np.zeros(3), I=PR.point_intensity((60.0, 50.0, 40.0)), cos_i=0.0, cos_o=0.0)
SPOT_AXIS = np.array([-0.9, -0.2, 0.3]) / np.linalg.norm([-0.9, -0.2, 0.3])
SPOT = dict(kind=1, pos=np.array([0.9, 0.2, 1.5]), axis=SPOT_AXIS, I=np.array([9.0, 8.0, 7.0]), cos_i=float(np.cos(np.radians(20.0))), cos_o=float(np.cos(np.radians(40.0))))
LIGHTS = {"point": POINT, "spot": SPOT}


def closest_approach(o, d, T, p):
    s = np.clip((p - o) @ d, 0.0, T)
    return float(np.linalg.norm(o + s * d - p))


@pytest.mark.parametrize("g", [0.0, 0.6])
@pytest.mark.parametrize("light", ["point", "spot"])
def test_the_rule_is_unbiased(light, g):
    """max_depth = 2: the expectation of the rule is single scattering from the camera ray,
    L_c = int_0^T sigma e^(-sigma s) albedo_c ph(dot(d, w(s))) E_c(x(s)) e^(-sigma r(s)) ds. 16 batches, |z| < 5 per channel; the batches'
    standard error below 3 % of the expected value, so that an estimate of zero cannot pass."""
    rec, f = LIGHTS[light], 0.5
    assert closest_approach(RAY_O, RAY_D, T_WALL, rec["pos"]) >= 0.5
    if light == "spot":                                                     # a smooth-edged cone that the ray enters and leaves
        assert rec["cos_i"] > rec["cos_o"]
        _, _, _, E = PR.light_eval(rec, RAY_O[None, :] + np.linspace(0.0, T_WALL, 400)[:, None] * RAY_D[None, :])
        assert (E[:, 0] == 0.0).any() and (E[:, 0] > 0.0).any()
    want, change = SH.single_scatter_expected(RAY_O, RAY_D, T_WALL, DENSITY, ALBEDO, g, rec)
    print(f"{light} g={g}: quadrature {want}, relative change on doubling the panels {change:.2e}")
    assert change < 1e-8 and (want > 0.0).all()
    # the wall: the plane z = T_WALL (its black quad is far wider than anything here); shadow rays that run away from the light never matter
    def wall(x, w):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (T_WALL - x[:, 2]) / w[:, 2]
        return np.where(np.isfinite(t) & (t > 1e-3), t, np.inf)
    rng = np.random.default_rng(2024)
    n_batches, per_batch = 16, 200_000
    batches = np.stack([SH.single_scatter_mc(rng, per_batch, RAY_O, RAY_D, T_WALL, DENSITY, ALBEDO, g, rec, f, wall).mean(axis=0) for _ in range(n_batches)])
    mean, sem = batches.mean(axis=0), batches.std(axis=0, ddof=1) / np.sqrt(n_batches)
    z = (mean - want) / sem
    print(f"  Monte Carlo {mean}, standard error {sem} ({(sem / want).max():.2%} of the value), z {z}")
    assert (sem < 0.03 * want).all() and (np.abs(z) < 5.0).all(), (z, sem / want)


def test_blocked_and_beyond():
    """the resolution's pieces: t_end, a collision below it, a surface beyond the light"""
    t, dl = np.array([1.0, 3.0, np.inf, np.inf]), np.array([2.0, 2.0, 2.0, np.inf])
    np.testing.assert_array_equal(SH.segment_end(t, dl), [1.0, 2.0, 2.0, np.inf])
    np.testing.assert_array_equal(SH.blocked(np.array([0.5, 2.0, 1.9, 1e300]), SH.segment_end(t, dl)), [True, False, True, True])   # a sun in an unbounded medium: always blocked
    np.testing.assert_array_equal(PR.visible(t, dl), [False, True, True, True])
    thr = SH.vertex_throughput(np.array([0.5, 0.5, 0.5]), (0.8, 0.6, 0.4), np.array([0.25]), np.array([[2.0, 4.0, 8.0]]), 0.5, 4)
    np.testing.assert_array_equal(thr, [[((0.5 * (0.8 * 0.25)) * 2.0) / 0.125, ((0.5 * (0.6 * 0.25)) * 4.0) / 0.125, ((0.5 * (0.4 * 0.25)) * 8.0) / 0.125]])


def test_word_layout_round_trips():
    corners = itertools.product((0, 1, SH.MAX_DEPTH - 1, SH.MAX_DEPTH), (0, 1, 2047, SH.MAX_MEDIUM), (False, True), (0, 1, 1024, SH.MAX_LIGHTS - 1))
    seen = set()
    for bounce, medium, shadow, k in corners:
        w = SH.pack(bounce, medium, shadow, k)
        assert 0 <= w < SH.SLOT_IDLE, (bounce, medium, shadow, k)             # never one of the two words that are no path state
        assert SH.unpack(w) == (bounce, medium, shadow, k if shadow else 0)
        if shadow:
            assert w not in seen
            seen.add(w)
        else:
            assert w == bounce | (medium << 20)                              # without a segment: the media forms' word, so K1 needs no form
    assert SH.pack(0, 5, False, 0) == 5 << 20                                 # a camera ray inside medium 5
    assert (SH.MAX_DEPTH, SH.MAX_LIGHTS, SH.MAX_MEDIUM) == (255, 2048, 4094)
    assert (SH.BOUNCE_BITS, SH.INDEX_SHIFT + SH.INDEX_BITS, SH.SHADOW_BIT + 1, SH.MEDIUM_SHIFT + SH.MEDIUM_BITS) == (SH.INDEX_SHIFT, SH.SHADOW_BIT, SH.MEDIUM_SHIFT, 32)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thu-acg-f2024-path-tracer_amd", "csrc", "pt_types.h")).read()
    assert "SHF_SHADOW_BIT = 1u << 19, SHF_INDEX_SHIFT = 8, SHF_BOUNCE_MASK = (1u << SHF_INDEX_SHIFT) - 1u" in src and "MEDIUM_SHIFT = 20" in src


def test_symbols_bindings_and_header(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pt.ABI_SYMBOLS and hasattr(pt.lib, sym) and sym + "(" in header, sym
        assert getattr(pt.lib, sym).argtypes is not None, sym
    assert hasattr(pt.Scene, "set_punctual_media") and hasattr(pt.Scene, "punctual_media")
    for text in ("thr' = ((thr * (albedo * ph)) * E) / pm", "t_end = t < D' ? t : D'", "BLOCKED", "max_depth must be at most 255", "always blocked",
                 "one bounce of depth per boundary", "The selector draw r is READ"):
        assert text in header, text
    hpp = open(os.path.join(os.path.dirname(pt.__file__), "host", "pt.hpp")).read()
    assert "punctual_media" in hpp and "pt_scene_set_punctual_media(" in hpp
    for doc, texts in (("INTEGRATION.md", ("pt_scene_set_punctual_media",)), ("README.md", ("--light-shafts",)), ("DESIGN.md", ("## 22", "pt_scene_set_punctual_media"))):
        body = open(os.path.join(pt.REPO_ROOT, doc)).read()
        for text in texts:
            assert text in body, (doc, text)


def test_null_scene_is_refused(pt):
    assert pt.lib.pt_scene_set_punctual_media(None, 1) == -1 and b"null scene" in pt.lib.pt_last_error()
    assert pt.lib.pt_scene_punctual_media(None) == -1


def test_setter_and_getter(pt):
    try:
        ctx = pt.Context(0)
    except pt.PtError as e:
        assert "no HIP device" in str(e)
        pytest.skip("a scene needs a context, and a context a device")
    gs = pt.Scene(ctx)
    assert gs.punctual_media() == 0
    gs.set_punctual_media(1)
    assert gs.punctual_media() == 1
    for bad in (2, -1, 255):
        with pytest.raises(pt.PtError, match="0 or 1"):
            gs.set_punctual_media(bad)
        assert gs.punctual_media() == 1
    gs.set_punctual_media(0)
    assert gs.punctual_media() == 0
    gs.close(); ctx.close()
