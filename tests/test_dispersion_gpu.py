"""Spectral dispersion of glass on the GPU (pt_mat_glass_set_dispersion; the rule is in include/pt_amd.h): validation,
the probe against the rule's restatement (tests/dispersion_rule.py), "off means off", the weight applied once and no draw moved, a
dispersive slab between two environment tones against quadrature, a scalar replay of whole paths through a rough dispersive sphere,
the structural identities (pixel lists, modes, adaptive, sample ranges, window sizes), the refusals at the render and the CLI.

Which k_shade shape a render launched: the DSP forms exist for the two window sizes of variant 42. Every render below but one has fewer
than blocks_shade * 16 windows of 8192 slots and launches the 4096-slot shape (22); the full-HD render runs once more with
PT_WIDE_WINDOW_MIN=1 and then launches the 8192-slot shape (32). window_slots() says which."""
import os
import subprocess

import numpy as np
import pytest

import dispersion_rule as DR
import refs_numpy as R
from common import SceneSpec, default_camera

pytestmark = pytest.mark.gpu

UPPER, LOWER = 255, 51                                       # the two-tone environment map's rows (RGB8)
TONE = lambda v: (1.0 / 255.0) * v                           # tex_image's RGB8 -> f64


def build(pt, ctx, spec):
    gs = pt.Scene(ctx)
    res = spec.replay(gs)
    return gs, spec.make_camera(pt.Camera, res), res


def window_slots(st, wide_window_min=16):
    """The window size of the render's first k_shade launch (launch_shade's rule for variant 42)."""
    n_alloc = (st.n_slots + 8191) // 8192 * 8192
    return 8192 if n_alloc // 8192 >= st.blocks_shade * wide_window_min else 4096


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def two_tone_map():
    img = np.empty((2, 4, 3), dtype=np.uint8)
    img[0], img[1] = UPPER, LOWER
    return img


# ---- 1. validation -------------------------------------------------------------------------------------------------------------------
def test_validation(pt, ctx):
    gs = pt.Scene(ctx)
    nan, inf = float("nan"), float("inf")
    one, rough = gs.tex_solid_rgb(1.0, 1.0, 1.0), gs.tex_solid_f(0.1)
    white = gs.mat_diffuse(one, -1)
    fog = gs.mat_medium(0.5, (1.0, 1.0, 1.0), 0.0)
    glass = gs.mat_glass(one, rough, 0.0, 1.5)
    assert gs.mat_glass_dispersion(glass) == 0.0               # off by default
    for bad_glass in (white, fog, 99, -1):
        with pytest.raises(pt.PtError):
            gs.mat_glass_set_dispersion(bad_glass, 20.0)
        assert gs.mat_glass_dispersion(bad_glass) == -1.0
    with pytest.raises(pt.PtError):
        gs.dispersion_probe(glass, 1, np.array([500.0]))        # the probe refuses a glass that does not disperse
    gs.mat_glass_set_dispersion(glass, 20.0)
    assert gs.mat_glass_dispersion(glass) == 20.0
    for bad in (-1.0, -0.0001, nan, inf, -inf, 0.2):            # 0.2: n(730) = 1.5 - 1.34 < 1
        with pytest.raises(pt.PtError):
            gs.mat_glass_set_dispersion(glass, bad)
        assert gs.mat_glass_dispersion(glass) == 20.0           # a refused call leaves the setting
    assert DR.ior(1.5, 0.2, 730.0) <= 1.0
    air = gs.mat_glass(one, rough, 0.0, 1.0)                    # n_d = 1: b = 0, n(lambda) = 1 everywhere — not above 1
    with pytest.raises(pt.PtError):
        gs.mat_glass_set_dispersion(air, 50.0)
    assert gs.mat_glass_dispersion(air) == 0.0
    for v in (60.0, 1e30, 0.0, 35.5):                           # the getter round-trips; 0 clears
        gs.mat_glass_set_dispersion(glass, v)
        assert gs.mat_glass_dispersion(glass) == v
    n_before = gs.mat_diffuse(one, -1)
    for a, b in ((white, glass), (glass, white)):               # a dispersive glass is no mix child, in either place
        with pytest.raises(pt.PtError):
            gs.mat_mix(0.5, a, b)
    assert gs.mat_diffuse(one, -1) == n_before + 1              # the refused calls created nothing
    gs.mat_glass_set_dispersion(glass, 0.0)
    glass2 = gs.mat_glass(one, rough, 0.0, 1.3)
    mix = gs.mat_mix(0.5, white, glass)                         # cleared, the glass mixes as before
    mix2 = gs.mat_mix(0.5, white, gs.mat_mix(0.25, glass2, white))
    assert mix2 == mix + 2
    for g in (glass, glass2):                                   # ... and is then refused a dispersion, one level down or two
        with pytest.raises(pt.PtError):
            gs.mat_glass_set_dispersion(g, 20.0)
        assert gs.mat_glass_dispersion(g) == 0.0
    with pytest.raises(pt.PtError):
        gs.dispersion_probe(glass, 0, np.array([[0.0, 0.0]]))
    free = gs.mat_glass(one, rough, 0.0, 1.5)
    gs.mat_glass_set_dispersion(free, 20.0)
    with pytest.raises(pt.PtError):
        gs.dispersion_probe(free, 2, np.array([500.0]))         # which
    with pytest.raises(pt.PtError):
        gs.dispersion_probe(free, 0, np.array([[0.5, 0.0]]))    # (pixel, sample) are integers
    gs.close()


# ---- 2. the probe against the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, (5 << 32) | 9])
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_probe_against_the_rule(pt, ctx, sampler, seed):
    n, n_d, abbe = 4096, 1.62, 36.0
    rng = np.random.default_rng(seed & 0xFFFF)
    ps = np.stack([rng.integers(0, 1 << 31, n), rng.integers(0, 1 << 20, n)], axis=1).astype(np.float64)
    ps[:4] = [[0, 0], [4294967295, 0], [0, 4294967295], [4294967295, 4294967295]]
    ps[4:260, 0], ps[4:260, 1] = 12345, np.arange(256)          # an aligned block of one pixel
    gs = pt.Scene(ctx)
    gs.set_sampler(sampler)
    glass = gs.mat_glass(gs.tex_solid_rgb(1.0, 1.0, 1.0), gs.tex_solid_f(0.1), 0.0, n_d)
    gs.mat_glass_set_dispersion(glass, abbe)
    out = gs.dispersion_probe(glass, 0, ps, seed=seed)
    assert out.shape == (n, 7)
    u, lam, j = DR.wavelength(seed, ps[:, 0].astype(np.uint64), ps[:, 1].astype(np.uint64), sobol=sampler == "sobol")
    np.testing.assert_array_equal(out[:, 0], u)
    np.testing.assert_array_equal(out[:, 2], j)
    want_n = DR.ior(n_d, abbe, lam)
    err_l, err_n = np.abs(out[:, 1] / lam - 1.0).max(), np.abs(out[:, 6] / want_n - 1.0).max()
    W = DR.weight_table()
    pos = W[j] > 0.0
    err_w = np.abs(out[:, 3:6][pos] / W[j][pos] - 1.0).max()
    print(f"{sampler}, seed {seed:#x}: max relative error lambda {err_l:.3g}, n(lambda) {err_n:.3g}, W {err_w:.3g}")
    assert err_l <= 1e-15 and err_n <= 1e-15
    np.testing.assert_allclose(out[:, 3:6], W[j], rtol=1e-12, atol=0.0)
    if sampler == "sobol":                                      # the aligned block: one wavelength per stratum of width 2^-8
        assert (np.sort(np.floor(out[4:260, 0] * 256)) == np.arange(256)).all()
    lams = np.linspace(380.0, 730.0, n)
    got = gs.dispersion_probe(glass, 1, lams)
    err = np.abs(got / DR.ior(n_d, abbe, lams) - 1.0).max()
    print(f"which 1: max relative error {err:.3g}; n(380) {got[0]:.6f}, n(730) {got[-1]:.6f}")
    assert err <= 1e-15 and lams[0] == 380.0 and lams[-1] == 730.0
    assert gs.dispersion_probe(glass, 1, np.array([DR.LAMBDA_D]))[0] == n_d
    gs.close()


# ---- 3. off means off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
@pytest.mark.parametrize("how", ["set_and_cleared", "unused_material"])
@pytest.mark.parametrize("which", [1, 6])
def test_dispersion_not_in_effect_changes_nothing(pt, ctx, which, how, sampler):
    def scene(extras):
        gs = pt.Scene(ctx)
        cam = gs.build_scene(which, 64, 8)
        glass = gs.mat_glass(gs.tex_solid_rgb(1.0, 1.0, 1.0), gs.tex_solid_f(0.001), 0.0, 1.5)
        gs.world_add_object(gs.sphere(1e-3, (0.0, -5000.0, 0.0), (0.0, -5000.0, 0.0), glass))
        spare = gs.mat_glass(gs.tex_solid_rgb(1.0, 1.0, 1.0), gs.tex_solid_f(0.2), 0.0, 1.7)      # used by nothing
        if extras and how == "set_and_cleared":
            gs.mat_glass_set_dispersion(glass, 20.0)
            gs.world_build()
            gs.mat_glass_set_dispersion(glass, 0.0)
        if extras and how == "unused_material":
            gs.mat_glass_set_dispersion(spare, 20.0)
        gs.world_build()
        gs.set_sampler(sampler)
        return gs, cam

    a, cam_a = scene(False)
    b, cam_b = scene(True)
    ra, sa = a.render(cam_a, 3, 0, 8, slots_per_pixel=1)
    rb, sb = b.render(cam_b, 3, 0, 8, slots_per_pixel=1)
    assert (sa.segments, sa.shade_variant, sa.launches_shade, sa.launches_extend) == (sb.segments, sb.shade_variant, sb.launches_shade, sb.launches_extend)
    np.testing.assert_array_equal(rb, ra)
    da, ta = a.render(cam_a, 3, 0, 8)
    db, tb = b.render(cam_b, 3, 0, 8)
    assert (ta.segments, ta.shade_variant, ta.launches_shade) == (tb.segments, tb.shade_variant, tb.launches_shade)
    fin = np.isfinite(da)
    np.testing.assert_allclose(db[fin], da[fin], rtol=1e-12, atol=1e-12)
    a.close(); b.close()


# ---- the scene of 4., 7. and 8.: a rough glass sphere over a diffuse floor under a quad light ------------------------------------------------
def ball_scene(abbe, width=32, aspect=1.0, max_depth=6, env_map=False, extra=None):
    spec = SceneSpec()
    tex = spec.add("tex_image_rgb8", two_tone_map()) if env_map else -1
    one = spec.add("tex_solid_rgb", 1.0, 1.0, 1.0)
    if extra in ("fog", "grid", "interior"):                    # (a medium's handle must be small: created first)
        if extra == "grid":
            med = spec.add("mat_medium_grid", 0.3, (0.8, 0.8, 0.8), 0.0, np.ones((2, 2, 2), dtype=np.float32), (-3.0, 0.0, -3.0), (3.0, 3.0, 3.0))
        else:
            med = spec.add("mat_medium", 0.2, (0.8, 0.8, 0.8), 0.0)
    floor = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.7, 0.6, 0.5), -1)
    glass = spec.add("mat_glass", one, spec.add("tex_solid_f", 0.1), 0.0, 1.5)
    if abbe:
        spec.add("mat_glass_set_dispersion", glass, abbe)
    if extra == "interior":
        spec.add("mat_glass_set_interior", glass, med)
    spec.add("world_add_object", spec.add("quad", (-8.0, 0.0, -8.0), (0.0, 0.0, 16.0), (16.0, 0.0, 0.0), floor))
    spec.add("world_add_object", spec.add("sphere", 1.0, (0.0, 1.05, 0.0), (0.0, 1.05, 0.0), glass))
    if extra in ("fog", "grid"):
        spec.add("world_add_object", spec.add("cuboid", (-3.0, 0.01, -3.0), (3.0, 3.0, 3.0), med))
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", 9.0, 8.0, 7.0))
    spec.add("world_add_light", spec.add("quad", (-1.0, 4.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), lm))
    if extra == "sphere_light":
        spec.add("world_add_light", spec.add("sphere", 0.3, (2.0, 3.0, 0.0), (2.0, 3.0, 0.0), lm))
    spec.add("world_build")
    spec.camera = default_camera(width=width, aspect=aspect, spp=1, look_from=(0.0, 1.6, -6.0), look_at=(0.0, 1.0, 0.0), vfov=30.0, focal_length=1.0,
                                 defocus_angle=0.0, env_color=(0.5, 0.6, 0.8), max_depth=max_depth, env_is_map=1 if env_map else 0, env_tex=tex)
    return spec


# ---- 4. W once, and no draw moved ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_weighted_once_and_no_draw_moved(pt, ctx, sampler):
    """abbe = 1e30: n(lambda) == n_d exactly, so every path is the plain render's path, draw for draw (max_depth 6: no roulette, whose
    probability the weight would change). A path adds radiance once, where it ends (a light or the environment): the dispersive sample is
    the plain one, or the plain one times its wavelength's row of W — applied once, though a path through the sphere meets glass at least
    twice (W twice would show as W^2)."""
    seed, n = 11, 64
    plain, pcam, _ = build(pt, ctx, ball_scene(0.0))
    disp, dcam, _ = build(pt, ctx, ball_scene(1e30))
    for gs in (plain, disp):
        gs.set_sampler(sampler)
    H = W = 32
    pix = np.arange(H * W, dtype=np.uint64)
    table = DR.weight_table()
    n_same = n_weighted = n_dark = 0
    worst = 0.0
    for s in range(n):
        a, sa = plain.render(pcam, seed, s, s + 1, slots_per_pixel=1)
        b, sb = disp.render(dcam, seed, s, s + 1, slots_per_pixel=1)
        assert sa.segments == sb.segments and window_slots(sb) == 4096
        a, b = a.reshape(-1, 3), b.reshape(-1, 3)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        _, _, j = DR.wavelength(seed, pix, np.uint64(s), sobol=sampler == "sobol")
        want = a * table[j]
        same = (a == b).all(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(want != 0.0, np.abs(b / want - 1.0), np.where(b == 0.0, 0.0, np.inf)).max(axis=1)
        weighted = ~same & (rel <= 1e-13)
        assert (same | weighted).all(), (s, np.flatnonzero(~(same | weighted))[:5], a[~(same | weighted)][:3], b[~(same | weighted)][:3])
        dark = (a == 0.0).all(axis=1)
        worst = max(worst, rel[weighted].max() if weighted.any() else 0.0)
        n_dark += dark.sum()
        n_same += (same & ~dark).sum()
        n_weighted += weighted.sum()
    total = n * H * W
    print(f"{sampler}: {total} (pixel, sample) pairs: {n_same} unweighted, {n_weighted} weighted once (max relative error {worst:.3g}), {n_dark} without radiance")
    assert n_same >= 0.05 * total and n_weighted >= 0.05 * total
    plain.close(); disp.close()


# ---- 5. the two-tone slab against quadrature -----------------------------------------------------------------------------------------------
SLAB_W, SLAB_N_D, SLAB_ABBE = 32, 1.5, 10.0


def test_two_tone_slab_against_quadrature(pt, ctx):
    """test_interior_gpu.py's slab turned horizontal, seen from above at about 55 degrees: a reflected path leaves into the bright upper
    half of the map, a transmitted one into the dark lower half, and R depends on n(lambda) — so the channels come out different.
    The n == n_d expectation is asserted to lie more than 6 standard errors of the frame mean away in at least one channel (blue: the
    red channel cannot, n_d sits near the middle of its weights) — a kernel that weights but does not disperse fails the z-test."""
    n = 4096
    spec = SceneSpec()
    tex = spec.add("tex_image_rgb8", two_tone_map())
    glass = spec.add("mat_glass", spec.add("tex_solid_rgb", 1.0, 1.0, 1.0), spec.add("tex_solid_f", 0.001), 0.0, SLAB_N_D)
    spec.add("mat_glass_set_dispersion", glass, SLAB_ABBE)
    spec.add("world_add_object", spec.add("cuboid", (-50.0, 0.0, -50.0), (50.0, 1.0, 50.0), glass))
    spec.add("world_build")
    ang = np.radians(55.0)
    look_from, look_at = (0.0, 1.0 + 4.0 * np.cos(ang), -4.0 * np.sin(ang)), (0.0, 1.0, 0.0)
    spec.camera = default_camera(width=SLAB_W, spp=1, look_from=look_from, look_at=look_at, vfov=10.0, focal_length=1.0, defocus_angle=0.0,
                                 blur_strength=0.0, env_color=(0.0, 0.0, 0.0), max_depth=400, env_is_map=1, env_tex=tex)
    gs, cam, _ = build(pt, ctx, spec)
    fr = R.camera_frame(SLAB_W, 1.0, 10.0, look_from, look_at, (0.0, 1.0, 0.0), 1.0)
    rows, cols = np.divmod(np.arange(fr["height"] * SLAB_W), SLAB_W)
    d = fr["pixel00"] + rows[:, None] * fr["dv"] + cols[:, None] * fr["du"] - fr["center"]
    d /= np.linalg.norm(d, axis=1)[:, None]
    hits = gs.intersect(np.concatenate([np.broadcast_to(fr["center"], d.shape), d, np.zeros((len(d), 1))], axis=1))
    assert (hits[:, 0] == 1.0).all() and (hits[:, 5] == 1.0).all() and (hits[:, 10] == 1.0).all()      # every camera ray meets the top face from outside
    cos_i = (-d[:, 1]).reshape(fr["height"], SLAB_W)
    img, st = gs.render(cam, 41, 0, n)
    gs.close()
    A, B = TONE(UPPER), TONE(LOWER)
    mean, second = DR.slab_two_tone(cos_i, SLAB_N_D, SLAB_ABBE, A, B)
    flat, _ = DR.slab_two_tone(cos_i, SLAB_N_D, None, A, B)
    var = second - mean ** 2
    z = (img / n - mean) / np.sqrt(var / n)
    se_frame = np.sqrt(var.sum(axis=(0, 1)) / n) / cos_i.size
    zg = (img.mean(axis=(0, 1)) / n - mean.mean(axis=(0, 1))) / se_frame
    apart = (flat.mean(axis=(0, 1)) - mean.mean(axis=(0, 1))) / se_frame
    print(f"incidence {np.degrees(np.arccos(cos_i.min())):.1f} .. {np.degrees(np.arccos(cos_i.max())):.1f} degrees; frame mean {img.mean(axis=(0, 1)) / n}, expected "
          f"{mean.mean(axis=(0, 1))}, with n == n_d {flat.mean(axis=(0, 1))}: {apart} standard errors away; {st.segments / st.samples:.2f} segments per sample")
    assert np.abs(apart).max() > 6.0, apart
    DR.accept(z, zg)


# ---- 6. replay of whole paths -----------------------------------------------------------------------------------------------------------
REPLAY = dict(width=16, vfov=30.0, look_from=(0.0, 0.3, -4.0), look_at=(0.0, 0.0, 0.0), max_depth=12, blur_strength=0.5, center=(0.1, 0.0, 0.0), radius=0.9,
              roughness=0.1, ior=1.5, abbe=20.0, upper=(TONE(UPPER),) * 3, lower=(TONE(LOWER),) * 3)


def replay_frame():
    c = REPLAY
    fr = R.camera_frame(c["width"], 1.0, c["vfov"], c["look_from"], c["look_at"], (0.0, 1.0, 0.0), 1.0)
    return fr, dict(width=c["width"], blur_strength=c["blur_strength"], max_depth=c["max_depth"])


@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_replay_of_whole_paths(pt, ctx, sampler):
    c = REPLAY
    spec = SceneSpec()
    tex = spec.add("tex_image_rgb8", two_tone_map())
    glass = spec.add("mat_glass", spec.add("tex_solid_rgb", 1.0, 1.0, 1.0), spec.add("tex_solid_f", c["roughness"]), 0.0, c["ior"])
    spec.add("mat_glass_set_dispersion", glass, c["abbe"])
    spec.add("world_add_object", spec.add("sphere", c["radius"], c["center"], c["center"], glass))
    spec.add("world_build")
    spec.camera = default_camera(width=c["width"], spp=1, vfov=c["vfov"], look_from=c["look_from"], look_at=c["look_at"], focal_length=1.0,
                                 defocus_angle=0.0, blur_strength=c["blur_strength"], env_color=(0.0, 0.0, 0.0), max_depth=c["max_depth"], env_is_map=1, env_tex=tex)
    gs, cam, _ = build(pt, ctx, spec)
    gs.set_sampler(sampler)
    fr, rcam = replay_frame()
    H, W, seed, n_samples = fr["height"], c["width"], 9, 4
    per_sample = [gs.render(cam, seed, s, s + 1, slots_per_pixel=1)[0].reshape(-1, 3) for s in range(n_samples)]
    gs.close()
    bad, reached, coloured = [], 0, 0
    for p in range(H * W):
        for s in range(n_samples):
            want, hits = DR.replay_dispersive_path(c["center"], c["radius"], c["roughness"], c["ior"], c["abbe"], fr, rcam, seed, p, s, c["upper"], c["lower"],
                                                   sobol=sampler == "sobol")
            reached += hits > 0
            coloured += len(set(want)) > 1
            if not np.allclose(per_sample[s][p], want, rtol=1e-12, atol=0.0):
                bad.append((p, s, per_sample[s][p], want))
    print(f"{sampler}: {H * W * n_samples} (pixel, sample) pairs, {reached} reached the glass, {coloured} came out coloured, {len(bad)} disagree")
    assert H * W * n_samples == 1024 and reached > 256
    assert len(bad) == 0, bad[:5]


# ---- 7. structure, with dispersion in effect -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_structure_with_dispersion(pt, ctx, sampler):
    gs, cam, _ = build(pt, ctx, ball_scene(20.0, width=32, max_depth=50))
    plain, pcam, _ = build(pt, ctx, ball_scene(0.0, width=32, max_depth=50))
    gs.set_sampler(sampler); plain.set_sampler(sampler)
    seed, n = 7, 8
    full, st = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    base, st0 = plain.render(pcam, seed, 0, n, slots_per_pixel=1)
    assert not np.array_equal(full, base) and st.shade_variant == st0.shade_variant      # the new code does act here
    np.testing.assert_array_equal(plain.render_aovs(pcam, seed, 0, 4), gs.render_aovs(cam, seed, 0, 4))       # AOVs do not change
    plain.close()
    h, w = full.shape[:2]
    parts = np.zeros_like(full)                                  # sample ranges add up: one sample at a time, bit for bit (the same order of additions)
    for k in range(n):
        gs.render(cam, seed, k, k + 1, accum=parts, slots_per_pixel=1)
    np.testing.assert_array_equal(parts, full)
    halves = np.zeros_like(full)                                 # the denoiser's two halves are pieces of the same frame (their sums associate differently)
    gs.render(cam, seed, 0, n // 2, accum=halves, slots_per_pixel=1)
    gs.render(cam, seed, n // 2, n, accum=halves, slots_per_pixel=1)
    np.testing.assert_allclose(halves, full, rtol=1e-11, atol=1e-11)
    px = np.sort(np.random.default_rng(3).choice(h * w, 300, replace=False)).astype(np.uint32)
    sentinel = np.full_like(full, -3.25)
    lst, _ = gs.render_pixels(cam, seed, px, 0, n, accum=sentinel.copy(), slots_per_pixel=1, overwrite=True)
    mask = np.zeros(h * w, bool)
    mask[px] = True
    mask = mask.reshape(h, w)
    np.testing.assert_array_equal(lst[mask], full[mask])         # a frame against a pixel list: equal bits in static mode
    np.testing.assert_array_equal(lst[~mask], sentinel[~mask])
    assert np.isfinite(full).all()
    dyn, sd = gs.render(cam, seed, 0, n)
    assert window_slots(sd) == 4096
    np.testing.assert_allclose(dyn, full, rtol=1e-11, atol=1e-11)
    dlst, _ = gs.render_pixels(cam, seed, px, 0, n)
    np.testing.assert_allclose(dlst[mask], full[mask], rtol=1e-11, atol=1e-11)
    ada, counts, ast = gs.render_adaptive(cam, seed, 2, n, 0.0, slots_per_pixel=1)
    assert (counts == n).all() and ast.samples == counts.sum()
    np.testing.assert_allclose(ada, full, rtol=1e-11, atol=1e-11)
    comm = pt.Comm(ctx, 0, 1)
    multi, _ = gs.render_multi(cam, seed, n, comm, slots_per_pixel=1)
    comm.close()
    np.testing.assert_array_equal(multi, full)
    gs.close()


def test_full_hd_both_window_sizes(pt, ctx):
    """1920 x 1080 at 8 spp: the 8192-slot windows (shape 32, with compaction and the shading-order output moving the flag) against the
    4096-slot render (shape 22) of the same frame."""
    gs, cam, _ = build(pt, ctx, ball_scene(20.0, width=1920, aspect=16.0 / 9.0, max_depth=50))
    narrow, sn = gs.render(cam, 5, 0, 8)
    wide, sw = _with_env({"PT_EXPERIMENT": "1", "PT_WIDE_WINDOW_MIN": "1"}, lambda: gs.render(cam, 5, 0, 8))
    gs.close()
    print(f"full HD: {sn.segments / sn.samples:.2f} segments per sample; {window_slots(sn)}-slot windows {sn.ms_total:.1f} ms, {window_slots(sw, 1)}-slot windows "
          f"{sw.ms_total:.1f} ms, {sw.compactions} compactions")
    assert narrow.shape == (1080, 1920, 3) and window_slots(sn) == 4096 and window_slots(sw, 1) == 8192
    assert sn.segments == sw.segments and np.isfinite(narrow).all()
    np.testing.assert_allclose(wide, narrow, rtol=1e-11, atol=1e-11)


# ---- 8. refusals at the render ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["env_sampling", "fog", "grid", "interior", "exact_lights"])
def test_render_refuses_dispersion_with(pt, ctx, what):
    extra = {"env_sampling": None, "exact_lights": "sphere_light"}.get(what, what)
    gs, cam, _ = build(pt, ctx, ball_scene(20.0, env_map=what == "env_sampling", extra=extra))
    if what == "env_sampling":
        gs.set_env_sampling(0.5)
    if what == "exact_lights":
        gs.set_light_sampling("exact")
    with pytest.raises(pt.PtError, match="dispersion"):
        gs.render(cam, 1, 0, 1)
    with pytest.raises(pt.PtError, match="dispersion"):
        gs.render_pixels(cam, 1, np.array([3, 5], dtype=np.uint32), 0, 1)
    assert "dispersion" in pt.lib.pt_last_error().decode()
    gs.close()
    # without the Abbe number the same scene renders
    gs, cam, _ = build(pt, ctx, ball_scene(0.0, env_map=what == "env_sampling", extra=extra))
    if what == "env_sampling":
        gs.set_env_sampling(0.5)
    if what == "exact_lights":
        gs.set_light_sampling("exact")
    gs.render(cam, 1, 0, 1)
    gs.close()


def test_render_refuses_a_depth_that_reaches_the_flag(pt, ctx):
    gs, cam, _ = build(pt, ctx, ball_scene(20.0))
    cam.max_depth = (1 << 31) - 1
    gs.render(cam, 1, 0, 1)
    cam.max_depth = 1 << 31
    with pytest.raises(pt.PtError, match="max_depth"):
        gs.render(cam, 1, 0, 1)
    assert "dispersion" in pt.lib.pt_last_error().decode()
    gs.close()


# ---- 9. the CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cli_dispersion(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = ["-q", "-s", "1", "--width", "96", "--spp", "8", "--assets", pt.ASSET_DIR]

    def run(name, *extra):
        out = tmp_path / name
        r = subprocess.run([exe] + common + list(extra) + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return pt.decode_image_rgb8(str(out)).astype(np.float64)

    clear = run("clear.png")
    prism = run("prism.png", "--dispersion", "20")
    sobol = run("sobol.png", "--dispersion", "20", "--sampler", "sobol")
    d_p, d_s = np.abs(prism - clear).mean(), np.abs(sobol - clear).mean()
    print(f"--dispersion 20: mean |difference| against the clear render: {d_p:.3f}, with the Sobol sampler {d_s:.3f}")
    assert d_p > 0.0 and d_s > 0.0
