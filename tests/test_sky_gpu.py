"""The physical sky on the GPU (pt_sky_probe, pt_sky_bake, pt_tex_sky): the device function against the host's, the baked map
against the header's rule (tests/sky_rule.py), the disc's energy, and the map at work as an environment: orientation, units, sampling, CLI."""
import math
import os
import subprocess

import numpy as np
import pytest

import sky_rule as R
from common import SceneSpec, default_camera

pytestmark = pytest.mark.gpu

SAMPLERS = ("independent", "sobol")


def sun_at(el_deg, az_deg):
    el, az = math.radians(el_deg), math.radians(az_deg)
    return (math.cos(el) * math.cos(az), math.sin(el), math.cos(el) * math.sin(az))


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def centre_dirs(ctx, W, H):
    """The texel centres' directions with the DEVICE's sin and cos (pt_math_probe: detmath, the functions the bake calls), in the header's order
    of operations: (H, W, 3)."""
    theta = ((np.arange(H, dtype=np.float64) + 0.5) * np.pi) / H
    phi = -np.pi + ((2.0 * np.pi) * (np.arange(W, dtype=np.float64) + 0.5)) / W
    pair = lambda x: np.stack([x, np.zeros_like(x)], axis=1)
    st, ct = ctx.math_probe(3, pair(theta))[:, None], ctx.math_probe(4, pair(theta))[:, None]
    sp, cp = ctx.math_probe(3, pair(phi))[None, :], ctx.math_probe(4, pair(phi))[None, :]
    return np.stack([st * cp, ct + 0.0 * cp, st * sp], axis=-1)


_bakes = {}


def baked(ctx, W, H, **kw):
    """One bake per (size, options) for the whole module; the arrays are shared: read only."""
    key = (W, H, tuple(sorted((k, tuple(v) if np.ndim(v) else v) for k, v in kw.items())))
    if key not in _bakes:
        m = ctx.sky_bake(W, H, **kw)
        m.setflags(write=False)
        _bakes[key] = m
    return _bakes[key]


def no_disc(pt, ctx, W, H, **kw):
    """The same map without the disc: float32(pt_sky_eval(texel centres)), which is what the bake adds the disc to (test 2 pins the two to the
    same bits). NOT a bake with sun_scale = 0: the ground's radiance holds the sun's term, so that map's lower half is darker."""
    key = ("no disc", W, H, tuple(sorted((k, tuple(v) if np.ndim(v) else v) for k, v in kw.items())))
    if key not in _bakes:
        m = pt.sky_eval(centre_dirs(ctx, W, H).reshape(-1, 3), **kw).reshape(H, W, 3).astype(np.float32)
        m.setflags(write=False)
        _bakes[key] = m
    return _bakes[key]


# ---- 1. the device function is the host's, bit for bit ------------------------------------------------------------------------------------
def test_probe_equals_eval_bit_for_bit(pt, ctx):
    rng = np.random.default_rng(5)
    d = rng.normal(size=(4099, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.concatenate([d, np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 1e-300, 0.8]], dtype=np.float64)])
    for kw in (dict(), dict(sun_dir=sun_at(45.0, 40.0), turbidity=1.7), dict(sun_dir=sun_at(5.0, -100.0), turbidity=10.0, ground_albedo=(0.1, 0.5, 0.9)),
               dict(sun_dir=sun_at(0.0, 10.0), turbidity=2.2, scale=1.0), dict(sun_dir=sun_at(-10.0, 200.0), sun_scale=3.0)):
        host, dev = pt.sky_eval(d, **kw), ctx.sky_probe(d, **kw)
        assert np.isfinite(host).all()
        assert host.tobytes() == dev.tobytes(), (kw, int((host != dev).sum()), np.abs(host - dev).max())


# ---- 2. without a disc the map is float32(pt_sky_eval(texel centres)) ---------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(64, 32), (1, 1), (257, 129), (16, 8)])
def test_bake_without_disc_is_eval_at_the_centres(pt, ctx, W, H):
    kw = dict(sun_dir=sun_at(30.0, 75.0), turbidity=4.0, ground_albedo=(0.2, 0.3, 0.4), sun_scale=0.0)
    got = ctx.sky_bake(W, H, **kw)
    assert got.shape == (H, W, 3) and got.dtype == np.float32
    want = pt.sky_eval(centre_dirs(ctx, W, H).reshape(-1, 3), **kw).reshape(H, W, 3).astype(np.float32)
    assert got.tobytes() == want.tobytes(), (int((got != want).sum()), np.abs(got - want).max())
    if H > 1:
        assert (got[: H // 2] != got[-1, 0]).any() and (got[H - H // 2:] == got[-1, 0]).all()    # sky above, one ground colour below


# ---- 3. the disc carries the sun's irradiance at every map size, through every shape of window ------------------------------------------------
DISC_CASES = {
    "smaller than a texel: the fallback": (64, 32, dict(sun_dir=sun_at(45.0, 30.0))),
    "3 degrees across many texels": (512, 256, dict(sun_dir=sun_at(45.0, 30.0), sun_radius_deg=3.0)),
    "at phi = +-pi: the window wraps": (512, 256, dict(sun_dir=(-1.0, 1.0, 0.0), sun_radius_deg=3.0)),
    "at the zenith: whole rows": (256, 128, dict(sun_dir=(0.0, 1.0, 0.0), sun_radius_deg=3.0)),
    "straddling the horizon": (512, 256, dict(sun_dir=sun_at(1.0, -60.0), sun_radius_deg=3.0)),
}


@pytest.mark.parametrize("case", list(DISC_CASES))
def test_disc_energy_and_counts(pt, ctx, case):
    W, H, kw = DISC_CASES[case]
    kw = dict(turbidity=3.0, **kw)
    with_disc, without = baked(ctx, W, H, **kw), no_disc(pt, ctx, W, H, **kw)
    o = R.options(**kw)
    omega = R.solid_angles(W, H)
    irr = pt.sky_sun_irradiance(**kw)
    assert (irr > 0.0).all()
    disc = (with_disc != without).any(axis=2)
    diff = with_disc.astype(np.float64) - without.astype(np.float64)
    got = (diff * omega[:, :, None]).sum(axis=(0, 1))
    # each disc texel is a rounded f32 in both maps: |fl(x) - x| <= 2^-24 |x|, so its difference is off by at most 2^-24 (|bake| + |bake without|)
    # <= 2^-23 |bake|; weighted and summed over the disc's texels (the others contribute an exact 0)
    bound = 2.0 ** -23 * (with_disc.astype(np.float64) * omega[:, :, None])[disc].sum(axis=0) * (1.0 + 1e-6)
    print(f"{case}: {int(disc.sum())} disc texels of {W * H}; sum disc * omega {got}, sun irradiance {irr}, |delta| {np.abs(got - irr)}, bound {bound}")
    assert (np.abs(got - irr) <= bound).all()
    # the rule's counts reproduce the map: the same texels, each to one f32 ulp
    want, n = R.bake(o, W, H)
    assert np.array_equal(disc, n > 0), (int(disc.sum()), int((n > 0).sum()))
    if "fallback" in case:
        assert disc.sum() == 1 and n.max() == 64
    want32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(want32))
    worst = (np.abs(with_disc.astype(np.float64) - want32.astype(np.float64)) / ulp.astype(np.float64)).max()
    print(f"{case}: worst difference from the numpy rule {worst:.2f} f32 ulp; counts from {n[n > 0].min()} to {n.max()}")
    assert worst <= 1.0


def test_window_shapes_are_what_the_cases_say(pt, ctx):
    """(guards the cases above: each must meet the window shape it is named after)"""
    W, H, kw = DISC_CASES["at phi = +-pi: the window wraps"]
    d = (baked(ctx, W, H, turbidity=3.0, **kw) != no_disc(pt, ctx, W, H, turbidity=3.0, **kw)).any(axis=2)
    assert d[:, 0].any() and d[:, W - 1].any() and not d[:, W // 2].any()
    W, H, kw = DISC_CASES["at the zenith: whole rows"]
    d = (baked(ctx, W, H, turbidity=3.0, **kw) != no_disc(pt, ctx, W, H, turbidity=3.0, **kw)).any(axis=2)
    assert d[0].all() and not d[H // 2].any()
    W, H, kw = DISC_CASES["straddling the horizon"]
    d = (baked(ctx, W, H, turbidity=3.0, **kw) != no_disc(pt, ctx, W, H, turbidity=3.0, **kw)).any(axis=2)
    assert d[H // 2 - 1].any() and d[H // 2].any()


def test_two_bakes_are_the_same_bytes(ctx):
    for case in ("3 degrees across many texels", "at the zenith: whole rows"):
        W, H, kw = DISC_CASES[case]
        a = baked(ctx, W, H, turbidity=3.0, **kw)
        for _ in range(2):
            assert ctx.sky_bake(W, H, turbidity=3.0, **kw).tobytes() == a.tobytes()


def test_bake_refusals(pt, ctx):
    for w, h in ((0, 4), (4, 0), (1 << 14, (1 << 12) + 1)):
        with pytest.raises(pt.PtError, match="2\\^26"):
            ctx.sky_bake(w, h)
    with pytest.raises(pt.PtError, match="turbidity"):
        ctx.sky_bake(8, 4, turbidity=1.0)
    with pytest.raises(pt.PtError, match="sun_dir"):
        ctx.sky_probe(np.array([[0.0, 1.0, 0.0]]), sun_dir=(0.0, 0.0, 0.0))


# ---- 4. orientation, end to end: the panorama of a sky map is the map --------------------------------------------------------------------------
def test_panorama_gives_the_sky_map_back(pt, ctx):
    W, H, spp = 64, 32, 4
    sky = dict(sun_dir=sun_at(40.0, 130.0), turbidity=3.0)
    env_img = baked(ctx, W, H, **sky)
    center = np.array([0.5, 1.0, -2.0])
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    phi = -np.pi + ((2.0 * np.pi) * (i + 0.5)) / W
    theta = (np.pi * (j + 0.5)) / H
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    ball_c, ball_r = center + 10.0 * d[12, 40], 0.05                         # pt_world_build refuses an empty world: one small far sphere
    gs = pt.Scene(ctx)
    env = gs.tex_sky(W, H, **sky)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.sphere(ball_r, tuple(ball_c), tuple(ball_c), grey))
    gs.world_build()
    spec = SceneSpec()
    spec.camera = default_camera(width=W, aspect=2.0, spp=spp, look_from=tuple(center), look_at=(0.0, 0.5, 0.0), defocus_angle=0.0, blur_strength=0.0,
                                 env_is_map=1, env_tex=env)
    cam = spec.make_camera(pt.Camera, [])
    gs.set_projection("panorama")
    oc = center - ball_c
    b = d @ oc
    meets = (b * b - (oc @ oc - ball_r * ball_r) >= 0.0) & (b < 0.0)
    assert meets[12, 40]
    out = meets.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out |= np.roll(np.roll(meets, dy, axis=0), dx, axis=1)
    print(f"panorama identity: {int(meets.sum())} pixel centres meet the sphere, {int(out.sum())} pixels left out")
    assert out.sum() <= 12
    expected = float(spp) * env_img.astype(np.float64)
    si, sj = R.texel_of(W, H, R.sun_unit(R.options(**sky)))
    assert not out[sj, si] and env_img[sj, si].max() > 100.0 * np.median(env_img)     # the sun's texel is among the pixels compared
    for sampler in SAMPLERS:
        gs.set_sampler(sampler)
        acc, st = gs.render(cam, 3, 0, spp)
        np.testing.assert_array_equal(acc[~out], expected[~out])
    gs.close()


# ---- 5. units, end to end: a diffuse plane under the sky receives the map's irradiance ---------------------------------------------------------
def test_plane_under_the_sky_receives_the_maps_irradiance(pt, ctx):
    W, H = 256, 128
    sky = dict(sun_dir=sun_at(40.0, 20.0), turbidity=3.0)
    env_img = baked(ctx, W, H, **sky).astype(np.float64)
    d = R.texel_dirs(W, H)[:, :, 0, 0, :]
    e = (env_img * (np.maximum(d[..., 1], 0.0) * R.solid_angles(W, H))[:, :, None]).sum(axis=(0, 1))
    want = 0.5 / np.pi * e
    gs = pt.Scene(ctx)
    env = gs.tex_sky(W, H, **sky)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.quad((-500.0, 0.0, -500.0), (0.0, 0.0, 1000.0), (1000.0, 0.0, 0.0), grey))
    gs.world_build()
    spec = SceneSpec()
    spec.camera = default_camera(width=32, aspect=1.0, spp=64, max_depth=4, vfov=40.0, look_from=(0.0, 5.0, 0.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 0.0, 1.0),
                                 focal_length=5.0, defocus_angle=0.0, blur_strength=0.0, env_is_map=1, env_tex=env)
    cam = spec.make_camera(pt.Camera, [])
    z = {}
    for f in (0.5, 0.0):
        gs.set_env_sampling(f)
        acc, st = gs.render(cam, 3, 0, 64)
        px = acc.reshape(-1, 3) / 64.0
        mean, se = px.mean(axis=0), px.std(axis=0, ddof=1) / np.sqrt(len(px))
        z[f] = (mean - want) / se
        print(f"env sampling {f}: mean {mean}, expected {want}, standard error {se}, z {z[f]}")
        assert np.isfinite(px).all()
    assert (np.abs(z[0.5]) <= 6.0).all()
    assert (np.abs(z[0.0]) <= 6.0).all()
    gs.close()


# ---- 6. the environment sampler finds the disc ---------------------------------------------------------------------------------------------------
def test_env_sampler_on_a_sky_map(pt, ctx):
    W, H = 128, 64
    sky = dict(sun_dir=sun_at(35.0, -45.0), turbidity=3.0, sun_radius_deg=2.0)
    with_disc, without = baked(ctx, W, H, **sky), no_disc(pt, ctx, W, H, **sky)
    disc = (with_disc != without).any(axis=2)
    w = lum(with_disc.astype(np.float64)) * R.solid_angles(W, H)
    share = w[disc].sum() / w.sum()
    gs = pt.Scene(ctx)
    env = gs.tex_sky(W, H, **sky)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.sphere(1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), grey))
    gs.world_build()
    spec = SceneSpec()
    spec.camera = default_camera(width=16, env_is_map=1, env_tex=env)
    cam = spec.make_camera(pt.Camera, [])
    s = R.sun_unit(R.options(**sky))
    pdf = gs.env_probe(cam, 1, np.array([s, [0.0, 1.0, 0.0]]))
    si, sj = R.texel_of(W, H, s)
    Z = lum(with_disc[sj, si].astype(np.float64)) / pdf[0]
    print(f"Z from the sun texel's pdf {Z}, sum lum * omega {w.sum()}; the disc: {int(disc.sum())} texels, share {share:.4f}")
    assert np.isfinite(Z) and Z > 0.0 and abs(Z - w.sum()) <= 1e-9 * Z and pdf[1] > 0.0
    n = 4096
    out = gs.env_probe(cam, 0, np.random.default_rng(9).random((n, 2)))
    dd = out[:, :3]
    jj = np.minimum((np.arccos(np.clip(dd[:, 1], -1.0, 1.0)) / np.pi * H).astype(int), H - 1)
    ii = np.minimum(((np.arctan2(dd[:, 2], dd[:, 0]) + np.pi) / (2.0 * np.pi) * W).astype(int), W - 1)
    hits = int(disc[jj, ii].sum())
    sd = np.sqrt(n * share * (1.0 - share))
    print(f"{hits} of {n} sampled directions fall in disc texels; expected {n * share:.1f} +- {sd:.1f}")
    assert 0.05 < share < 0.95 and abs(hits - n * share) <= 6.0 * sd
    gs.close()


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------------------
def test_cli_sky(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = [exe, "-s", "6", "--width", "64", "--spp", "4", "--assets", pt.ASSET_DIR]
    png, hdr = tmp_path / "sky.png", tmp_path / "sky.hdr"
    r = subprocess.run(common + ["--sky", "35,120", "--env-sampling", "0.5", "--tonemap", "aces", "--exposure", "-1", "--out", str(png), "--out-hdr", str(hdr)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert png.stat().st_size > 100
    img = pt.load_hdr_rgbf32(str(hdr))
    assert img.shape[1] == 64 and np.isfinite(img).all() and img.max() > 0.0
    r = subprocess.run(common + ["--sky", "35,120", "--sky-no-disc", "--out", str(tmp_path / "nodisc.png")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("--sun ")]
    assert len(line) == 1, r.stdout
    x = np.array([float(v) for v in line[0].split()[1].split(",")])
    s = sun_at(35.0, 120.0)
    np.testing.assert_array_equal(x[:3], -np.array(s))
    np.testing.assert_array_equal(x[3:], pt.sky_sun_irradiance(sun_dir=s))
    for bad, text in (("35", "ELEVATION_DEG,AZIMUTH_DEG"), ("35,120,99", "turbidity"), ("35,x", "finite numbers"), ("35,120,3,7.5", "WIDTH")):
        r = subprocess.run(common + ["--sky", bad, "--out", str(tmp_path / "bad.png")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, (bad, r.stderr)
        assert not (tmp_path / "bad.png").exists()
