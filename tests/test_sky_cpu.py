"""The physical sky's host-only entry points (pt_sky_eval, pt_sky_sun_irradiance, pt_sky_opts_check) against tests/sky_rule.py, the numpy
restatement of the header's rule, and against closed forms that do not go through it. No GPU."""
import ctypes as C

import numpy as np
import pytest

import sky_rule as R

ELEVATIONS = (90.0, 45.0, 5.0, 0.0, -10.0)
TURBIDITIES = (1.7, 3.0, 10.0)
AZ = 0.7   # the sun's azimuth in the tests that need one off the axes


def sun_at(el_deg, az=AZ):
    el = np.radians(el_deg)
    if el_deg == 90.0:
        return (0.0, 1.0, 0.0)
    if el_deg == 0.0:
        return (np.cos(az), 0.0, np.sin(az))
    return (np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az))


def directions():
    rng = np.random.default_rng(24)
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    return np.concatenate([d, axes])


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def test_symbols_are_exported(pt):
    for name in ("pt_sky_opts_default", "pt_sky_opts_check", "pt_sky_eval", "pt_sky_sun_irradiance", "pt_sky_probe", "pt_sky_bake", "pt_tex_sky"):
        assert hasattr(pt.lib, name) and name in pt.ABI_SYMBOLS


def test_defaults(pt):
    o = pt.SkyOpts(sun_dir=(1.0, 2.0, 3.0), turbidity=9.0, ground_albedo=0.9, sun_radius_deg=1.0, sun_scale=2.0, scale=7.0)
    assert pt.lib.pt_sky_opts_default(C.byref(o)) == 0
    fresh = pt.SkyOpts()
    assert bytes(o) == bytes(fresh)
    assert tuple(o.sun_dir) == (0.0, 1.0, 0.0) and o.turbidity == 3.0 and tuple(o.ground_albedo) == (0.3, 0.3, 0.3)
    assert o.sun_radius_deg == 0.2665 and o.sun_scale == 1.0 and o.scale == 0.04
    assert pt.lib.pt_sky_opts_default(None) == -1


@pytest.mark.parametrize("T", TURBIDITIES)
@pytest.mark.parametrize("el", ELEVATIONS)
def test_eval_matches_the_rule(pt, T, el):
    """|delta| <= 1e-12 x the sample's largest channel. detmath is within 1-2 ulp of libm (test_detmath.py) and the chain is about 40
    operations whose worst conditioning is tan(chi) at chi < 1.4: the difference stays well under 1e-13."""
    d = directions()
    kw = dict(sun_dir=sun_at(el), turbidity=T, ground_albedo=(0.2, 0.3, 0.4), sun_scale=1.5, scale=0.05)
    got = pt.sky_eval(d, **kw)
    want = R.sky_eval(R.options(**kw), d)
    assert np.isfinite(got).all() and (got >= 0.0).all()
    big = np.maximum(want.max(axis=1, keepdims=True), got.max(axis=1, keepdims=True))
    err = np.abs(got - want) / big
    print(f"T={T} el={el}: max |delta| / largest channel = {err.max():.3e}")
    assert err.max() <= 1e-12


def test_a_long_or_short_sun_dir_is_normalised(pt):
    d = directions()
    a = pt.sky_eval(d, sun_dir=sun_at(30.0))
    for k in (1e-200, 3.0, 1e200):
        b = pt.sky_eval(d, sun_dir=tuple(k * x for x in sun_at(30.0)))
        assert np.abs(a - b).max() <= 1e-12 * a.max()


@pytest.mark.parametrize("T", TURBIDITIES)
def test_zenith_luminance_is_yz(pt, T):
    """Looking at the zenith with the sun at the zenith, F / F(0, theta_s) = 1: Y = Yz = (4.0453 T - 4.9710) tan((4/9 - T/120) pi) - 0.2155 T + 2.4192,
    to 1e-9 relative. The luminance of the output is the Y row of the INVERSE of the rule's XYZ -> RGB matrix, (0.21267, 0.71515, 0.07217):
    the rounded weights (0.2126, 0.7152, 0.0722) times that matrix are (-2.8e-4,1 + 2.0e-4, 6.5e-5), not (0, 1, 0), so with them the
    closed form holds only to 3e-5 (numpy rule: 3.4e-5, 3.0e-5, 1.1e-5 at T = 1.7, 3, 10), whatever the product does."""
    scale = 0.04
    c = pt.sky_eval(np.array([[0.0, 1.0, 0.0]]), sun_dir=(0.0, 1.0, 0.0), turbidity=T, scale=scale)[0]
    assert (c > 0.0).all()                     # no channel was clamped: the luminance below is the sky's Y
    yz = (4.0453 * T - 4.9710) * np.tan((4.0 / 9.0 - T / 120.0) * np.pi) - 0.2155 * T + 2.4192
    y_row = np.linalg.inv(R.XYZ_TO_RGB)[1]
    Y = float(y_row @ c)
    print(f"T={T}: Y row {y_row}, Y {Y:.12g} scale*Yz {scale * yz:.12g} relative {abs(Y - scale * yz) / (scale * yz):.3e}; "
          f"with the rounded weights {abs(lum(c) - scale * yz) / (scale * yz):.3e}")
    assert abs(Y - scale * yz) <= 1e-9 * scale * yz


def test_mirror_symmetry_about_the_suns_plane(pt):
    s = np.array(sun_at(35.0, az=1.1))
    n = np.array([-np.sin(1.1), 0.0, np.cos(1.1)])          # the normal of the vertical plane through the sun
    d = directions()
    m = d - 2.0 * (d @ n)[:, None] * n[None, :]
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    a, b = pt.sky_eval(d, sun_dir=tuple(s), turbidity=4.0), pt.sky_eval(m, sun_dir=tuple(s), turbidity=4.0)
    err = np.abs(a - b).max(axis=1) / a.max(axis=1)
    print(f"mirror symmetry: max relative difference {err.max():.3e}")
    assert err.max() <= 1e-12


def test_every_direction_below_the_horizon_is_the_same_ground(pt):
    d = directions()
    c = pt.sky_eval(d, sun_dir=sun_at(20.0), ground_albedo=(0.1, 0.5, 0.9))
    below = d[:, 1] <= 0.0
    assert below.sum() > 900 and (d[below][:, 1] == 0.0).any()
    g = c[below]
    assert (g == g[0]).all() and (g[0] > 0.0).all()
    assert not (c[~below] == g[0]).all(axis=1).any()


def test_sun_irradiance_reddens_and_dims_towards_the_horizon(pt):
    e = [pt.sky_sun_irradiance(sun_dir=sun_at(el)) for el in (60.0, 30.0, 10.0, 3.0)]
    for hi, lo in zip(e, e[1:]):
        assert (lo < hi).all() and (lo > 0.0).all()          # dimmer in every channel
        assert lo[0] / lo[2] > hi[0] / hi[2]                    # and redder
        assert lo[0] / lo[1] > hi[0] / hi[1]
    for el in (0.0, -10.0):
        assert (pt.sky_sun_irradiance(sun_dir=sun_at(el)) == 0.0).all()
    # the factors in front: scale * sun_scale
    a = pt.sky_sun_irradiance(sun_dir=sun_at(40.0), scale=1.0, sun_scale=1.0)
    b = pt.sky_sun_irradiance(sun_dir=sun_at(40.0), scale=0.5, sun_scale=3.0)
    np.testing.assert_allclose(b, 1.5 * a, rtol=1e-15)
    want = R.sun_irradiance(R.options(sun_dir=sun_at(40.0), scale=1.0))
    np.testing.assert_allclose(a, want, rtol=1e-12)


def test_opts_check(pt):
    check = lambda **o: pt.lib.pt_sky_opts_check(C.byref(pt.SkyOpts(**o)))
    assert pt.lib.pt_sky_opts_check(None) == 0 and check() == 0
    nan = float("nan")
    bad = [("sun_dir", dict(sun_dir=(nan, 1.0, 0.0))), ("sun_dir", dict(sun_dir=(0.0, 0.0, 0.0))), ("sun_dir", dict(sun_dir=(0.0, float("inf"), 0.0))),
           ("turbidity", dict(turbidity=1.6)), ("turbidity", dict(turbidity=10.1)), ("turbidity", dict(turbidity=nan)),
           ("ground_albedo", dict(ground_albedo=(0.3, 1.1, 0.3))), ("ground_albedo", dict(ground_albedo=(nan, 0.3, 0.3))), ("ground_albedo", dict(ground_albedo=-0.1)),
           ("sun_radius_deg", dict(sun_radius_deg=0.0)), ("sun_radius_deg", dict(sun_radius_deg=10.5)), ("sun_radius_deg", dict(sun_radius_deg=nan)),
           ("sun_scale", dict(sun_scale=-1.0)), ("sun_scale", dict(sun_scale=nan)), ("sun_scale", dict(sun_scale=float("inf"))),
           ("scale", dict(scale=0.0)), ("scale", dict(scale=nan)), ("scale", dict(scale=float("inf")))]
    for field, o in bad:
        assert check(**o) == -1, o
        assert field in pt.lib.pt_last_error().decode(), (o, pt.lib.pt_last_error())
    for o in (dict(turbidity=1.7), dict(turbidity=10.0), dict(sun_radius_deg=10.0), dict(sun_scale=0.0), dict(ground_albedo=(0.0, 1.0, 0.5)), dict(sun_dir=(0.0, -5.0, 0.0))):
        assert check(**o) == 0, o
    # the evaluating entry points apply the same test and write nothing
    out = np.full((1, 3), 7.0)
    d = np.array([[0.0, 1.0, 0.0]])
    assert pt.lib.pt_sky_eval(C.byref(pt.SkyOpts(turbidity=11.0)), d.ctypes.data, 1, out.ctypes.data) == -1 and (out == 7.0).all()
    with pytest.raises(pt.PtError, match="turbidity"):
        pt.sky_sun_irradiance(turbidity=0.5)


def test_cli_refuses_a_malformed_sky_before_it_needs_a_gpu(pt):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    for bad, text in (("35", "ELEVATION_DEG,AZIMUTH_DEG"), ("35,120,99", "turbidity must be in [1.7, 10]"), ("35,x", "finite numbers"), ("35,120,3,7.5", "WIDTH"),
                      ("35,120,3,1024,5", "ELEVATION_DEG,AZIMUTH_DEG")):
        r = subprocess.run([exe, "-s", "6", "--sky", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (bad, r.stderr)
    r = subprocess.run([exe, "-s", "6", "--sky-no-disc"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--sky-no-disc needs --sky" in r.stderr
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--sky ELEVATION_DEG,AZIMUTH_DEG[,TURBIDITY[,WIDTH]]" in r.stdout


@pytest.mark.parametrize("el", (50.0, 8.0, -10.0))
def test_ground_is_the_lambertian_plane_under_this_sky(pt, el):
    """G = albedo / pi x (the irradiance of pt_sky_eval's own sky by a 256 x 1024 midpoint quadrature + the sun's term). The product's E_sky is
    a 16 x 64 quadrature: the margin is twice the difference between the two quadratures, measured here on the numpy rule."""
    albedo = np.array([0.25, 0.5, 0.75])
    kw = dict(sun_dir=sun_at(el), turbidity=3.0, ground_albedo=tuple(albedo), sun_scale=1.0, scale=0.04)
    o = R.options(**kw)
    coarse, fine = R.sky_irradiance_unscaled(o, 16, 64), R.sky_irradiance_unscaled(o, 256, 1024)
    margin = 2.0 * np.abs(coarse - fine) * o["scale"] * albedo / np.pi
    print(f"el={el}: rule E_sky 16x64 {coarse} 256x1024 {fine}; margin on G {margin}")
    # the same fine quadrature, of the product's sky
    na, nb = 256, 1024
    a, b = np.arange(na, dtype=np.float64), np.arange(nb, dtype=np.float64)
    theta = ((a + 0.5) * (np.pi / 2.0)) / na
    phi = -np.pi + ((2.0 * np.pi) * (b + 0.5)) / nb
    w = np.cos(theta) * (np.cos((a * (np.pi / 2.0)) / na) - np.cos(((a + 1.0) * (np.pi / 2.0)) / na)) * ((2.0 * np.pi) / nb)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    d = np.stack([st * np.cos(phi)[None, :], ct + 0.0 * phi[None, :], st * np.sin(phi)[None, :]], axis=-1)
    e_sky = (pt.sky_eval(d.reshape(-1, 3), **kw).reshape(na, nb, 3) * w[:, None, None]).sum(axis=(0, 1))
    e_sun = pt.sky_sun_irradiance(**kw) * max(0.0, R.sun_unit(o)[1])
    want = albedo / np.pi * (e_sky + e_sun)
    got = pt.sky_eval(np.array([[0.0, -1.0, 0.0]]), **kw)[0]
    print(f"el={el}: G {got} expected {want} |delta| {np.abs(got - want)}")
    assert (np.abs(got - want) <= margin + 1e-12 * want).all()
