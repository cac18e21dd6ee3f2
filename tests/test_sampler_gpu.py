"""The Owen-scrambled Sobol sampler (pt_scene_set_sampler) on the GPU.

The oracle does not know the sampler, so exactness rests on the numpy restatement of the rule (tests/sampler_rule.py) against the
device's draw functions (pt_sampler_probe) and against whole renders of a scene whose pixel values count camera rays; correctness
of full light transport rests on expectation tests against the independent sampler, and on structure tests."""
import os
import subprocess

import numpy as np
import pytest

import sampler_rule as R
from common import GOLDEN_DIR, MIS_ALBEDO, MIS_CAM, MIS_EMISSION, MIS_QUAD, SceneSpec, default_camera

pytestmark = pytest.mark.gpu


# ---- 3. the setting and the draw functions --------------------------------------------------------------------------------
def test_setting_validation(pt, ctx):
    gs = pt.Scene(ctx)
    assert gs.sampler() == 0
    for ok in (1, 0, "sobol", "independent", 1):
        gs.set_sampler(ok)
        assert gs.sampler() == pt.SAMPLERS.get(ok, ok)
    for bad in (2, -1, "halton"):
        with pytest.raises(pt.PtError):
            gs.set_sampler(bad)
        assert gs.sampler() == 1
    gs.set_sampler(0)
    for bad in (2, -1):
        with pytest.raises(pt.PtError):
            gs.set_sampler(bad)
        assert gs.sampler() == 0
    gs.close()


PROBE_CASES = [(1, 0, 0, 64), (7, 4095, 4090, 40), ((5 << 32) | 9, 123456, 4000, 200), (0xFFFFFFFFFFFFFFFF, 0x7FFFFFFE, 0xFFFFFFE0, 16),
               (2 ** 32, 77, 1 << 20, 33)]


@pytest.mark.parametrize("seed, pixel, s0, ns", PROBE_CASES)
def test_probe_is_the_numpy_rule_bit_for_bit(pt, ctx, seed, pixel, s0, ns):
    got = ctx.sampler_probe("sobol", seed, pixel, s0, ns, 0, 64)
    s = (np.arange(ns, dtype=np.uint64) + np.uint64(s0))[:, None]
    d = np.arange(64, dtype=np.uint64)[None, :]
    np.testing.assert_array_equal(got, R.sobol_u64(seed, pixel, s, d))
    # a draw range that does not start at zero (or at an even index) reads the same values
    np.testing.assert_array_equal(ctx.sampler_probe(1, seed, pixel, s0, ns, 5, 9), got[:, 5:14])
    ind = ctx.sampler_probe("independent", seed, pixel, s0, ns, 0, 64)
    np.testing.assert_array_equal(ind, R.independent_u64(seed, pixel, s, d))
    assert (ind != got).all()


def test_probe_kind0_is_the_existing_stream(pt, ctx, orc):
    seed, pixel = 12345, 678
    v = ctx.sampler_probe(0, seed, pixel, 7, 1, 0, 64)[0]
    old = ctx.math_probe(9, np.array([[float(seed), float(pixel)]] * 64))          # rng uniform(seed, pixel, sample 7, draw i)
    np.testing.assert_array_equal(R.unit(v), old)
    assert [orc.rng_uniform(seed, pixel, 7, i) for i in range(64)] == list(old)
    with pytest.raises(pt.PtError):
        ctx.sampler_probe(2, 1, 0, 0, 1, 0, 1)


# ---- 4. the default is untouched -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", [3, 6])
def test_default_renders_the_committed_golden(pt, ctx, sid):
    g = np.load(os.path.join(GOLDEN_DIR, f"scene{sid}_w64_spp16_seed1.npz"))
    gs = pt.Scene(ctx)
    cam = gs.build_scene(sid, 64, 16)
    acc, st = gs.render(cam, 1, 0, 16, slots_per_pixel=1)                          # never set
    np.testing.assert_array_equal(acc, g["accum"])
    assert st.segments == int(g["segments"])
    gs.set_sampler("sobol")
    sob, _ = gs.render(cam, 1, 0, 16, slots_per_pixel=1)
    assert not np.array_equal(sob, g["accum"])                                     # (the setting does act)
    gs.set_sampler("independent")
    acc, st = gs.render(cam, 1, 0, 16, slots_per_pixel=1)                          # set, and set back
    np.testing.assert_array_equal(acc, g["accum"])
    assert st.segments == int(g["segments"])
    gs.close()


# ---- 5, 6. one emissive quad in the image plane: a pixel's value counts its camera rays that hit it --------------------------
# Camera at (0, 0, -5) looking at the origin, focal length 5: the image plane is z = 0, and the quad lies IN it, so a camera ray hits
# the quad exactly when its sample location on the image plane is inside the parallelogram. Its edges are tilted against the pixel
# grid (three different orientations and offsets per side pair) so that no pixel row or column runs along an edge.
QUAD_Q, QUAD_U, QUAD_V = np.array([-0.9, -0.6, 0.0]), np.array([1.6, 0.5, 0.0]), np.array([-0.4, 1.5, 0.0])
QUAD_EMISSION = (2.0, 1.0, 0.5)             # powers of two: emission * count is exact
QUAD_W, QUAD_BLUR = 64, 0.5
EDGE_GUARD = 1e-9                            # pixels


def quad_scene(pt, ctx):
    spec = SceneSpec()
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", *QUAD_EMISSION))
    spec.add("world_add_object", spec.add("quad", tuple(QUAD_Q), tuple(QUAD_U), tuple(QUAD_V), lm))
    spec.add("world_build")
    spec.camera = default_camera(width=QUAD_W, aspect=1.0, spp=64, max_depth=8, vfov=40.0, look_from=(0.0, 0.0, -5.0), look_at=(0.0, 0.0, 0.0),
                                 vup=(0.0, 1.0, 0.0), focal_length=5.0, defocus_angle=0.0, blur_strength=QUAD_BLUR, env_color=(0.0, 0.0, 0.0))
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    frame, h = pt.camera_init(cam)
    assert h == QUAD_W
    return gs, cam, frame


def edge_distances(frame, rows, cols):
    """Signed distances, in pixels, of image-plane locations (row, col: fractional pixel coordinates) to the quad's four edge
    lines, positive inside. The plane z = 0 is spanned by pixel_dv (rows) and pixel_du (columns), orthogonal and of equal length."""
    du, dv, p00 = frame["pixel_du"], frame["pixel_dv"], frame["pixel00"]
    px = np.linalg.norm(du)
    assert abs(np.linalg.norm(dv) - px) < 1e-12 * px and abs(du @ dv) < 1e-12 * px * px and abs(p00[2]) < 1e-12
    x = p00[0] + dv[0] * rows + du[0] * cols
    y = p00[1] + dv[1] * rows + du[1] * cols
    out = []
    for a, e, inward in ((QUAD_Q, QUAD_U, QUAD_V), (QUAD_Q + QUAD_V, QUAD_U, -QUAD_V), (QUAD_Q, QUAD_V, QUAD_U), (QUAD_Q + QUAD_U, QUAD_V, -QUAD_U)):
        n = np.array([-e[1], e[0]])
        n = n / np.linalg.norm(n)
        if n @ inward[:2] < 0:
            n = -n
        out.append(((x - a[0]) * n[0] + (y - a[1]) * n[1]) / px)
    return np.stack(out)


def numpy_hit_counts(frame, seed, n_samples, sobol):
    """Per pixel: the number of samples whose location is inside the quad, and whether every sample clears every edge by the guard."""
    pixels = np.arange(QUAD_W * QUAD_W)
    rows, cols = R.camera_locations(frame, QUAD_BLUR, QUAD_W, seed, pixels, np.arange(n_samples), sobol=sobol)
    d = edge_distances(frame, rows, cols)
    inside = (d > 0.0).all(axis=0)
    clear = (np.abs(d) > EDGE_GUARD).all(axis=(0, 2))
    return inside.sum(axis=1), clear


def exact_coverage(frame, n=512):
    """Per pixel: the share of the footprint (radius = sqrt(u0) * blur, angle = 2 pi u1) inside the quad, by midpoint quadrature over
    n x n (u0, u1) cells for the pixels whose footprint disc reaches an edge, exactly 0 or 1 elsewhere. The quadrature's error on an
    indicator of a smooth boundary is O(n^-1.5) ~ 1e-4: squared, four orders below the errors it is compared with."""
    pixels = np.arange(QUAD_W * QUAD_W)
    rows, cols = np.divmod(pixels, QUAD_W)
    dc = edge_distances(frame, rows.astype(float), cols.astype(float))
    cov = (dc > 0.0).all(axis=0).astype(float)
    edge = (dc > -QUAD_BLUR).all(axis=0) & ~(dc > QUAD_BLUR).all(axis=0)              # the disc is neither wholly outside nor wholly inside
    g = (np.arange(n) + 0.5) / n
    rad, ang = np.sqrt(g)[:, None] * QUAD_BLUR, (2.0 * np.pi * g)[None, :]
    bx, by = (rad * np.cos(ang)).reshape(-1), (rad * np.sin(ang)).reshape(-1)
    for p in pixels[edge]:
        d = edge_distances(frame, rows[p] + bx, cols[p] + by)
        cov[p] = (d > 0.0).all(axis=0).mean()
    edge &= (cov > 0.0) & (cov < 1.0)
    return cov, edge


def test_camera_stream_counts_exactly(pt, ctx):
    gs, cam, frame = quad_scene(pt, ctx)
    cov, edge = exact_coverage(frame, n=128)
    n_edge = int(edge.sum())
    assert n_edge >= 100
    h = QUAD_W
    for seed, spp in ((1, 64), ((9 << 32) | 4, 48)):
        for sobol in (True, False):                                  # the independent sampler validates the restatement of generate_ray
            gs.set_sampler(1 if sobol else 0)
            acc, st = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
            aov = gs.render_aovs(cam, seed, 0, spp)
            count, clear = numpy_hit_counts(frame, seed, spp, sobol)
            left_out = int((~clear).sum())
            print(f"quad scene seed {seed} spp {spp} sobol {sobol}: {n_edge} edge pixels, {left_out} pixels left out by the guard")
            assert left_out <= 0.02 * n_edge
            hits = aov.reshape(h * h, 8)[:, 7]
            got = acc.reshape(h * h, 3)
            np.testing.assert_array_equal(hits[clear], count[clear].astype(float))
            for c in range(3):
                np.testing.assert_array_equal(got[clear, c], QUAD_EMISSION[c] * count[clear])
            assert (count[edge & clear] > 0).any() and (count[edge & clear] < spp).any()
            assert st.samples == h * h * spp
    gs.close()


SOBOL_EDGE_MSE_RATIO_MAX = 0.35     # simulated with this rule and the camera's mapping on half-plane edges: 0.006-0.12 at 64 samples; three times the worst


def test_edge_pixel_variance_ratio(pt, ctx):
    gs, cam, frame = quad_scene(pt, ctx)
    cov, edge = exact_coverage(frame)
    n_edge = int(edge.sum())
    n_seeds = max(16, -(-2000 // n_edge))
    spp = 64
    se = {0: [], 1: []}
    for kind in (0, 1):
        gs.set_sampler(kind)
        for k in range(n_seeds):
            acc, _ = gs.render(cam, 1000 + k, 0, spp)
            mean = acc[..., 1].reshape(-1) / (spp * QUAD_EMISSION[1])
            se[kind].append(((mean[edge] - cov[edge]) ** 2).sum())
    gs.close()
    ind, sob = np.array(se[0]), np.array(se[1])
    assert n_edge * n_seeds >= 2000
    expected_ind = (cov[edge] * (1.0 - cov[edge])).sum() / spp                        # binomial variance of the independent means
    spread = ind.std(ddof=1) / np.sqrt(n_seeds) / ind.mean()
    ratio = sob.sum() / ind.sum()
    print(f"edge pixels {n_edge} x seeds {n_seeds}: summed squared error independent {ind.sum():.5g} (binomial expectation {expected_ind * n_seeds:.5g}, "
          f"relative standard error {spread:.3f}), sobol {sob.sum():.5g}, ratio {ratio:.4f}")
    assert spread < 0.10
    assert abs(ind.sum() / (expected_ind * n_seeds) - 1.0) < 0.2                      # the coverage reference and the independent side agree
    assert ratio <= SOBOL_EDGE_MSE_RATIO_MAX, ratio


# ---- 7. same expectation as the independent sampler on full light transport --------------------------------------------------
def env_map():
    """A 16 x 8 f32 environment with a bright texel, a dark row and a dark texel."""
    rng = np.random.default_rng(5)
    f32 = (rng.random((8, 16, 3)) * 0.4 + 0.1).astype(np.float32)
    f32[6] = 0.0
    f32[2, 3] = 0.0
    f32[1, 9] = (12.0, 10.0, 8.0)
    return f32


def floor_scene(pt, ctx, floor, light):
    """A floor of the given kind under the image environment, seen from straight above; optionally a quad in the lights list."""
    spec = SceneSpec()
    tex = spec.add("tex_image_rgbf32", env_map())
    alb = spec.add("tex_solid_rgb", *MIS_ALBEDO)
    if floor == "diffuse":
        m = spec.add("mat_diffuse", alb, -1)
    elif floor == "metal":
        m = spec.add("mat_metal", alb, spec.add("tex_solid_f", 0.3))
    elif floor == "glass":
        m = spec.add("mat_glass", alb, spec.add("tex_solid_f", 0.2), 0.0, 1.5)
    else:
        m = spec.add("mat_principled", alb, [0.3, 0.4, 0.1, 0.5, 0.1, 1.5, 0.0, 0.2, 0.5, 0.3, 0.6])
    spec.add("world_add_object", spec.add("quad", (-4.0, 0.0, -4.0), (0.0, 0.0, 8.0), (8.0, 0.0, 0.0), m))
    if light:
        spec.add("world_add_light", spec.add("quad", *MIS_QUAD, spec.add("mat_light", spec.add("tex_solid_rgb", *MIS_EMISSION))))
    spec.add("world_build")
    c = MIS_CAM
    spec.camera = default_camera(width=c["width"], aspect=c["aspect"], spp=1, max_depth=4, vfov=c["vfov"], look_from=c["look_from"],
                                 look_at=c["look_at"], vup=c["vup"], focal_length=c["focal_length"], defocus_angle=0.0, blur_strength=0.5,
                                 env_color=(0.0, 0.0, 0.0), env_is_map=1, env_tex=tex)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    return gs, cam


def two_sample_z(render_a, render_b, n_batches=16, spp=256, seed=300):
    """Per-pixel and frame-mean z of two estimators of the same thing. Every batch takes a seed of its own: consecutive sample
    ranges of one seed are stratified against each other under Sobol, not independent. Where both sides are the same constant
    (no variance, no difference: a pixel that only sees an emitter) z is 0."""
    a = np.stack([render_a(seed + k, 0, spp) / spp for k in range(n_batches)])
    b = np.stack([render_b(seed + 1000 + k, 0, spp) / spp for k in range(n_batches)])
    se2 = lambda x: x.var(axis=0, ddof=1) / n_batches
    diff = a.mean(axis=0) - b.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(diff == 0.0, 0.0, diff / np.sqrt(se2(a) + se2(b)))
    ga, gb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
    zg = (ga.mean(axis=0) - gb.mean(axis=0)) / np.sqrt(se2(ga) + se2(gb))
    return z, zg


def with_sampler(gs, cam, kind, env_f=None):
    def r(seed, a, b):
        gs.set_sampler(kind)
        if env_f is not None:
            gs.set_env_sampling(env_f)
        return gs.render(cam, seed, a, b)[0]
    return r


def check_z(z, zg, what):
    print(f"{what}: max |z| {np.abs(z).max():.2f}, std {z.std():.2f}, share |z| > 4 {(np.abs(z) > 4.0).mean():.4f}, frame-mean z {zg}")
    assert np.isfinite(z).all() and np.isfinite(zg).all()
    assert (np.abs(z) > 4.0).mean() < 0.01, (what, np.abs(z).max(), z.std())
    assert np.abs(zg).max() < 4.0, (what, zg)


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("floor", ["diffuse", "metal", "glass", "principled"])
def test_sobol_keeps_expectation(pt, ctx, floor, light):
    gs, cam = floor_scene(pt, ctx, floor, light)
    z, zg = two_sample_z(with_sampler(gs, cam, 1), with_sampler(gs, cam, 0))
    gs.close()
    check_z(z, zg, f"{floor} floor, light {light}")


def test_sobol_keeps_expectation_scene3(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 16)
    z, zg = two_sample_z(with_sampler(gs, cam, 1), with_sampler(gs, cam, 0))
    gs.close()
    check_z(z, zg, "scene 3")


# ---- 8. structure ---------------------------------------------------------------------------------------------------------------
def test_structure(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(6, 64, 6)
    seed, n, a = 7, 6, 2
    fig = {}
    for kind in (0, 1):
        gs.set_sampler(kind)
        full, st = gs.render(cam, seed, 0, n, slots_per_pixel=1)
        fin = np.isfinite(full)
        dyn, _ = gs.render(cam, seed, 0, n)
        assert (np.isfinite(dyn) == fin).all()
        parts = np.zeros_like(full)
        gs.render(cam, seed, 0, a, accum=parts, slots_per_pixel=1)
        gs.render(cam, seed, a, n, accum=parts, slots_per_pixel=1)
        fig[kind] = dict(dyn=(np.abs(dyn[fin] - full[fin]) / np.maximum(np.abs(full[fin]), 1e-6)).max(), parts=np.abs(parts[fin] - full[fin]).max(), full=full, fin=fin)
    print(f"static vs dynamic, max relative difference: independent {fig[0]['dyn']:.3g}, sobol {fig[1]['dyn']:.3g}; "
          f"[0, a) + [a, b) vs [0, b), max difference: independent {fig[0]['parts']:.3g}, sobol {fig[1]['parts']:.3g}")
    # the dynamic mode adds the same samples with f64 atomics in any order: 1e-12 is the bound the project's other static / dynamic
    # comparisons use for that; ten times the independent sampler's own figure where that is larger
    assert fig[1]["dyn"] <= max(10.0 * fig[0]["dyn"], 1e-12)
    assert fig[1]["parts"] <= 10.0 * fig[0]["parts"]                                  # (the static mode adds in sample order: both are 0)
    assert not np.array_equal(fig[0]["full"], fig[1]["full"])
    full, fin = fig[1]["full"], fig[1]["fin"]                                         # the sampler is Sobol from here on
    h, w = full.shape[:2]
    px = np.sort(np.random.default_rng(3).choice(h * w, 700, replace=False)).astype(np.uint32)
    sentinel = np.full_like(full, -3.25)
    lst, _ = gs.render_pixels(cam, seed, px, 0, n, accum=sentinel.copy(), slots_per_pixel=1, overwrite=True)
    mask = np.zeros(h * w, bool)
    mask[px] = True
    mask = mask.reshape(h, w)
    np.testing.assert_array_equal(lst[mask], full[mask])
    np.testing.assert_array_equal(lst[~mask], sentinel[~mask])
    ada, counts, st = gs.render_adaptive(cam, seed, 2, 24, 0.05)
    assert int(counts.sum()) == st.samples and counts.min() >= 2 and counts.max() <= 24
    ada, counts, _ = gs.render_adaptive(cam, seed, 2, n, 0.0, slots_per_pixel=1)      # threshold 0: every pixel takes all n samples
    assert (counts == n).all()
    np.testing.assert_allclose(ada[fin], full[fin], rtol=1e-12, atol=1e-12)
    gs.close()


def test_sobol_with_env_sampling_keeps_the_frame_mean(pt, ctx):
    gs = pt.Scene(ctx)
    gs.set_float_hdr(True)
    cam = gs.build_scene(6, 96, 16)
    ra, rb = with_sampler(gs, cam, 1, 0.5), with_sampler(gs, cam, 1, 0.0)
    a = np.stack([ra(500 + k, 0, 128) / 128 for k in range(16)]).mean(axis=(1, 2))
    b = np.stack([rb(900 + k, 0, 128) / 128 for k in range(16)]).mean(axis=(1, 2))
    gs.close()
    z = (a.mean(axis=0) - b.mean(axis=0)) / np.sqrt(a.var(axis=0, ddof=1) / 16 + b.var(axis=0, ddof=1) / 16)
    print(f"scene 6 float HDR under Sobol, frame means: env sampling on {a.mean(axis=0)}, off {b.mean(axis=0)}, z {z}")
    assert np.isfinite(z).all() and np.abs(z).max() < 4.0, z


# ---- the noise it removes on the headline scene ------------------------------------------------------------------------------
def rel_mse_trimmed(x, ref):
    """mean over pixels of the channel-mean (x - ref)^2 / (ref^2 + 1e-2), without the 0.1 % largest."""
    e = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(axis=2).reshape(-1)
    return np.sort(e)[: int(len(e) * 0.999)].mean()


SCENE6_RELMSE_RATIO_MEASURED = 0.68          # Sobol / independent trimmed relMSE at 64 spp, scene 6 at 240 x 135, three seeds


def test_scene6_noise_ratio(pt, ctx):
    """Pinned to min(1.0, 1.25 x the measured ratio): 25 % is the seed-to-seed spread §9 / §10 saw for this statistic at three seeds."""
    gs = pt.Scene(ctx)
    cam = gs.build_scene(6, 240, 64)
    gs.set_sampler(0)
    ref = np.stack([gs.render(cam, 100 + k, 0, 512)[0] / 512 for k in range(16)]).mean(axis=0)   # 8192 spp, independent sampler
    r = {0: [], 1: []}
    for kind in (0, 1):
        gs.set_sampler(kind)
        for seed in (1, 2, 3):
            r[kind].append(rel_mse_trimmed(gs.render(cam, seed, 0, 64)[0] / 64, ref))
    gs.close()
    ratio = np.mean(r[1]) / np.mean(r[0])
    print(f"scene 6, 64 spp, trimmed relMSE: independent {r[0]}, sobol {r[1]}, ratio {ratio:.4f}")
    assert ratio <= min(1.0, 1.25 * SCENE6_RELMSE_RATIO_MEASURED), ratio


# ---- 9. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_sampler(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = [exe, "-q", "-s", "3", "--width", "96", "--spp", "64", "--assets", pt.ASSET_DIR]

    def run(name, extra):
        out = tmp_path / name
        r = subprocess.run(common + extra + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return pt.decode_image_rgb8(str(out)).astype(np.float64)

    default, sobol, independent = run("d.png", []), run("s.png", ["--sampler", "sobol"]), run("i.png", ["--sampler", "independent"])
    np.testing.assert_array_equal(default, independent)
    assert not np.array_equal(default, sobol)
    # "within the noise": the frame mean's noise is measured on the default sampler over eight seeds; the Sobol render's mean must
    # lie within six of those standard deviations (a t statistic with 7 degrees of freedom; the 8-bit image is gamma-encoded, so
    # a sampler with less variance has a slightly higher mean — a fraction of one standard deviation here)
    ind = np.stack([default.mean(axis=(0, 1))] + [run(f"k{k}.png", ["--seed", str(k)]).mean(axis=(0, 1)) for k in range(2, 9)])
    t = (sobol.mean(axis=(0, 1)) - ind.mean(axis=0)) / (ind.std(axis=0, ddof=1) * np.sqrt(1.0 + 1.0 / len(ind)))
    print(f"CLI frame means: independent {ind.mean(axis=0)} +- {ind.std(axis=0, ddof=1)}, sobol {sobol.mean(axis=(0, 1))}, t {t}")
    assert np.abs(t).max() < 6.0, t
    r = subprocess.run(common + ["--sampler", "bogus", "--out", str(tmp_path / "y.png")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
