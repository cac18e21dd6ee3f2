"""Punctual lights on the GPU (pt_light_point, pt_light_spot, pt_light_directional; the rule is in include/pt_amd.h): the
device functions against the numpy rule (tests/punctual_rule.py) through pt_punctual_probe, replays of whole renders from the library's own
probes (camera_probe, intersect, sampler_probe) plus the rule and an independent ray / quad test, the forms of k_shade, "off means off", the
refusals and the CLI.

Every replayed scene is made of diffuse quads, looked at from above with max_depth = 2, blur_strength = 0 and no lens: a sample's radiance is
what its first bounce's branch brings in."""
import os
import subprocess

import numpy as np
import pytest

import punctual_rule as PR
from common import FORMS_H, FORMS_W, GOLDEN_DIR, SceneSpec, _with_env, default_camera, forms_scene

pytestmark = pytest.mark.gpu

FLOOR = dict(q=(-2.0, 0.0, -2.0), u=(4.0, 0.0, 0.0), v=(0.0, 0.0, 4.0), albedo=(0.8, 0.6, 0.4))
OCCLUDER = dict(q=(-0.35, 0.9, -0.45), u=(0.6, 0.0, 0.0), v=(0.0, 0.0, 0.7), albedo=(0.5, 0.5, 0.5))
CEILING = dict(q=(-2.0, 3.0, -2.0), u=(4.0, 0.0, 0.0), v=(0.0, 0.0, 4.0), albedo=(0.7, 0.7, 0.7))   # beyond the light: must not shadow it
EMITTER = dict(q=(2.3, 1.0, -0.3), u=(0.5, 0.0, 0.0), v=(0.0, 0.0, 0.6), albedo=None, emission=(6.0, 5.0, 4.0))   # outside the camera's view
POINT = ("light_point", (0.3, 1.7, -0.2), (40.0, 40.0, 40.0))
W = 48
# (the ceiling quad would hide the floor from a camera above it: the camera sits below it, at y = 2.9 with vfov 64)
CAM = dict(width=W, aspect=1.0, max_depth=2, vfov=64.0, look_from=(0.0, 2.9, 0.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 0.0, -1.0), blur_strength=0.0,
           defocus_angle=0.0, focal_length=1.0, env_color=(0.0, 0.0, 0.0))


def make_scene(pt, ctx, quads, lights, f=0.5, env=(0.0, 0.0, 0.0), sampler="independent", max_depth=2):
    """(scene, camera, quads in primitive-id order: the lights list first, then the objects)"""
    gs = pt.Scene(ctx)
    order = [q for q in quads if q.get("emission")] + [q for q in quads if not q.get("emission")]
    for q in order:
        if q.get("emission"):
            gs.world_add_light(gs.quad(q["q"], q["u"], q["v"], gs.mat_light(gs.tex_solid_rgb(*q["emission"]))))
        else:
            gs.world_add_object(gs.quad(q["q"], q["u"], q["v"], gs.mat_diffuse(gs.tex_solid_rgb(*q["albedo"]), -1)))
    for call in lights:
        getattr(gs, call[0])(*call[1:])
    gs.set_punctual_fraction(f)
    gs.set_sampler(sampler)
    gs.world_build()
    spec = SceneSpec()
    spec.camera = default_camera(**dict(CAM, env_color=env, max_depth=max_depth))
    return gs, spec.make_camera(pt.Camera, []), order


def replay(pt, ctx, gs, cam, order, seed, samples, f, env=(0.0, 0.0, 0.0), sampler="independent"):
    """The expected radiance of every (pixel, sample), samples = range(...): dict with `rad` (P, S, 3), `known` (P, S) — False where the
    first bounce took the lights-list branch, or the BSDF branch of a scene whose continued ray can bring something in that the rule here
    does not restate —, `branch`, `k`, `margin` (the smallest distance of a shadow ray to a quad's edge in the quad's (u, v), and of its hit
    to the light), `occluded`, `beyond` (the shadow ray hit something beyond the light)."""
    n_lights_list = sum(1 for q in order if q.get("emission"))
    lights = n_lights_list > 0
    n = gs.punctual_count()
    recs = [PR.record(gs.punctual_light(k)) for k in range(n)]
    P, S = W * W, len(samples)
    ps = np.stack(np.meshgrid(np.arange(P), np.asarray(samples), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    cr = gs.camera_probe(cam, seed, ps)
    hit = gs.intersect(cr[:, :7])
    c0 = int(cr[0, 7])
    assert (cr[:, 7] == c0).all()
    ND = 64                                                                # (gen_range rejects half of the draws when n is a power of two)
    draws = np.concatenate([ctx.sampler_probe(sampler, seed, p, int(samples[0]), S, c0, ND) for p in range(P)])     # (P * S, ND), pixel-major like ps
    N = P * S
    rad = np.zeros((N, 3))
    known = np.ones(N, bool)
    margin = np.full(N, np.inf)
    occluded, beyond = np.zeros(N, bool), np.zeros(N, bool)
    kk = np.full(N, -1)
    missed = hit[:, 0] == 0.0
    rad[missed] = np.asarray(env, dtype=np.float64)
    prim = hit[:, 2].astype(int)
    assert not any(order[p].get("emission") for p in np.unique(prim[~missed])), "the emitter is out of the camera's view"
    albedo = np.array([order[p]["albedo"] if not missed[i] else (0.0, 0.0, 0.0) for i, p in enumerate(prim)])
    point, gn, sn = hit[:, 6:9], hit[:, 9:12], hit[:, 12:15]
    branch = np.where(missed, -1, PR.branch_of(PR.unit(draws[:, 0]), f, lights))
    known[branch == 0] = False
    quads = [(q["q"], q["u"], q["v"]) for q in order]
    # the punctual branch
    rows = np.nonzero(branch == 1)[0]
    for i in rows:
        kk[i], _ = PR.index_of_draws(draws[i, 1:], n)
    for k, rec in enumerate(recs):
        r = rows[kk[rows] == k]
        if len(r) == 0:
            continue
        w, D, d2, E = PR.light_eval(rec, point[r])
        e = np.abs(PR.LR.quat_mul(PR.LR.frame_to_z(sn[r]), w)[..., 2])[:, None] * (albedo[r] / PR.PI)   # Lambert: |l.z| * (a / pi)
        thr2 = PR.branch_throughput(np.ones(3), e, E, f, n)
        ends = PR.branch_ends(d2, thr2)
        o = PR.shadow_origin(point[r], gn[r], w)
        t, m = PR.first_hit(o, w, quads)
        dl = PR.shadow_distance(rec, o)
        vis = PR.visible(t, dl)
        rad[r] = np.where((~ends & vis)[:, None], thr2, 0.0)
        gap = np.abs(np.where(np.isfinite(t) & np.isfinite(dl), t, 0.0) - np.where(np.isfinite(t) & np.isfinite(dl), dl, np.inf))   # of a hit to the light
        margin[r] = np.where(ends, np.inf, np.minimum(m, gap))
        occluded[r] = ~ends & ~vis
        beyond[r] = ~ends & vis & np.isfinite(t)
    # the BSDF branch: a diffuse bounce whose continued ray adds the environment when it leaves the scene, and nothing else at max_depth = 2
    rows = np.nonzero(branch == 2)[0]
    if any(env) and len(rows):
        assert sampler == "independent" and not lights
        a, b = draws[rows, 1], draws[rows, 2]
        phi = (a >> np.uint64(12)).astype(np.float64) * (1.0 / 4503599627370496.0) * (2.0 * PR.PI)
        r2 = PR.unit(b)
        local = np.stack([np.sqrt(r2) * np.cos(phi), np.sqrt(r2) * np.sin(phi), np.sqrt(1.0 - r2)], axis=-1)
        q = PR.LR.frame_to_z(sn[rows])
        d = PR.LR.quat_mul((-q[0], -q[1], -q[2], q[3]), local)
        o = PR.shadow_origin(point[rows], gn[rows], d)
        second = gs.intersect(np.concatenate([o, d, cr[rows, 6:7]], axis=1))
        _, m = PR.first_hit(o, d, quads)
        margin[rows] = m
        lz = np.abs(local[:, 2])
        p_bsdf = PR.probabilities(f, lights)[2]
        att = (lz[:, None] * (albedo[rows] / PR.PI)) / (p_bsdf * (lz / PR.PI) + 0.0)[:, None]
        rad[rows] = np.where((second[:, 0] == 0.0)[:, None], att * np.asarray(env, dtype=np.float64), 0.0)
    elif lights:
        known[rows] = False                                                # (its continued ray may reach the emitter)
    sh = lambda x: x.reshape(P, S, *x.shape[1:])
    return dict(rad=sh(rad), known=sh(known), branch=sh(branch), k=sh(kk), margin=sh(margin), occluded=sh(occluded), beyond=sh(beyond))


def sums(rp):
    """a pixel's sum as the static pool forms it: the samples in order"""
    acc = np.zeros_like(rp["rad"][:, 0])
    for s in range(rp["rad"].shape[1]):
        acc = acc + rp["rad"][:, s]
    return acc.reshape(W, W, 3)


def assert_no_sample_left_out(rp):
    m = rp["margin"].min()
    print(f"smallest margin of a shadow / continued ray: {m:.3e}")
    assert (rp["margin"] >= 1e-6).all(), m


# ---- 1. the probe ----------------------------------------------------------------------------------------------------------------
def test_probe_equals_the_rule(pt, ctx):
    lights = [POINT, ("light_spot", (0.3, 1.7, -0.2), (0.1, 0.0, 0.4), 15.0, 25.0, (9.0, 8.0, 7.0)), ("light_spot", (-0.5, 1.2, 0.3), (0.0, 0.0, 0.0), 20.0, 20.0, (3.0, 3.0, 3.0)),
              ("light_directional", (0.3, -1.0, 0.2), (3.0, 2.5, 2.0))]
    gs, cam, _ = make_scene(pt, ctx, [FLOOR], lights)
    n = gs.punctual_count()
    assert n == 4
    recs = [PR.record(gs.punctual_light(k)) for k in range(n)]
    assert [r["kind"] for r in recs] == [0, 1, 1, 2]
    np.testing.assert_array_equal(recs[0]["I"], PR.point_intensity((40.0, 40.0, 40.0)))
    np.testing.assert_array_equal(recs[1]["axis"], PR.LR.normalize(np.array([0.1, 0.0, 0.4]) - np.array([0.3, 1.7, -0.2])))
    np.testing.assert_array_equal(recs[3]["axis"], PR.LR.normalize(np.array([0.3, -1.0, 0.2])))
    np.testing.assert_allclose([recs[1]["cos_i"], recs[1]["cos_o"]], np.cos(np.radians([15.0, 25.0])), rtol=1e-15)
    assert recs[2]["cos_i"] == recs[2]["cos_o"]
    rng = np.random.default_rng(77)
    m = 3000
    pts = rng.uniform(-3.0, 3.0, (m, 3))
    pts[:4] = [r["pos"] for r in recs]                                     # at the lights: d2 = 0
    # which 1: every light at every point
    for k, rec in enumerate(recs):
        got = gs.punctual_probe(1, np.concatenate([np.full((m, 1), float(k)), pts], axis=1))
        assert got.tobytes() == PR.eval7(rec, pts).tobytes(), k
    # which 0: the index draw of (seed 0, pixel i, sample 0) from draw 0, then the evaluation
    got = gs.punctual_probe(0, pts)
    picked = set()
    for i in range(400):
        k, used = PR.index_of_draws(ctx.sampler_probe("independent", 0, i, 0, 1, 0, 64)[0], n)
        assert (got[i, 0], got[i, 8]) == (k, used), i
        picked.add(k)
    for k, rec in enumerate(recs):
        sel = got[:, 0] == k
        assert got[sel, 1:8].tobytes() == PR.eval7(rec, pts[sel]).tobytes(), k
    assert set(np.unique(got[:, 0])) == {0.0, 1.0, 2.0, 3.0} and got[:, 8].min() >= 1
    assert picked == {0, 1, 2, 3}
    with pytest.raises(pt.PtError, match="k a light"):
        gs.punctual_probe(1, [[4.0, 0.0, 0.0, 0.0]])
    gs.close()


# ---- 2. a point light and its shadow --------------------------------------------------------------------------------------------------
def test_point_light_with_shadow(pt, ctx):
    spp, seed, f = 32, 11, 0.5
    gs, cam, order = make_scene(pt, ctx, [FLOOR, OCCLUDER, CEILING], [POINT], f)
    acc, st = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
    rp = replay(pt, ctx, gs, cam, order, seed, range(spp), f)
    assert rp["known"].all()
    assert_no_sample_left_out(rp)
    want = sums(rp)
    np.testing.assert_allclose(acc, want, rtol=1e-12, atol=0.0)
    punct = rp["branch"] == 1
    dark = (rp["occluded"] | ~punct).all(axis=1) & rp["occluded"].any(axis=1)        # every punctual sample of the pixel is shadowed
    dark = dark.reshape(W, W)
    assert dark.sum() >= 10 and not acc[dark].any()                                    # exactly 0
    lit_beyond = rp["beyond"].any(axis=1).reshape(W, W)                                # the shadow ray reached the ceiling, beyond the light
    assert lit_beyond.sum() >= 100 and (acc[lit_beyond] > 0.0).all()
    assert st.samples == W * W * spp
    dyn, dst = gs.render(cam, seed, 0, spp)
    assert dst.slots_per_pixel == 0 and dst.samples == st.samples and dst.segments == st.segments
    np.testing.assert_allclose(dyn, acc, rtol=1e-11, atol=1e-11)
    gs.close()


# ---- 3. a spot light ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner, outer", [(15.0, 25.0), (20.0, 20.0)])
def test_spot_light(pt, ctx, inner, outer):
    spp, seed, f = 16, 5, 0.5
    spot = ("light_spot", (0.3, 1.7, -0.2), (0.1, 0.0, 0.4), inner, outer, (9.0, 8.0, 7.0))
    gs, cam, order = make_scene(pt, ctx, [FLOOR, OCCLUDER, CEILING], [spot], f)
    acc, _ = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
    rp = replay(pt, ctx, gs, cam, order, seed, range(spp), f)
    assert rp["known"].all()
    assert_no_sample_left_out(rp)
    np.testing.assert_allclose(acc, sums(rp), rtol=1e-12, atol=0.0)
    # the three zones, by the rule on the first hits
    rec = PR.record(gs.punctual_light(0))
    ps = np.stack([np.arange(W * W), np.zeros(W * W)], axis=1)
    hit = gs.intersect(gs.camera_probe(cam, seed, ps)[:, :7])
    w, D, d2, E = PR.light_eval(rec, hit[:, 6:9])
    c = -PR.dot(w, rec["axis"][None, :])
    outside, inside = (c < rec["cos_o"]).reshape(W, W), (c >= rec["cos_i"]).reshape(W, W)
    assert outside.sum() >= 100 and not acc[outside].any()                              # exactly 0 outside the outer cone
    assert inside.sum() >= 50
    np.testing.assert_array_equal(E[inside.reshape(-1)], rec["I"][None, :] / d2[inside.reshape(-1), None])   # the point formula inside the inner cone
    between = ~outside & ~inside
    if inner < outer:
        fall = (E[:, 0] * d2 / rec["I"][0]).reshape(W, W)[between]
        assert between.sum() >= 50 and (fall > 0.0).any() and (fall < 1.0).all()
    else:
        assert not between.any()
    gs.close()


# ---- 4. a sun and a grey environment --------------------------------------------------------------------------------------------------------
def test_sun_with_grey_environment(pt, ctx):
    spp, seed, f, env = 16, 3, 0.5, (0.3, 0.3, 0.3)
    gs, cam, order = make_scene(pt, ctx, [FLOOR, OCCLUDER], [("light_directional", (0.3, -1.0, 0.2), (3.0, 2.5, 2.0))], f, env=env)
    acc, _ = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
    rp = replay(pt, ctx, gs, cam, order, seed, range(spp), f, env=env)
    assert rp["known"].all()
    assert_no_sample_left_out(rp)
    np.testing.assert_allclose(acc, sums(rp), rtol=1e-12, atol=0.0)
    # a punctual sample brings e * E / pm and no environment (its shadow ray leaves the scene); a BSDF sample that leaves brings a * env / p_bsdf
    punct, bsdf = rp["branch"] == 1, rp["branch"] == 2
    rec = PR.record(gs.punctual_light(0))
    cos = -rec["axis"][1]
    lit = punct & ~rp["occluded"] & (rp["rad"][..., 0] > 0.0)
    floor_lit = lit & np.isclose(rp["rad"][..., 0], cos * (0.8 / PR.PI) * 3.0 / f, rtol=1e-12)
    assert floor_lit.sum() >= 1000 and rp["occluded"].sum() >= 100
    left = rp["rad"][bsdf & (rp["rad"][..., 0] > 0.0)]                        # the BSDF samples that left the scene: from the floor, or from the occluder's top
    p_bsdf = PR.probabilities(f, False)[2]
    from_floor = np.isclose(left, np.array(FLOOR["albedo"]) * 0.3 / p_bsdf, rtol=1e-12).all(axis=1)
    from_top = np.isclose(left, np.array(OCCLUDER["albedo"]) * 0.3 / p_bsdf, rtol=1e-12).all(axis=1)
    assert (from_floor | from_top).all() and from_floor.sum() >= 1000 and from_top.sum() >= 10
    gs.close()


# ---- 5. three lights of three kinds beside a lights list ----------------------------------------------------------------------------------
def test_three_kinds_and_a_lights_list(pt, ctx):
    spp, seed, f = 8, 9, 0.4
    lights = [POINT, ("light_spot", (-0.6, 1.5, 0.4), (-0.2, 0.0, 0.1), 20.0, 35.0, (9.0, 8.0, 7.0)), ("light_directional", (0.3, -1.0, 0.2), (3.0, 2.5, 2.0))]
    gs, cam, order = make_scene(pt, ctx, [FLOOR, OCCLUDER, EMITTER], lights, f)
    assert PR.probabilities(f, True) == ((1.0 - f) / 2.0, f, 1.0 - (1.0 - f) / 2.0 - f)
    seen, n_checked, branches = set(), 0, set()
    for s in range(spp):
        acc, _ = gs.render(cam, seed, s, s + 1, slots_per_pixel=1)
        rp = replay(pt, ctx, gs, cam, order, seed, range(s, s + 1), f)
        assert_no_sample_left_out(rp)
        k = rp["known"][:, 0].reshape(W, W)
        np.testing.assert_allclose(acc[k], rp["rad"][:, 0].reshape(W, W, 3)[k], rtol=1e-12, atol=0.0)
        n_checked += int(k.sum())
        seen |= set(np.unique(rp["k"][rp["branch"] == 1]))
        branches |= set(np.unique(rp["branch"]))
    assert seen == {0, 1, 2} and branches >= {0, 1, 2}
    share = n_checked / (W * W * spp)
    assert abs(share - f) < 0.02, share                                     # p_punct = f of the samples took the punctual branch
    gs.close()


# ---- 6. the fraction does not change the mean -------------------------------------------------------------------------------------------
def test_fraction_does_not_change_the_mean(pt, ctx):
    gs = pt.Scene(ctx)
    wall = lambda q, u, v, c: gs.world_add_object(gs.quad(q, u, v, gs.mat_diffuse(gs.tex_solid_rgb(*c), -1)))
    wall((-1.0, 0.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.7, 0.7, 0.7))       # floor
    wall((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.7, 0.7, 0.7))       # ceiling
    wall((-1.0, 0.0, -1.0), (0.0, 2.0, 0.0), (0.0, 0.0, 2.0), (0.7, 0.2, 0.2))       # left
    wall((1.0, 0.0, -1.0), (0.0, 2.0, 0.0), (0.0, 0.0, 2.0), (0.2, 0.7, 0.2))        # right
    wall((-1.0, 0.0, 1.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.7, 0.7, 0.7))        # back
    gs.light_point((0.2, 1.5, 0.1), (20.0, 20.0, 20.0))
    gs.world_build()
    spec = SceneSpec()
    spec.camera = default_camera(width=64, aspect=1.0, max_depth=8, vfov=50.0, look_from=(0.0, 1.0, -3.1), look_at=(0.0, 1.0, 0.0), vup=(0.0, 1.0, 0.0),
                                 blur_strength=0.5, defocus_angle=0.0, focal_length=1.0, env_color=(0.0, 0.0, 0.0))
    cam = spec.make_camera(pt.Camera, [])
    spp, frames = 256, {}
    for f in (0.25, 0.75):
        gs.set_punctual_fraction(f)
        frames[f] = [gs.render(cam, seed, 0, spp)[0] / spp for seed in (1, 2)]
    N = 64 * 64
    var = {f: (a - b).reshape(N, 3).var(axis=0, ddof=1) for f, (a, b) in frames.items()}     # of a pixel's difference between two seeds: twice a pixel's
    mean = {f: ((a + b) / 2.0).reshape(N, 3).mean(axis=0) for f, (a, b) in frames.items()}
    sigma = np.sqrt((var[0.25] + var[0.75]) / (4.0 * N))                                    # of the difference of the two settings' frame means
    z = (mean[0.25] - mean[0.75]) / sigma
    print(f"frame means {mean[0.25]} (f = 0.25) {mean[0.75]} (f = 0.75), sigma {sigma}, z {z}")
    assert (mean[0.25] > 0.01).all() and (np.abs(z) < 5.0).all(), z
    gs.close()


# ---- 7. every PLT form launches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
@pytest.mark.parametrize("lights", [True, False], ids=["lights", "nolights"])
def test_every_plt_form(pt, ctx, lights, sampler):
    spec = forms_scene("PLAIN", lights)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    plain, _ = gs.render(cam, 7, 0, 4, slots_per_pixel=1)
    gs.light_point((0.5, 3.0, 0.5), (200.0, 180.0, 160.0))
    gs.light_spot((-2.0, 3.5, -1.0), (0.0, 0.0, 0.0), 20.0, 40.0, (30.0, 30.0, 40.0))
    gs.light_directional((0.2, -1.0, 0.3), (1.0, 0.9, 0.8))
    gs.world_build()
    gs.set_sampler(sampler)
    forced = lambda v, fn: _with_env({"PT_EXPERIMENT": "1", "PT_SHADE_VARIANT": str(v)}, fn)
    ref, rst = gs.render(cam, 7, 0, 4, slots_per_pixel=1)
    assert rst.samples == FORMS_W * FORMS_H * 4
    fin = np.isfinite(ref)
    assert fin.mean() >= 0.99 and (sampler == "sobol" or (ref != plain)[fin].mean() > 0.3)       # the lights are in the picture
    sel = np.sort(np.random.default_rng(65).choice(FORMS_W * FORMS_H, size=65, replace=False)).astype(np.uint32)
    m = np.zeros(FORMS_W * FORMS_H, bool)
    m[sel] = True
    m = m.reshape(FORMS_H, FORMS_W)
    same = lambda a, b: ((a == b) | (np.isnan(a) & np.isnan(b))).all()
    for v in (22, 32):
        acc, st = forced(v, lambda: gs.render(cam, 7, 0, 4, slots_per_pixel=1))
        assert st.shade_variant == v and same(acc, ref) and (st.segments, st.samples) == (rst.segments, rst.samples), v
        out, st = forced(v, lambda: gs.render_pixels(cam, 7, sel, 0, 4, slots_per_pixel=1))
        assert st.shade_variant == v and st.samples == 65 * 4 and same(out[m], ref[m]) and not out[~m].any(), v
        dyn, st = forced(v, lambda: gs.render(cam, 7, 0, 4))
        assert st.shade_variant == v and (st.segments, st.samples) == (rst.segments, rst.samples)
        np.testing.assert_allclose(dyn[fin], ref[fin], rtol=1e-11, atol=1e-11)
        dl, st = forced(v, lambda: gs.render_pixels(cam, 7, sel, 0, 4))
        np.testing.assert_allclose(dl[m][fin[m]], ref[m][fin[m]], rtol=1e-11, atol=1e-11)
    ada, counts, ast = gs.render_adaptive(cam, 7, 2, 6, 0.05)
    assert ast.samples == int(counts.sum()) and counts.min() >= 2 and counts.max() <= 6
    gs.close()


# ---- 8. off means off ----------------------------------------------------------------------------------------------------------------------
def test_off_means_off(pt, ctx):
    g = np.load(os.path.join(GOLDEN_DIR, "scene3_w64_spp16_seed1.npz"))
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 16)
    assert gs.punctual_fraction() == 0.5
    gs.set_punctual_fraction(0.9)
    assert gs.punctual_fraction() == 0.9 and gs.punctual_count() == 0
    acc, st = gs.render(cam, 1, 0, 16, slots_per_pixel=1)
    np.testing.assert_array_equal(acc, g["accum"])
    assert st.segments == int(g["segments"])
    gs.close()
    gs, cam, _ = make_scene(pt, ctx, [FLOOR, OCCLUDER, EMITTER], [])
    cam.max_depth = 4
    unlit, ust = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    gs.light_point(*POINT[1:])
    again, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)                        # the list takes effect at the next build
    np.testing.assert_array_equal(again, unlit)
    gs.world_build()
    lit, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    assert (lit != unlit).mean() > 0.5
    gs.clear_punctual_lights()
    gs.world_build()
    back, bst = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    np.testing.assert_array_equal(back, unlit)
    assert bst.segments == ust.segments
    gs.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(pt, ctx):
    gs = pt.Scene(ctx)
    nan, inf = float("nan"), float("inf")
    bad = [("light_point", (0, 1, 0), (1, -1, 1)), ("light_point", (0, 1, 0), (1, nan, 1)), ("light_point", (0, 1, 0), (inf, 1, 1)), ("light_point", (0, nan, 0), (1, 1, 1)),
           ("light_spot", (0, 1, 0), (0, 1, 0), 10, 20, (1, 1, 1)), ("light_spot", (0, 1, 0), (0, 0, 0), 20, 10, (1, 1, 1)), ("light_spot", (0, 1, 0), (0, 0, 0), -1, 10, (1, 1, 1)),
           ("light_spot", (0, 1, 0), (0, 0, 0), 10, 180, (1, 1, 1)), ("light_spot", (0, 1, 0), (0, 0, 0), nan, 20, (1, 1, 1)), ("light_spot", (0, 1, 0), (0, 0, 0), 10, 20, (1, 1, -0.5)),
           ("light_spot", (0, 1, 0), (0, inf, 0), 10, 20, (1, 1, 1)), ("light_directional", (0, 0, 0), (1, 1, 1)), ("light_directional", (0, -1, 0), (1, 1, -1)),
           ("light_directional", (0, nan, 0), (1, 1, 1)), ("light_directional", (0, -1, 0), (1, inf, 1))]
    for call in bad:
        with pytest.raises(pt.PtError):
            getattr(gs, call[0])(*call[1:])
        assert gs.punctual_count() == 0, call
    for f in (0.0, 1.0, -0.1, 1.5, nan, inf):
        with pytest.raises(pt.PtError, match="0 < f < 1"):
            gs.set_punctual_fraction(f)
        assert gs.punctual_fraction() == 0.5
    assert gs.light_spot((0, 1, 0), (0, 0, 0), 0.0, 0.0, (0, 0, 0)) == 0 and gs.light_spot((0, 1, 0), (0, 0, 0), 30.0, 179.9, (1, 1, 1)) == 1
    with pytest.raises(pt.PtError, match="no such light"):
        gs.punctual_light(2)
    for i in range(2, 2048):
        assert gs.light_point((0.0, 1.0 + i * 1e-3, 0.0), (1.0, 1.0, 1.0)) == i
    with pytest.raises(pt.PtError, match="full"):
        gs.light_point((0.0, 1.0, 0.0), (1.0, 1.0, 1.0))
    with pytest.raises(pt.PtError, match="full"):
        gs.light_directional((0.0, -1.0, 0.0), (1.0, 1.0, 1.0))
    assert gs.punctual_count() == 2048
    gs.clear_punctual_lights()
    assert gs.punctual_count() == 0 and gs.light_point((0.0, 1.0, 0.0), (1.0, 1.0, 1.0)) == 0
    with pytest.raises(pt.PtError, match="not built"):
        gs.punctual_probe(0, [[0.0, 0.0, 0.0]])
    gs.close()


def test_a_full_list_renders(pt, ctx):
    """2048 lights: the index field of the bounce word at its largest"""
    gs, cam, order = make_scene(pt, ctx, [FLOOR, OCCLUDER], [("light_point", (0.3 + 1e-4 * i, 1.7, -0.2), (40.0, 40.0, 40.0)) for i in range(2048)])
    acc, st = gs.render(cam, 4, 0, 4, slots_per_pixel=1)
    rp = replay(pt, ctx, gs, cam, order, 4, range(4), 0.5)
    assert rp["k"].max() > 1900
    ok = (rp["margin"] >= 1e-6).all(axis=1).reshape(W, W)
    assert ok.mean() > 0.95
    np.testing.assert_allclose(acc[ok], sums(rp)[ok], rtol=1e-12, atol=0.0)
    dyn, _ = gs.render(cam, 4, 0, 4)
    np.testing.assert_allclose(dyn, acc, rtol=1e-11, atol=1e-11)
    gs.close()


def feature_scenes(pt, ctx):
    """(name, the word its refusal names, a scene with that feature in effect, its camera, how to switch the feature off)"""
    def base():
        gs = pt.Scene(ctx)
        gs.world_add_object(gs.quad(FLOOR["q"], FLOOR["u"], FLOOR["v"], gs.mat_diffuse(gs.tex_solid_rgb(*FLOOR["albedo"]), -1)))
        spec = SceneSpec()
        spec.camera = default_camera(**dict(CAM, env_color=(0.2, 0.2, 0.2), max_depth=4))
        return gs, spec.make_camera(pt.Camera, [])

    gs, cam = base()
    env = gs.tex_image_rgbf32(np.random.default_rng(1).uniform(0.1, 1.0, size=(4, 8, 3)).astype(np.float32))
    cam.env_is_map, cam.env_tex = 1, env
    gs.set_env_sampling(0.5)
    yield "env", "environment importance sampling", gs, cam
    gs, cam = base()
    gs.world_add_object(gs.sphere(0.4, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), gs.mat_medium(1.0, (0.8, 0.8, 0.8), 0.0)))
    yield "medium", "media", gs, cam
    gs, cam = base()
    gs.world_add_light(gs.sphere(0.2, (1.0, 2.0, 0.0), (1.0, 2.0, 0.0), gs.mat_light(gs.tex_solid_rgb(5.0, 5.0, 5.0))))
    gs.set_light_sampling("exact")
    yield "lse", "exact light sampling", gs, cam
    gs, cam = base()
    glass = gs.mat_glass(gs.tex_solid_rgb(1.0, 1.0, 1.0), gs.tex_solid_f(0.05), 0.0, 1.5)
    gs.mat_glass_set_dispersion(glass, 30.0)
    gs.world_add_object(gs.sphere(0.4, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), glass))
    yield "dispersion", "dispersion", gs, cam
    gs, cam = base()
    box = gs.cuboid((0.0, 0.0, 0.0), (0.3, 0.3, 0.3), gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1))
    gs.world_add_object(gs.instance_moving(box, (0.0, 1.0, 0.0), 0.0, 0.0, (0.0, 0.5, 0.0), (0.5, 0.5, 0.0)))
    yield "motion", "motion", gs, cam


def test_refusals(pt, ctx):
    for name, word, gs, cam in feature_scenes(pt, ctx):
        gs.world_build()
        alone, _ = gs.render(cam, 1, 0, 2, slots_per_pixel=1)                  # the feature alone renders
        gs.light_point(*POINT[1:])
        gs.world_build()
        px = np.arange(10, dtype=np.uint32)
        for fn in (lambda: gs.render(cam, 1, 0, 2, slots_per_pixel=1), lambda: gs.render(cam, 1, 0, 2), lambda: gs.render_pixels(cam, 1, px, 0, 2),
                   lambda: gs.render_adaptive(cam, 1, 2, 4, 0.1)):
            with pytest.raises(pt.PtError, match="punctual lights") as e:
                fn()
            assert word in str(e.value), (name, str(e.value))
        gs.clear_punctual_lights()                                             # the way back
        gs.world_build()
        back, _ = gs.render(cam, 1, 0, 2, slots_per_pixel=1)
        np.testing.assert_array_equal(back, alone, err_msg=name)
        gs.close()
    gs, cam, _ = make_scene(pt, ctx, [FLOOR, OCCLUDER], [POINT])
    cam.max_depth = 1 << 20
    with pytest.raises(pt.PtError, match="punctual lights") as e:
        gs.render(cam, 1, 0, 1, slots_per_pixel=1)
    assert "2^20" in str(e.value)
    cam.max_depth = (1 << 20) - 1
    deep, _ = gs.render(cam, 1, 0, 1, slots_per_pixel=1)
    assert np.isfinite(deep).all() and deep.any()
    gs.clear_punctual_lights()
    gs.world_build()
    cam.max_depth = 1 << 20
    gs.render(cam, 1, 0, 1, slots_per_pixel=1)                                 # without the lights the bound is gone
    gs.close()


# ---- 10. the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_point_light(pt, ctx, tmp_path):
    """The Cornell box with a strong point light under its ceiling: the floor pixels whose way to the light a box blocks (the library's
    intersect probe says which) are darker than the floor pixels that see the light."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "lamp.png"
    light = np.array([278.0, 500.0, 278.0])
    r = subprocess.run([exe, "-s", "3", "--width", "64", "--spp", "32", "--point-light", "278,500,278,3e7,3e7,3e7", "--punctual-fraction", "0.6", "--out", str(out),
                        "--assets", pt.ASSET_DIR], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = pt.decode_image_rgb8(str(out)).astype(np.float64)
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 32)
    cam.blur_strength = 0.0
    n = img.shape[0] * img.shape[1]
    hit = gs.intersect(gs.camera_probe(cam, 1, np.stack([np.arange(n), np.zeros(n)], axis=1))[:, :7])
    floor = (hit[:, 0] == 1.0) & (np.abs(hit[:, 7]) < 1e-6)
    o = hit[:, 6:9] + np.array([0.0, 1e-3, 0.0])
    L = light[None, :] - o
    D = np.sqrt(PR.dot(L, L))
    sh = gs.intersect(np.concatenate([o, L / D[:, None], np.zeros((n, 1))], axis=1))
    blocked = floor & (sh[:, 0] == 1.0) & (sh[:, 1] < D - 1.0)
    free = floor & ~((sh[:, 0] == 1.0) & (sh[:, 1] < D + 1.0))
    assert blocked.sum() >= 20 and free.sum() >= 100
    lum = img.reshape(n, 3).mean(axis=1)
    print(f"floor pixels: {blocked.sum()} shadowed, mean {lum[blocked].mean():.1f}; {free.sum()} lit, mean {lum[free].mean():.1f}")
    assert lum[free].mean() > lum[blocked].mean() + 20.0
    r = subprocess.run([exe, "-s", "3", "--width", "32", "--spp", "2", "--spot-light", "278,500,278,278,0,278,20,30,1e5,1e5,1e5", "--sun", "0.2,-1,0.3,1,1,1",
                        "--point-light", "100,300,100,1e6,1e6,1e6", "--point-light", "400,300,100,1e6,1e6,1e6", "--sampler", "sobol", "--out", str(tmp_path / "all.png"),
                        "--assets", pt.ASSET_DIR], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    gs.close()
