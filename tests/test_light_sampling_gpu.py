"""Exact light sampling on the GPU (pt_scene_set_light_sampling; the rule is in include/pt_amd.h): validation, the
device functions against the numpy rule (tests/light_rule.py) through pt_light_probe, "off means off", the estimator against
quadrature of the TRUE radiance, a scalar replay of whole paths, the structural identities and the refusals.

Which k_shade shape a render launched: the LSE forms exist for the two window sizes of variant 42. Every render below with fewer than
blocks_shade * 16 windows of 8192 slots launches the 4096-slot shape (22); the full-HD render runs with PT_WIDE_WINDOW_MIN=1 and
launches the 8192-slot shape (32), the one that holds the most LDS."""
import os
import subprocess

import numpy as np
import pytest

import light_rule as LR
from common import (MIS_BOX, MIS_CAM, MIS_EMISSION, MIS_INST, MIS_QUAD, SceneSpec, default_camera, icosphere, mis_expected, mis_scene,
                    mis_zscores)

pytestmark = pytest.mark.gpu


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
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def light_only_scene(pt, ctx, P, I, scale, chained, device_bvh=False):
    """One mesh, alone in the lights list, directly or under the probe's two-level instance chain."""
    gs = pt.Scene(ctx)
    lm = gs.mat_light(gs.tex_solid_rgb(4.0, 4.0, 4.0))
    obj = gs.mesh(scale, P, I, None, None, lm)
    if chained:
        for axis, angle, tr in reversed(LR.probe_chain_spec()):     # innermost first
            obj = gs.instance(obj, axis, angle, tr)
    gs.world_add_light(obj)
    if device_bvh:
        gs.set_device_bvh_threshold(1)
    gs.world_build()
    return gs


# ---- 1. validation ---------------------------------------------------------------------------------------------------------------
def test_validation(pt, ctx):
    gs = pt.Scene(ctx)
    assert gs.light_sampling() == 0
    gs.set_light_sampling("exact")
    assert gs.light_sampling() == 1
    for bad in (2, -1, 7):
        with pytest.raises(pt.PtError, match="kind must be 0"):
            gs.set_light_sampling(bad)
        assert gs.light_sampling() == 1                             # the setting is kept
    with pytest.raises(pt.PtError):
        gs.set_light_sampling("fast")
    gs.set_light_sampling(0)
    assert gs.light_sampling() == 0
    gs.set_light_sampling("exact")
    with pytest.raises(pt.PtError, match="not built"):
        gs.light_probe(0, np.zeros((1, 4)))
    floor = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.quad((-1.0, 0.0, -1.0), (0.0, 0.0, 2.0), (2.0, 0.0, 0.0), floor))
    gs.world_build()
    with pytest.raises(pt.PtError, match="no lights list"):
        gs.light_probe(1, np.zeros((1, 7)))
    lm = gs.mat_light(gs.tex_solid_rgb(1.0, 1.0, 1.0))
    gs.world_add_light(gs.sphere(0.5, (0.0, 2.0, 0.0), (0.0, 2.0, 0.0), lm))
    with pytest.raises(pt.PtError, match="not built"):             # adding to the world unbuilds it
        gs.light_probe(0, np.zeros((1, 4)))
    gs.world_build()
    assert gs.light_sampling() == 1                                 # a build keeps the setting
    with pytest.raises(pt.PtError, match="which must be 0 or 1"):
        gs.light_probe(2, np.zeros((1, 4)))
    assert gs.light_probe(0, np.zeros((0, 4))).shape == (0, 6)
    out = gs.light_probe(0, np.array([[0.0, 0.0, 0.0, 0.0]]))
    assert out.shape == (1, 6) and out[0, 3] == 0.0 and out[0, 4] == -1.0
    gs.close()


# ---- 2. the device functions against the rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chained", [False, True], ids=["direct", "chain"])
@pytest.mark.parametrize("name", LR.PROBE_MESHES)
def test_probe_mesh_against_the_rule(pt, ctx, name, chained):
    c = LR.probe_case(name, chained)
    gs = light_only_scene(pt, ctx, c["P"], c["I"], c["scale"], chained)
    gs.set_light_sampling("exact")
    s = c["sample"]
    out = gs.light_probe(0, s["origins"])
    np.testing.assert_array_equal(out[:, 3], s["light"])
    np.testing.assert_array_equal(out[:, 4], s["face"])            # every row
    np.testing.assert_array_equal(out[:, 5], s["draws"])
    err = np.abs(out[:, :3] - s["dirs"]).max()
    print(f"{name} chained={chained}: {len(c['tris'])} triangles; sample: max |direction - rule| {err:.2e} (unit vectors)")
    assert err <= 1e-12                                             # rtol 1e-12 of a unit vector: per component against its length
    keep = c["keep"]
    pdf = gs.light_probe(1, c["rays"])
    multi = (c["hits"][keep] >= 2).mean()
    rel = np.abs(pdf[keep] - c["pdf"][keep]) / np.maximum(c["pdf"][keep], 1e-300)
    rel[(c["pdf"][keep] == 0.0) & (pdf[keep] == 0.0)] = 0.0
    print(f"   pdf: {len(keep)} rays, {1.0 - keep.mean():.3%} left out, {multi:.1%} of the kept with two or more hits, max relative error {rel.max():.2e}")
    assert 1.0 - keep.mean() <= 0.01
    assert multi >= 0.3 or name == "quad"                           # (a planar mesh cannot be met twice by one ray)
    np.testing.assert_allclose(pdf[keep], c["pdf"][keep], rtol=1e-11, atol=0.0)
    gs.close()
    # the GPU builder's tree: the same pdfs (only the order of the sum is the tree's)
    gd = light_only_scene(pt, ctx, c["P"], c["I"], c["scale"], chained, device_bvh=True)
    gd.set_light_sampling("exact")
    n_dev, deepest = gd.device_bvh_info()
    pdf_d = gd.light_probe(1, c["rays"])
    out_d = gd.light_probe(0, s["origins"])
    gd.close()
    assert n_dev == 1
    np.testing.assert_allclose(pdf_d[keep], c["pdf"][keep], rtol=1e-11, atol=0.0)
    np.testing.assert_allclose(pdf_d[keep], pdf[keep], rtol=1e-11, atol=0.0)
    np.testing.assert_array_equal(out_d, out)                       # the sampler reads no tree


def test_probe_sphere_against_the_rule(pt, ctx):
    """Both branches, on a MOVING sphere (the centre at the ray's time): origins outside and inside."""
    p1, p2, r = np.array([0.2, 1.0, -0.3]), np.array([0.5, 1.3, -0.2]), 0.7
    gs = pt.Scene(ctx)
    gs.world_add_light(gs.sphere(r, tuple(p1), tuple(p2), gs.mat_light(gs.tex_solid_rgb(3.0, 3.0, 3.0))))
    gs.world_build()
    gs.set_light_sampling("exact")
    rng = np.random.default_rng(21)
    n = 4096
    time = rng.uniform(0.0, 1.0, n)
    centre = p1 + (p2 - p1) * time[:, None]
    x = rng.normal(size=(n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    inside = np.arange(n) % 4 == 0
    origin = centre + x * np.where(inside, rng.uniform(0.0, 0.95, n), rng.uniform(1.2, 5.0, n))[:, None] * r
    dr = LR.Draws(0, np.arange(n), 0)
    light = dr.index(1)
    u1, u2 = dr.pair()
    want = LR.sample_sphere(centre, r, origin, u1, u2)
    out = gs.light_probe(0, np.concatenate([origin, time[:, None]], axis=1))
    np.testing.assert_array_equal(out[:, 3], light)
    np.testing.assert_array_equal(out[:, 4], -1.0)
    np.testing.assert_array_equal(out[:, 5], dr.draw.astype(np.int64))
    err = np.abs(out[:, :3] - want).max()
    assert err <= 1e-12, err
    # pdf: half of the rays are the sampled directions, half random; rows whose ray passes within 1e-9 r^2 of tangency are left out
    d = np.where((np.arange(n) % 2 == 0)[:, None], want * rng.uniform(0.5, 2.0, (n, 1)), rng.normal(size=(n, 3)))
    L = centre - origin
    dn = LR.normalize(d)
    dd = LR.dot(L, L) - LR.dot(L, dn) ** 2
    keep = inside | (np.abs(dd - r * r) > 1e-9 * r * r)
    pdf = gs.light_probe(1, np.concatenate([origin, d, time[:, None]], axis=1))
    gs.close()
    ref = LR.pdf_sphere(centre, r, origin, d)
    print(f"sphere: max |direction - rule| {err:.2e}; pdf: {1.0 - keep.mean():.3%} left out, {(ref[keep] > 0).mean():.1%} of the kept rows hit")
    assert 1.0 - keep.mean() <= 0.01 and (ref[keep & ~inside] > 0).mean() > 0.3 and (ref[keep & ~inside] == 0).mean() > 0.3   # a third aimed, the random rays mostly miss
    np.testing.assert_allclose(pdf[keep], ref[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_array_equal(pdf[inside], 1.0 / (4.0 * np.pi))


# ---- 3. off means off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", [3, 7])
def test_quad_lights_only_kind_1_is_kind_0(pt, ctx, sid):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(sid, 64, 4)
    ref, st0 = gs.render(cam, 5, 0, 4, slots_per_pixel=1)
    dyn0, sd0 = gs.render(cam, 5, 0, 4)
    gs.set_light_sampling("exact")
    got, st1 = gs.render(cam, 5, 0, 4, slots_per_pixel=1)
    dyn1, sd1 = gs.render(cam, 5, 0, 4)
    gs.close()
    np.testing.assert_array_equal(got, ref)
    for a, b in ((st0, st1), (sd0, sd1)):
        assert (a.shade_variant, a.launches_shade, a.launches_extend, a.segments, a.blocks_shade) == \
               (b.shade_variant, b.launches_shade, b.launches_extend, b.segments, b.blocks_shade)


def test_toggling_back_gives_kind_0_bits(pt, ctx):
    gs, cam, _ = build(pt, ctx, mis_scene("two"))
    ref, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    gs.set_light_sampling("exact")
    on, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    gs.set_light_sampling("reference")
    off, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    gs.close()
    assert not np.array_equal(on, ref)
    np.testing.assert_array_equal(off, ref)


# ---- 4. the estimator against quadrature of the TRUE radiance -----------------------------------------------------------------------------
def mis_mesh_scene(kind):
    """common.mis_scene's floor and camera under a MESH light: the quad as the irregular 128-triangle mesh, the same under MIS_INST, or
    the box as a closed mesh whose faces are tessellated 4 x 4 x 2."""
    s = SceneSpec()
    floor = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.8, 0.6, 0.4), -1)
    s.add("world_add_object", s.add("quad", (-4.0, 0.0, -4.0), (0.0, 0.0, 8.0), (8.0, 0.0, 0.0), floor))
    lm = s.add("mat_light", s.add("tex_solid_rgb", *MIS_EMISSION))
    P, I = LR.tessellate_box(*MIS_BOX, 4) if kind == "cuboid" else LR.tessellate_quad(*MIS_QUAD, 8)
    mesh = s.add("mesh", 1.0, P, I, None, None, lm)
    s.add("world_add_light", s.add("instance", mesh, *MIS_INST) if kind == "instquad" else mesh)
    s.add("world_build")
    c = MIS_CAM
    s.camera = default_camera(width=c["width"], aspect=c["aspect"], spp=1, max_depth=2, vfov=c["vfov"], look_from=c["look_from"], look_at=c["look_at"],
                              vup=c["vup"], focal_length=c["focal_length"], defocus_angle=0.0, blur_strength=0.5, env_color=(0.0, 0.0, 0.0))
    return s


@pytest.mark.parametrize("case", ["two", "sphere", "quad", "instquad", "cuboid"])
def test_exact_estimator_matches_the_true_radiance(pt, ctx, case):
    """test_gpu_parity.py's MIS test with its acceptance, against the TRUE radiance: the two-light scene (whose mesh light the
    reference's rule gets wrong) and the sphere light (which it gets 18x wrong) as common.mis_scene builds them, and the quad, the tilted
    quad and the box as MESH lights. The box fails if only the first hit counts (the far faces are sampled too); the irregular meshes
    fail if sampler and pdf disagree about the area weighting."""
    spec = mis_scene(case) if case in ("two", "sphere") else mis_mesh_scene(case)
    gs, cam, _ = build(pt, ctx, spec)
    gs.set_light_sampling("exact")
    _, true = mis_expected(case)
    z, zg, mean = mis_zscores(lambda seed, a, b: gs.render(cam, seed, a, b)[0], true)
    gs.close()
    print(f"{case}: image mean / true {mean.mean() / true.mean():.4f}, zg {zg}, share |z| > 4 {(np.abs(z) > 4.0).mean():.4f}, std {z.std():.3f}")
    assert np.isfinite(z).all()
    assert np.abs(zg).max() < 4.0, zg
    assert (np.abs(z) > 4.0).mean() < 0.01 and 0.85 < z.std() < 1.3, (np.abs(z).max(), z.std())


# ---- 5. replay -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_replay_of_light_sampled_paths(pt, ctx, sampler):
    spec = mis_scene("two")
    spec.camera["image_width"] = 16
    gs, cam, _ = build(pt, ctx, spec)
    gs.set_light_sampling("exact")
    gs.set_sampler(sampler)
    fr = LR.mis_frame(16)
    H, W, seed, n_samples = fr["height"], 16, 9, 4
    per_sample = [gs.render(cam, seed, s, s + 1, slots_per_pixel=1)[0].reshape(-1, 3) for s in range(n_samples)]
    gs.close()
    bad, replayed, lit = [], 0, 0
    for p in range(H * W):
        for s in range(n_samples):
            want = LR.replay_two(fr, dict(width=W, blur_strength=0.5), seed, p, s, sobol=sampler == "sobol")
            if want is None:
                continue
            replayed += 1
            lit += bool(want.any())
            if not np.allclose(per_sample[s][p], want, rtol=1e-12, atol=0.0):
                bad.append((p, s, per_sample[s][p], want))
    print(f"{sampler}: {replayed} of {H * W * n_samples} (pixel, sample) pairs replayed, {lit} lit, {len(bad)} disagree")
    assert replayed >= 0.4 * H * W * n_samples and lit > 0.9 * replayed
    assert len(bad) <= 1, bad[:5]


# ---- 6. structure ------------------------------------------------------------------------------------------------------------------------
def lit_cornell(pt, ctx):
    """Scene 3 (quad light, instances) plus an emissive 320-triangle icosphere and a sphere light, each in the world and in the lights list."""
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 6)
    P, I = icosphere(2)
    P = (np.asarray(P, dtype=np.float64) * 45.0 + np.array([150.0, 330.0, 250.0])).astype(np.float32)
    ball = gs.mesh(1.0, P, I, None, None, gs.mat_light(gs.tex_solid_rgb(3.0, 5.0, 8.0)))
    bulb = gs.sphere(30.0, (420.0, 380.0, 300.0), (420.0, 380.0, 300.0), gs.mat_light(gs.tex_solid_rgb(9.0, 6.0, 3.0)))
    for o in (ball, bulb):
        gs.world_add_object(o)
        gs.world_add_light(o)
    gs.world_build()
    return gs, cam


def test_structure_with_exact_light_sampling(pt, ctx):
    gs, cam = lit_cornell(pt, ctx)
    seed, n = 7, 6
    base, st0 = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    aov0 = gs.render_aovs(cam, seed, 0, 4)
    gs.set_light_sampling("exact")
    full, st = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    assert not np.array_equal(full, base) and st.shade_variant == st0.shade_variant      # the new code does act here
    parts = np.zeros_like(full)
    for s in range(n):                                   # sample ranges add up, bit for bit
        gs.render(cam, seed, s, s + 1, accum=parts, slots_per_pixel=1)
    np.testing.assert_array_equal(parts, full)
    h, w = full.shape[:2]
    px = np.sort(np.random.default_rng(3).choice(h * w, 700, replace=False)).astype(np.uint32)
    sentinel = np.full_like(full, -3.25)
    lst, _ = gs.render_pixels(cam, seed, px, 0, n, accum=sentinel.copy(), slots_per_pixel=1, overwrite=True)
    mask = np.zeros(h * w, bool)
    mask[px] = True
    mask = mask.reshape(h, w)
    np.testing.assert_array_equal(lst[mask], full[mask])
    np.testing.assert_array_equal(lst[~mask], sentinel[~mask])
    fin = np.isfinite(full)
    dyn, _ = gs.render(cam, seed, 0, n)
    np.testing.assert_allclose(dyn[fin], full[fin], rtol=1e-12, atol=1e-12)
    dlst, _ = gs.render_pixels(cam, seed, px, 0, n)
    np.testing.assert_allclose(dlst[mask & fin.all(axis=2)], full[mask & fin.all(axis=2)], rtol=1e-12, atol=1e-12)
    comm = pt.Comm(ctx, 0, 1)
    multi, _ = gs.render_multi(cam, seed, n, comm, slots_per_pixel=1)
    comm.close()
    np.testing.assert_array_equal(multi, full)
    ada, counts, ast = gs.render_adaptive(cam, seed, 2, n, 0.0, slots_per_pixel=1)
    assert (counts == n).all() and ast.samples == counts.sum()
    np.testing.assert_allclose(ada[fin], full[fin], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(gs.render_aovs(cam, seed, 0, 4), aov0)      # AOVs are unchanged by the kind
    gs.set_sampler("sobol")                              # the Sobol forms: the same identities
    qfull, _ = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    assert not np.array_equal(qfull, full)
    qparts = np.zeros_like(qfull)
    for s in range(n):
        gs.render(cam, seed, s, s + 1, accum=qparts, slots_per_pixel=1)
    np.testing.assert_array_equal(qparts, qfull)
    qdyn, _ = gs.render(cam, seed, 0, n)
    qfin = np.isfinite(qfull)
    np.testing.assert_allclose(qdyn[qfin], qfull[qfin], rtol=1e-12, atol=1e-12)
    qlst, _ = gs.render_pixels(cam, seed, px, 0, n, accum=sentinel.copy(), slots_per_pixel=1, overwrite=True)
    np.testing.assert_array_equal(qlst[mask], qfull[mask])
    gs.close()


def test_full_hd_over_8192_slot_windows(pt, ctx):
    """1920 x 1080, 8 spp of the quad-as-mesh scene with the 8192-slot windows — the shape whose LDS holds the walk's stack next to the
    largest sort — against the 4096-slot render of the same frame."""
    spec = mis_mesh_scene("quad")
    spec.camera.update(image_width=1920, aspect_ratio=16.0 / 9.0)
    gs, cam, _ = build(pt, ctx, spec)
    gs.set_light_sampling("exact")
    wide, st = _with_env({"PT_EXPERIMENT": "1", "PT_WIDE_WINDOW_MIN": "1"}, lambda: gs.render(cam, 4, 0, 8))
    narrow, st22 = _with_env({"PT_EXPERIMENT": "1", "PT_SHADE_VARIANT": "22"}, lambda: gs.render(cam, 4, 0, 8))
    gs.close()
    print(f"full HD: {st.samples} samples, {st.segments / st.samples:.2f} segments per sample, first launch over {window_slots(st, 1)}-slot windows")
    assert wide.shape[:2] == (1080, 1920) and st.shade_variant == 42 and window_slots(st, 1) == 8192 and st22.shade_variant == 22
    fin = np.isfinite(wide) & np.isfinite(narrow)
    assert fin.mean() > 0.999 and wide[fin].sum() > 0.0
    np.testing.assert_allclose(wide[fin], narrow[fin], rtol=1e-11, atol=0.0)


# ---- 7. refusals and the CLI ----------------------------------------------------------------------------------------------------------
def test_env_sampling_with_exact_light_sampling_is_refused(pt, ctx):
    gs = pt.Scene(ctx)
    gs.set_float_hdr(True)
    cam = gs.build_scene(6, 32, 2)
    gs.set_env_sampling(0.5)
    gs.set_light_sampling("exact")
    gs.render(cam, 1, 0, 1)                                  # no mesh or sphere light: kind 1 is not in effect
    gs.world_add_light(gs.sphere(0.3, (0.0, 3.0, 0.0), (0.0, 3.0, 0.0), gs.mat_light(gs.tex_solid_rgb(5.0, 5.0, 5.0))))
    gs.world_build()
    with pytest.raises(pt.PtError, match="light sampling"):
        gs.render(cam, 1, 0, 1)
    with pytest.raises(pt.PtError, match="light sampling"):
        gs.render_pixels(cam, 1, np.array([1, 5], dtype=np.uint32), 0, 1)
    gs.set_light_sampling("reference")
    gs.render(cam, 1, 0, 1)
    gs.close()


def test_media_with_exact_light_sampling_are_refused(pt, ctx):
    gs, cam, _ = build(pt, ctx, mis_scene("sphere"))
    gs.set_light_sampling("exact")
    gs.render(cam, 1, 0, 1)
    fog = gs.mat_medium(0.2, (0.9, 0.9, 0.9), 0.0)
    gs.world_add_object(gs.cuboid((-3.0, 0.01, -3.0), (3.0, 3.0, 3.0), fog))
    gs.world_build()
    with pytest.raises(pt.PtError, match="light sampling"):
        gs.render(cam, 1, 0, 1)
    with pytest.raises(pt.PtError, match="light sampling"):
        gs.render_adaptive(cam, 1, 2, 4, 0.0)
    gs.set_light_sampling("reference")
    gs.render(cam, 1, 0, 1)
    gs.close()


def test_zero_area_light_mesh_is_refused(pt, ctx):
    spec = SceneSpec()
    floor = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.5, 0.5, 0.5), -1)
    spec.add("world_add_object", spec.add("quad", (-4.0, 0.0, -4.0), (0.0, 0.0, 8.0), (8.0, 0.0, 0.0), floor))
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", 2.0, 2.0, 2.0))
    line = np.array([(0.0, 2.0, 0.0), (0.5, 2.0, 0.0), (1.0, 2.0, 0.0)], dtype=np.float32)     # three points of one line
    spec.add("world_add_light", spec.add("mesh", 1.0, line, np.array([0, 1, 2], dtype=np.uint32), None, None, lm))
    spec.add("world_build")
    spec.camera = default_camera(width=16, spp=1, max_depth=2)
    gs, cam, _ = build(pt, ctx, spec)
    gs.render(cam, 1, 0, 1)                                  # kind 0 renders as it always did
    gs.set_light_sampling("exact")
    with pytest.raises(pt.PtError, match="area"):
        gs.render(cam, 1, 0, 1)
    with pytest.raises(pt.PtError, match="area"):
        gs.light_probe(0, np.zeros((1, 4)))
    gs.close()


def test_cli_mesh_light(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = ["-s", "3", "--width", "64", "--spp", "8", "--assets", pt.ASSET_DIR]

    def run(name, *extra):
        out = tmp_path / name
        r = subprocess.run([exe] + common + list(extra) + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return pt.decode_image_rgb8(str(out)).astype(np.float64)

    plain = run("plain.png")
    same = run("same.png", "--light-sampling", "exact")                   # quad lights only: not in effect
    lit = run("lit.png", "--mesh-light", "278,278,278,60,4,7,12")
    ref = run("ref.png", "--mesh-light", "278,278,278,60,4,7,12", "--light-sampling", "reference")
    d_lit, d_ref = np.abs(lit - plain).mean(), np.abs(ref - lit).mean()
    print(f"--mesh-light: mean |difference| against the plain render {d_lit:.2f}; exact against reference sampling of the same light {d_ref:.2f}")
    np.testing.assert_array_equal(same, plain)
    assert d_lit > 2.0 and d_ref > 0.0
    for extra in (["--env-sampling", "0.5"], ["--fog", "0.1"], ["--smoke", "0.1"], ["--interior", "2"]):
        r = subprocess.run([exe] + common + ["--mesh-light", "278,278,278,60"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--mesh-light" in r.stderr, r.stderr
    for bad in (["--mesh-light", "1,2,3"], ["--mesh-light", "1,2,3,-1"], ["--light-sampling", "best"]):
        r = subprocess.run([exe] + common + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, r.stderr
