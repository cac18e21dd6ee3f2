"""The short-path pass's deferred miss proofs. A bounce ray that enters a mesh's box no longer walks the mesh's BVH on the
spot, a few lanes of its wave at a time: it waits in a ring of 64 records per wave, and a pass walks all waiting records at once, one per lane.
Which records share a pass may not change anything: a sample's outcome depends on (tile, pixel, sample, budgets) alone. So every count of
the pass equals the count of the form that walks on the spot (PT_SHORT_DEFER=0), the frame is that form's and the wavefront's
(PT_SHORT_PASS=0) to 1e-12 relative — the bound for reordered f64 atomic adds of tests/test_short_pass_gpu.py —, and one-sample slices,
which add one value per pixel, equal the wavefront's bit for bit."""
import numpy as np
import pytest

from common import SceneSpec, _with_env, default_camera, icosphere
from test_sky_pass_gpu import _same_bits, _script_scene
from test_short_pilot_gpu import ANY_RANGE, LONG, NO_PILOT, OFF, X, _counts_equal

gpu = pytest.mark.gpu                                                     # (every test but the scene's premise, which is numpy alone)

INLINE = dict(X, PT_SHORT_DEFER="0")
COUNTS = ("samples", "segments", "short_samples", "hard_samples", "short_pixels", "pilot_tiles", "short_fallback")


def _same_counts(st, st0):
    assert all(getattr(st, f) == getattr(st0, f) for f in COUNTS), [(f, getattr(st, f), getattr(st0, f)) for f in COUNTS]


@gpu
@pytest.mark.parametrize("pilot", [True, False])
@pytest.mark.parametrize("width", [64, 68])
def test_deferral_against_the_inline_form(pt, ctx, width, pilot):
    base = X if pilot else NO_PILOT
    gs, cam = _script_scene(pt, ctx, 6, width)
    on, st = _with_env(base, lambda: gs.render(cam, 1, 0, LONG))
    inl, st_i = _with_env(dict(base, PT_SHORT_DEFER="0"), lambda: gs.render(cam, 1, 0, LONG))
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 1, 0, LONG))
    print(f"scene 6 {width}x36 @ {LONG}, pilot {pilot}: finished {st.short_samples}, hard {st.hard_samples}, walked {st.short_walks} in {st.short_walk_passes} passes")
    _same_counts(st, st_i)
    assert (st.pilot_tiles > 0) == pilot and st_i.short_walks == 0 and st_i.short_walk_passes == 0
    assert st.short_walks > 0 and 0 < st.short_walk_passes <= st.short_walks <= 64 * st.short_walk_passes
    np.testing.assert_allclose(on, inl, rtol=1e-12, atol=0.0)
    for s in (st, st_i):
        _counts_equal(s, st0, width * 36, LONG)
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(inl, off, rtol=1e-12, atol=0.0)
    gs.close()


# ---- a scene whose bounces nearly all wait: two wide, empty meshes over a floor, and a small solid one ----
ROOF_Y = 8.0
CORNERS_A = [(-40.0, ROOF_Y, -40.0), (40.0, ROOF_Y + 0.6, 40.0)]          # the first mesh's two clusters: its root box spans the sky over the floor
CORNERS_B = [(-40.0, ROOF_Y + 0.9, 40.0), (40.0, ROOF_Y + 0.3, -40.0)]    # the second one's, on the other diagonal: its box overlaps the first's
CAM_FROM, CAM_AT = (0.0, 3.0, -6.0), (0.0, 0.0, 0.0)


def _clusters(corners, n=8):
    """Two clusters of `n` small triangles (more than the builder's leaves hold, 4: the mesh's root is a node) at `corners`."""
    P, I = [], []
    for c in corners:
        for k in range(n):
            base = np.array(c) + np.array([0.05 * k, 0.0, 0.03 * k])
            I.append([len(P), len(P) + 1, len(P) + 2])
            P += [base, base + np.array([0.04, 0.0, 0.0]), base + np.array([0.0, 0.02, 0.04])]
    return np.array(P, dtype=np.float32), np.array(I, dtype=np.uint32)


def _ring_scene():
    s = SceneSpec()
    floor = s.add("mat_diffuse", s.add("tex_checker", 0.8, s.add("tex_solid_rgb", 0.2, 0.3, 0.1), s.add("tex_solid_rgb", 0.9, 0.9, 0.9)), -1)
    red = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.8, 0.2, 0.2), -1)
    s.add("world_add_object", s.add("quad", (-60.0, 0.0, -60.0), (0.0, 0.0, 120.0), (120.0, 0.0, 0.0), floor))
    for corners in (CORNERS_A, CORNERS_B):
        P, I = _clusters(corners)
        s.add("world_add_object", s.add("instance", s.add("mesh", 1.0, P, I, None, None, red), (0.0, 1.0, 0.0), 0.0, (0.0, 0.0, 0.0)))
    P, I = icosphere(2)
    s.add("world_add_object", s.add("instance", s.add("mesh", 0.5, P, I, None, None, red), (0.0, 1.0, 0.0), 0.4, (0.5, 0.8, 1.0)))
    s.add("world_build")
    s.camera = default_camera(width=64, aspect=64 / 40.5, spp=LONG, look_from=CAM_FROM, look_at=CAM_AT, env_color=(0.5, 0.5, 0.5))
    return s


def test_most_bounces_enter_the_first_root_box():
    """The scene's premise, on the CPU: of the cosine-weighted bounces from the floor points the camera's pixel centres see under the first
    mesh, more than half enter its root box (a slab of 0.6 over the whole floor, 8 above it)."""
    rng = np.random.default_rng(3)
    f, a = np.array(CAM_FROM), np.array(CAM_AT)
    w = (f - a) / np.linalg.norm(f - a)
    u = np.cross([0.0, 1.0, 0.0], w); u /= np.linalg.norm(u)
    v = np.cross(w, u)
    h = np.tan(np.radians(50.0) / 2)
    ys, xs = np.meshgrid((np.arange(40) + 0.5) / 40, (np.arange(64) + 0.5) / 64, indexing="ij")
    d = -w[None, None] + (2 * xs[..., None] - 1) * h * (64 / 40) * u[None, None] + (1 - 2 * ys[..., None]) * h * v[None, None]
    t = -f[1] / d[..., 1]
    p = (f + t[..., None] * d)[(d[..., 1] < 0)]
    p = p[(np.abs(p[:, 0]) < 40) & (np.abs(p[:, 2]) < 40)]
    assert len(p) > 0.8 * 64 * 40                                         # (nearly every pixel sees the floor under the mesh)
    p = np.repeat(p, 16, axis=0)
    r1, r2 = rng.random(len(p)), rng.random(len(p))
    dirs = np.stack([np.cos(2 * np.pi * r1) * np.sqrt(r2), np.sqrt(1 - r2), np.sin(2 * np.pi * r1) * np.sqrt(r2)], axis=1)
    lo, hi = np.array([-40.0, ROOF_Y, -40.0]), np.array([40.4, ROOF_Y + 0.62, 40.4])
    with np.errstate(divide="ignore"):
        t0, t1 = (lo - p) / dirs, (hi - p) / dirs
    enter = np.minimum(t0, t1).max(axis=1) <= np.maximum(t0, t1).min(axis=1)
    print(f"{enter.mean():.3f} of {len(p)} bounces enter the root box")
    assert enter.mean() > 0.5


@pytest.fixture(scope="module")
def ring(pt, ctx):
    """Test 2's scene and its renders at 256 spp, shared: the default, the form that walks on the spot and the wavefront alone."""
    spec, gs = _ring_scene(), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    assert pt.image_height(cam) == 40
    r = {"gs": gs, "cam": cam}
    r["on"], r["st"] = gs.render(cam, 2, 0, LONG)
    r["inl"], r["st_i"] = _with_env(INLINE, lambda: gs.render(cam, 2, 0, LONG))
    r["off"], r["st0"] = _with_env(OFF, lambda: gs.render(cam, 2, 0, LONG))
    yield r
    gs.close()


@gpu
def test_the_ring_turns_over(ring):
    st, st_i, st0, gs, cam = ring["st"], ring["st_i"], ring["st0"], ring["gs"], ring["cam"]
    _, no_stack = _with_env(dict(X, PT_PILOT_STACK="0"), lambda: gs.render(cam, 2, 0, LONG))
    waves = st.short_tiles * (LONG // 32)                                # (chunks of 32 samples: 40 tiles or fewer on a device of 3 CUs or more)
    fill = st.short_walks / (64 * max(1, st.short_walk_passes))
    print(f"short tiles {st.short_tiles} (by yield {st.pilot_tiles}), finished {st.short_samples}, hard {st.hard_samples}; walked {st.short_walks} in "
          f"{st.short_walk_passes} passes of {waves} waves, mean fill {fill:.3f}; finished with a stack budget of 0: {no_stack.short_samples}")
    assert st.short_tiles > 0 and st.short_walk_passes >= 2 * waves
    assert fill >= 0.5
    _same_counts(st, st_i)
    for s in (st, st_i):
        _counts_equal(s, st0, 64 * 40, LONG)
    np.testing.assert_allclose(ring["on"], ring["inl"], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(ring["on"], ring["off"], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(ring["inl"], ring["off"], rtol=1e-12, atol=0.0)
    assert st.short_samples > no_stack.short_samples and st.hard_samples > 0


@gpu
@pytest.mark.parametrize("stack", ["0", "2"])
def test_budgets(ring, stack):
    gs, cam = ring["gs"], ring["cam"]
    env = dict(X, PT_PILOT_STACK=stack)
    on, st = _with_env(env, lambda: gs.render(cam, 2, 0, LONG))
    inl, st_i = _with_env(dict(env, PT_SHORT_DEFER="0"), lambda: gs.render(cam, 2, 0, LONG))
    print(f"stack {stack}: finished {st.short_samples}, hard {st.hard_samples}, walked {st.short_walks}")
    _same_counts(st, st_i)
    assert st.short_walks > 0
    np.testing.assert_allclose(on, inl, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(on, ring["off"], rtol=1e-12, atol=0.0)


@gpu
def test_one_sample_slices_are_the_wavefronts_bit_for_bit(ring):
    gs, cam = ring["gs"], ring["cam"]
    walked = 0
    for i in range(8):
        on, st = _with_env(ANY_RANGE, lambda: gs.render(cam, 3, i, i + 1))
        off, _ = _with_env(OFF, lambda: gs.render(cam, 3, i, i + 1))
        walked += st.short_walks
        assert st.short_tiles > 0 and _same_bits(on, off), i
    assert walked > 0


@gpu
def test_ranges(ring):
    gs, cam = ring["gs"], ring["cam"]
    whole, st_w = gs.render(cam, 7, 0, 600)
    parts, st_a = gs.render(cam, 7, 0, 300)
    parts, st_b = gs.render(cam, 7, 300, 600, accum=parts)
    assert st_a.samples + st_b.samples == st_w.samples and st_a.segments + st_b.segments == st_w.segments
    assert st_w.short_walks > 0 and st_a.short_walks > 0 and st_b.short_walks > 0
    np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0.0)
    # (each range's pilot sees other samples and may take other tiles; over the proven tiles alone every count of the pass adds up as well)
    _, np_w = _with_env(NO_PILOT, lambda: gs.render(cam, 7, 0, 600))
    _, np_a = _with_env(NO_PILOT, lambda: gs.render(cam, 7, 0, 300))
    _, np_b = _with_env(NO_PILOT, lambda: gs.render(cam, 7, 300, 600))
    for f in ("samples", "segments", "short_samples", "hard_samples", "short_walks"):
        assert getattr(np_a, f) + getattr(np_b, f) == getattr(np_w, f), f
    # a range shorter than PILOT_MIN: the pilot does not run, the proven tiles' bounces wait all the same
    short, st = gs.render(cam, 7, 0, 16)
    inl, st_i = _with_env(INLINE, lambda: gs.render(cam, 7, 0, 16))
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 7, 0, 16))
    _same_counts(st, st_i)
    _counts_equal(st, st0, 64 * 40, 16)
    assert st.pilot_tiles == 0 and st.short_walks > 0
    np.testing.assert_allclose(short, inl, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(short, off, rtol=1e-12, atol=0.0)
