"""Cached device buffers on a REUSED scene. A scene keeps its path pool, tiled accumulator, compaction scratch, pixel list and
environment tables between calls and only ever grows them; every other test renders once or twice per scene, so a buffer that is
carved from its cached capacity instead of from the call's own size, or a stale size after a regrow, would pass them all. Here one
scene goes through a sequence that grows and then under-uses every cached buffer, with probes and refused calls in between, and every
result is compared with the same call on a freshly built scene: bit for bit where the sample order is fixed (slots_per_pixel = 1, the
probes), and at the project's bound for dynamic-order f64 sums (rtol = atol = 1e-11 on finite pixels, counts exact) where it is not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 5
# (scene, width, spp) of the dynamic step: test_gpu_parity.py::test_end_of_frame_pool_compaction_changes_no_result's frames, which
# compact. Scene 3: Cornell box, batch K2, lights list. Scene 6: meshes, two-phase K2.
CASES = ((3, 160, 24), (6, 192, 20))


def _resized(pt, cam, width):
    c = pt.Camera.from_buffer_copy(cam)
    c.image_width = width
    return c


def _fresh(pt, ctx, sid, call):
    """`call(scene, camera)` on a scene nothing has rendered on yet."""
    gs = pt.Scene(ctx)
    try:
        return call(gs, gs.build_scene(sid, 16, 4))
    finally:
        gs.close()


def _same(got, want):
    (acc, st), (ref, st_ref) = got, want
    assert (st.samples, st.segments) == (st_ref.samples, st_ref.segments)
    np.testing.assert_array_equal(acc, ref)


@pytest.mark.parametrize("sid,dyn_width,dyn_spp", CASES)
def test_reused_scene_equals_fresh_scenes(pt, ctx, sid, dyn_width, dyn_spp):
    rng = np.random.default_rng(20241)
    gs = pt.Scene(ctx)                      # the reused scene
    cam = gs.build_scene(sid, 16, 4)
    solid = gs.tex_solid_rgb(0.5, 0.5, 0.5)   # (step 6's texture; a new texture asks for a rebuild)
    gs.world_build()
    list_cam = _resized(pt, cam, dyn_width)
    long_list = np.sort(rng.choice(dyn_width * pt.image_height(list_cam), size=1500, replace=False)).astype(np.uint32)
    short_list = long_list[:100]
    # the probes (step 7): 1 ray and 5000 rays from the camera, 1 and 5000 divisions (pt_math_probe 1 is the correctly rounded divide)
    d = rng.normal(size=(5000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.broadcast_to(np.array(cam.look_from[:]), d.shape), d, rng.uniform(0.0, 1.0, (5000, 1))], axis=1)
    ab = np.stack([rng.uniform(-1e3, 1e3, 5000), rng.uniform(0.5, 1e3, 5000)], axis=1)

    small = lambda s, c: s.render(_resized(pt, c, 16), SEED, 0, 4, slots_per_pixel=1)
    large = lambda s, c: s.render(_resized(pt, c, 48), SEED, 0, 4, slots_per_pixel=1)
    dynamic = lambda s, c: s.render(_resized(pt, c, dyn_width), SEED, 0, dyn_spp)
    pixels = lambda px: (lambda s, c: s.render_pixels(_resized(pt, c, dyn_width), SEED, px, 0, 4, slots_per_pixel=1))
    want_small, want_large, want_dyn, want_short, want_long = (_fresh(pt, ctx, sid, f) for f in (small, large, dynamic, pixels(short_list), pixels(long_list)))
    assert want_dyn[1].compactions >= 1, "precondition: the dynamic frame compacts (tiled accumulator, ordered area, scratch)"
    want_hits1, want_hits = _fresh(pt, ctx, sid, lambda s, c: (s.intersect(rays[:1]), s.intersect(rays)))
    want_div1, want_div = ctx.math_probe(1, ab[:1]), ctx.math_probe(1, ab)
    np.testing.assert_array_equal(want_div, ab[:, 0] / ab[:, 1])

    def probes(s):
        np.testing.assert_array_equal(s.intersect(rays[:1]), want_hits1)
        np.testing.assert_array_equal(ctx.math_probe(1, ab[:1]), want_div1)
        np.testing.assert_array_equal(s.intersect(rays), want_hits)
        np.testing.assert_array_equal(ctx.math_probe(1, ab), want_div)

    _same(small(gs, cam), want_small)       # 1
    probes(gs)
    _same(large(gs, cam), want_large)       # 2: the pool grows
    probes(gs)
    _same(small(gs, cam), want_small)       # 3: the pool is larger than needed: the layout must come from this call
    probes(gs)
    dyn, st = dynamic(gs, cam)              # 4: tiled accumulator, ordered output area, compaction scratch
    ref, st_ref = want_dyn
    assert (st.samples, st.segments) == (st_ref.samples, st_ref.segments)
    fin = np.isfinite(ref)
    np.testing.assert_allclose(dyn[fin], ref[fin], rtol=1e-11, atol=1e-11)
    probes(gs)
    _same(pixels(short_list)(gs, cam), want_short)   # 5: the list buffer, grown, then under-used
    _same(pixels(long_list)(gs, cam), want_long)
    probes(gs)
    _same(pixels(short_list)(gs, cam), want_short)
    with pytest.raises(pt.PtError, match="spp_end < spp_begin"):   # 6: refused calls leave the scene as it was
        gs.render(_resized(pt, cam, 16), SEED, 4, 0, slots_per_pixel=1)
    mapped = _resized(pt, cam, 16)
    mapped.env_is_map, mapped.env_tex = 1, solid
    with pytest.raises(pt.PtError, match="env_tex must be an image texture"):
        gs.render(mapped, SEED, 0, 4, slots_per_pixel=1)
    probes(gs)
    _same(small(gs, cam), want_small)
    gs.close()                              # 8: teardown with every buffer kind live


def test_refused_build_then_corrected_equals_a_fresh_scene(pt, ctx):
    """A build refused half-way — the light grid's table over 2^25 entries: after the placements and the derived flags, before the top
    level and any upload — leaves a scene that, rebuilt with the setting corrected, renders what a fresh scene with that setting does."""
    import test_light_grid_gpu as LG

    lights = LG.many_points(129)            # 64^3 cells x 129 lights: just over 2^25
    quads = [LG.FLOOR, LG.OCCLUDER, LG.CEILING]
    fresh, cam, _ = LG.grid_scene(pt, ctx, quads, lights, dims=(4, 4, 4))
    cam = _resized(pt, cam, 32)             # (aspect 1: 32 x 32)
    assert pt.image_height(cam) == 32
    want = fresh.render(cam, SEED, 0, 4, slots_per_pixel=1)
    fresh.close()
    gs, _, _ = LG.TP.make_scene(pt, ctx, quads, lights)   # built once, uniform selection
    gs.set_punctual_selection("grid")
    gs.set_punctual_grid(64, 64, 64)
    with pytest.raises(pt.PtError, match="2\\^25"):
        gs.world_build()
    with pytest.raises(pt.PtError):
        gs.render(cam, SEED, 0, 4, slots_per_pixel=1)     # (a refused build leaves the world unbuilt)
    gs.set_punctual_grid(4, 4, 4)
    gs.world_build()
    assert gs.punctual_grid()[0] == (4, 4, 4)
    _same(gs.render(cam, SEED, 0, 4, slots_per_pixel=1), want)
    gs.close()
