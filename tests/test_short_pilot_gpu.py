"""The short-path pass's yield pilot, miss proof and projected hard list. On a sample range of PILOT_MIN = 256 samples per
pixel or more the pass first counts, over 8 samples of every tile of the wavefront's, how many samples k_short would finish, and takes the
tiles whose yield reaches the threshold besides the proven ones; inside k_short a ray that enters a mesh's box is finished all the same
when a box-only walk of the mesh's BVH proves that it misses; and the hard list holds the taken tiles' projected hard samples with a margin,
with a second run over the proven tiles alone when that is not enough. None of this may change a frame: the yardstick is the wavefront
alone (PT_SHORT_PASS=0) — equal sample and segment counts, sums to 1e-12 relative (the bound for reordered f64 atomic adds of
tests/test_short_pass_gpu.py) — and, sample by sample, the oracle."""
import numpy as np
import pytest

from common import SceneSpec, _with_env, default_camera, icosphere
from test_sky_pass_gpu import SPP, _clipped_pixels, _entry_boxes, _same_bits, _script_scene
from test_short_pass_gpu import _scene6_tiles

pytestmark = pytest.mark.gpu

X = {"PT_EXPERIMENT": "1"}
OFF = dict(X, PT_SHORT_PASS="0")
NO_PILOT = dict(X, PT_SHORT_PILOT="0")
ANY_RANGE = dict(X, PT_PILOT_ANY_RANGE="1")
LONG = 256                                                               # PILOT_MIN: the shortest range the pilot runs on by itself


def _counts_equal(st, st0, n_pixels, spp):
    assert st.samples == st0.samples == n_pixels * spp and st.segments == st0.segments


@pytest.mark.parametrize("width", [64, 68])
def test_frame_equals_the_wavefront_alone(pt, ctx, width):
    gs, cam = _script_scene(pt, ctx, 6, width)
    tiles = _scene6_tiles(pt, gs, cam)
    n_proven, proven_pixels = int((tiles == 2).sum()), _clipped_pixels(tiles == 2, width, 36)
    on, st = gs.render(cam, 1, 0, LONG)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 1, 0, LONG))
    print(f"scene 6 {width}x36 @ {LONG}: proven {n_proven} of {tiles.size} tiles, taken by yield {st.pilot_tiles}, short pixels {st.short_pixels}, "
          f"finished {st.short_samples}, hard {st.hard_samples}, list bytes {st.short_list_bytes}, fallback {st.short_fallback}, "
          f"max rel diff {np.max(np.abs(on - off) / np.maximum(np.abs(off), 1e-300))}")
    _counts_equal(st, st0, width * 36, LONG)
    assert st0.short_tiles == 0 and st0.pilot_tiles == 0 and st.sky_tiles == st0.sky_tiles == (tiles == 1).sum()
    assert st.short_fallback == 0 and st.pilot_tiles > 0 and st.short_tiles == n_proven + st.pilot_tiles > n_proven > 0
    # the taken tiles' pixels: every proven tile's, and between a ragged corner tile's (4 x 4 at 68 x 36) and 64 of each tile taken by yield
    assert proven_pixels + 16 * st.pilot_tiles <= st.short_pixels <= proven_pixels + 64 * st.pilot_tiles
    assert st.short_samples + st.hard_samples == st.short_pixels * LONG and st.hard_samples > 0
    assert st.short_list_bytes < st.short_pixels * LONG * 4           # (less than the worst case)
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_every_sample_of_the_frame_is_the_oracles(pt, ctx, det):
    """Sixteen one-sample slices at 68x36 with the pilot forced on, every pixel of the frame — so every pixel of every tile taken, whichever
    they are in a slice — against the oracle's trace_sample, bit for bit. That rays which enter a mesh's box are among the samples the pass
    finishes is shown over the proven tiles, which are the same tiles with and without the walk: with the walk's stack budget at 0 (it then
    proves only what needs no stack) the pass finishes fewer samples than with the whole budget."""
    W = 68
    gs, cam = _script_scene(pt, ctx, 6, W)
    os_ = det.Scene()
    ocam = os_.build_scene(6, W, SPP)
    ocam.aspect_ratio = cam.aspect_ratio
    n_proven = int((_scene6_tiles(pt, gs, cam) == 2).sum())
    finished = hard = taken = 0
    for i in range(SPP):
        acc, st = _with_env(ANY_RANGE, lambda: gs.render(cam, 3, i, i + 1))
        assert st.short_fallback == 0 and st.short_tiles == n_proven + st.pilot_tiles
        finished, hard, taken = finished + st.short_samples, hard + st.hard_samples, taken + st.pilot_tiles
        for p in range(36 * W):
            rad, _, nseg = os_.trace_sample(ocam, 3, p, i, 4)
            assert _same_bits(np.ascontiguousarray(acc[p // W, p % W]), rad), (i, p // W, p % W, nseg)
    _, with_walk = _with_env(NO_PILOT, lambda: gs.render(cam, 3, 0, SPP))
    _, no_stack = _with_env(dict(NO_PILOT, PT_PILOT_STACK="0"), lambda: gs.render(cam, 3, 0, SPP))
    print(f"16 slices: tiles taken by yield {taken}, finished {finished}, hard {hard}; proven tiles @ {SPP}: finished {with_walk.short_samples} "
          f"with the walk, {no_stack.short_samples} with a stack budget of 0")
    assert taken > 0 and finished > 0 and hard > 0
    assert with_walk.short_tiles == no_stack.short_tiles == n_proven and with_walk.short_samples > no_stack.short_samples
    os_.close(); gs.close()


def _mesh_scene(moving=False):
    """A diffuse floor under a grey environment, one small mesh above it under an instance (`moving`: a moving one) — two pixels across, so
    the tiles that look into its box finish nearly every sample — and a metal sphere to the side, whose tiles finish few."""
    s = SceneSpec()
    grey = s.add("mat_diffuse", s.add("tex_checker", 0.8, s.add("tex_solid_rgb", 0.2, 0.3, 0.1), s.add("tex_solid_rgb", 0.9, 0.9, 0.9)), -1)
    red = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.8, 0.2, 0.2), -1)
    s.add("world_add_object", s.add("quad", (-30.0, 0.0, -30.0), (0.0, 0.0, 60.0), (60.0, 0.0, 0.0), grey))
    P, I = icosphere(2)
    metal = s.add("mat_metal", s.add("tex_solid_rgb", 0.9, 0.8, 0.6), s.add("tex_solid_f", 0.1))
    mesh = s.add("mesh", 0.12, P, I, None, None, red)
    if moving:
        s.add("world_add_object", s.add("instance_moving", mesh, (0.0, 1.0, 0.0), 0.4, 0.4, (0.0, 1.6, 0.0), (0.0, 1.6, 0.3)))
    else:
        s.add("world_add_object", s.add("instance", mesh, (0.0, 1.0, 0.0), 0.4, (0.0, 1.6, 0.0)))
    s.add("world_add_object", s.add("sphere", 0.7, (2.2, 0.7, 0.0), (2.2, 0.7, 0.0), metal))
    s.add("world_build")
    s.camera = default_camera(width=64, aspect=64 / 40.5, spp=LONG, look_from=(0.0, 1.2, -6.0), look_at=(0.0, 1.0, 0.0), env_color=(0.5, 0.5, 0.5))
    return s


def test_host_api_scene_with_a_mesh(pt, ctx):
    spec, gs = _mesh_scene(), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    assert pt.image_height(cam) == 40
    boxes = _entry_boxes(pt, gs)                                         # the floor, the mesh, the sphere
    tiles = pt.short_tiles(cam, boxes, [1, 0, 0])
    n_wave = int((tiles == 0).sum())
    n_mesh = int((pt.short_tiles(cam, boxes, [1, 0, 1]) == 0).sum())    # the tiles around the mesh: a camera ray of theirs can enter its box
    on, st = gs.render(cam, 2, 0, LONG)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 2, 0, LONG))
    print(f"tiles: sky {(tiles == 1).sum()}, proven {(tiles == 2).sum()}, the wavefront's {n_wave}, around the mesh {n_mesh}; taken by yield {st.pilot_tiles}, finished {st.short_samples}, "
          f"hard {st.hard_samples}")
    assert 0 < n_mesh <= st.pilot_tiles < n_wave and st.short_tiles == (tiles == 2).sum() + st.pilot_tiles and st.short_fallback == 0
    assert st.short_samples + st.hard_samples == st.short_pixels * LONG
    _counts_equal(st, st0, 64 * 40, LONG)
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()
    # the same mesh under a moving instance: nothing the pass or its walk may take
    spec, gs = _mesh_scene(moving=True), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    on, st = gs.render(cam, 2, 0, LONG)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 2, 0, LONG))
    assert st.short_tiles == 0 and st.pilot_tiles == 0 and st.short_samples == 0 and st.hard_samples == 0
    _counts_equal(st, st0, 64 * 40, LONG)
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_a_stack_budget_of_two_makes_more_samples_hard(pt, ctx):
    gs, cam = _script_scene(pt, ctx, 6, 64)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 4, 0, LONG))
    # over the proven tiles, which do not depend on the walk: the smaller budget proves fewer misses
    _, whole = _with_env(NO_PILOT, lambda: gs.render(cam, 4, 0, LONG))
    _, two = _with_env(dict(NO_PILOT, PT_PILOT_STACK="2"), lambda: gs.render(cam, 4, 0, LONG))
    assert whole.short_tiles == two.short_tiles > 0 and two.hard_samples > whole.hard_samples
    assert two.short_samples + two.hard_samples == whole.short_samples + whole.hard_samples
    # and with the pilot on the frame is the wavefront's
    on, st = _with_env(dict(X, PT_PILOT_STACK="2"), lambda: gs.render(cam, 4, 0, LONG))
    print(f"stack 2: taken by yield {st.pilot_tiles}; proven tiles: hard {two.hard_samples} against {whole.hard_samples} with the whole budget")
    assert st.pilot_tiles > 0 and st.short_samples + st.hard_samples == st.short_pixels * LONG
    _counts_equal(st, st0, 64 * 36, LONG)
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_a_list_too_small_falls_back_to_the_proven_tiles(pt, ctx):
    gs, cam = _script_scene(pt, ctx, 6, 64)
    tiles = _scene6_tiles(pt, gs, cam)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 6, 0, LONG))
    _, ok = gs.render(cam, 6, 0, LONG)
    on, st = _with_env(dict(X, PT_PILOT_MARGIN="0.05"), lambda: gs.render(cam, 6, 0, LONG))
    _, st_np = _with_env(NO_PILOT, lambda: gs.render(cam, 6, 0, LONG))
    print(f"margin 0.05: fallback {st.short_fallback}, tiles {st.short_tiles} (by yield {st.pilot_tiles}); default: fallback {ok.short_fallback}, by yield {ok.pilot_tiles}, "
          f"hard {ok.hard_samples}")
    assert ok.short_fallback == 0 and ok.pilot_tiles > 0 and ok.hard_samples > 0
    assert st.short_fallback == 1 and st.pilot_tiles == 0 and st.short_tiles == (tiles == 2).sum()
    assert (st.short_samples, st.hard_samples, st.short_pixels) == (st_np.short_samples, st_np.hard_samples, st_np.short_pixels)
    _counts_equal(st, st0, 64 * 36, LONG)
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_ranges_and_reuse(pt, ctx):
    gs, cam = _script_scene(pt, ctx, 6, 64)
    fields = ("pilot_tiles", "short_fallback", "short_list_bytes", "short_pixels", "short_tiles", "short_samples", "hard_samples", "sky_tiles", "sky_samples",
              "samples", "segments")
    # a range shorter than PILOT_MIN: the pilot does not run
    _, st = gs.render(cam, 7, 0, SPP)
    _, st_np = _with_env(NO_PILOT, lambda: gs.render(cam, 7, 0, SPP))
    assert st.pilot_tiles == 0 and all(getattr(st, f) == getattr(st_np, f) for f in fields)
    # two ranges accumulate to the whole
    whole, st_w = gs.render(cam, 7, 0, 600)
    parts, st_a = gs.render(cam, 7, 0, 300)
    parts, st_b = gs.render(cam, 7, 300, 600, accum=parts)
    assert st_w.pilot_tiles > 0 and st_a.pilot_tiles > 0 and st_b.pilot_tiles > 0
    assert st_a.samples + st_b.samples == st_w.samples and st_a.segments + st_b.segments == st_w.segments
    np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0.0)
    # a scene reused after a larger render lays out as a fresh one
    big = pt.Camera.from_buffer_copy(cam)
    big.image_width, big.aspect_ratio = 128, 128 / 72.5
    gs.render(big, 7, 0, LONG)
    again, st_again = gs.render(cam, 7, 0, LONG)
    fresh_scene, fresh_cam = _script_scene(pt, ctx, 6, 64)
    fresh, st_fresh = fresh_scene.render(fresh_cam, 7, 0, LONG)
    assert all(getattr(st_again, f) == getattr(st_fresh, f) for f in fields) and st_again.pilot_tiles > 0
    np.testing.assert_allclose(again, fresh, rtol=1e-12, atol=0.0)
    fresh_scene.close(); gs.close()
