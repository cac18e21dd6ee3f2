"""The sky pass: the tiles whose camera rays provably enter no box of the world are rendered by k_sky outside the path pool.
The frame must be the one the wavefront alone renders (PT_SKY_PASS=0) — the same sample and segment counts, the same sums up to the order
of the dynamic mode's f64 additions (1e-12 relative, as in tests/test_shading_order_gpu.py) — and where the pass must be off nothing may
change at all.

"Bit for bit" between two renders of the dynamic mode: the order in which the samples of one pixel reach the frame accumulator is not
fixed from run to run, so two runs of the same kernels on the same arguments differ in the last bits wherever a pixel gets three or more
non-zero contributions. One sample's own contributions do arrive in order (one per bounce, launch after launch), so those comparisons
render the 16 samples as 16 one-sample slices added up on the host: every slice is deterministic, and so is the host's sum."""
import numpy as np
import pytest

from common import SceneSpec, _with_env, default_camera

pytestmark = pytest.mark.gpu

SPP = 16
OFF = {"PT_EXPERIMENT": "1", "PT_SKY_PASS": "0"}


def _entry_boxes(pt, gs):
    boxes = []
    while True:
        try:
            boxes.append(gs.entry_box(len(boxes)))
        except pt.PtError:
            return np.array(boxes).reshape(-1, 6)


def _clipped_pixels(tiles, W, H):
    ty, tx = np.nonzero(tiles)
    return int((np.minimum(8, H - ty * 8) * np.minimum(8, W - tx * 8)).sum())


def _script_scene(pt, ctx, sid, width):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(sid, width, SPP)
    cam.aspect_ratio = width / 36.5      # 36 rows: a ragged bottom tile row, and at 68 columns a ragged right one
    assert pt.image_height(cam) == 36
    return gs, cam


def _slices(render, env=None):
    """The frame as SPP one-sample slices summed on the host (see the module's docstring); the statistics of the last slice."""
    acc, st = None, None
    for i in range(SPP):
        a, st = _with_env(env, lambda: render(i, i + 1)) if env else render(i, i + 1)
        acc = a if acc is None else acc + a
    return acc, st


def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


@pytest.mark.parametrize("sid, width", [(6, 64), (4, 64), (5, 64), (6, 68)])
def test_frame_equals_the_wavefront_alone(pt, ctx, sid, width):
    gs, cam = _script_scene(pt, ctx, sid, width)
    tiles = pt.sky_tiles(cam, _entry_boxes(pt, gs))                      # the host's classification: the device runs the same function
    for seed in (1, 2):
        on, st = gs.render(cam, seed, 0, SPP)
        off, st0 = _with_env(OFF, lambda: gs.render(cam, seed, 0, SPP))
        print(f"scene {sid} {width}x36 seed {seed}: sky tiles {st.sky_tiles} of {tiles.size}, sky samples {st.sky_samples}, max rel diff "
              f"{np.max(np.abs(on - off) / np.maximum(np.abs(off), 1e-300))}")
        assert st0.sky_tiles == 0 and st0.sky_samples == 0
        assert st.samples == st0.samples == width * 36 * SPP and st.segments == st0.segments
        assert st.sky_tiles == tiles.sum() > 0
        assert st.sky_samples == _clipped_pixels(tiles, width, 36) * SPP
        np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_scene_3_has_no_sky_tile(pt, ctx):
    """Scene 3, the Cornell box, in its own square frame at 64 pixels: no tile is sure sky and the frame is the switch-off frame bit for bit.
    (The box is open towards the camera and the frame is a little wider than the opening — a rim of 4.6 % of the width on each side, three
    pixels here — so no 8x8 tile lies wholly beside the walls. From about 180 pixels of width on the rim holds whole tiles: 4700 of 57 600
    at 1920x1920, profiles/r20_sky_pass.md. Their samples add exact zeros under the scene's black environment.)"""
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, SPP)
    assert pt.image_height(cam) == 64
    assert not pt.sky_tiles(cam, _entry_boxes(pt, gs)).any()
    on, st = _slices(lambda a, b: gs.render(cam, 1, a, b))
    off, st0 = _slices(lambda a, b: gs.render(cam, 1, a, b), OFF)
    assert st.sky_tiles == 0 and st.sky_samples == 0 and st0.sky_tiles == 0
    assert st.samples == st0.samples == 64 * 64 and st.segments == st0.segments
    assert _same_bits(on, off)
    gs.close()


def test_black_environment_keeps_the_wavefront_alone(pt, ctx):
    """Scene 3 in a 16:9 frame, wide enough for whole tiles beside the box: the tile test clears them, but under the scene's black constant
    environment their samples would add exact zeros, so the pass stays off: no sure-sky tile is reported and the frame is
    the switch-off frame bit for bit. With a grey environment the same tiles are rendered by the pass."""
    gs, cam = _script_scene(pt, ctx, 3, 64)
    tiles = pt.sky_tiles(cam, _entry_boxes(pt, gs))
    assert tiles.sum() > 0
    on, st = _slices(lambda a, b: gs.render(cam, 1, a, b))
    off, st0 = _slices(lambda a, b: gs.render(cam, 1, a, b), OFF)
    assert st.sky_tiles == 0 and st0.sky_tiles == 0 and st.samples == st0.samples == 64 * 36 and st.segments == st0.segments
    assert _same_bits(on, off)
    cam.env_color[0] = cam.env_color[1] = cam.env_color[2] = 0.25
    grey, st = gs.render(cam, 1, 0, SPP)
    grey0, st0 = _with_env(OFF, lambda: gs.render(cam, 1, 0, SPP))
    assert st.sky_tiles == tiles.sum() and st.samples == st0.samples and st.segments == st0.segments
    np.testing.assert_allclose(grey, grey0, rtol=1e-12, atol=0.0)
    rows, cols = np.nonzero(np.kron(tiles, np.ones((8, 8), dtype=np.uint8))[:36, :64])
    assert (grey[rows, cols] == 0.25 * SPP).all()
    gs.close()


def test_sample_ranges_accumulate(pt, ctx):
    gs, cam = _script_scene(pt, ctx, 6, 64)
    whole, st = gs.render(cam, 5, 0, SPP)
    parts, st_a = gs.render(cam, 5, 0, 7)
    parts, st_b = gs.render(cam, 5, 7, SPP, accum=parts)                 # (overwrite 0: added to what is there)
    assert st.sky_tiles == st_a.sky_tiles == st_b.sky_tiles > 0
    assert st_a.sky_samples * SPP == st.sky_samples * 7 and st_a.sky_samples + st_b.sky_samples == st.sky_samples
    assert st_a.samples + st_b.samples == st.samples and st_a.segments + st_b.segments == st.segments
    np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0.0)
    gs.close()


@pytest.mark.parametrize("sid", [6, 5])
def test_every_ray_of_a_cleared_tile_misses(pt, ctx, sid):
    gs, cam = _script_scene(pt, ctx, sid, 64)
    tiles = pt.sky_tiles(cam, _entry_boxes(pt, gs))
    _, st = gs.render(cam, 1, 0, SPP)
    assert st.sky_tiles == tiles.sum() > 0
    ty, tx = np.nonzero(tiles)
    rows = (ty[:, None] * 8 + np.arange(8)[None, :])                     # (n, 8)
    cols = (tx[:, None] * 8 + np.arange(8)[None, :])
    pix = (rows[:, :, None] * 64 + cols[:, None, :])
    pix = pix[(rows[:, :, None] < 36) & (cols[:, None, :] < 64)]
    ps = np.stack([np.repeat(pix, SPP), np.tile(np.arange(SPP), len(pix))], axis=1)
    rays = gs.camera_probe(cam, 1, ps)
    hits = gs.intersect(rays[:, :7])
    assert len(rays) == _clipped_pixels(tiles, 64, 36) * SPP and not hits[:, 0].any()
    gs.close()


def _open_scene(kind):
    """A floor, a ball and a light under a small float environment map, seen by a camera that looks above the horizon. kind "motion": the ball
    moves and the shutter is (0.2, 0.7); "medium": the camera stands in a thin fog; "allsky": one far box behind the camera and nothing else."""
    rng = np.random.default_rng(9)
    s = SceneSpec()
    env = s.add("tex_image_rgbf32", rng.uniform(0.05, 1.5, size=(4, 8, 3)).astype(np.float32))
    grey = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.6, 0.6, 0.55), -1)
    if kind == "allsky":
        s.add("world_add_object", s.add("cuboid", (-1.0, 0.0, -40.0), (1.0, 2.0, -38.0), grey))
    else:
        s.add("world_add_object", s.add("quad", (-20.0, 0.0, -20.0), (0.0, 0.0, 40.0), (40.0, 0.0, 0.0), grey))
        p2 = (0.4, 1.1, 0.0) if kind == "motion" else (0.0, 0.7, 0.0)
        s.add("world_add_object", s.add("sphere", 0.7, (0.0, 0.7, 0.0), p2, s.add("mat_metal", s.add("tex_solid_rgb", 0.9, 0.8, 0.6), s.add("tex_solid_f", 0.1))))
        s.add("world_add_light", s.add("quad", (-0.5, 3.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), s.add("mat_light", s.add("tex_solid_rgb", 6.0, 6.0, 5.0))))
    if kind == "medium":
        s.add("set_camera_medium", s.add("mat_medium", 0.03, (0.9, 0.9, 0.9), 0.2))
    s.add("world_build")
    if kind == "motion":
        s.add("set_shutter", 0.2, 0.7)
    s.camera = default_camera(width=64, aspect=64 / 36.5, spp=SPP, look_from=(0.0, 1.2, -6.0), look_at=(0.0, 2.2, 0.0), env_is_map=1, env_tex=env)
    return s


def _built(pt, ctx, kind):
    spec, gs = _open_scene(kind), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    return gs, cam


@pytest.mark.parametrize("case", ["pixels", "sobol", "medium", "orthographic", "fisheye", "panorama", "motion", "static"])
def test_pass_is_off_where_it_must_be(pt, ctx, case):
    gs, cam = _built(pt, ctx, {"medium": "medium", "motion": "motion"}.get(case, "plain"))
    if case == "sobol":
        gs.set_sampler("sobol")
    if case in ("orthographic", "fisheye", "panorama"):
        cam.defocus_angle = 0.0                                          # (the fisheye and panorama cameras have no lens)
        gs.set_projection(case)
    if case == "motion":
        assert gs.motion()
    if case == "pixels":
        pixels = np.arange(0, 64 * 36, 3)
        render = lambda a, b: gs.render_pixels(cam, 4, pixels, a, b)
    elif case == "static":
        render = lambda a, b: gs.render(cam, 4, a, b, slots_per_pixel=1)
    else:
        render = lambda a, b: gs.render(cam, 4, a, b)
    on, st = _slices(render)
    off, st0 = _slices(render, OFF)
    assert st.sky_tiles == 0 and st.sky_samples == 0 and st.samples == st0.samples > 0 and st.segments == st0.segments
    assert _same_bits(on, off), case
    gs.close()


def test_the_plain_case_of_that_scene_has_sky_tiles(pt, ctx):
    """... so that the cases above are switched off by what they set, not by the scene."""
    gs, cam = _built(pt, ctx, "plain")
    on, st = gs.render(cam, 4, 0, SPP)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 4, 0, SPP))
    assert st.sky_tiles > 0 and st.samples == st0.samples and st.segments == st0.segments
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_a_frame_that_is_all_sky_skips_the_wavefront(pt, ctx):
    gs, cam = _built(pt, ctx, "allsky")
    on, st = gs.render(cam, 6, 0, SPP)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 6, 0, SPP))
    assert st.sky_tiles == 8 * 5 and st.sky_samples == 64 * 36 * SPP == st.samples == st.segments
    assert st.iterations == 0 and st.launches_extend == 0 and st.launches_shade == 0
    assert st0.samples == st.samples and st0.segments == st.segments and st0.iterations > 0
    assert (on > 0.0).all()
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()
