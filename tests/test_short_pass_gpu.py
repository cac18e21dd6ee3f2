"""The short-path pass: the tiles whose camera rays can enter only boxes of shadeable entries are rendered by k_short ahead of
the path pool as far as a sample's path is camera -> miss or camera -> one diffuse hit -> miss; the other samples of those tiles — the hard
ones — are work items of the wavefront. The frame must be the one the wavefront renders without the pass (PT_SHORT_PASS=0): the same sample
and segment counts, the same sums up to the order of the dynamic mode's f64 additions (1e-12 relative, as in tests/test_sky_pass_gpu.py),
and where the pass must be off nothing may change at all ("bit for bit" between two dynamic-mode renders: as 16 one-sample slices, see
there)."""
import numpy as np
import pytest

from common import SceneSpec, _with_env, default_camera
from test_sky_pass_gpu import SPP, _clipped_pixels, _entry_boxes, _open_scene, _same_bits, _script_scene, _slices

pytestmark = pytest.mark.gpu

OFF = {"PT_EXPERIMENT": "1", "PT_SHORT_PASS": "0"}


def _scene6_tiles(pt, gs, cam):
    """The host's classification of scene 6: its ground quad is entry 0, the one shadeable entry."""
    boxes = _entry_boxes(pt, gs)
    flags = np.zeros(len(boxes), dtype=np.uint8)
    flags[0] = 1
    return pt.short_tiles(cam, boxes, flags)


@pytest.mark.parametrize("width", [64, 68])
def test_frame_equals_the_wavefront_alone(pt, ctx, width):
    gs, cam = _script_scene(pt, ctx, 6, width)
    tiles = _scene6_tiles(pt, gs, cam)
    for seed in (1, 2):
        on, st = gs.render(cam, seed, 0, SPP)
        off, st0 = _with_env(OFF, lambda: gs.render(cam, seed, 0, SPP))
        print(f"scene 6 {width}x36 seed {seed}: short tiles {st.short_tiles}, finished {st.short_samples}, hard {st.hard_samples}, sky tiles {st.sky_tiles}, "
              f"max rel diff {np.max(np.abs(on - off) / np.maximum(np.abs(off), 1e-300))}")
        assert st0.short_tiles == 0 and st0.short_samples == 0 and st0.hard_samples == 0 and st0.sky_tiles == st.sky_tiles == (tiles == 1).sum()
        assert st.samples == st0.samples == width * 36 * SPP and st.segments == st0.segments
        assert st.short_tiles == (tiles == 2).sum() > 0 and st.short_samples > 0 and st.hard_samples > 0
        assert st.short_samples + st.hard_samples == _clipped_pixels(tiles == 2, width, 36) * SPP
        np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_sample_ranges_accumulate(pt, ctx):
    gs, cam = _script_scene(pt, ctx, 6, 64)
    whole, st = gs.render(cam, 5, 0, SPP)
    parts, st_a = gs.render(cam, 5, 0, 7)
    parts, st_b = gs.render(cam, 5, 7, SPP, accum=parts)                 # (overwrite 0: added to what is there)
    assert st.short_tiles == st_a.short_tiles == st_b.short_tiles > 0
    assert st_a.short_samples + st_b.short_samples == st.short_samples and st_a.hard_samples + st_b.hard_samples == st.hard_samples > 0
    assert st_a.samples + st_b.samples == st.samples and st_a.segments + st_b.segments == st.segments
    np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0.0)
    gs.close()


def test_every_sample_of_a_short_tile_is_the_oracles(pt, ctx, det):
    """Sixteen one-sample slices against the oracle's trace_sample, bit for bit, for every pixel of the short tiles: the samples the pass finishes
    (camera misses at the horizon, ground -> sky) and the hard ones the wavefront renders from their list entries — each exactly once, or a
    slice would hold none or two of them."""
    W = 68                                                               # (at 68 columns a short tile of the ragged right column holds the horizon)
    gs, cam = _script_scene(pt, ctx, 6, W)
    os_ = det.Scene()
    ocam = os_.build_scene(6, W, SPP)
    ocam.aspect_ratio = cam.aspect_ratio
    tiles = _scene6_tiles(pt, gs, cam)
    rows, cols = np.nonzero(np.kron(tiles == 2, np.ones((8, 8), dtype=bool))[:36, :W])
    kinds = {1: 0, 2: 0, 3: 0}
    finished = hard = 0
    for i in range(SPP):
        acc, st = gs.render(cam, 3, i, i + 1)
        finished, hard = finished + st.short_samples, hard + st.hard_samples
        for r, c in zip(rows, cols):
            rad, _, nseg = os_.trace_sample(ocam, 3, int(r) * W + int(c), i, 4)
            assert _same_bits(np.ascontiguousarray(acc[r, c]), rad), (i, r, c, nseg)
            kinds[min(nseg, 3)] += 1
    print(f"samples compared {len(rows) * SPP}: one segment {kinds[1]}, two {kinds[2]}, more {kinds[3]}; finished by the pass {finished}, hard {hard}")
    assert finished + hard == len(rows) * SPP and min(kinds.values()) > 0 and hard >= kinds[3] > 0
    os_.close(); gs.close()


def _floor_scene(ground="diffuse", n_extra=0, lights=False):
    """A quad under a grey environment and one metal sphere standing on it. ground: "diffuse" (shadeable), "metal", "instanced" (the diffuse
    quad under an instance), "moving" (under a moving instance); n_extra: that many small spheres more, far behind the camera (a top level
    beyond the flat walk's limit); lights: a lights list."""
    s = SceneSpec()
    grey = s.add("mat_diffuse", s.add("tex_checker", 0.8, s.add("tex_solid_rgb", 0.2, 0.3, 0.1), s.add("tex_solid_rgb", 0.9, 0.9, 0.9)), -1)
    metal = s.add("mat_metal", s.add("tex_solid_rgb", 0.9, 0.8, 0.6), s.add("tex_solid_f", 0.1))
    quad = s.add("quad", (-30.0, 0.0, -30.0), (0.0, 0.0, 60.0), (60.0, 0.0, 0.0), metal if ground == "metal" else grey)
    if ground == "instanced":
        quad = s.add("instance", quad, (0.0, 1.0, 0.0), 0.3, (0.0, 0.0, 0.0))
    if ground == "moving":
        quad = s.add("instance_moving", quad, (0.0, 1.0, 0.0), 0.0, 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.5))
    s.add("world_add_object", quad)
    s.add("world_add_object", s.add("sphere", 0.7, (0.0, 0.7, 0.0), (0.0, 0.7, 0.0), metal))
    for k in range(n_extra):
        s.add("world_add_object", s.add("sphere", 0.1, (-3.0 + 0.25 * k, 0.1, -40.0), (-3.0 + 0.25 * k, 0.1, -40.0), metal))
    if lights:
        s.add("world_add_light", s.add("quad", (-0.5, 3.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), s.add("mat_light", s.add("tex_solid_rgb", 6.0, 6.0, 5.0))))
    s.add("world_build")
    s.camera = default_camera(width=64, aspect=64 / 40.5, spp=SPP, look_from=(0.0, 1.2, -6.0), look_at=(0.0, 1.0, 0.0), env_color=(0.5, 0.5, 0.5))
    return s


def _built(pt, ctx, **kw):
    spec, gs = _floor_scene(**kw), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    assert pt.image_height(cam) == 40
    return gs, cam


def test_host_api_scene_has_every_kind_of_tile(pt, ctx):
    gs, cam = _built(pt, ctx)
    tiles = pt.short_tiles(cam, _entry_boxes(pt, gs), [1, 0])
    n_sky, n_short, n_wave = (tiles == 1).sum(), (tiles == 2).sum(), (tiles == 0).sum()
    assert n_sky > 0 and n_short > 0 and n_wave > 0
    on, st = gs.render(cam, 2, 0, SPP)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 2, 0, SPP))
    print(f"tiles: sky {n_sky}, short {n_short}, wavefront {n_wave}; finished {st.short_samples}, hard {st.hard_samples}")
    assert st.sky_tiles == st0.sky_tiles == n_sky and st.short_tiles == n_short and st0.short_tiles == 0
    assert st.hard_samples > 0 and st.short_samples + st.hard_samples == _clipped_pixels(tiles == 2, 64, 40) * SPP
    assert st.samples == st0.samples == 64 * 40 * SPP and st.segments == st0.segments
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    # a camera so close to the sphere that every tile looks into its box: no tile is short, and the frame is the switch-off frame bit for bit
    for k, v in dict(look_from=(0.0, 0.7, -1.2), look_at=(0.0, 0.7, 0.0)).items():
        for i, x in enumerate(v):
            getattr(cam, k)[i] = x
    assert not pt.short_tiles(cam, _entry_boxes(pt, gs), [1, 0]).any()
    near, st = _slices(lambda a, b: gs.render(cam, 2, a, b))
    near0, st0 = _slices(lambda a, b: gs.render(cam, 2, a, b), OFF)
    assert st.short_tiles == 0 and st.hard_samples == 0 and st.samples == st0.samples and st.segments == st0.segments
    assert _same_bits(near, near0)
    gs.close()


@pytest.mark.parametrize("case", ["lights", "sky-pass-lights", "tree", "metal", "instanced", "moving"])
def test_pass_is_off_where_it_must_be(pt, ctx, case):
    if case == "sky-pass-lights":                                        # the sky pass's own test scene: a lights list, and sure-sky tiles
        spec, gs = _open_scene("plain"), pt.Scene(ctx)
        cam = spec.make_camera(pt.Camera, spec.replay(gs))
    else:
        gs, cam = _built(pt, ctx, **{"lights": dict(lights=True), "tree": dict(n_extra=24), "metal": dict(ground="metal"),
                                     "instanced": dict(ground="instanced"), "moving": dict(ground="moving")}[case])
    on, st = _slices(lambda a, b: gs.render(cam, 4, a, b))
    off, st0 = _slices(lambda a, b: gs.render(cam, 4, a, b), OFF)
    assert st.short_tiles == 0 and st.short_samples == 0 and st.hard_samples == 0 and st.samples == st0.samples > 0 and st.segments == st0.segments
    assert st.sky_tiles == st0.sky_tiles and _same_bits(on, off), case
    gs.close()


def test_the_diffuse_floor_of_those_scenes_has_short_tiles(pt, ctx):
    """... so that the cases above are switched off by what they change, not by the scene."""
    gs, cam = _built(pt, ctx)
    _, st = gs.render(cam, 4, 0, 1)
    assert st.short_tiles > 0
    gs.close()


def test_the_byte_cap_takes_fewer_tiles(pt, ctx):
    gs, cam = _script_scene(pt, ctx, 6, 64)
    tiles = _scene6_tiles(pt, gs, cam)
    assert (tiles == 2).sum() > 2
    # two tiles' worst case — 64 pixels x SPP samples x 4 bytes each — and a little: the pass takes the first two short tiles in tile order
    capped = dict(OFF, PT_SHORT_PASS="1", PT_SHORT_CAP_BYTES=str(2 * 64 * SPP * 4 + 100))
    on, st = _with_env(capped, lambda: gs.render(cam, 1, 0, SPP))
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 1, 0, SPP))
    first_two = np.zeros_like(tiles)
    first_two.reshape(-1)[np.flatnonzero(tiles.reshape(-1) == 2)[:2]] = 1
    assert st.short_tiles == 2 and st.short_samples + st.hard_samples == _clipped_pixels(first_two, 64, 36) * SPP
    assert st.samples == st0.samples and st.segments == st0.segments and st.sky_tiles == st0.sky_tiles
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    none, st = _with_env(dict(capped, PT_SHORT_CAP_BYTES="100"), lambda: gs.render(cam, 1, 0, SPP))   # room for no tile at all
    assert st.short_tiles == 0 and st.hard_samples == 0 and st.samples == st0.samples and st.segments == st0.segments
    np.testing.assert_allclose(none, off, rtol=1e-12, atol=0.0)
    gs.close()
