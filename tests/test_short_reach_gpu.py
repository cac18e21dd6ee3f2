"""The short-path pass's reach masks, direct hits and untested self-hits. k_short's camera rays test only the entries the
tile test could not clear (step 1), a tile whose mask names one shadeable entry rebuilds the hit without the top level's loop (step 2), and a
bounce does not test the quad it left (step 3). Each step has a switch under PT_EXPERIMENT=1, and none may change a result: sample and
segment counts are equal, frames agree with every switch off and with the wavefront alone (PT_SHORT_PASS=0) to 1e-12 relative — the bound
for reordered f64 atomic adds of tests/test_short_pass_gpu.py —, and one-sample slices, which add one value per pixel, are equal bit for
bit. A sample may finish with the masks that was hard without (an f32 false positive on a mesh's box is gone), never the other way; in a
scene without meshes no box test decides an outcome and the pass's counts are equal too."""
import numpy as np
import pytest

from common import SceneSpec, _with_env, default_camera
from test_sky_pass_gpu import SPP, _entry_boxes, _same_bits, _script_scene, _slices
from test_short_pilot_gpu import ANY_RANGE, LONG, OFF, X

pytestmark = pytest.mark.gpu

ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_REACH, NO_DIRECT, NO_SELF = dict(X, PT_SHORT_REACH="0"), dict(X, PT_SHORT_DIRECT="0"), dict(X, PT_SHORT_SELF="0")
NONE = dict(X, PT_SHORT_REACH="0", PT_SHORT_DIRECT="0", PT_SHORT_SELF="0")
SWITCHES = {"reach": NO_REACH, "direct": NO_DIRECT, "self": NO_SELF, "none": NONE}


def _forced(env):
    return dict(env, PT_PILOT_ANY_RANGE="1")


@pytest.mark.parametrize("width", [64, 68])
def test_scene6_against_every_switch(pt, ctx, width):
    gs, cam = _script_scene(pt, ctx, 6, width)
    on, st = gs.render(cam, 1, 0, LONG)
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 1, 0, LONG))
    print(f"scene 6 {width}x36 @ {LONG}: short tiles {st.short_tiles} (by yield {st.pilot_tiles}, direct {st.short_direct_tiles}), self quads {st.short_self_prims}, "
          f"finished {st.short_samples}, hard {st.hard_samples}")
    assert st.pilot_tiles > 0 and 0 < st.short_direct_tiles <= st.short_tiles and st.short_self_prims == 1   # the ground quad
    assert st.samples == st0.samples == width * 36 * LONG and st.segments == st0.segments
    assert st.short_samples + st.hard_samples == st.short_pixels * LONG
    np.testing.assert_allclose(on, off, rtol=1e-12, atol=0.0)
    for name, env in SWITCHES.items():
        alt, st_a = _with_env(env, lambda: gs.render(cam, 1, 0, LONG))
        print(f"  {name} off: direct {st_a.short_direct_tiles}, self quads {st_a.short_self_prims}, finished {st_a.short_samples}, hard {st_a.hard_samples}")
        assert st_a.samples == st.samples and st_a.segments == st.segments
        assert st_a.short_tiles == st.short_tiles and st_a.pilot_tiles == st.pilot_tiles and st_a.short_pixels == st.short_pixels
        assert st_a.short_samples + st_a.hard_samples == st_a.short_pixels * LONG
        assert st.short_samples >= st_a.short_samples                    # the masks only take box tests away
        if name in ("direct", "self"):                                   # (these two take no box test of a mesh away)
            assert st_a.short_samples == st.short_samples
        assert (st_a.short_direct_tiles == 0) == (name != "self") and (st_a.short_self_prims == 0) == (name in ("self", "none"))
        np.testing.assert_allclose(alt, on, rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(alt, off, rtol=1e-12, atol=0.0)
    gs.close()


def test_every_sample_of_the_frame_is_the_oracles(pt, ctx, det):
    """Sixteen one-sample slices with the pilot forced, all steps on, against the oracle's trace_sample: every pixel, bit for bit."""
    W = 68
    gs, cam = _script_scene(pt, ctx, 6, W)
    os_ = det.Scene()
    ocam = os_.build_scene(6, W, SPP)
    ocam.aspect_ratio = cam.aspect_ratio
    finished = hard = taken = direct = 0
    for i in range(SPP):
        acc, st = _with_env(ANY_RANGE, lambda: gs.render(cam, 3, i, i + 1))
        finished, hard, taken, direct = finished + st.short_samples, hard + st.hard_samples, taken + st.pilot_tiles, direct + st.short_direct_tiles
        ref = np.array([os_.trace_sample(ocam, 3, p, i, 1)[0] for p in range(36 * W)]).reshape(36, W, 3)
        bad = np.argwhere((acc.view(np.uint64) != ref.view(np.uint64)).any(axis=2))
        assert len(bad) == 0, (i, bad[:4])
    print(f"samples compared {36 * W * SPP}; finished by the pass {finished}, hard {hard}, tiles by yield {taken}, direct {direct}")
    assert finished > 0 and hard > 0 and taken > 0 and direct > 0
    os_.close(); gs.close()


# ---- a scene without meshes: a checker floor, a diffuse sphere and a metal one, both in the sky above the horizon ----
DIFFUSE, METAL = ((-1.0, 2.4, 0.0), 1.0), ((0.9, 2.3, 0.0), 0.9)
OUTSIDE = dict(look_from=(0.0, 1.2, -6.0), look_at=(0.0, 1.0, 0.0))
INSIDE = dict(look_from=DIFFUSE[0], look_at=(-1.0, 2.2, 5.0))           # the camera at the diffuse sphere's centre


ALONE = ((2.6, 3.2, 0.0), 0.45)                                         # a metal sphere whose box shares no tile with another entry's


def _spheres_scene(pt, ctx, half=30.0, metal_at=METAL, **camera):
    s = SceneSpec()
    floor = s.add("mat_diffuse", s.add("tex_checker", 0.8, s.add("tex_solid_rgb", 0.2, 0.3, 0.1), s.add("tex_solid_rgb", 0.9, 0.9, 0.9)), -1)
    red = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.8, 0.3, 0.2), -1)
    metal = s.add("mat_metal", s.add("tex_solid_rgb", 0.9, 0.8, 0.6), s.add("tex_solid_f", 0.1))
    s.add("world_add_object", s.add("quad", (-half, 0.0, -half), (0.0, 0.0, 2.0 * half), (2.0 * half, 0.0, 0.0), floor))
    s.add("world_add_object", s.add("sphere", DIFFUSE[1], DIFFUSE[0], DIFFUSE[0], red))
    s.add("world_add_object", s.add("sphere", metal_at[1], metal_at[0], metal_at[0], metal))
    s.add("world_build")
    s.camera = default_camera(width=64, aspect=64 / 40.5, spp=SPP, env_color=(0.5, 0.5, 0.5), **camera)
    gs = pt.Scene(ctx)
    cam = s.make_camera(pt.Camera, s.replay(gs))
    assert pt.image_height(cam) == 40
    return gs, cam


def _metal_cover(pt, cam, ty, tx, metal_at=METAL):
    """The share of the tile's pixel centres whose pinhole ray hits the metal sphere."""
    frame, _ = pt.camera_init(cam)
    rows, cols = np.meshgrid(np.arange(ty * 8, ty * 8 + 8), np.arange(tx * 8, tx * 8 + 8), indexing="ij")
    o = np.array(cam.look_from[:])
    d = frame["pixel00"] + frame["pixel_dv"] * rows.reshape(-1, 1) + frame["pixel_du"] * cols.reshape(-1, 1) - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    oc = o - np.array(metal_at[0])
    b = d @ oc
    return float(((b * b - (oc @ oc - metal_at[1] ** 2) >= 0.0) & (b < 0.0)).mean())


def _equal_with_every_switch(gs, cam, seed, expect_direct, expect_self):
    """Counts at 256 spp (the pilot runs) and forced-pilot one-sample slices: the default against every switch, and against the wavefront alone."""
    _, st = gs.render(cam, seed, 0, LONG)
    _, st0 = _with_env(OFF, lambda: gs.render(cam, seed, 0, LONG))
    assert st.samples == st0.samples == 64 * 40 * LONG and st.segments == st0.segments
    assert st.short_tiles > 0 and st.hard_samples > 0 and st.short_samples + st.hard_samples == st.short_pixels * LONG
    assert (st.short_direct_tiles > 0) == expect_direct and st.short_self_prims == expect_self
    on, st_s = _slices(lambda a, b: gs.render(cam, seed, a, b), _forced(X))
    off, _ = _slices(lambda a, b: gs.render(cam, seed, a, b), OFF)
    assert _same_bits(on, off)
    for name, env in SWITCHES.items():
        _, st_a = _with_env(env, lambda: gs.render(cam, seed, 0, LONG))
        for f in ("samples", "segments", "short_samples", "hard_samples", "short_tiles", "pilot_tiles", "short_pixels"):
            assert getattr(st_a, f) == getattr(st, f), (name, f, getattr(st_a, f), getattr(st, f))
        alt, st_b = _slices(lambda a, b: gs.render(cam, seed, a, b), _forced(env))
        assert st_b.short_samples == st_s.short_samples and st_b.hard_samples == st_s.hard_samples and _same_bits(alt, on), name
    return st


def test_a_frame_with_every_kind_of_tile(pt, ctx):
    gs, cam = _spheres_scene(pt, ctx, **OUTSIDE)
    masks = pt.tile_reach(cam, _entry_boxes(pt, gs))                     # entries: 0 the floor, 1 the diffuse sphere, 2 the metal one
    kinds = {int(m): int((masks == m).sum()) for m in np.unique(masks)}
    print(f"tiles per mask: {kinds}")
    # sure sky; the floor alone and the diffuse sphere alone (the direct hit of a quad and of a sphere); two and three entries; the metal sphere alone
    assert all(kinds.get(m, 0) > 0 for m in (0, 1, 2, 4, 7)) and any(kinds.get(m, 0) > 0 for m in (3, 5, 6))
    st = _equal_with_every_switch(gs, cam, 2, True, 1)
    n_direct = kinds[1] + kinds[2]
    # a tile whose one uncleared entry is the metal sphere is the wavefront's by the rule; where the sphere covers a quarter of it or less the
    # pilot's yield is far above one half and the pass takes it: the masked loop over one entry that is not shadeable
    sure = sum(_metal_cover(pt, cam, ty, tx) <= 0.25 for ty, tx in np.argwhere(masks == 4))
    print(f"direct tiles {st.short_direct_tiles} of {n_direct} with one shadeable entry; by yield {st.pilot_tiles}, metal-only tiles taken for sure {sure}")
    assert sure >= 1 and st.pilot_tiles >= sure and st.short_direct_tiles == n_direct and st.sky_tiles == kinds[0]
    gs.close()


def test_the_tiles_taken_by_yield_reach_the_metal_sphere_alone(pt, ctx):
    """The same frame with the metal sphere by itself in the sky: every tile of the wavefront's class reaches that one entry and nothing else,
    so every tile the pilot takes is rendered by the masked loop over one entry that is not shadeable — and it takes those the sphere covers
    a quarter of or less (a yield far above one half)."""
    gs, cam = _spheres_scene(pt, ctx, metal_at=ALONE, **OUTSIDE)
    boxes = _entry_boxes(pt, gs)
    masks, classes = pt.tile_reach(cam, boxes), pt.short_tiles(cam, boxes, [1, 1, 0])
    assert ((classes == 0) == (masks == 4)).all() and (masks == 4).sum() >= 2
    sure = sum(_metal_cover(pt, cam, ty, tx, ALONE) <= 0.25 for ty, tx in np.argwhere(masks == 4))
    st = _equal_with_every_switch(gs, cam, 3, True, 1)
    print(f"metal-only tiles {(masks == 4).sum()}, taken by yield {st.pilot_tiles}, for sure {sure}")
    assert 1 <= sure <= st.pilot_tiles <= (masks == 4).sum() - 1 and st.short_tiles == (classes == 2).sum() + st.pilot_tiles
    gs.close()


@pytest.mark.parametrize("n_extra, flat", [(28, True), (34, False)])
def test_a_flat_top_level_of_more_entries_than_the_masks_hold(pt, ctx, n_extra, flat):
    """PT_FLAT_MAX=40 (read at the world's build) walks up to 40 entries flat. 30 entries: the pass runs, its masks all ones (the reach
    masks are kept for the product's limit of 24 entries). 36 entries: more than a 32-bit mask names, the pass is off. Either way the frame
    is the wavefront's."""
    from test_short_pass_gpu import _built
    gs, cam = _with_env(dict(X, PT_FLAT_MAX="40"), lambda: _built(pt, ctx, n_extra=n_extra))
    _, st = gs.render(cam, 4, 0, LONG)
    _, st0 = _with_env(OFF, lambda: gs.render(cam, 4, 0, LONG))
    assert (st.short_tiles > 0) == flat and st.short_direct_tiles == 0 and st.samples == st0.samples == 64 * 40 * LONG and st.segments == st0.segments
    assert (st.short_samples > 0) == flat and st.short_samples + st.hard_samples == st.short_pixels * LONG
    on, _ = _slices(lambda a, b: gs.render(cam, 4, a, b), _forced(X))
    off, _ = _slices(lambda a, b: gs.render(cam, 4, a, b), OFF)
    assert _same_bits(on, off)
    gs.close()


def test_camera_inside_the_diffuse_sphere(pt, ctx):
    """The masks are all ones; every camera ray hits the sphere from inside, the bounce goes inwards and must hit it again: nothing of the
    sphere's test may be taken away (step 3 is for quads)."""
    gs, cam = _spheres_scene(pt, ctx, **INSIDE)
    assert (pt.tile_reach(cam, _entry_boxes(pt, gs)) == ALL).all()
    st = _equal_with_every_switch(gs, cam, 4, False, 1)
    assert st.short_samples == 0 and st.hard_samples == st.short_pixels * LONG   # camera -> sphere -> sphere: every sample is hard
    gs.close()


def test_a_floor_beyond_the_bound_keeps_its_test(pt, ctx):
    gs, cam = _spheres_scene(pt, ctx, half=2.0e6, **OUTSIDE)            # corners at 2e6: beyond step 3's 1e6
    st = _equal_with_every_switch(gs, cam, 5, True, 0)
    assert st.short_samples > 0
    gs.close()


def test_sample_ranges(pt, ctx):
    gs, cam = _spheres_scene(pt, ctx, **OUTSIDE)
    # a range below PILOT_MIN: the pilot does not run, the proven tiles are rendered with their masks all the same
    short, st = gs.render(cam, 7, 0, SPP)
    none, st_n = _with_env(NONE, lambda: gs.render(cam, 7, 0, SPP))
    off, st0 = _with_env(OFF, lambda: gs.render(cam, 7, 0, SPP))
    assert st.pilot_tiles == 0 and st.short_direct_tiles > 0 and st_n.short_direct_tiles == 0
    assert st.short_samples == st_n.short_samples > 0 and st.hard_samples == st_n.hard_samples and st.samples == st0.samples and st.segments == st0.segments
    np.testing.assert_allclose(short, none, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(short, off, rtol=1e-12, atol=0.0)
    # two ranges accumulating against one
    whole, st_w = gs.render(cam, 7, 0, 2 * LONG)
    parts, st_a = gs.render(cam, 7, 0, LONG)
    parts, st_b = gs.render(cam, 7, LONG, 2 * LONG, accum=parts)
    assert st_a.samples + st_b.samples == st_w.samples and st_a.segments + st_b.segments == st_w.segments
    assert st_a.short_direct_tiles == st_b.short_direct_tiles == st_w.short_direct_tiles > 0
    np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0.0)
    gs.close()
