"""The short-path pass's tile rule (pt_short_tiles, csrc/pt_sky_tiles.h sky_tile_class) without a device: a tile is SHORT when
every box the sky pass's plane tests cannot clear is flagged shadeable. The rule is conservative — no camera ray of a short tile enters a box
that is not flagged, the extreme lens and jitter offsets included — it leaves the sure-sky tiles what they were, and it says nothing where
nothing can be said. Cameras, boxes and rays are those of tests/test_sky_tiles_cpu.py and tests/camera_rule.py."""
import ctypes as C
import os

import numpy as np

import camera_rule as CR
import test_sky_tiles_cpu as T

H = T.H


def _ground(cam, frame):
    """A wide slab three units below the camera: the kind of box the pass is for."""
    c = np.array(cam.look_from[:])
    return np.concatenate([c + [-60.0, -3.2, -60.0], c + [60.0, -3.0, 60.0]])


def test_symbol_and_binding(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    assert "pt_short_tiles" in pt.ABI_SYMBOLS and hasattr(pt.lib, "pt_short_tiles") and "pt_short_tiles(" in header
    assert pt.lib.pt_short_tiles.argtypes == [C.POINTER(pt.Camera), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    for f in ("short_tiles", "short_samples", "hard_samples", "ms_short"):
        assert f in pt.RenderStats().as_dict() and f in header
    out = np.zeros(45, dtype=np.uint8)
    assert pt.lib.pt_short_tiles(None, 0, None, None, out.ctypes.data) == -1 and b"bad arguments" in pt.lib.pt_last_error()


def test_short_tiles_are_entered_through_flagged_boxes_only(pt):
    rng = np.random.default_rng(23)
    n_short = n_rays = 0
    for k, (cam, frame) in enumerate(T._random_cameras(pt)):
        W = cam.image_width
        boxes = np.concatenate([T._boxes(rng, cam, frame, 6), _ground(cam, frame)[None, :]])
        flags = np.zeros(len(boxes), dtype=np.uint8)
        flags[6] = 1                                                    # the ground ...
        if k % 2:
            flags[1 + k % 5] = 1                                        # ... and, for every other camera, one of the random boxes
        tiles = pt.short_tiles(cam, boxes, flags)
        assert tiles.shape == ((H + 7) // 8, (W + 7) // 8) and set(np.unique(tiles)) <= {0, 1, 2}
        assert ((tiles == 1) == (pt.sky_tiles(cam, boxes) == 1)).all()   # every sure-sky tile is still sure sky, and nothing else is
        assert (pt.short_tiles(cam, boxes, np.zeros(len(boxes), dtype=np.uint8)) == (tiles == 1)).all()   # no shadeable entry: no short tile
        short = np.argwhere(tiles == 2)
        if len(short) == 0:
            continue
        n_short += len(short)
        others = boxes[flags == 0]
        pix = np.concatenate([(r[:, None] * W + c[None, :]).reshape(-1) for r, c in (T._tile_pixels(ty, tx, W) for ty, tx in short)])
        P, S = np.repeat(pix, T.N_SAMPLES), np.tile(np.arange(T.N_SAMPLES), len(pix))
        o, d, _, _ = CR.camera_rays("perspective", frame, H, cam, 31 + k, P, S, sobol=False)
        assert not T._enters(o, d, others).any(), (k, "random rays")
        for ty, tx in short:
            oe, de = T._extreme_rays(frame, cam, ty, tx)
            assert not T._enters(oe, de, others).any(), (k, ty, tx, "extreme rays")
            n_rays += len(oe)
        n_rays += len(P)
    print(f"short tiles {n_short}, rays {n_rays}")
    # (a test that finds no short tile proves nothing; short tiles crowd the ragged bottom row, whose tiles hold 4 x 8 pixels: 32 x 32 + 288 rays)
    assert n_short >= 40 and n_rays >= 1312 * n_short


def test_a_short_tile_has_a_ray_into_a_flagged_box(pt):
    """... so that short is not another word for sure sky: the tile below the horizon of a camera over the ground alone is short, and one of its
    rays enters the ground's box."""
    cam, frame = T._camera(pt, 64, defocus_angle=0.0, blur_strength=0.0, look_from=(0.0, 1.5, 0.0), look_at=(0.0, 1.5, 10.0))
    ground = np.array([[-100.0, -1e-4, -100.0, 100.0, 1e-4, 100.0]])
    tiles = pt.short_tiles(cam, ground, [1])
    assert (tiles[0] == 1).all() and (tiles[-1] == 2).all()
    rows, cols = T._tile_pixels(tiles.shape[0] - 1, 3, 64)
    R, Cc = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(rows, cols, indexing="ij"))
    z = np.zeros(len(R))
    o, d = T._rays(frame, cam, R, Cc, z, z, z, z)
    assert T._enters(o, d, ground).all()
    assert (pt.short_tiles(cam, ground, [0]) == (tiles == 1)).all()     # the same box not flagged: those tiles are the path pool's


def test_nothing_is_short_where_nothing_can_be_said(pt):
    rng = np.random.default_rng(5)
    for kw in (dict(defocus_angle=0.0, blur_strength=0.0), dict(defocus_angle=3.0, blur_strength=2.0)):
        cam, frame = T._camera(pt, 68, **kw)
        c = np.array(cam.look_from[:])
        ground = _ground(cam, frame)
        inside = np.concatenate([c - 1.0, c + 1.0])
        # a camera inside (or on a face of) a box that is not flagged: that box is never cleared
        assert not pt.short_tiles(cam, np.stack([ground, inside]), [1, 0]).any()
        touching = np.concatenate([c - [1.0, 1.0, 0.0], c + [1.0, 1.0, 5.0]])
        assert not pt.short_tiles(cam, np.stack([ground, touching]), [1, 0]).any()
        # a NaN among the boxes, flagged or not
        for b in (0, 1):
            bad = np.stack([ground, np.concatenate([c + 50.0, c + 51.0])])
            bad[b, 4] = np.nan
            assert not pt.short_tiles(cam, bad, [1, 0]).any() and not pt.short_tiles(cam, bad, [1, 1]).any()
        # no shadeable entry, and no boxes at all
        assert not (pt.short_tiles(cam, ground[None, :], [0]) == 2).any()
        assert (pt.short_tiles(cam, np.zeros((0, 6)), []) == 1).all()
    # more boxes than the cap are walked as their union: nothing is shadeable
    cam, frame = T._camera(pt, 64, defocus_angle=1.0, blur_strength=0.5)
    c = np.array(cam.look_from[:])
    lo = c - frame["forward"] * 6.0 + frame["right"] * 3.0 + rng.uniform(-0.5, 0.5, (70, 3))
    boxes = np.concatenate([lo, lo + 0.3], axis=1)
    many = pt.short_tiles(cam, boxes, np.ones(70, dtype=np.uint8))
    assert not (many == 2).any() and ((many == 1) == (pt.sky_tiles(cam, boxes) == 1)).all() and (many == 1).any()
    assert (pt.short_tiles(cam, boxes[:64], np.ones(64, dtype=np.uint8)) == 2).any()   # 64 boxes are walked one by one
