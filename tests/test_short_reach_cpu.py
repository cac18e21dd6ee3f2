"""The reach masks of the short-path pass (pt_tile_reach, csrc/pt_sky_tiles.h sky_tile_reach) without a device: bit b of a
tile's mask is 0 only where no camera ray of the tile enters box b — k_short then never loads that entry — the mask is 0 exactly for the
sure-sky tiles, and it is all ones wherever the test says nothing. Cameras, boxes and rays are those of tests/test_short_tiles_cpu.py and
tests/camera_rule.py. (A tile outside the image has no place in the host function's output: its all-ones answer is sky_tile_reach's first
line, which the device's classification shares.)"""
import ctypes as C
import os

import numpy as np
import pytest

import camera_rule as CR
import test_short_tiles_cpu as S
import test_sky_tiles_cpu as T

H = T.H
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def _bits(masks, n):
    """(tiles_y, tiles_x, n) bool: bit b of every tile's mask."""
    return ((masks[:, :, None] >> np.arange(n, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)


def test_symbol_and_binding(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    assert "pt_tile_reach" in pt.ABI_SYMBOLS and hasattr(pt.lib, "pt_tile_reach") and "pt_tile_reach(" in header
    assert pt.lib.pt_tile_reach.argtypes == [C.POINTER(pt.Camera), C.c_uint32, C.c_void_p, C.c_void_p]
    out = np.zeros(45, dtype=np.uint64)
    assert pt.lib.pt_tile_reach(None, 0, None, out.ctypes.data) == -1 and b"bad arguments" in pt.lib.pt_last_error()
    cam, _ = T._camera(pt, 64)
    assert pt.lib.pt_tile_reach(C.byref(cam), 1, None, out.ctypes.data) == -1
    assert pt.lib.pt_tile_reach(C.byref(cam), 0, None, None) == -1


def _cases(pt):
    """The twelve random cameras, each with six random boxes and a ground slab."""
    rng = np.random.default_rng(23)
    return [(cam, frame, np.concatenate([T._boxes(rng, cam, frame, 6), S._ground(cam, frame)[None, :]])) for cam, frame in T._random_cameras(pt)]


@pytest.mark.parametrize("k", range(12))
def test_no_ray_enters_a_box_whose_bit_is_zero(pt, k):
    """Every tile of the camera's frame: the same 32 random rays per pixel and the rays at the extreme lens and jitter offsets, in exact f64."""
    cam, frame, boxes = _cases(pt)[k]
    W = cam.image_width
    masks = pt.tile_reach(cam, boxes)
    assert masks.shape == ((H + 7) // 8, (W + 7) // 8) and masks.dtype == np.uint64
    assert ((masks == 0) == (pt.sky_tiles(cam, boxes) == 1)).all()      # a mask of 0 exactly where the tile is sure sky
    assert ((masks >> np.uint64(len(boxes))) == 0).all()                # (no box of these cameras holds the lens: no mask is all ones)
    bits = _bits(masks, len(boxes))
    # a tile is short exactly when its mask names flagged boxes only: the classes are the masks read against the flags
    flags = np.zeros(len(boxes), dtype=np.uint8)
    flags[6] = 1
    flags[1 + k % 5] = 1
    assert ((pt.short_tiles(cam, boxes, flags) == 2) == ((masks != 0) & ~(bits & (flags == 0)[None, None, :]).any(axis=2))).all()
    # the random rays of every pixel of the frame in one call of the rule, each ray under its pixel's tile
    pix = np.arange(H * W)
    P, Sm = np.repeat(pix, T.N_SAMPLES), np.tile(np.arange(T.N_SAMPLES), len(pix))
    o, d, _, _ = CR.camera_rays("perspective", frame, H, cam, 31 + k, P, Sm, sobol=False)
    tile_of = (P // W // 8) * masks.shape[1] + (P % W) // 8
    hit = T._enters(o, d, boxes)
    entered = np.stack([np.bincount(tile_of[hit[:, b]], minlength=masks.size) > 0 for b in range(len(boxes))], axis=1).reshape(bits.shape)
    n_tiles, n_rays = 0, len(P)
    for ty in range(masks.shape[0]):
        for tx in range(masks.shape[1]):                                # every tile is checked, none is left out
            oe, de = T._extreme_rays(frame, cam, ty, tx)
            ent = entered[ty, tx] | T._enters(oe, de, boxes).any(axis=0)
            assert not (ent & ~bits[ty, tx]).any(), (k, ty, tx, np.flatnonzero(ent & ~bits[ty, tx]))
            n_tiles += 1
            n_rays += len(oe)
    assert n_tiles == masks.size == 5 * ((W + 7) // 8) and n_rays == H * W * T.N_SAMPLES + 288 * n_tiles


def test_the_masks_clear_boxes_one_by_one(pt):
    """A mask that clears nothing proves nothing, and a mask that is all or nothing is the sky pass's test again."""
    n_zero_bits = n_partial = 0
    for cam, frame, boxes in _cases(pt):
        n = _bits(pt.tile_reach(cam, boxes), len(boxes)).sum(axis=2)
        n_zero_bits += int((len(boxes) - n).sum())
        n_partial += int(((0 < n) & (n < len(boxes))).sum())
    print(f"zero bits {n_zero_bits}, tiles with some but not all boxes {n_partial}")
    # (510 tiles x 7 boxes, of which those behind the lens plane alone — a third of _boxes' range of depths — are cleared for every tile)
    assert n_zero_bits >= 1000 and n_partial >= 100


def test_all_ones_where_the_test_says_nothing(pt):
    rng = np.random.default_rng(5)
    for kw in (dict(defocus_angle=0.0, blur_strength=0.0), dict(defocus_angle=3.0, blur_strength=2.0)):
        cam, frame = T._camera(pt, 68, **kw)
        c = np.array(cam.look_from[:])
        ground = S._ground(cam, frame)
        far = np.concatenate([c + 50.0, c + 51.0])
        # a camera inside a box, or on a face of one: whatever else there is, and whichever box it is
        inside = np.concatenate([c - 1.0, c + 1.0])
        touching = np.concatenate([c - [1.0, 1.0, 0.0], c + [1.0, 1.0, 5.0]])
        for held in (inside, touching):
            for boxes in (np.stack([ground, held]), np.stack([held, far, ground]), held[None, :]):
                assert (pt.tile_reach(cam, boxes) == ALL).all()
        # the same boxes without the one that holds the camera: something is cleared again
        assert (pt.tile_reach(cam, np.stack([far, ground])) != ALL).all()
        # a NaN or an infinity among the boxes
        for b in (0, 1):
            for v in (np.nan, np.inf):
                bad = np.stack([ground, far])
                bad[b, 4] = v
                assert (pt.tile_reach(cam, bad) == ALL).all()
        assert (pt.tile_reach(cam, np.zeros((0, 6))) == 0).all()        # no boxes: every tile is sure sky
    # more boxes than the cap are walked as their union: all ones, but for the tiles whose union is cleared (the sure-sky ones: 0)
    cam, frame = T._camera(pt, 64, defocus_angle=1.0, blur_strength=0.5)
    c = np.array(cam.look_from[:])
    lo = c - frame["forward"] * 6.0 + frame["right"] * 3.0 + rng.uniform(-0.5, 0.5, (70, 3))
    boxes = np.concatenate([lo, lo + 0.3], axis=1)
    many, sky = pt.tile_reach(cam, boxes), pt.sky_tiles(cam, boxes) == 1
    assert (many[sky] == 0).all() and (many[~sky] == ALL).all() and sky.any() and not sky.all()
    few = pt.tile_reach(cam, boxes[:64])                                # 64 boxes are walked one by one
    assert ((few == 0) == (pt.sky_tiles(cam, boxes[:64]) == 1)).all() and ((few != 0) & (few != ALL)).any()
