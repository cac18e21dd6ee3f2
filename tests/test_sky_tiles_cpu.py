"""The sky pass's tile test (pt_sky_tiles, csrc/pt_sky_tiles.h) without a device: it is conservative — no camera ray of a
cleared tile enters a box, the extreme lens and jitter offsets included — and it is not vacuous: a pinhole camera clears every tile whose
pixels, grown by one pixel, lie beside the box's projection. The rays come from the camera rule's restatement (tests/camera_rule.py)."""
import ctypes as C
import os

import numpy as np

import camera_rule as CR
from common import SceneSpec, default_camera

H = 36
U_MAX = 1.0 - 2.0 ** -53          # the largest unit draw: the rule's largest lens and jitter radius
N_SAMPLES = 32                     # random samples per pixel of a cleared tile: 2048 rays, and 4 x 8 x 9 = 288 extreme ones


def _camera(pt, width, **kw):
    spec = SceneSpec()
    spec.camera = default_camera(width=width, aspect=width / (H + 0.5), **kw)   # (height = floor(width / aspect) = 36)
    cam = spec.make_camera(pt.Camera, [])
    frame, h = pt.camera_init(cam)
    assert h == H
    return cam, frame


def _random_cameras(pt):
    rng = np.random.default_rng(20)
    cams = []
    for i in range(12):
        look_from = rng.uniform(-3.0, 3.0, 3)
        look_at = look_from + rng.normal(size=3) * 4.0
        vup = (0.0, 1.0, 0.0) if i % 3 else tuple(rng.normal(size=3))
        cams.append(_camera(pt, 68 if i % 2 else 64, vfov=float(rng.uniform(20.0, 100.0)), look_from=tuple(look_from), look_at=tuple(look_at), vup=vup,
                            focal_length=float(rng.uniform(0.5, 8.0)), defocus_angle=(0.0, 1.5, 6.0)[i % 3], blur_strength=(0.0, 0.5, 2.0)[(i // 3) % 3]))
    return cams


def _boxes(rng, cam, frame, n):
    """Boxes in front of, beside and behind the camera, one of them straddling the lens plane."""
    c = np.array(cam.look_from[:])
    out = np.empty((n, 6))
    for i in range(n):
        along = rng.uniform(-6.0, 12.0)                         # behind the camera when negative
        centre = c - frame["forward"] * along + frame["right"] * rng.uniform(-8.0, 8.0) + frame["up"] * rng.uniform(-6.0, 6.0)
        half = rng.uniform(0.1, 2.5, 3)
        if i == 0:                                              # one straddles the lens plane, beside the camera
            centre = c + frame["right"] * 4.0 + frame["up"] * rng.uniform(-1.0, 1.0)
            half = np.array([1.5, 1.5, 1.5])
        out[i, :3], out[i, 3:] = centre - half, centre + half
    return out


def _rays(frame, cam, rows, cols, bx, by, px, py):
    """The perspective rule of camera_rule.camera_rays for given offsets: bx, by the jitter (already times blur_strength), px, py the lens point."""
    radius = CR.lens_radius(float(cam.defocus_angle), float(cam.focal_length))
    S = frame["pixel00"] + frame["pixel_dv"] * (rows + bx)[:, None] + frame["pixel_du"] * (cols + by)[:, None]
    O = np.broadcast_to(np.array(cam.look_from[:]), S.shape)
    if radius != 0.0:
        O = O + (frame["right"] * radius) * px[:, None] + (frame["up"] * radius) * py[:, None]
    return np.array(O), CR._normalize(S - O)


def _enters(o, d, boxes):
    """(n_rays, n_boxes): the f64 slab test finds the box entered for some t >= 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (boxes[None, :, :3] - o[:, None, :]) / d[:, None, :]
        t1 = (boxes[None, :, 3:] - o[:, None, :]) / d[:, None, :]
    par = d[:, None, :] == 0.0                                  # parallel to a slab: inside it for every t, or never
    inside = (o[:, None, :] >= boxes[None, :, :3]) & (o[:, None, :] <= boxes[None, :, 3:])
    near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    return far.min(axis=2) >= np.maximum(near.max(axis=2), 0.0)


def _tile_pixels(ty, tx, W):
    rows = np.arange(ty * 8, min(ty * 8 + 8, H))
    cols = np.arange(tx * 8, min(tx * 8 + 8, W))
    return rows, cols


def _extreme_rays(frame, cam, ty, tx):
    """Corner pixels of the tile x jitter at the largest radius in the eight octant directions x the lens centre and the largest lens
    radius in the eight octant directions."""
    W = cam.image_width
    rows, cols = _tile_pixels(ty, tx, W)
    ang = np.arange(8) * (np.pi / 4.0)
    r = np.sqrt(U_MAX)
    jit = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1) * float(cam.blur_strength)
    lens = np.concatenate([np.zeros((1, 2)), np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)])
    R, Cc, J, L = np.meshgrid([rows[0], rows[-1]], [cols[0], cols[-1]], np.arange(8), np.arange(9), indexing="ij")
    R, Cc, J, L = (a.reshape(-1) for a in (R, Cc, J, L))
    return _rays(frame, cam, R.astype(np.float64), Cc.astype(np.float64), jit[J, 0], jit[J, 1], lens[L, 0], lens[L, 1])


def test_symbol_and_binding(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    assert "pt_sky_tiles" in pt.ABI_SYMBOLS and hasattr(pt.lib, "pt_sky_tiles") and "pt_sky_tiles(" in header
    assert pt.lib.pt_sky_tiles.argtypes == [C.POINTER(pt.Camera), C.c_uint32, C.c_void_p, C.c_void_p]
    for f in ("sky_tiles", "sky_samples", "ms_sky"):
        assert f in pt.RenderStats().as_dict() and f in header
    assert [n for n, _ in pt.RenderStats._fields_][-3:] == ["sky_tiles", "sky_samples", "ms_sky"]
    out = np.zeros(45, dtype=np.uint8)
    assert pt.lib.pt_sky_tiles(None, 0, None, out.ctypes.data) == -1 and b"bad arguments" in pt.lib.pt_last_error()
    cam, _ = _camera(pt, 64)
    assert pt.lib.pt_sky_tiles(C.byref(cam), 1, None, out.ctypes.data) == -1


def test_cleared_tiles_are_entered_by_no_ray(pt):
    rng = np.random.default_rng(7)
    n_cleared = n_rays = 0
    for k, (cam, frame) in enumerate(_random_cameras(pt)):
        W = cam.image_width
        boxes = _boxes(rng, cam, frame, 6)
        tiles = pt.sky_tiles(cam, boxes)
        assert tiles.shape == ((H + 7) // 8, (W + 7) // 8)
        cleared = np.argwhere(tiles == 1)
        if len(cleared) == 0:
            continue
        n_cleared += len(cleared)
        # the random rays of every pixel of every cleared tile, N_SAMPLES samples each, in one call of the rule
        pix = np.concatenate([(r[:, None] * W + c[None, :]).reshape(-1) for r, c in (_tile_pixels(ty, tx, W) for ty, tx in cleared)])
        P, S = np.repeat(pix, N_SAMPLES), np.tile(np.arange(N_SAMPLES), len(pix))
        o, d, _, _ = CR.camera_rays("perspective", frame, H, cam, 11 + k, P, S, sobol=False)
        assert not _enters(o, d, boxes).any(), (k, "random rays")
        for ty, tx in cleared:
            oe, de = _extreme_rays(frame, cam, ty, tx)
            assert not _enters(oe, de, boxes).any(), (k, ty, tx, "extreme rays")
            n_rays += len(oe)
        n_rays += len(P)
    print(f"cleared tiles {n_cleared}, rays {n_rays}")
    assert n_cleared >= 60 and n_rays >= 2000 * n_cleared          # (a test that clears nothing proves nothing)


def test_the_slab_test_sees_a_hit(pt):
    """The checker itself: rays through a box's centre enter it, and an uncleared tile in front of a box has a ray that enters."""
    cam, frame = _camera(pt, 64, defocus_angle=0.0, blur_strength=0.0, look_from=(0.0, 1.0, -6.0), look_at=(0.0, 1.0, 0.0))
    box = np.array([[-0.5, 0.5, -0.5, 0.5, 1.5, 0.5]])
    tiles = pt.sky_tiles(cam, box)
    ty, tx = H // 2 // 8, 64 // 2 // 8
    assert tiles[ty, tx] == 0
    rows, cols = _tile_pixels(ty, tx, 64)
    R, Cc = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(rows, cols, indexing="ij"))
    z = np.zeros(len(R))
    o, d = _rays(frame, cam, R, Cc, z, z, z, z)
    assert _enters(o, d, box).any()


def test_pinhole_clears_every_tile_beside_the_projection(pt):
    rng = np.random.default_rng(3)
    n_must = 0
    for k in range(8):
        W = 68 if k % 2 else 64
        look_from = rng.uniform(-2.0, 2.0, 3)
        cam, frame = _camera(pt, W, vfov=float(rng.uniform(30.0, 90.0)), look_from=tuple(look_from), look_at=tuple(look_from + rng.normal(size=3) * 3.0),
                             focal_length=float(rng.uniform(0.5, 5.0)), defocus_angle=0.0, blur_strength=0.0)
        c, fwd = np.array(cam.look_from[:]), frame["forward"]
        centre = c - fwd * rng.uniform(4.0, 9.0) + frame["right"] * rng.uniform(-2.0, 2.0) + frame["up"] * rng.uniform(-1.5, 1.5)
        half = rng.uniform(0.2, 0.9, 3)
        box = np.concatenate([centre - half, centre + half])
        corners = np.array([[box[3 * ((j >> a) & 1) + a] for a in range(3)] for j in range(8)])
        depth = -(corners - c) @ fwd
        assert (depth > 0.0).all()                                      # wholly in front of the lens plane
        s = c + (corners - c) * (float(cam.focal_length) / depth)[:, None] - frame["pixel00"]
        fx = s @ frame["pixel_du"] / (frame["pixel_du"] @ frame["pixel_du"])
        fy = s @ frame["pixel_dv"] / (frame["pixel_dv"] @ frame["pixel_dv"])
        tiles = pt.sky_tiles(cam, box[None, :])
        for ty in range(tiles.shape[0]):
            for tx in range(tiles.shape[1]):
                rows, cols = _tile_pixels(ty, tx, W)
                disjoint = (fx.min() > cols[-1] + 1.5 or fx.max() < cols[0] - 1.5 or fy.min() > rows[-1] + 1.5 or fy.max() < rows[0] - 1.5)
                if disjoint:
                    n_must += 1
                    assert tiles[ty, tx] == 1, (k, ty, tx)
    assert n_must >= 100


def test_camera_inside_a_box_and_no_boxes(pt):
    for kw in (dict(defocus_angle=0.0, blur_strength=0.0), dict(defocus_angle=3.0, blur_strength=2.0)):
        cam, frame = _camera(pt, 68, **kw)
        c = np.array(cam.look_from[:])
        assert not pt.sky_tiles(cam, np.concatenate([c - 1.0, c + 1.0])[None, :]).any()
        assert not pt.sky_tiles(cam, np.concatenate([c - [1.0, 1.0, 0.0], c + [1.0, 1.0, 5.0]])[None, :]).any()   # touching: the camera on a face
        far = np.concatenate([c + 50.0, c + 51.0])
        assert not pt.sky_tiles(cam, np.stack([far, np.concatenate([c - 1.0, c + 1.0])])).any()                  # ... whatever else there is
        assert pt.sky_tiles(cam, np.zeros((0, 6))).all()
        bad = np.concatenate([c + 50.0, c + 51.0])
        bad[4] = np.nan
        assert not pt.sky_tiles(cam, bad[None, :]).any()                # a NaN clears nothing


def test_more_boxes_than_the_cap_are_their_union(pt):
    rng = np.random.default_rng(5)
    cam, frame = _camera(pt, 64, defocus_angle=1.0, blur_strength=0.5)
    c = np.array(cam.look_from[:])
    lo = c - frame["forward"] * 6.0 + frame["right"] * 3.0 + rng.uniform(-0.5, 0.5, (70, 3))
    boxes = np.concatenate([lo, lo + 0.3], axis=1)
    union = np.concatenate([boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)])[None, :]
    a, b = pt.sky_tiles(cam, boxes), pt.sky_tiles(cam, union)
    assert (a == b).all() and a.any() and not a.all()
    assert (pt.sky_tiles(cam, boxes[:64]) >= a).all()                   # 64 boxes are walked one by one: never fewer tiles than their union clears
