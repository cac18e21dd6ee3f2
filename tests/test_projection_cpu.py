"""Camera projections (pt_scene_set_projection) without a device: the ABI symbols and bindings, the setter's validation,
the CLI's --projection argument, and self-checks of the rule's restatement in tests/camera_rule.py, which the GPU tests compare the
kernels with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_rule as CR
from common import SceneSpec, default_camera

NEW_SYMBOLS = ("pt_scene_set_projection", "pt_scene_projection", "pt_camera_probe")


def test_symbols_and_bindings(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pt.ABI_SYMBOLS and hasattr(pt.lib, sym) and sym + "(" in header, sym
    for method in ("set_projection", "projection", "camera_probe"):
        assert hasattr(pt.Scene, method), method
    assert pt.PROJECTIONS == {"perspective": 0, "orthographic": 1, "fisheye": 2, "panorama": 3} == CR.KINDS
    assert pt.lib.pt_scene_set_projection.argtypes == [C.c_void_p, C.c_int]
    hpp = open(os.path.join(os.path.dirname(pt.__file__), "host", "pt.hpp")).read()
    assert "pt_scene_set_projection(" in hpp and "int projection" in hpp


def test_null_scene_is_refused(pt):
    assert pt.lib.pt_scene_set_projection(None, 1) == -1
    assert b"null scene" in pt.lib.pt_last_error()
    assert pt.lib.pt_scene_projection(None) == 0
    cam = pt.Camera()
    one = (C.c_double * 2)(0.0, 0.0)
    out = (C.c_double * 8)()
    assert pt.lib.pt_camera_probe(None, C.byref(cam), 0, one, 1, out) == -1


# ---- the rule's restatement ----------------------------------------------------------------------------------------------------------
def _camera(pt, **kw):
    spec = SceneSpec()
    spec.camera = default_camera(**kw)
    cam = spec.make_camera(pt.Camera, [])
    frame, h = pt.camera_init(cam)                        # host arithmetic only: no device
    return cam, frame, h


def test_fisheye_180_reaches_90_degrees_at_the_top_edge(pt):
    W = H = 48
    cam, frame, h = _camera(pt, width=W, aspect=1.0, vfov=180.0, defocus_angle=0.0, blur_strength=0.0, look_from=(0.3, 1.0, -2.0), look_at=(0.1, 0.2, 4.0))
    assert h == H
    # blur_strength 0: the ray of pixel (row 0, col W/2) goes through that pixel's centre, half a pixel below the top edge and half a
    # pixel right of the centre column line; the rule is linear in rho, so the edge itself is at th * 1 = 90 degrees exactly
    o, d, t, n = CR.camera_rays("fisheye", frame, h, cam, 5, [W // 2, (H // 2) * W + W // 2], [0, 0], sobol=False)
    xn, yn = 1.0 / H, (H - 1.0) / H
    rho = np.hypot(xn, yn)
    assert abs(np.degrees(np.arccos(-d[0] @ frame["forward"])) - 90.0 * rho) < 1e-12
    assert np.degrees(np.arccos(np.clip(-d[1] @ frame["forward"], -1, 1))) == pytest.approx(90.0 * np.hypot(1.0 / H, 1.0 / H), abs=1e-9)
    # the edge: fy = -0.5 exactly, on the centre line fx = W/2 - 0.5: theta = (pi / 2) * 1
    th = (180.0 * (np.pi / 180.0)) / 2.0
    yn_edge = (H - 2.0 * (-0.5 + 0.5)) / H
    assert yn_edge == 1.0 and np.minimum(yn_edge * th, np.pi) == np.pi / 2.0
    assert abs(d[0] @ frame["up"]) > 0.99 * np.sin(np.radians(90.0 * rho))   # and it points up
    assert n == 5 and (o == np.array([0.3, 1.0, -2.0])).all()


def test_panorama_pixel_centres_are_the_environment_texels(pt):
    W, H = 64, 32
    cam, frame, h = _camera(pt, width=W, aspect=2.0, defocus_angle=0.0, blur_strength=0.0)
    assert h == H
    pixels = np.arange(W * H)
    for sobol in (False, True):
        o, d, t, n = CR.camera_rays("panorama", frame, h, cam, 1, pixels, np.zeros(W * H, dtype=np.int64), sobol=sobol)
        np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, rtol=0.0, atol=4e-16)
        i, j = CR.environment_texel(d, W, H)
        np.testing.assert_array_equal(i, pixels % W)
        np.testing.assert_array_equal(j, pixels // W)
        assert n == 5
    # it does not read look_at, vup or vfov
    cam2, frame2, _ = _camera(pt, width=W, aspect=2.0, defocus_angle=0.0, blur_strength=0.0, look_at=(3.0, -1.0, 2.0), vup=(0.0, 0.0, 1.0), vfov=17.0)
    first = pixels[:64], np.zeros(64, dtype=np.int64)
    d1 = CR.camera_rays("panorama", frame, h, cam, 1, *first, sobol=False)[1]
    d2 = CR.camera_rays("panorama", frame2, h, cam2, 1, *first, sobol=False)[1]
    np.testing.assert_array_equal(d2, d1)


@pytest.mark.parametrize("defocus", [0.0, 2.0])
def test_orthographic_rays_are_parallel(pt, defocus):
    W = 32
    cam, frame, h = _camera(pt, width=W, aspect=4.0 / 3.0, defocus_angle=defocus, blur_strength=0.5)
    pixels = np.repeat(np.arange(W * h), 2)
    samples = np.tile(np.arange(2), W * h)
    o, d, t, n = CR.camera_rays("orthographic", frame, h, cam, (7 << 32) | 3, pixels, samples, sobol=True)
    if defocus == 0.0:
        assert np.abs(d + frame["forward"]).max() < 1e-15
        # origins lie in the plane through the centre, across the forward axis (to the rounding of S + forward * F)
        assert np.abs((o - np.array(cam.look_from[:])) @ frame["forward"]).max() < 1e-14
    else:
        # a lens: the rays of one pixel converge on the focal plane, so they are no longer parallel, but all pass through S
        assert np.abs(d + frame["forward"]).max() > 1e-4
        S = o + d * ((-(o - np.array(cam.look_from[:])) @ frame["forward"] + cam.focal_length) / (-d @ frame["forward"]))[:, None]
        rows, cols = np.divmod(pixels, W)
        on_plane = (S - frame["pixel00"]) @ np.stack([frame["pixel_dv"], frame["pixel_du"]], axis=1) / np.array([frame["pixel_dv"] @ frame["pixel_dv"], frame["pixel_du"] @ frame["pixel_du"]])
        assert np.abs(on_plane[:, 0] - rows).max() <= 0.5 + 1e-9 and np.abs(on_plane[:, 1] - cols).max() <= 0.5 + 1e-9
    # an object at distance F keeps its size: the sample locations S = O - forward * F are kind 0's
    o0, d0, _, _ = CR.camera_rays("perspective", frame, h, cam, (7 << 32) | 3, pixels, samples, sobol=True)
    if defocus == 0.0:
        S1 = o - frame["forward"] * cam.focal_length
        S0 = o0 + d0 * (cam.focal_length / (-d0 @ frame["forward"]))[:, None]
        assert np.abs(S1 - S0).max() < 1e-12


def test_kind0_of_the_restatement_is_the_existing_camera_rule(pt):
    import sampler_rule as R

    W = 16
    cam, frame, h = _camera(pt, width=W, aspect=2.0, defocus_angle=0.0, blur_strength=0.5)
    pixels = np.arange(W * h)
    for sobol in (False, True):
        fy, fx = R.camera_locations(frame, 0.5, W, 11, pixels, np.arange(3), sobol=sobol)
        for s in range(3):
            o, d, t, n = CR.camera_rays(0, frame, h, cam, 11, pixels, np.full(W * h, s), sobol=sobol)
            S = frame["pixel00"] + frame["pixel_dv"] * fy[:, s, None] + frame["pixel_du"] * fx[:, s, None]
            w = S - o
            np.testing.assert_allclose(d, w / np.linalg.norm(w, axis=1)[:, None], rtol=0.0, atol=1e-13)   # libm's cos / sin against the deterministic ones


def test_fisheye_refusal_rule():
    assert not CR.fisheye_refused(48, 48, 180.0)
    assert not CR.fisheye_refused(48, 48, 254.0)           # sqrt(2) * 127 = 179.6 degrees
    assert CR.fisheye_refused(48, 48, 255.0)               # sqrt(2) * 127.5 = 180.3
    assert CR.fisheye_refused(48, 48, 300.0)
    assert CR.fisheye_refused(64, 36, 180.0)               # 16:9: the corner is at 2.04 * 90 degrees
    assert not CR.fisheye_refused(64, 36, 176.0)
    for bad in (0.0, -10.0, float("nan"), float("inf")):
        assert CR.fisheye_refused(48, 48, bad)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def _exe(pt):
    return os.path.join(os.path.dirname(pt.__file__), "pt_render")


@pytest.mark.parametrize("value", ["", "ortho", "Panorama", "2", "fisheye,panorama", "latlong"])
def test_cli_refuses_bad_projection(pt, value):
    # status 2 before any device is opened: this runs on a machine without a GPU
    r = subprocess.run([_exe(pt), "-s", "3", "--projection", value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (value, r.returncode, r.stderr)
    assert "--projection" in r.stderr
    for name in ("perspective", "orthographic", "fisheye", "panorama"):
        assert name in r.stderr


def test_cli_help_lists_the_projection(pt):
    r = subprocess.run([_exe(pt), "--projection"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    r = subprocess.run([_exe(pt), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--projection perspective|orthographic|fisheye|panorama" in r.stdout
