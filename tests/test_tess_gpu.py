"""Mesh tessellation and displacement on the GPU (pt_mesh_tessellate): the device stage against its host twin, byte for
byte, on the shapes of test_tess_cpu.py and at sizes around a block, a wave and a scan tile; then the tessellated mesh at work in a
scene (pt_intersect) and on the command line."""
import os
import subprocess

import numpy as np
import pytest

import tess_rule as R
from test_tess_cpu import SHAPES, UP, _raw, refusals, same

pytestmark = pytest.mark.gpu


def smooth_image(w, h, seed=0):
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    return (0.5 + 0.25 * np.sin(2 * np.pi * (2 * x + 0.1 * seed)) * np.cos(2 * np.pi * 1.5 * y) + 0.2 * np.sin(2 * np.pi * (x + y))).astype(np.float32)


@pytest.mark.parametrize("levels", (0, 1, 3))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_matches_the_twin(pt, ctx, name, levels):
    same(ctx.tessellate(*SHAPES[name], levels=levels), pt.tessellate_host(*SHAPES[name], levels=levels))
    same(ctx.tessellate(*SHAPES[name], levels=levels, normals="smooth"), pt.tessellate_host(*SHAPES[name], levels=levels, normals="smooth"))


@pytest.mark.parametrize("faces", (85, 86, 341, 342))
def test_strips_around_a_block_and_a_wave(pt, ctx, faces):
    """3 * faces = 255 / 258 / 1023 / 1026 edge slots: one short of and just past a 256-lane block's multiple"""
    mesh = R.strip(faces)
    img = smooth_image(8, 4)
    for kw in (dict(levels=1), dict(levels=2, height=img, scale=0.1), dict(levels=1, normals="smooth")):
        got = ctx.tessellate(*mesh, **kw)
        same(got, pt.tessellate_host(*mesh, **kw))
        assert len(got[1]) == 3 * faces * 4 ** kw["levels"]


def test_octahedron_level_8(pt, ctx):
    """2^19 faces and 1.5 M sorted pairs at the last level: more than one scan tile and sort pass"""
    got = ctx.tessellate(*SHAPES["octahedron"], levels=8, normals="smooth")
    assert len(got[1]) == 3 * 8 * 4 ** 8 and len(got[0]) == 2 + 4 ** 9       # V = F / 2 + 2 on a closed genus-0 mesh
    same(got, pt.tessellate_host(*SHAPES["octahedron"], levels=8, normals="smooth"))
    assert np.all(np.isfinite(got[2])) and np.all(np.abs(np.linalg.norm(got[2].astype(np.float64), axis=1) - 1.0) < 1e-6)


def test_grid_64_level_3_displaced(pt, ctx):
    mesh = pt.mesh_grid(UP["q"], UP["u"], UP["v"], 64, 64)
    kw = dict(levels=3, height=smooth_image(32, 32), scale=0.05, midlevel=0.5, normals="smooth")
    got = ctx.tessellate(*mesh, **kw)
    assert len(got[1]) == 3 * 524288 and len(got[0]) == 513 * 513
    same(got, pt.tessellate_host(*mesh, **kw))
    assert got[0][:, 1].max() > 0.01 and got[0][:, 1].min() < -0.01


def test_modes_wraps_and_attributes(pt, ctx):
    img = smooth_image(7, 5, seed=3)
    pos, idx, nrm, uv = SHAPES["grid_3x2"]
    far = uv * 3.0 - 1.25
    for normals in ("auto", "keep", "smooth", "none"):
        for wrap in ("clamp", "repeat"):
            for n_in in (nrm, None):
                kw = dict(levels=2, height=img, scale=0.3, midlevel=0.4, wrap=wrap, normals=normals)
                same(ctx.tessellate(pos, idx, n_in, far, **kw), pt.tessellate_host(pos, idx, n_in, far, **kw))
        for n_in in (nrm, None):
            for t_in in (uv, None):
                same(ctx.tessellate(pos, idx, n_in, t_in, levels=2, normals=normals), pt.tessellate_host(pos, idx, n_in, t_in, levels=2, normals=normals))
    for name in ("three_faces_one_edge", "unreferenced", "triangle", "pair_consistent"):
        kw = dict(levels=3, height=img, scale=0.2, wrap="repeat")
        same(ctx.tessellate(*SHAPES[name], **kw), pt.tessellate_host(*SHAPES[name], **kw))


def test_non_finite_data_passes_through(pt, ctx):
    pos, idx, nrm, uv = (a.copy() for a in SHAPES["grid_8x4"])
    pos[5], pos[17, 1] = np.nan, np.inf
    uv[9, 0], uv[21] = np.nan, (np.inf, -np.inf)
    img = smooth_image(6, 6)
    img[2, 3] = np.inf
    for normals in ("keep", "smooth"):
        kw = dict(levels=2, height=img, scale=0.2, normals=normals)
        same(ctx.tessellate(pos, idx, nrm, uv, **kw), pt.tessellate_host(pos, idx, nrm, uv, **kw))
    got = ctx.tessellate(pos, idx, None, uv, levels=1, height=img, normals="smooth")[2]
    assert np.all(np.isfinite(got)) and np.all(np.abs(got).max(axis=1) > 0)      # never a zero or NaN normal


def test_twice_the_same_bytes(ctx):
    mesh = R.strip(342)
    kw = dict(levels=4, height=smooth_image(16, 16), scale=0.1, wrap="repeat")
    same(ctx.tessellate(*mesh, **kw), ctx.tessellate(*mesh, **kw))


def test_refusals_on_the_device_path(pt, ctx):
    refusals(pt, ctx.tessellate, lambda *a, **k: _raw(pt, *a, host=False, ctx=ctx.handle, **k))


def test_empty_mesh(pt, ctx):
    none = (np.zeros((0, 3), np.float32), np.zeros(0, np.uint32))
    lone = (np.ones((2, 3), np.float32), np.zeros(0, np.uint32))
    for mesh in (none, lone):
        same(ctx.tessellate(*mesh, levels=2, normals="smooth"), pt.tessellate_host(*mesh, levels=2, normals="smooth"))


# ---- the result at work: a displaced floor through Scene.mesh, world_build and pt_intersect -------------------------------------------
def test_rays_meet_the_displaced_surface(pt, ctx):
    q, u, v = (-2.0, 0.0, -2.0), (0.0, 0.0, 4.0), (4.0, 0.0, 0.0)                # N = (0, 1, 0): a height field over the xz-plane
    grid = pt.mesh_grid(q, u, v, 31, 31)
    # height amplitude 0.1 over wavelengths of 2 and more scene units: slopes stay below 0.4
    kw = dict(levels=2, height=smooth_image(64, 64), scale=0.2, midlevel=0.5)
    pos, idx, nrm, uv = ctx.tessellate(*grid, **kw)
    same((pos, idx, nrm, uv), pt.tessellate_host(*grid, **kw))
    tri = idx.reshape(-1, 3)
    assert len(tri) == 30752
    gs = pt.Scene(ctx)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.mesh(1.0, pos, idx, nrm, uv, grey))
    gs.world_build()
    pick = np.random.default_rng(11).choice(len(tri), 4096, replace=False)
    P = pos.astype(np.float64)[tri[pick]]                                          # (4096, 3 corners, xyz)
    c = P.mean(axis=1)
    y0 = 5.0
    rays = np.zeros((4096, 7))
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 4] = c[:, 0], y0, c[:, 2], -1.0
    out = gs.intersect(rays)
    gs.close()
    # barycentrics of (c.x, c.z) in the triangle's projection, then everything as the blend of the twin's corner values
    e1, e2, d = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], rays[:, :3] - P[:, 0]
    det = e1[:, 0] * e2[:, 2] - e1[:, 2] * e2[:, 0]
    bu = (d[:, 0] * e2[:, 2] - d[:, 2] * e2[:, 0]) / det
    bv = (e1[:, 0] * d[:, 2] - e1[:, 2] * d[:, 0]) / det
    w = np.stack([1.0 - bu - bv, bu, bv], axis=1)
    height = (w * P[:, :, 1]).sum(axis=1)
    blend_n = (w[:, :, None] * nrm.astype(np.float64)[tri[pick]]).sum(axis=1)
    blend_n /= np.linalg.norm(blend_n, axis=1, keepdims=True)
    blend_t = (w[:, :, None] * uv.astype(np.float64)[tri[pick]]).sum(axis=1)
    err_t = np.abs(out[:, 1] - (y0 - height)).max()
    err_n = np.abs(out[:, 12:15] - blend_n).max()
    err_uv = np.abs(out[:, 3:5] - blend_t).max()
    print(f"hits {int(out[:, 0].sum())} of 4096; max |t - plane| {err_t:.3e}, max |shading normal - blend| {err_n:.3e}, max |uv - blend| {err_uv:.3e}")
    assert np.all(out[:, 0] == 1.0)
    assert err_t <= 1e-9 * y0
    assert err_n <= 1e-12
    assert err_uv <= 1e-12


# ---- the command line: pt_render -s 7 --displace ------------------------------------------------------------------------------------------
def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(x) for x in f.readline().split())
        assert float(f.readline()) < 0.0                       # little-endian
        return np.frombuffer(f.read(), dtype="<f4").reshape(h, w, 3)[::-1]


def test_cli_displace(pt, tmp_path):
    """The displaced wall changes the pixels whose paths touch the wall and no others. The mask is rendered, not drawn: a path's sample depends
    on the wall only if it meets the wall, so the pixels that change when the wall alone changes — its normal map dropped on the flat wall
    (plain against scale 0), its relief altered (scale 8 against scale 7.5) — are the pixels some light-carrying path of which meets the flat
    or the displaced wall. The masks compare the f32 images exactly; the difference under test is taken from the 8-bit images."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = [exe, "-q", "-s", "7", "--width", "96", "--spp", "2", "--assets", pt.ASSET_DIR]

    def render(name, *flags):
        png, pfm = tmp_path / (name + ".png"), tmp_path / (name + ".pfm")
        r = subprocess.run(common + list(flags) + ["--out", str(png), "--out-hdr", str(pfm)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return pt.load_png_rgb8(str(png)), read_pfm(str(pfm))

    plain8, plain = render("plain")
    disp8, disp = render("disp", "--displace", "assets/bricks/color.png,8")
    _, flat = render("flat", "--displace", "assets/bricks/color.png,0")
    _, other = render("other", "--displace", "assets/bricks/color.png,7.5")
    assert np.isfinite(disp).all() and disp.max() > 0.0
    changed = (plain8 != disp8).any(axis=2)
    mask = (plain != flat).any(axis=2) | (disp != other).any(axis=2)
    print(f"{int(changed.sum())} of {changed.size} pixels differ; the mask holds {int(mask.sum())}; outside it {int((changed & ~mask).sum())}")
    assert changed.sum() > 0.02 * changed.size          # the wall is in view and is lit
    assert mask.sum() < mask.size                       # the mask says something: some pixels never meet the wall
    assert not (changed & ~mask).any()
    # LEVELS and MIDLEVEL are read; the same command twice gives the same image
    a8, _ = render("a", "--displace", "assets/bricks/color.png,8,1,0.25")
    b8, _ = render("b", "--displace", "assets/bricks/color.png,8,1,0.25")
    assert np.array_equal(a8, b8) and (a8 != disp8).any()


def test_cli_displace_refusals(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "bad.png"
    for scene, value, text in (("3", "assets/bricks/color.png,8", "scene 7 only"), ("7", "assets/bricks/color.png", "FILE,SCALE"), ("7", "assets/bricks/color.png,x", "FILE,SCALE"),
                               ("7", "assets/bricks/color.png,8,13", "LEVELS"), ("7", "assets/bricks/color.png,8,1.5", "LEVELS"), ("7", "no/such/file.png,8", "--displace")):
        r = subprocess.run([exe, "-s", scene, "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, "--displace", value, "--out", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and text in r.stderr, (value, r.stderr)
        assert not out.exists()
