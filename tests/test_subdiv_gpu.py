"""Loop subdivision on the GPU (pt_mesh_subdivide): the device stage against its host twin, byte for byte, on the shapes
of test_subdiv_cpu.py and at sizes around a wave and a block; then the subdivided mesh at work in a scene (pt_intersect) and on the
command line."""
import os
import subprocess

import numpy as np
import pytest

import subdiv_rule as S
import tess_rule as R
from test_subdiv_cpu import OPTIONS, SHAPES, _raw, refusals, same
from test_tess_gpu import read_pfm

pytestmark = pytest.mark.gpu


def twin(pt, ctx, mesh, **kw):
    pos, idx, uv, crease = mesh
    got = ctx.subdivide(pos, idx, uv, crease, **kw)
    same(got, pt.subdivide_host(pos, idx, uv, crease, **kw))
    return got


@pytest.mark.parametrize("levels", (0, 1, 3))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_matches_the_twin(pt, ctx, name, levels):
    pos, idx, uv, crease = SHAPES[name]
    for kw in OPTIONS.values():
        twin(pt, ctx, (pos, idx, uv, crease), levels=levels, **kw)
    twin(pt, ctx, (pos, idx, None if uv is not None else pos[:, :2] * 0.5, crease), levels=levels, limit=True)


@pytest.mark.parametrize("faces", (63, 64, 65, 255, 256, 257))
def test_strips_around_a_wave_and_a_block(pt, ctx, faces):
    pos, idx, _, uv = R.strip(faces)
    for kw in (dict(levels=1), dict(levels=2, limit=True, corner_deg=100.0), dict(levels=1, crease_deg=10.0, normals="none")):
        got = twin(pt, ctx, (pos, idx, uv, None), **kw)
        assert len(got[1]) == 3 * faces * 4 ** kw["levels"]


@pytest.mark.parametrize("valence", (40, 300))
def test_fans(pt, ctx, valence):
    """The hub's run of `valence` neighbours is walked by a single lane; 300 is longer than a block"""
    for closed in (True, False):
        twin(pt, ctx, S.fan(valence, closed), levels=2, limit=True)


def test_grid_33x31_level_3(pt, ctx):
    pos, idx, _, uv = R.mesh_grid((-1.0, 0.25, 2.0), (2.0, 0.0, 0.5), (0.0, 0.1, -3.0), 33, 31)
    pos = pos.copy()
    pos[:, 1] += (0.1 * np.sin(np.arange(len(pos)) * 0.7)).astype(np.float32)
    got = twin(pt, ctx, (pos, idx, uv, None), levels=3, limit=True, corner_deg=135.0)
    assert len(got[1]) == 3 * 2 * 33 * 31 * 64


def test_cow_level_2(pt, ctx):
    pos, idx, uv = pt.load_obj(os.path.join(pt.ASSET_DIR, "cow.obj"))
    assert np.bincount(idx).max() == 14                                 # closed and manifold: a vertex's corners are as many as its edges
    got = twin(pt, ctx, (pos, idx, None, None), levels=2, limit=True)
    assert len(got[1]) == 3 * 92864


def test_bunny_with_boundary(pt, ctx):
    pos, idx, uv = pt.load_obj(os.path.join(pt.ASSET_DIR, "bunny.obj"))
    twin(pt, ctx, (pos, idx, pos[:, :2].copy(), None), levels=1, crease_deg=60.0, corner_deg=120.0, limit=True)


def test_octahedron_level_7(pt, ctx):
    """2^17 faces out, 393 216 sorted edge slots and as many neighbour pairs at the last level: more than one scan tile and sort pass"""
    pos, idx, uv, crease = SHAPES["octahedron"]
    got = twin(pt, ctx, (pos, idx, None, None), levels=7, limit=True)
    assert len(got[1]) == 3 * 8 * 4 ** 7 and len(got[0]) == 2 + 4 ** 8
    r = np.linalg.norm(got[0].astype(np.float64), axis=1)
    assert r.max() < 1.0 and r.min() > 0.3                              # the limit surface lies inside the cage, and it is round
    assert np.all(np.abs(np.linalg.norm(got[2].astype(np.float64), axis=1) - 1.0) < 1e-6)


def test_non_finite_positions_pass_through(pt, ctx):
    pos, idx, uv, _ = (None if a is None else np.array(a) for a in SHAPES["grid_8x4"])
    pos[5], pos[17, 1], uv[9, 0], uv[21] = np.nan, np.inf, np.nan, (np.inf, -np.inf)
    for kw in (dict(levels=2), dict(levels=2, limit=True, crease_deg=30.0, corner_deg=100.0), dict(levels=0, limit=True)):
        got = twin(pt, ctx, (pos, idx, uv, None), **kw)
        assert not np.isfinite(got[0]).all() and np.isfinite(got[0]).any()
        assert np.all(np.isfinite(got[2])) and np.all(np.abs(got[2]).max(axis=1) > 0)      # never a zero or NaN normal


def test_empty_mesh(pt, ctx):
    none = (np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), None, None)
    lone = (np.ones((2, 3), np.float32), np.zeros(0, np.uint32), np.ones((2, 2), np.float32), None)
    for mesh in (none, lone):
        twin(pt, ctx, mesh, levels=2, limit=True)


def test_twice_the_same_bytes(pt, ctx):
    pos, idx, _, uv = R.strip(257)
    kw = dict(levels=3, limit=True, crease_deg=20.0, corner_deg=90.0)
    same(ctx.subdivide(pos, idx, uv, **kw), ctx.subdivide(pos, idx, uv, **kw))


def test_refusals_on_the_device_path(pt, ctx):
    refusals(pt, ctx.subdivide, lambda *a, **k: _raw(pt, *a, host=False, ctx=ctx.handle, **k))


def test_subdivide_then_displace(pt, ctx):
    """The stage in front of pt_mesh_tessellate: its output is that stage's input"""
    pos, idx, uv, _ = S.fan(12)
    p, i, n, t, _ = ctx.subdivide(pos, idx, uv, levels=2, limit=True)
    img = (0.5 + 0.4 * np.sin(np.arange(48, dtype=np.float32))).reshape(6, 8)
    got = ctx.tessellate(p, i, n, t, levels=1, height=img, scale=0.05)
    want = pt.tessellate_host(p, i, n, t, levels=1, height=img, scale=0.05)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- the result at work: the creased cube through Scene.mesh, world_build and pt_intersect ---------------------------------------------
def test_rays_meet_the_creased_cube(pt, ctx):
    pos, idx, _, crease = S.cube(True)
    p, i, n, _, _ = twin(pt, ctx, (pos, idx, None, crease), levels=3, limit=True)
    gs = pt.Scene(ctx)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.mesh(1.0, p, i, n, None, grey))
    gs.world_build()
    xz = 0.25 + 0.5 * np.random.default_rng(7).random((4096, 2))        # inside [0.25, 0.75]^2: away from the edge vertices, whose normals blend two faces
    y0 = 5.0
    rays = np.zeros((4096, 7))
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 4] = xz[:, 0], y0, xz[:, 1], -1.0
    out = gs.intersect(rays)
    gs.close()
    err_t = np.abs(out[:, 1] - (y0 - 1.0)).max()
    err_n = np.abs(out[:, 12:15] - np.array([0.0, 1.0, 0.0])).max()
    print(f"hits {int(out[:, 0].sum())} of 4096; max |t - plane| {err_t:.3e}, max |shading normal - (0, 1, 0)| {err_n:.3e}")
    assert np.all(out[:, 0] == 1.0)
    assert err_t <= 5e-9
    assert err_n <= 1e-12


# ---- the command line: pt_render -s 6 --subdivide ----------------------------------------------------------------------------------------
def test_cli_subdivide(pt, tmp_path):
    """The subdivided meshes change the pixels whose paths touch bunny, spot or cow, and no others. The mask is rendered, not drawn, as
    test_cli_displace's is: a path's sample depends on the three meshes only if it meets one of them, so the pixels that change when the
    meshes alone change — the cages kept but shaded smooth (plain against CREASE_DEG 0: every edge a crease, so the surface is the
    cage's, with the stage's smooth normals where the plain meshes shade flat), the cages' vertices moved and nothing else (plain
    against LEVELS 0: the limit projection alone), the smooth surface altered (one level against two) — are the pixels some
    light-carrying path of which meets the cages or the smooth surfaces. The second pair is needed at silhouettes: the limit surface
    lies inside its cage, so a pixel between the two outlines changes (cage hit against sky) while one level and two agree there (both
    miss), and flat against smooth normals need not differ for the one path that grazes the cage (measured: 1 such pixel of 698
    changed at this size without the pair, none with it). The masks compare the f32 images exactly; the difference under test is taken
    from the 8-bit images."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = [exe, "-q", "-s", "6", "--width", "96", "--spp", "2", "--assets", pt.ASSET_DIR]

    def render(name, *flags):
        png, pfm = tmp_path / (name + ".png"), tmp_path / (name + ".pfm")
        r = subprocess.run(common + list(flags) + ["--out", str(png), "--out-hdr", str(pfm)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return pt.load_png_rgb8(str(png)), read_pfm(str(pfm))

    plain8, plain = render("plain")
    sub8, sub = render("sub", "--subdivide", "1")
    _, faceted = render("faceted", "--subdivide", "1,0")               # every edge a crease: the cages' own surfaces, four times the faces
    _, moved = render("moved", "--subdivide", "0")                     # no level: the cages with their vertices at the limit positions
    _, other = render("other", "--subdivide", "2")
    assert np.isfinite(sub).all() and sub.max() > 0.0
    changed = (plain8 != sub8).any(axis=2)
    mask = (plain != faceted).any(axis=2) | (plain != moved).any(axis=2) | (sub != other).any(axis=2)
    print(f"{int(changed.sum())} of {changed.size} pixels differ; the mask holds {int(mask.sum())}; outside it {int((changed & ~mask).sum())}")
    assert changed.sum() > 0.01 * changed.size          # the meshes are in view
    assert mask.sum() < mask.size                       # the mask says something: some pixels never meet a mesh
    assert not (changed & ~mask).any()
    again8, _ = render("again", "--subdivide", "1")
    assert np.array_equal(again8, sub8)


def test_cli_subdivide_refusals(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "bad.png"
    for scene, value, text in (("3", "1", "scene 6 only"), ("7", "1", "scene 6 only"), ("6", "x", "LEVELS"), ("6", "1.5", "LEVELS"), ("6", "-1", "LEVELS"),
                               ("6", "1,200", "CREASE_DEG"), ("6", "1,30,-4", "CORNER_DEG"), ("6", "1,2,3,4", "LEVELS"), ("6", "4", "2^19"), ("6", "12", "2^19")):
        r = subprocess.run([exe, "-s", scene, "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, "--subdivide", value, "--out", str(out)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and text in r.stderr, (value, r.stderr)
        assert not out.exists()
