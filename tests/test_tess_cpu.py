"""Mesh tessellation and displacement, the host twin (pt_mesh_tessellate_host, pt_mesh_grid, pt_height_from_rgb8) against
the header's rule restated in numpy (tests/tess_rule.py). Every comparison is of bytes. No GPU."""
import ctypes as C

import numpy as np
import pytest

import tess_rule as R

SHAPES = R.shapes()
CLOSED = ("tetrahedron", "octahedron")
UP = dict(q=(0.0, 0.0, 0.0), u=(0.0, 0.0, 1.0), v=(1.0, 0.0, 0.0))   # cross(u, v) = (0, 1, 0): a floor in the xz-plane, u along z


def same(got, want):
    assert len(got) == len(want) == 4
    for name, g, w in zip(("pos", "idx", "nrm", "uv"), got, want):
        if w is None:
            assert g is None, f"{name}: expected none"
            continue
        assert g is not None, f"{name}: missing"
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(-1).view(np.uint32) != w.reshape(-1).view(np.uint32)))
            raise AssertionError(f"{name}: {len(bad)} of {g.size} values differ, first at {bad[0]}: {g.reshape(-1)[bad[0]]!r} vs {w.reshape(-1)[bad[0]]!r}")


@pytest.mark.parametrize("levels", (0, 1, 3))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_matches_rule(pt, name, levels):
    same(pt.tessellate_host(*SHAPES[name], levels=levels), R.tessellate(*SHAPES[name], levels=levels))


@pytest.mark.parametrize("normals", ("auto", "keep", "smooth", "none"))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_normal_modes_match_rule(pt, name, normals):
    same(pt.tessellate_host(*SHAPES[name], levels=2, normals=normals), R.tessellate(*SHAPES[name], levels=2, normals=normals))


@pytest.mark.parametrize("nu,nv", ((1, 1), (3, 2), (8, 4)))
def test_mesh_grid_matches_rule(pt, nu, nv):
    q, u, v = (-1.0, 0.25, 2.0), (2.0, 0.0, 0.5), (0.0, 0.1, -3.0)
    got = pt.mesh_grid(q, u, v, nu, nv)
    same(got, R.mesh_grid(q, u, v, nu, nv))
    pos, idx, nrm, uv = got
    assert len(pos) == (nu + 1) * (nv + 1) and len(idx) == 6 * nu * nv
    assert idx[:6].tolist() == [0, 1, nu + 2, 0, nu + 2, nu + 1]


def test_opposite_normals_fall_back_to_the_smaller_index(pt):
    pos, idx, nrm, uv = pt.tessellate_host(*SHAPES["opposite_normals"], levels=1)
    # edges in key order: (0, 1) -> vertex 3, (0, 2) -> 4, (1, 2) -> 5; n0 + n1 = 0
    assert nrm[3].tolist() == [0.0, 0.0, 1.0]
    assert np.all(np.isfinite(nrm)) and np.all(np.abs(nrm).max(axis=1) > 0)


def test_cancelling_face_normals_fall_back(pt):
    pos, idx, nrm, uv = SHAPES["cancelling"]
    kept = pt.tessellate_host(pos, idx, nrm, None, levels=0, normals="smooth")[2]
    assert kept.tobytes() == np.asarray(nrm, np.float32).tobytes()
    bare = pt.tessellate_host(pos, idx, None, None, levels=1, normals="smooth")[2]
    assert np.all(bare == np.array([0, 1, 0], np.float32))


@pytest.mark.parametrize("name", CLOSED)
def test_counts_of_closed_shapes(pt, name):
    pos, idx, nrm, uv = SHAPES[name]
    n, F = len(pos), len(idx) // 3
    for levels in (1, 2, 3):
        E = 3 * F // 2
        p, i, _, _ = pt.tessellate_host(pos, idx, levels=levels)
        n, F = n + E, 4 * F
        assert len(p) == n and len(i) == 3 * F
        tri = i.reshape(-1, 3).astype(np.int64)
        directed = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
        codes = directed[:, 0] * n + directed[:, 1]
        assert len(np.unique(codes)) == len(codes) == 3 * F        # each directed edge once ...
        assert set(codes.tolist()) == set((directed[:, 1] * n + directed[:, 0]).tolist())   # ... and its reverse too: closed
        # the next level's E, from this level's mesh
        assert len(np.unique(np.sort(directed, axis=1), axis=0)) == 3 * F // 2


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_counts(pt, name):
    pos, idx, nrm, uv = SHAPES[name]
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    p, i, _, _ = pt.tessellate_host(pos, idx, levels=1)
    assert len(p) == len(pos) + len(np.unique(edges, axis=0)) and len(i) == 4 * len(np.asarray(idx))
    assert p[: len(pos)].tobytes() == np.asarray(pos, np.float32).tobytes()


def test_constant_image_moves_along_the_normal(pt):
    pos, idx, nrm, uv = pt.mesh_grid(UP["q"], UP["u"], UP["v"], 4, 4)
    assert np.all(nrm == np.array([0, 1, 0], np.float32))
    flat = pt.tessellate_host(pos, idx, nrm, uv, levels=1)
    for wrap in ("clamp", "repeat"):
        p, i, n, t = pt.tessellate_host(pos, idx, nrm, uv, levels=1, height=np.full((4, 8), 0.75, np.float32), scale=2.0, midlevel=0.5, wrap=wrap)
        want = (flat[0].astype(np.float64) + flat[2].astype(np.float64) * (2.0 * (0.75 - 0.5))).astype(np.float32)
        assert p.tobytes() == want.tobytes()
        assert np.all(p[:, 1] == np.float32(0.5))
        assert n.tobytes() == flat[2].tobytes()      # auto = smooth when displacing: a shifted plane keeps N
        assert i.tobytes() == flat[1].tobytes() and t.tobytes() == flat[3].tobytes()


@pytest.mark.parametrize("ti,tj", ((0, 0), (3, 1), (7, 3), (5, 2)))
def test_single_texel_displaces_its_vertex(pt, ti, tj):
    img = np.zeros((4, 8), np.float32)
    img[tj, ti] = 1.0
    pos, idx, nrm, uv = pt.mesh_grid(UP["q"], UP["u"], UP["v"], 16, 8)
    scale = 0.375
    p, _, _, _ = pt.tessellate_host(pos, idx, nrm, uv, levels=0, height=img, scale=scale, midlevel=0.0)
    moved = (p[:, 1] - pos[:, 1]).reshape(9, 17)          # [grid row j (v = j / 8), grid column i (u = i / 16)]
    gi, gj = 2 * ti + 1, 8 - (2 * tj + 1)
    assert uv[gj * 17 + gi].tolist() == [(2 * ti + 1) / 16, 1 - (2 * tj + 1) / 8]
    assert moved[gj, gi] == np.float32(scale)
    jj, ii = np.meshgrid(np.arange(9), np.arange(17), indexing="ij")
    far = (np.abs(ii - gi) >= 4) | (np.abs(jj - gj) >= 4)   # two texels = four grid steps
    assert np.all(moved[far] == 0.0)
    assert np.all(p[:, [0, 2]] == pos[:, [0, 2]])


def test_ramp_clamp_against_repeat(pt):
    img = np.tile(np.array([0.0, 0.25, 0.5, 0.75], np.float32), (2, 1))
    pos, idx, nrm, uv = pt.mesh_grid(UP["q"], UP["u"], UP["v"], 4, 1)
    lift = lambda wrap: pt.tessellate_host(pos, idx, nrm, uv, levels=0, height=img, scale=1.0, midlevel=0.0, wrap=wrap)[0][:, 1].reshape(2, 5)
    clamp, repeat = lift("clamp"), lift("repeat")
    assert np.all(clamp[:, 0] == 0.0) and np.all(clamp[:, 4] == 0.75)           # u = 0 and u = 1: the edge texels
    assert np.all(repeat[:, 0] == 0.375) and np.all(repeat[:, 4] == 0.375)      # halfway between the last texel and the first
    assert np.array_equal(clamp[:, 1:4], repeat[:, 1:4])                        # texel centres inside the image: (0, 0.25, 0.5) + 1/8
    same(pt.tessellate_host(pos, idx, nrm, uv, levels=2, height=img, wrap="repeat"), R.tessellate(pos, idx, nrm, uv, levels=2, height=img, wrap="repeat"))
    far = uv * 3.0 - 1.25                                                        # texcoords outside [0, 1], both signs
    for wrap in ("clamp", "repeat"):
        same(pt.tessellate_host(pos, idx, nrm, far, levels=1, height=img, wrap=wrap), R.tessellate(pos, idx, nrm, far, levels=1, height=img, wrap=wrap))


def test_non_finite_texcoords_do_not_displace(pt):
    pos, idx, nrm, uv = pt.mesh_grid(UP["q"], UP["u"], UP["v"], 4, 4)
    uv = uv.copy()
    uv[3, 0], uv[7, 1], uv[11] = np.nan, np.inf, (-np.inf, np.nan)
    img = np.full((4, 4), 1.0, np.float32)
    p = pt.tessellate_host(pos, idx, nrm, uv, levels=0, height=img, scale=1.0, midlevel=0.0)[0]
    lifted = p[:, 1] - pos[:, 1]
    assert np.all(lifted[[3, 7, 11]] == 0.0) and np.all(np.delete(lifted, [3, 7, 11]) == 1.0)
    img[1, 2] = np.inf                                   # a texel that is not finite: the vertices it reaches stay
    same(pt.tessellate_host(pos, idx, nrm, uv, levels=1, height=img), R.tessellate(pos, idx, nrm, uv, levels=1, height=img))


def test_displacement_matches_rule(pt):
    rng = np.random.default_rng(5)
    img = rng.random((5, 7)).astype(np.float32)
    for name in ("triangle", "three_faces_one_edge", "unreferenced", "grid_3x2", "pair_consistent"):
        for normals in ("auto", "keep", "smooth", "none"):
            kw = dict(levels=2, height=img, scale=0.3, midlevel=0.4, wrap="repeat", normals=normals)
            same(pt.tessellate_host(*SHAPES[name], **kw), R.tessellate(*SHAPES[name], **kw))


def test_height_from_rgb8(pt):
    rng = np.random.default_rng(3)
    rgb = np.concatenate([np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1), rng.integers(0, 256, (512, 3), dtype=np.uint8)]).reshape(24, 32, 3)
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    want = (((0.2126 * r + 0.7152 * g) + 0.0722 * b) / 255.0).astype(np.float32)
    got = pt.height_from_rgb8(rgb)
    assert got.shape == (24, 32) and got.tobytes() == want.tobytes()
    assert got.reshape(-1)[0] == 0.0 and abs(float(got.reshape(-1)[255]) - 1.0) < 1e-6


def _raw(pt, opts, n_pos, pos, idx, outs=None, host=True, ctx=None):
    """pt_mesh_tessellate(_host) with counts and pointers given as they are"""
    o = pt._MeshOut()
    refs = list(o.refs()) if outs is None else outs
    args = (C.byref(opts), n_pos, pos.ctypes.data, len(idx), idx.ctypes.data, 0, None, 0, None, *refs)
    return pt.lib.pt_mesh_tessellate_host(*args) if host else pt.lib.pt_mesh_tessellate(ctx, *args)


def refusals(pt, call, raw):
    """Every refusal of the rule, through `call` (tessellate_host's signature) and `raw` (_raw's)"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    nrm2, uv2 = np.zeros((2, 3), np.float32), np.zeros((2, 2), np.float32)
    uv3, img = np.zeros((3, 2), np.float32), np.zeros((2, 2), np.float32)
    cases = [
        ("multiple of 3", lambda: call(tri, [0, 1, 2, 0])),
        ("position index", lambda: call(tri, [0, 1, 3])),
        ("normal index", lambda: call(tri, [0, 1, 2], nrm2)),
        ("texcoord index", lambda: call(tri, [0, 1, 2], None, uv2)),
        ("needs texcoords", lambda: call(tri, [0, 1, 2], height=img)),
        ("levels", lambda: call(tri, [0, 1, 2], levels=13)),
        ("too many triangles", lambda: call(tri, [0, 1, 2] * 8, levels=12)),
        ("wrap", lambda: call(tri, [0, 1, 2], None, uv3, wrap=2)),
        ("wrap", lambda: call(tri, [0, 1, 2], None, uv3, wrap=-1)),
        ("normals", lambda: call(tri, [0, 1, 2], normals=4)),
        ("normals", lambda: call(tri, [0, 1, 2], normals=-1)),
    ]
    for words, run in cases:
        with pytest.raises(pt.PtError, match=words):
            run()
    idx = np.array([0, 1, 2], np.uint32)
    assert raw(pt.TessOpts(levels=1), 0xFFFFFFFF, tri, idx) == -1          # n + (4^levels - 1) F past 32 bits; the positions are never read
    assert "32 bits" in pt.lib.pt_last_error().decode()
    o = pt._MeshOut()
    for k in range(6):
        refs = list(o.refs())
        refs[k] = None
        assert raw(pt.TessOpts(), 3, tri, idx, outs=refs) == -1
        assert "null output" in pt.lib.pt_last_error().decode()


def test_refusals(pt):
    refusals(pt, pt.tessellate_host, lambda *a, **k: _raw(pt, *a, **k))
    with pytest.raises(pt.PtError):
        pt.mesh_grid((0, 0, 0), (1, 0, 0), (2, 0, 0), 2, 2)      # u x v = 0
    with pytest.raises(pt.PtError):
        pt.mesh_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, 2)


def test_defaults(pt):
    o = pt.TessOpts(levels=7, scale=3.0, midlevel=0.0, wrap="repeat", normals="none")
    assert pt.lib.pt_tess_opts_default(C.byref(o)) == 0
    assert (o.levels, o.height, o.scale, o.midlevel, o.wrap, o.normals) == (1, None, 1.0, 0.5, 0, 0)
    d = pt.TessOpts()
    assert (d.levels, d.height, d.scale, d.midlevel, d.wrap, d.normals) == (1, None, 1.0, 0.5, 0, 0)
