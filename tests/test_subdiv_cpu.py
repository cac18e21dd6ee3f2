"""Loop subdivision, the host twin (pt_mesh_subdivide_host) against the header's rule restated in numpy
(tests/subdiv_rule.py), byte for byte, and against properties that need no rule: counts, the bounding box, linear precision on a flat
grid, the creased cube, chaining through out_crease. No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import subdiv_rule as S
import tess_rule as R


def _shapes():
    out = {name: (pos, idx, uv, None) for name, (pos, idx, nrm, uv) in R.shapes().items()}
    out["cube_flagged"] = S.cube(True)
    out["cube_plain"] = S.cube(False)
    out["fan_40"] = S.fan(40)
    out["fan_40_open"] = S.fan(40, closed=False)
    pos, idx, uv, _ = out["pair_consistent"]
    out["pair_one_side_flagged"] = (pos, idx, uv, np.array([0, 0, 1, 0, 0, 0], np.uint8))     # the shared edge, flagged in face 0 only
    return out


SHAPES = _shapes()
# crease_deg / corner_deg as the wrappers take them; the rule file takes the cosines the wrappers make of them
OPTIONS = {
    "plain": dict(),
    "limit": dict(limit=True),
    "no_normals": dict(normals="none"),
    "angles": dict(crease_deg=40.0, corner_deg=100.0),
    "angles_limit": dict(crease_deg=75.0, corner_deg=135.0, limit=True, normals="none"),
}


def rule_kw(kw):
    kw = dict(kw)
    crease, corner = kw.pop("crease_deg", None), kw.pop("corner_deg", None)
    kw["crease_cos"] = -2.0 if crease is None else math.cos(math.radians(crease))
    kw["corner_cos"] = 2.0 if corner is None else math.cos(math.radians(corner))
    return kw


def same(got, want):
    assert len(got) == len(want) == 5
    for name, g, w in zip(("pos", "idx", "nrm", "uv", "crease"), got, want):
        if w is None:
            assert g is None, f"{name}: expected none"
            continue
        assert g is not None, f"{name}: missing"
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        if g.tobytes() != w.tobytes():
            view = np.uint8 if g.dtype == np.uint8 else np.uint32
            bad = np.flatnonzero(g.reshape(-1).view(view) != w.reshape(-1).view(view))
            raise AssertionError(f"{name}: {len(bad)} of {g.size} values differ, first at {bad[0]}: {g.reshape(-1)[bad[0]]!r} vs {w.reshape(-1)[bad[0]]!r}")


def against_rule(pt, mesh, **kw):
    pos, idx, uv, crease = mesh
    same(pt.subdivide_host(pos, idx, uv, crease, **kw), S.subdivide(pos, idx, uv, crease, **rule_kw(kw)))


@pytest.mark.parametrize("levels", (0, 1, 3))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_matches_rule(pt, name, levels):
    pos, idx, uv, crease = SHAPES[name]
    for kw in OPTIONS.values():
        against_rule(pt, (pos, idx, uv, crease), levels=levels, **kw)
    if uv is not None:
        against_rule(pt, (pos, idx, None, crease), levels=levels, limit=True)
    else:
        against_rule(pt, (pos, idx, pos[:, :2] * 0.5, crease), levels=levels, limit=True)


@pytest.fixture(scope="module")
def bunny(pt):
    pos, idx, uv = pt.load_obj(os.path.join(pt.ASSET_DIR, "bunny.obj"))
    return pos, idx


@pytest.mark.parametrize("levels,kw", ((0, "limit"), (1, "plain"), (1, "angles_limit"), (3, "limit")))
def test_bunny_matches_rule(pt, bunny, levels, kw):
    pos, idx = bunny
    tri = np.sort(idx.reshape(-1, 3).astype(np.int64), axis=1)
    edges = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [0, 2]]])
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 1).sum() == 42                                   # the boundary edges that make this the boundary case
    against_rule(pt, (pos, idx, pos[:, :2].copy(), None), levels=levels, **OPTIONS[kw])


# ---- checks that need no rule -----------------------------------------------------------------------------------------------------------
def edge_count(idx):
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    return np.unique(edges, axis=0, return_counts=True)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_counts_and_indices(pt, name):
    pos, idx, uv, crease = SHAPES[name]
    n, F = len(pos), len(idx) // 3
    E = len(edge_count(idx)[0])
    p, i, nr, t, cr = pt.subdivide_host(pos, idx, uv, crease, levels=1)
    assert len(p) == n + E and len(i) == 12 * F and len(cr) == 12 * F and nr.shape == p.shape
    assert set(np.unique(cr).tolist()) <= {0, 1}
    for levels in (0, 1, 3):
        got = pt.subdivide_host(pos, idx, uv, crease, levels=levels)
        assert got[1].tobytes() == pt.tessellate_host(pos, idx, levels=levels)[1].tobytes()
        assert len(got[4]) == len(got[1])
    # V - E + F of the referenced part is unchanged by a level: E' = 2E + 3F. (Two faces on the same three vertices share their three
    # inner edges, and a face (a, a, b) has fewer than three: the count holds for every shape but "cancelling" and "face_aab".)
    used = len(np.unique(np.asarray(idx)))
    E1 = len(edge_count(i)[0])
    faces = np.sort(np.asarray(idx, np.int64).reshape(-1, 3), axis=1)
    if len(np.unique(faces, axis=0)) == F and np.all(faces[:, 0] != faces[:, 1]) and np.all(faces[:, 1] != faces[:, 2]):
        assert E1 == 2 * E + 3 * F and used - E + F == (used + E) - E1 + 4 * F
    else:
        assert name in ("cancelling", "face_aab") and E1 < 2 * E + 3 * F


@pytest.mark.parametrize("asset", ("cow.obj", "spot.obj"))
def test_closed_meshes_stay_closed(pt, asset):
    pos, idx, uv = pt.load_obj(os.path.join(pt.ASSET_DIR, asset))
    assert np.all(edge_count(idx)[1] == 2)
    p, i, _, _, cr = pt.subdivide_host(pos, idx, levels=1, limit=True, normals="none")
    keys, counts = edge_count(i)
    assert np.all(counts == 2) and len(p) == len(pos) + 3 * len(idx) // 6 and not cr.any()
    assert len(p) - len(keys) + len(i) // 3 == len(pos) - 3 * len(idx) // 6 + len(idx) // 3


@pytest.mark.parametrize("limit", (False, True))
@pytest.mark.parametrize("levels", (1, 2))
def test_bunny_stays_inside_its_bounding_box(pt, bunny, levels, limit):
    """Every mask is a convex combination (weights >= 0 that sum to 1 up to rounding) and rounding to f32 is monotone"""
    pos, idx = bunny
    p = pt.subdivide_host(pos, idx, levels=levels, limit=limit, normals="none")[0]
    assert np.all(p >= pos.min(axis=0)) and np.all(p <= pos.max(axis=0))


def test_linear_precision_on_a_flat_grid(pt):
    pos, idx, _, uv = R.mesh_grid((0.0, 0.0, 0.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), 6, 6)     # integer coordinates, y = 0
    assert np.all(pos == np.round(pos))
    p, i, nrm, t, cr = pt.subdivide_host(pos, idx, uv, levels=3, corner_deg=135.0)
    assert p[: len(pos)].tobytes() == pos.tobytes()                    # the old vertices come back unchanged
    assert np.all(p * 8 == np.round(p * 8)) and np.all(p[:, 1] == 0.0)
    assert p.min() >= 0.0 and p.max() <= 6.0
    # its normals: the grid's winding decides the sign, every one the same axis
    assert np.all(np.abs(nrm[:, 1]) == 1.0) and np.all(nrm[:, [0, 2]] == 0.0)
    rounded = pt.subdivide_host(pos, idx, uv, levels=1)[0]             # without a corner angle the corners are crease vertices
    assert rounded[0].tolist() == [0.125, 0.0, 0.125]


def test_creased_cube(pt):
    pos, idx, _, crease = S.cube(True)
    p, i, _, _, cr = pt.subdivide_host(pos, idx, None, crease, levels=4, normals="none")
    assert p[:8].tobytes() == pos.tobytes()                            # s = 3: corners
    assert p.min() == 0.0 and p.max() == 1.0
    assert np.all(((p == 0.0) | (p == 1.0)).any(axis=1))               # every vertex lies on a face of the cube
    assert cr.sum() == 12 * 2 * 2 ** 4                                 # 12 edges of 16 segments, flagged on both sides
    q = pt.subdivide_host(pos, idx, levels=4, normals="none")[0]
    assert q.min() > 0.0 and q.max() < 1.0 and np.all(q.min(axis=0) > 0.0) and np.all(q.max(axis=0) < 1.0)


def test_crease_angle_finds_the_cube_edges(pt):
    pos, idx, _, crease = S.cube(True)
    for kw in (dict(levels=0), dict(levels=2, limit=True)):
        same(pt.subdivide_host(pos, idx, crease_deg=45.0, **kw), pt.subdivide_host(pos, idx, None, crease, **kw))


def test_one_sided_flag_is_carried_by_both_sides(pt):
    pos, idx, uv, crease = SHAPES["pair_one_side_flagged"]
    both = np.array([0, 0, 1, 1, 0, 0], np.uint8)                      # edge (0, 2): e2 of face 0 and e0 of face 1
    a, b = pt.subdivide_host(pos, idx, uv, crease, levels=2), pt.subdivide_host(pos, idx, uv, both, levels=2)
    same(a, b)
    first = pt.subdivide_host(pos, idx, uv, crease, levels=1)[4].reshape(-1, 3)
    assert first[[0, 4]].tolist() == [[0, 0, 1], [1, 0, 0]]            # child 0 of face 0 keeps e2, child 0 of face 1 keeps e0


@pytest.mark.parametrize("name", ("cube_flagged", "fan_40_open", "grid_3x2", "three_faces_one_edge", "octahedron"))
def test_chaining_through_out_crease(pt, name):
    pos, idx, uv, crease = SHAPES[name]
    for limit in (False, True):
        for normals in ("smooth", "none"):
            whole = pt.subdivide_host(pos, idx, uv, crease, levels=3, crease_deg=50.0, corner_deg=120.0, limit=limit, normals=normals)
            p, i, _, t, cr = pt.subdivide_host(pos, idx, uv, crease, levels=1, crease_deg=50.0, corner_deg=120.0, normals="none")
            same(pt.subdivide_host(p, i, t, cr, levels=2, corner_deg=120.0, limit=limit, normals=normals), whole)


def test_non_finite_positions_are_data(pt):
    pos, idx, uv, _ = (None if a is None else np.array(a) for a in SHAPES["grid_8x4"])
    pos[5], pos[17, 1], uv[9, 0] = np.nan, np.inf, -np.inf
    against_rule(pt, (pos, idx, uv, None), levels=2, limit=True, crease_deg=30.0, corner_deg=100.0)
    p = pt.subdivide_host(pos, idx, uv, levels=2)[0]
    assert np.isfinite(p).any() and not np.isfinite(p).all()


def _raw(pt, opts, n_pos, pos, idx, outs=None, host=True, ctx=None, uv=None, n_uv=0, crease=None, want_crease=True, n_idx=None):
    """pt_mesh_subdivide(_host) with counts and pointers given as they are (n_idx: the count to pass; default len(idx))"""
    o, flags = pt._MeshOut(), C.POINTER(C.c_uint8)()
    refs = list(o.refs()) if outs is None else outs
    n_idx = (0 if idx is None else len(idx)) if n_idx is None else n_idx
    args = (None if opts is None else C.byref(opts), n_pos, None if pos is None else pos.ctypes.data, n_idx, None if idx is None or not len(idx) else idx.ctypes.data,
            n_uv, None if uv is None else uv.ctypes.data, None if crease is None else crease.ctypes.data, *refs, C.byref(flags) if want_crease else None)
    rc = pt.lib.pt_mesh_subdivide_host(*args) if host else pt.lib.pt_mesh_subdivide(ctx, *args)
    if rc == 0:
        o.free()
        pt.lib.pt_free(flags)
    else:
        assert not (o.pos or o.idx or o.nrm or o.uv or flags)          # a refused call leaves nothing behind
    return rc


def refusals(pt, call, raw):
    """Every refusal of the rule, through `call` (subdivide_host's signature) and `raw` (_raw's)"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    uv2 = np.zeros((2, 2), np.float32)
    cases = [
        ("multiple of 3", lambda: call(tri, [0, 1, 2, 0])),
        ("position index", lambda: call(tri, [0, 1, 3])),
        ("texcoord index", lambda: call(tri, [0, 1, 2], uv2)),
        ("levels", lambda: call(tri, [0, 1, 2], levels=13)),
        ("too many triangles", lambda: call(tri, [0, 1, 2] * 8, levels=12)),
        ("NaN", lambda: call(tri, [0, 1, 2], crease_deg=float("nan"))),
        ("NaN", lambda: call(tri, [0, 1, 2], corner_deg=float("nan"))),
        ("normals", lambda: call(tri, [0, 1, 2], normals=2)),
        ("normals", lambda: call(tri, [0, 1, 2], normals=-1)),
        ("limit", lambda: call(tri, [0, 1, 2], limit=2)),
        ("limit", lambda: call(tri, [0, 1, 2], limit=-1)),
    ]
    for words, run in cases:
        with pytest.raises(pt.PtError, match=words):
            run()
    with pytest.raises(ValueError):
        call(tri, [0, 1, 2], None, [1, 0])                              # a crease array of the wrong length never reaches the library
    idx = np.array([0, 1, 2], np.uint32)
    err = lambda: pt.lib.pt_last_error().decode()
    assert raw(pt.SubdivOpts(levels=1), 0xFFFFFFFF, tri, idx) == -1     # n + (4^levels - 1) F past 32 bits; the positions are never read
    assert "32 bits" in err()
    assert raw(pt.SubdivOpts(), 3, None, idx) == -1 and "null input" in err()
    assert raw(pt.SubdivOpts(), 3, tri, idx, n_uv=3) == -1 and "null input" in err()
    assert raw(pt.SubdivOpts(), 3, tri, None, n_idx=3) == -1 and "null input" in err()
    empty = np.zeros(0, np.uint32)
    assert raw(pt.SubdivOpts(), 3, tri, empty) == 0 and raw(pt.SubdivOpts(), 0, None, empty) == 0   # counts of 0 need no arrays
    o = pt._MeshOut()
    for k in range(6):
        refs = list(o.refs())
        refs[k] = None
        assert raw(pt.SubdivOpts(), 3, tri, idx, outs=refs) == -1
        assert "null output" in err()
    assert raw(pt.SubdivOpts(), 3, tri, idx, want_crease=False) == 0    # out_crease alone may be NULL
    assert raw(None, 3, tri, idx) == 0                                  # NULL options: the defaults


def test_refusals(pt):
    refusals(pt, pt.subdivide_host, lambda *a, **k: _raw(pt, *a, **k))


def test_defaults(pt):
    o = pt.SubdivOpts(levels=7, crease_cos=0.5, corner_cos=0.25, limit=1, normals="none")
    assert pt.lib.pt_subdiv_opts_default(C.byref(o)) == 0
    assert (o.levels, o.crease_cos, o.corner_cos, o.limit, o.normals) == (1, -2.0, 2.0, 0, 0)
    d = pt.SubdivOpts()
    assert (d.levels, d.crease_cos, d.corner_cos, d.limit, d.normals) == (1, -2.0, 2.0, 0, 0)
    assert pt.lib.pt_subdiv_opts_default(None) == -1
