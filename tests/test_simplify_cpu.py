"""Mesh welding and simplification, the host twin (pt_mesh_simplify_host) against the header's rule restated in numpy
(tests/simplify_rule.py), byte for byte: the closed shapes of the voxelisation tests at four grids under every option, unreferenced
vertices, repeated indices, copies of one triangle that cancel by orientation, welding of a mesh taken apart face by face (with -0 / +0
pairs), welding twice, every refusal. Then properties that need no rule: closed stays balanced, flat stays flat, and quadric placement
keeps the edges and corners of a cube that the mean rounds off. No GPU.

The bounds of the cube test are the issue's: quadric within 1e-2 cell of the surface and 0.1 cell of every corner (the prototype: 4.5e-4
and 0.06), the mean more than 0.1 cell off somewhere and further than 0.3 cell from some corner (0.22 and 0.55)."""
import ctypes as C

import numpy as np
import pytest

import simplify_rule as S
from test_sdf_cpu import shapes

GRIDS = (1, 2, 5, 17)
OPTIONS = tuple(dict(placement=p, dedup=d) for p in ("quadric", "mean") for d in (True, False))
NAMES = ("cube", "octahedron", "torus", "sphere")


def same(got, want):
    assert len(got) == len(want) == 5
    for name, g, w in zip(("pos", "idx", "nrm", "uv", "map"), got, want):
        assert (g is None) == (w is None), name
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            a, b = g.reshape(-1), w.reshape(-1)
            bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError(f"{name}: {len(bad)} of {a.size} values differ, first at {bad[0]}: {a[bad[0]]!r} vs {b[bad[0]]!r}")


def some_uv(pos):
    return np.stack([pos[:, 0] * np.float32(0.5) + pos[:, 2], pos[:, 1] - np.float32(0.25)], axis=1).astype(np.float32)


def shape(pt, name):
    pos, idx = shapes(pt)[name][:2]
    return pos, idx, some_uv(pos)


def triangle_copies(k, j):
    """k copies of one triangle (rotated: still even) and j flipped ones among the faces of a tetrahedron far from it"""
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5], [5, 5, 6]], np.float32)
    even, odd = [(0, 1, 2), (1, 2, 0), (2, 0, 1)], [(0, 2, 1), (2, 1, 0), (1, 0, 2)]
    faces = [(3, 5, 4)] + [even[i % 3] for i in range(k)] + [(3, 4, 6)] + [odd[i % 3] for i in range(j)] + [(4, 5, 6), (5, 3, 6)]
    return pos, np.array(faces, np.uint32).reshape(-1)


def exploded_with_zeros(pt):
    """The torus and a cube around the origin's planes, every face with vertices of its own; zero coordinates alternate -0 / +0"""
    tp, ti = shapes(pt)["torus"][:2]
    cp, ci, _ = S.grid_cube(2)
    cp = cp.astype(np.float32) - np.float32(0.5)                         # coordinates -0.5, 0, 0.5
    pos, idx, _ = S.exploded(*_merge((tp, ti), (cp, ci)))
    zero = np.flatnonzero(pos.reshape(-1) == 0)
    assert len(zero) > 20
    flat = pos.reshape(-1).copy()
    flat[zero[::2]] = np.float32(-0.0)
    return flat.reshape(-1, 3), idx


def _merge(*meshes):
    pos, idx, base = [], [], 0
    for p, i in meshes:
        pos.append(np.asarray(p, np.float32))
        idx.append(np.asarray(i, np.uint32) + np.uint32(base))
        base += len(p)
    return np.concatenate(pos), np.concatenate(idx)


_CUBE = {}


def rotated_cube():
    if not _CUBE:
        _CUBE["mesh"] = S.grid_cube(24, S.rotation(0.4, 0.7))
    return _CUBE["mesh"]


def odd_cases(pt):
    """(label, pos, idx, uv, kw): shared with test_simplify_gpu.py"""
    out = []
    pos, idx, uv = shape(pt, "octahedron")
    far = np.array([[100, 100, 100], [-50, 0, 3]], np.float32)
    pos2 = np.concatenate([far[:1], pos[:3], far[1:], pos[3:], far])
    remap = np.array([1, 2, 3, 5, 6, 7], np.uint32)
    for kw in (dict(grid_n=2), dict(grid_n=5, placement="mean"), dict(mode="weld")):
        out.append(("unreferenced", pos2, remap[idx], some_uv(pos2), kw))
    pos, idx, uv = shape(pt, "sphere")
    rep = np.concatenate([idx[:30], np.array([4, 4, 9, 7, 3, 7, 2, 2, 2], np.uint32), idx[30:]])
    for kw in (dict(grid_n=5), dict(grid_n=17, dedup=False), dict(mode="weld"), dict(mode="weld", dedup=False)):
        out.append(("repeated index", pos, rep, uv, kw))
    for k, j in ((1, 1), (3, 1), (1, 3), (2, 2)):
        p, i = triangle_copies(k, j)
        for kw in (dict(mode="weld"), dict(mode="weld", dedup=False), dict(grid_n=8), dict(grid_n=8, dedup=False)):
            out.append((f"copies {k} {j}", p, i, None, kw))
    p, i = exploded_with_zeros(pt)
    out.append(("exploded", p, i, some_uv(p), dict(mode="weld")))
    out.append(("exploded", p, i, None, dict(mode="weld", normals="none")))
    p, i, _ = rotated_cube()
    for cell in (0.13, 0.21):
        for placement in ("quadric", "mean"):
            out.append(("rotated cube", p, i, None, dict(cell=cell, placement=placement)))
    return out


@pytest.mark.parametrize("grid_n", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_shape_matches_rule(pt, name, grid_n):
    pos, idx, uv = shape(pt, name)
    for kw in OPTIONS:
        for t in (None, uv):
            got = pt.simplify_host(pos, idx, t, grid_n=grid_n, **kw)
            same(got, S.simplify(pos, idx, t, grid_n=grid_n, **kw))
            if kw["dedup"]:
                S.assert_balanced(got[1])                                # closed in, closed out
    same(pt.simplify_host(pos, idx, uv, grid_n=grid_n, normals="none"), S.simplify(pos, idx, uv, grid_n=grid_n, normals="none"))
    got = pt.simplify_host(pos, idx, None, cell=0.37, grid_n=grid_n, reg=0.5)
    same(got, S.simplify(pos, idx, None, cell=0.37, grid_n=grid_n, reg=0.5))
    assert len(got[1]) > 0                                               # cell wins over grid_n


def test_odd_cases_match_rule(pt):
    for label, pos, idx, uv, kw in odd_cases(pt):
        try:
            same(pt.simplify_host(pos, idx, uv, **kw), S.simplify(pos, idx, uv, **kw))
        except AssertionError as e:
            raise AssertionError(f"{label} {kw}: {e}") from e


def test_default_options_are_the_wrappers(pt):
    o = pt.SimplifyOpts()
    d = pt.SimplifyOpts(mode=0, cell=2.0, grid_n=3, placement=1, reg=0.5, dedup=False, normals=1)
    assert pt.lib.pt_simplify_opts_default(C.byref(d)) == 0
    assert bytes(o) == bytes(d) and (d.mode, d.cell, d.grid_n, d.placement, d.reg, d.dedup, d.normals) == (1, 0.0, 64, 0, 1e-3, 1, 0)
    assert pt.lib.pt_simplify_opts_default(None) == -1
    pos, idx, uv = shape(pt, "torus")
    same(_raw(pt, pos, idx, uv, None), pt.simplify_host(pos, idx, uv))


def test_unreferenced_vertices_are_dropped(pt):
    pos, idx, uv = shape(pt, "octahedron")
    far = np.array([[100, 100, 100], [-50, 0, 3]], np.float32)
    pos2 = np.concatenate([far[:1], pos[:3], far[1:], pos[3:], far])
    remap = np.array([1, 2, 3, 5, 6, 7], np.uint32)
    for kw in (dict(grid_n=2), dict(mode="weld")):
        a, b = pt.simplify_host(pos, idx, **kw), pt.simplify_host(pos2, remap[idx], **kw)
        same(a[:4] + (a[4],), b[:4] + (b[4][remap],))                       # the bounds ignore them too
        assert np.all(b[4][[0, 4, 8, 9]] == S.NONE)


@pytest.mark.parametrize("k,j", ((1, 1), (3, 1), (1, 3), (2, 2)))
def test_copies_cancel_by_orientation(pt, k, j):
    pos, idx = triangle_copies(k, j)
    tri = idx.reshape(-1, 3)
    first = 1 if k > j else 2 + k                                            # the face index of the first copy of the majority
    want = np.concatenate([tri[:1], tri[first:first + abs(k - j)], tri[1 + k:2 + k], tri[-2:]]) if k >= j else \
        np.concatenate([tri[:1], tri[1 + k:2 + k], tri[first:first + abs(k - j)], tri[-2:]])
    p, i, _, _, m = pt.simplify_host(pos, idx, mode="weld")
    if k == j:
        assert len(p) == 4 and np.all(m[:3] == S.NONE)                         # the triangle's vertices go with it
        assert np.array_equal(i.reshape(-1, 3), want - 3)
    else:
        assert np.array_equal(p, pos) and np.array_equal(i.reshape(-1, 3), want)
    assert len(pt.simplify_host(pos, idx, mode="weld", dedup=False)[1]) == len(idx)


def test_total_collapse_is_an_empty_mesh(pt):
    pos = triangle_copies(2, 2)[0][:3]
    idx = np.array([0, 1, 2, 1, 2, 0, 0, 2, 1, 2, 1, 0], np.uint32)              # two copies and two flipped ones, nothing else
    got = pt.simplify_host(pos, idx, some_uv(pos), mode="weld")
    assert [len(a) for a in got[:4]] == [0, 0, 0, 0] and np.all(got[4] == S.NONE) and got[0].shape == (0, 3)
    same(got, S.simplify(pos, idx, some_uv(pos), mode="weld"))
    got = pt.simplify_host(pos, idx, cell=10.0, dedup=False)                     # one cell holds everything
    assert len(got[0]) == 0 and len(got[1]) == 0
    same(got, S.simplify(pos, idx, cell=10.0, dedup=False))


def test_weld_puts_an_exploded_mesh_together(pt):
    pos, idx = exploded_with_zeros(pt)
    assert np.signbit(pos[pos == 0]).any() and not np.signbit(pos[pos == 0]).all()
    p, i, n, _, m = pt.simplify_host(pos, idx, mode="weld")
    assert len(p) == len(np.unique(pos + np.float32(0.0), axis=0)) < len(pos) // 3
    assert np.array_equal(p[m], pos)                                            # as floats: -0 == +0
    S.assert_balanced(i)
    use = S.directed_edges(i)
    assert set(use.values()) == {1}                                             # a manifold again: every directed edge once
    # welding twice: the second pass is the identity
    again = pt.simplify_host(p, i, mode="weld")
    assert again[0].tobytes() == p.tobytes() and again[1].tobytes() == i.tobytes() and again[2].tobytes() == n.tobytes()
    assert np.array_equal(again[4], np.arange(len(p)))
    t = some_uv(p)
    assert pt.simplify_host(p, i, t, mode="weld")[3].tobytes() == t.tobytes()


def test_flat_stays_flat(pt):
    q, u, v = np.array((0.1, 0.2, 0.3)), np.array((2.0, 0.5, 0.3)), np.array((-0.4, 1.5, 0.8))
    pos, idx, _, uv = pt.mesh_grid(q, u, v, 20, 17)
    normal = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
    for grid_n in (3, 6):
        _, cell = S.grid_of(pos, idx, 0.0, grid_n)
        p, i, n, t, m = pt.simplify_host(pos, idx, uv, grid_n=grid_n)
        off = np.abs((p.astype(np.float64) - q) @ normal)
        print(f"grid_n {grid_n}: {len(i) // 3} of {len(idx) // 3} faces, largest distance to the plane {off.max() / cell:.3e} cell")
        assert 0 < len(i) < len(idx)
        assert off.max() <= 1e-5 * cell


@pytest.mark.parametrize("cell", (0.13, 0.21))
def test_quadric_keeps_features_the_mean_rounds_off(pt, cell):
    pos, idx, rot = rotated_cube()
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64) @ rot.T
    stats = {}
    S.simplify(pos, idx, cell=cell, normals="none", stats=stats)
    worst = {}
    for placement in ("quadric", "mean"):
        p = pt.simplify_host(pos, idx, cell=cell, placement=placement, reg=1e-3)[0].astype(np.float64)
        surface = S.cube_surface_distance(p, rot) / cell
        corner = np.array([np.linalg.norm(p - c, axis=1).min() for c in corners]) / cell
        worst[placement] = (surface.max(), corner.max())
        print(f"cell {cell} {placement}: {len(p)} vertices, largest surface error {surface.max():.3e} cell, worst corner {corner.max():.3f} cell")
    print(f"quadric solves that fell back to the mean: {stats['fallbacks']} of {stats['clusters']}")
    assert worst["quadric"][0] <= 1e-2 and worst["quadric"][1] <= 0.1
    assert worst["mean"][0] > 0.1 and worst["mean"][1] > 0.3


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _raw(pt, pos, idx, uv, opts, host=True, ctx=None, null=(), n_idx=None, n_uv=None):
    """The C call itself; `null`: the output pointers to pass as NULL. -> the five arrays, or the return code when it is not 0"""
    fp, upt = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    o = dict(pos=fp(), n_pos=C.c_uint32(7), idx=upt(), n_idx=C.c_uint32(7), nrm=fp(), uv=fp(), map=upt())
    refs = [None if k in null else C.byref(o[k]) for k in ("pos", "n_pos", "idx", "n_idx", "nrm", "uv", "map")]
    args = (6 if pos is None else len(pos), None if pos is None else pos.ctypes.data, len(idx) if n_idx is None else n_idx, idx.ctypes.data if len(idx) else None,
            (0 if uv is None else len(uv)) if n_uv is None else n_uv, None if uv is None else uv.ctypes.data)
    op = None if opts is None else C.byref(opts)
    rc = pt.lib.pt_mesh_simplify_host(op, *args, *refs) if host else pt.lib.pt_mesh_simplify(ctx, op, *args, *refs)
    if rc != 0:
        assert rc == -1 and not o["pos"] and not o["idx"] and not o["nrm"] and not o["uv"] and not o["map"]
        return rc
    n, m = o["n_pos"].value, o["n_idx"].value
    arr = lambda p, count, k, dt: (np.ctypeslib.as_array(p, (count * k,)).copy().reshape(-1, k) if count else np.zeros((0, k), dt))
    out = (arr(o["pos"], n, 3, np.float32), arr(o["idx"], m, 1, np.uint32).reshape(-1), arr(o["nrm"], n, 3, np.float32) if o["nrm"] else None,
           arr(o["uv"], n, 2, np.float32) if o["uv"] else None, None if "map" in null else arr(o["map"], len(pos), 1, np.uint32).reshape(-1))
    for k in ("pos", "idx", "nrm", "uv", "map"):
        if o[k]:
            pt.lib.pt_free(o[k])
    return out


def refusals(pt, call, raw):
    """call(pos, idx, uv, **kw) raises PtError; raw(pos, idx, uv, opts, **kw) returns -1"""
    pos, idx = shapes(pt)["octahedron"][:2]
    uv = some_uv(pos)

    def refused(text, p=pos, i=idx, t=None, **kw):
        with pytest.raises(pt.PtError, match=text):
            call(p, i, t, **kw)

    refused("multiple of 3", i=idx[:-1])
    refused("multiple of 3", i=idx[:0])
    refused("position index", i=np.concatenate([idx[:-1], [6]]).astype(np.uint32))
    refused("texcoord index", t=uv[:5])
    bad = pos.copy()
    bad[3, 1] = np.inf
    refused("finite", p=bad)
    bad[3, 1] = np.nan
    refused("finite", p=bad, mode="weld")
    t = uv.copy()
    t[2] = (np.nan, np.inf)                                                     # texcoords are data
    assert np.isnan(call(pos, idx, t, mode="weld")[3]).any()
    for kw, text in ((dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(placement=2), "placement"), (dict(dedup=2), "dedup"), (dict(normals=2), "normals"),
                     (dict(cell=-1.0), "cell"), (dict(cell=np.inf), "cell"), (dict(cell=np.nan), "cell"), (dict(grid_n=0), "grid_n"),
                     (dict(reg=1e-7), "reg"), (dict(reg=1.5), "reg"), (dict(reg=np.nan), "reg"), (dict(cell=1e-7), "2\\^21"), (dict(grid_n=1 << 22), "2\\^21")):
        refused(text, **kw)
    call(pos, idx, None, mode="weld", reg=5.0, cell=-1.0, grid_n=0, placement=0)   # mode 0 reads none of them
    call(pos, idx, None, grid_n=(1 << 21) - 1)
    point = np.repeat(pos[:1], 3, axis=0)
    refused("extent", p=point, i=np.array([0, 1, 2], np.uint32))
    refused("extent", p=point, i=np.array([0, 1, 2], np.uint32), cell=0.5)
    assert len(call(point, np.array([0, 1, 2], np.uint32), None, mode="weld")[0]) == 0
    # the C call: NULL pointers
    o = pt.SimplifyOpts()
    for name in ("pos", "n_pos", "idx", "n_idx", "nrm", "uv"):
        assert raw(pos, idx, uv, o, null=(name,)) == -1 and "null output" in pt.lib.pt_last_error().decode()
    got = raw(pos, idx, uv, o, null=("map",))
    assert got[4] is None and got[0].tobytes() == call(pos, idx, uv)[0].tobytes()
    assert raw(None, idx, None, o) == -1 and "null input" in pt.lib.pt_last_error().decode()
    assert raw(pos, idx, None, o, n_uv=6) == -1 and "null input" in pt.lib.pt_last_error().decode()
    assert raw(pos, idx[:0], None, o, n_idx=6) == -1 and "null input" in pt.lib.pt_last_error().decode()


def test_refusals(pt):
    refusals(pt, pt.simplify_host, lambda *a, **k: _raw(pt, *a, **k))


def test_too_many_faces_is_refused_before_the_indices_are_read(pt):
    pos, idx = shapes(pt)["octahedron"][:2]
    assert _raw(pt, pos, idx, None, pt.SimplifyOpts(), n_idx=3 * 0x08000000) == -1 and "too many triangles" in pt.lib.pt_last_error().decode()
