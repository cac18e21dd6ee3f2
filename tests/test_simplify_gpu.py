"""Mesh welding and simplification on the GPU (pt_mesh_simplify): the device stage against its host twin, byte for byte, on
every case of test_simplify_cpu.py; at cluster counts around a block of sixteen-lane groups; at corner runs and member runs around a
tile of TSUM (16) and far past it; at a total collapse; past the launch caps; on spot, whose vertices are duplicated along its texcoord
seams; then the result at work: after voxelisation and isosurface extraction, under rays, and on the command line."""
import os
import subprocess

import numpy as np
import pytest

import simplify_rule as S
from test_simplify_cpu import GRIDS, NAMES, OPTIONS, _raw, odd_cases, refusals, same, shape, some_uv

pytestmark = pytest.mark.gpu

RUNS = (1, 15, 16, 17, 32, 33, 5000)


def twin(pt, ctx, pos, idx, uv=None, **kw):
    got = ctx.simplify(pos, idx, uv, **kw)
    same(got, pt.simplify_host(pos, idx, uv, **kw))
    return got


@pytest.mark.parametrize("name", NAMES)
def test_shape_matches_the_twin(pt, ctx, name):
    pos, idx, uv = shape(pt, name)
    for grid_n in GRIDS:
        for kw in OPTIONS:
            for t in (None, uv):
                twin(pt, ctx, pos, idx, t, grid_n=grid_n, **kw)
        twin(pt, ctx, pos, idx, uv, grid_n=grid_n, normals="none")
        twin(pt, ctx, pos, idx, None, cell=0.37, grid_n=grid_n, reg=0.5)
    for kw in (dict(), dict(dedup=False), dict(normals="none")):
        twin(pt, ctx, pos, idx, uv, mode="weld", **kw)


def test_odd_cases_match_the_twin(pt, ctx):
    for label, pos, idx, uv, kw in odd_cases(pt):
        try:
            twin(pt, ctx, pos, idx, uv, **kw)
        except AssertionError as e:
            raise AssertionError(f"{label} {kw}: {e}") from e


def test_flat_grid_matches_the_twin(pt, ctx):
    pos, idx, _, uv = pt.mesh_grid((0.1, 0.2, 0.3), (2.0, 0.5, 0.3), (-0.4, 1.5, 0.8), 20, 17)
    for grid_n in (3, 6):
        twin(pt, ctx, pos, idx, uv, grid_n=grid_n)


@pytest.mark.parametrize("clusters", (1, 63, 64, 65, 257))
def test_cluster_counts(pt, ctx, clusters):
    """A zig-zag strip whose every vertex has a cell of its own: sixteen clusters fill a block of the placement kernel"""
    k = max(clusters, 3)
    i = np.arange(k)
    pos = np.stack([i + 0.25, (i % 2) * 0.3, 0.1 * np.sin(i)], axis=1).astype(np.float32)
    idx = np.stack([i[:-2], i[1:-1], i[2:]], axis=1).reshape(-1).astype(np.uint32)
    cell = 1.0 if clusters > 1 else 1000.0
    for kw in (dict(), dict(placement="mean", dedup=False)):
        got = twin(pt, ctx, pos, idx, some_uv(pos), cell=cell, **kw)
    assert len(got[0]) == (clusters if clusters > 1 else 0)


@pytest.mark.parametrize("run", RUNS)
def test_corner_runs(pt, ctx, run):
    """One vertex in a cell with `run` corners: a fan; beside it a cell whose single vertex has one corner"""
    pos, idx, cell = S.fan(run, 1)
    for kw in (dict(), dict(dedup=False, normals="none")):
        p, i, n, t, m = twin(pt, ctx, pos, idx, some_uv(pos), cell=cell, **kw)
    corners = np.bincount(m[idx])
    assert corners[m[0]] == run and corners[m[-1]] == 1 and np.count_nonzero(m == m[0]) == 1


@pytest.mark.parametrize("run", RUNS)
def test_member_runs(pt, ctx, run):
    pos, idx, cell = S.fan(run, run)
    for kw in (dict(), dict(placement="mean")):
        p, i, n, t, m = twin(pt, ctx, pos, idx, some_uv(pos), cell=cell, **kw)
    assert np.count_nonzero(m == m[0]) == run and np.count_nonzero(m == m[-1]) == 1
    twin(pt, ctx, np.repeat(pos[:1], run + 2, axis=0), np.arange(3 * ((run + 2) // 3), dtype=np.uint32), mode="weld")   # one weld run of that length


def test_total_collapse(pt, ctx):
    pos, idx, uv = shape(pt, "torus")
    for kw in (dict(cell=100.0), dict(cell=100.0, placement="mean", dedup=False, normals="none")):
        got = twin(pt, ctx, pos, idx, uv, **kw)
        assert len(got[0]) == 0 and len(got[1]) == 0 and np.all(got[4] == S.NONE)
    flat = np.repeat(pos[:1], 6, axis=0)
    got = twin(pt, ctx, flat, np.arange(6, dtype=np.uint32), mode="weld")
    assert len(got[0]) == 0 and len(got[1]) == 0


def test_past_the_launch_caps(pt, ctx):
    """A 600 x 600 grid: 720 000 faces and 2.16 M corners, more than 4096 blocks of 256 lanes take in one pass; at grid_n 200 it has more
    than 32 768 clusters, which the placement kernel's 2048 blocks of sixteen groups do not take in one pass either"""
    pos, idx, _, uv = pt.mesh_grid((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 600, 600)
    assert len(idx) == 2160000 > 4096 * 256
    pos = pos.copy()
    pos[:, 2] = (0.001 * np.sin(np.arange(len(pos)) * 0.37)).astype(np.float32)
    p, i, n, t, m = twin(pt, ctx, pos, idx, uv, grid_n=200)
    assert 2048 * 16 < len(p) <= 201 * 201 and len(i) < len(idx) // 4
    twin(pt, ctx, pos, idx, None, mode="weld", normals="none")


def test_twice_the_same_bytes(pt, ctx):
    pos, idx, uv = shape(pt, "torus")
    same(ctx.simplify(pos, idx, uv, grid_n=9), ctx.simplify(pos, idx, uv, grid_n=9))


def test_refusals_on_the_device_path(pt, ctx):
    refusals(pt, ctx.simplify, lambda *a, **k: _raw(pt, *a, host=False, ctx=ctx.handle, **k))
    pos, idx, uv = shape(pt, "octahedron")
    assert _raw(pt, pos, idx, uv, None, host=False, ctx=None) == -1 and "context" in pt.lib.pt_last_error().decode()


# ---- spot: one index per corner attribute pair, so vertices are duplicated along the texcoord seams -------------------------------------
@pytest.fixture(scope="module")
def spot(pt):
    return pt.load_obj_single_index(os.path.join(pt.ASSET_DIR, "spot.obj"))


def boundary_edges(idx):
    use = S.directed_edges(idx)
    return sum(1 for (a, b) in use if (b, a) not in use)


def test_weld_closes_spot(pt, ctx, spot):
    pos, idx = spot[0], spot[1]
    assert boundary_edges(idx) > 0                                              # the seams
    p, i, n, t, m = twin(pt, ctx, pos, idx, mode="weld")
    assert len(p) < len(pos) and len(i) == len(idx)
    S.assert_balanced(i)
    assert boundary_edges(i) == 0
    assert np.array_equal(p[m], pos)
    sub = ctx.subdivide(p, i, levels=1)
    assert boundary_edges(sub[1]) == 0 and len(sub[1]) == 4 * len(i)
    assert boundary_edges(ctx.subdivide(pos, idx, levels=1)[1]) > 0             # what welding is for


# ---- the result at work -----------------------------------------------------------------------------------------------------------------
def test_simplify_after_voxelise_and_isosurface(pt, ctx):
    pos, idx, _ = pt.load_obj(os.path.join(pt.ASSET_DIR, "spot.obj"))
    dims, lo, hi = pt.mesh_fit_grid(pos, 48, 2.0)
    depth = ctx.mesh_sdf(pos, idx, dims, lo, hi)
    ip, ii, _ = ctx.isosurface(depth, lo, hi, iso=0.0, closed=True, outside=float(depth.min()))
    S.assert_balanced(ii)
    p, i, n, t, m = twin(pt, ctx, ip, ii, grid_n=32)
    print(f"{len(ii) // 3} faces in, {len(i) // 3} out; {len(ip)} vertices in, {len(p)} out")
    assert 0 < len(i) < len(ii) // 2
    S.assert_balanced(i)
    gs = pt.Scene(ctx)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.mesh(1.0, p, i, n, None, grey))
    gs.world_build()
    c = 0.5 * (p.astype(np.float64).min(axis=0) + p.astype(np.float64).max(axis=0))
    d = np.random.default_rng(5).normal(size=(1024, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(d), 7))
    rays[:, 0:3], rays[:, 3:6] = c + 10.0 * d, -d
    out = gs.intersect(rays)
    gs.close()
    print(f"hits {int(out[:, 0].sum())} of {len(d)}")
    assert out[:, 0].sum() > 0.9 * len(d)                                       # spot's body surrounds the centre of its bounds


def test_cli_simplify(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    png = tmp_path / "simplified.png"
    r = subprocess.run([exe, "-q", "-s", "6", "--width", "96", "--spp", "2", "--assets", pt.ASSET_DIR, "--simplify", "48", "--out", str(png)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    img = pt.load_png_rgb8(str(png))
    assert img.shape[1] == 96 and img.max() > 0
    bad = tmp_path / "bad.png"
    for flags, text in ((("--simplify", "x"), "GRID_N"), (("--simplify", "0"), "GRID_N"), (("--simplify", "48,median"), "GRID_N")):
        r = subprocess.run([exe, "-q", "-s", "6", "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, *flags, "--out", str(bad)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and text in r.stderr and not bad.exists()
    r = subprocess.run([exe, "-q", "-s", "3", "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, "--simplify", "48", "--out", str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "scene 6" in r.stderr and not bad.exists()
