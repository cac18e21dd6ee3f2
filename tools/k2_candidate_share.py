#!/usr/bin/env python3
"""CPU estimate of what K2's candidate list sees on scene 6 (profiles/r27_k2_split.md). Oracle only, no GPU.

k_extend2 keeps the rays of a window that enter a mesh instance's box in a list of half the window; a fuller window walks the rest in
phase A. This tool estimates, from the oracle's per-sample path dumps, how many of the wavefront's rays are such candidates and how they
are spread over tiles:

  * every sample of the frame is traced by trace_sample (seed 1) and cut into its segments;
  * a sample-level model of the sky and short-path passes takes away what never enters the path pool: 8x8 tiles none of whose samples hits
    anything (sky tiles); and, in tiles where at least 9/16 of the samples are camera -> miss or camera -> one diffuse hit -> miss, those
    samples (the short pass's yield rule);
  * a segment is a candidate when it ends on a mesh triangle or crosses the world box of a mesh instance before its hit. The dump holds
    no direction for a path's final miss: the LOWER bound counts such a segment only when it starts inside a mesh's box (it left that
    mesh), the UPPER bound counts every one of them that left a surface;
  * a K2 window is one or two tiles' rays of one bounce (the pool is written in shading order), so "tile x bounce" stands for "window".

    python tools/k2_candidate_share.py [--width 480] [--spp 2] [--seed 1]      prints one JSON line
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# scene 6's mesh instances as host/scenes.cpp everything_scene builds them: (asset, scale, angle about Y, translation), in world order
MESHES = (("bunny.obj", 10.0, 3.14, (0.1, -0.327, 5.0)), ("spot.obj", 0.65, 0.87, (-1.5, 2.8, 4.3)), ("cow.obj", 0.75, 0.93, (2.5, 3.8, 12.0)))
FIRST_MESH_PRIM = 9            # the ground quad, two spheres and the cuboid's six faces come first
SHADEABLE = (0, 3, 4, 5, 6, 7, 8)   # the diffuse quad and cuboid faces: what the short pass can shade
YIELD = 9.0 / 16.0


def _boxes(orc, hits_by_mesh):
    """World boxes of the three instances and their primitive ranges. The turn's sense is the one under which the box holds every hit point
    the oracle reported on that mesh."""
    out, first = [], FIRST_MESH_PRIM
    for k, (name, scale, angle, tr) in enumerate(MESHES):
        P, I, _ = orc.load_obj(os.path.join(orc.ASSET_DIR, name))
        P = P.astype(np.float64) * scale
        n_tris = len(I) // 3
        fits = []
        for sgn in (1.0, -1.0):
            c, s = np.cos(angle), sgn * np.sin(angle)
            Q = np.stack([c * P[:, 0] + s * P[:, 2], P[:, 1], -s * P[:, 0] + c * P[:, 2]], axis=1) + np.array(tr)
            lo, hi = Q.min(axis=0) - 1e-6, Q.max(axis=0) + 1e-6
            h = hits_by_mesh(first, first + n_tris)
            fits.append((bool(((h >= lo) & (h <= hi)).all()), lo, hi))
        ok = [f for f in fits if f[0]]
        assert ok, f"{name}: no sense of the turn holds the oracle's hit points"
        out.append((first, first + n_tris, ok[0][1], ok[0][2]))
        first += n_tris
    return out, first


def _crosses(o, e, lo, hi, unbounded):
    """Segments o -> e (unbounded: rays from o through e) against one box: the f64 slab test."""
    d = e - o
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    par = d == 0.0
    inside = (o >= lo) & (o <= hi)
    near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1)).max(axis=1)
    far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1)).min(axis=1)
    return far >= np.maximum(near, 0.0) if unbounded else (far >= np.maximum(near, 0.0)) & (near <= 1.0)


def estimate(width=480, spp=2, seed=1):
    import oracle_py as orc

    sc = orc.Scene()
    cam = sc.build_scene(6, width, spp)
    frame, height = orc.camera_init(cam)
    n_pix = width * height
    eye = np.array(cam.look_from[:])
    pix, smp, seg, prim, org, end, final = [], [], [], [], [], [], []
    n_segs = np.zeros((n_pix, spp), dtype=np.int64)
    first_prim = np.full((n_pix, spp), -1, dtype=np.int64)
    for p in range(n_pix):
        toward = frame["pixel00"] + frame["pixel_dv"] * (p // width) + frame["pixel_du"] * (p % width)   # the pixel's centre on the focal plane
        for s in range(spp):
            _, rec, n = sc.trace_sample(cam, seed, p, s, 64)
            n_segs[p, s] = n
            o = eye
            for k in range(min(n, 64)):
                hit = rec[k, 0] > 0.0                                 # (the row of a final miss is left at zero: a hit's t is above 1e-3)
                pix.append(p); smp.append(s); seg.append(k); org.append(o); final.append(not hit)
                prim.append(int(rec[k, 1]) if hit else -1)
                end.append(rec[k, 2:5] if hit else (toward if k == 0 else o))   # a final miss after a hit has no known direction
                o = rec[k, 2:5] if hit else o
            if len(rec) and rec[0, 0] > 0.0:
                first_prim[p, s] = int(rec[0, 1])
    pix, smp, seg, prim, final = (np.array(a) for a in (pix, smp, seg, prim, final))
    org, end = np.array(org, dtype=np.float64).reshape(-1, 3), np.array(end, dtype=np.float64).reshape(-1, 3)
    boxes, n_prims = _boxes(orc, lambda a, b: end[(prim >= a) & (prim < b)])
    assert n_prims + 3 == sc.prim_count(), "scene 6's primitive order is not what this tool assumes"
    on_mesh = (prim >= FIRST_MESH_PRIM) & (prim < n_prims)
    known = ~final | (seg == 0)                                       # segments with a direction: hits, and camera rays that miss
    cross = np.zeros(len(pix), dtype=bool)
    starts_in = np.zeros(len(pix), dtype=bool)
    for _, _, lo, hi in boxes:
        cross |= known & _crosses(org, end, lo, hi, False) & ~final
        cross |= final & (seg == 0) & _crosses(org, end, lo, hi, True)
        starts_in |= ((org >= lo) & (org <= hi)).all(axis=1)
    lower = on_mesh | cross | (final & (seg > 0) & starts_in)
    upper = lower | (final & (seg > 0))

    # ---- the sky and short-path passes, per sample
    tiles_x = (width + 7) // 8
    tile_of_pixel = (np.arange(n_pix) // width // 8) * tiles_x + (np.arange(n_pix) % width) // 8
    n_tiles = int(tile_of_pixel.max()) + 1
    hits = np.zeros((n_pix, spp), dtype=np.int64)
    np.add.at(hits, (pix[~final], smp[~final]), 1)
    short = ((n_segs == 1) & (hits == 0)) | ((n_segs == 2) & (hits == 1) & np.isin(first_prim, SHADEABLE))
    per_tile = lambda v: np.bincount(np.repeat(tile_of_pixel, spp), weights=v.reshape(-1).astype(np.float64), minlength=n_tiles)
    n_in_tile = per_tile(np.ones((n_pix, spp)))
    sky_tile = per_tile(hits > 0) == 0
    taken = ~sky_tile & (per_tile(short) >= YIELD * n_in_tile)
    wave = ~sky_tile[tile_of_pixel][:, None] & ~(taken[tile_of_pixel][:, None] & short)   # samples of the path pool
    w = wave[pix, smp]                                                # ... and their segments
    tile = tile_of_pixel[pix]
    out = {"width": width, "height": int(height), "spp": spp, "seed": seed, "samples": int(n_pix * spp),
           "wavefront_share_of_samples": float(wave.mean()), "segments_per_wavefront_sample": float(w.sum() / max(1, wave.sum())),
           "sky_tiles": int(sky_tile.sum()), "short_tiles": int(taken.sum()), "tiles": n_tiles}
    for name, cand in (("lower", lower), ("upper", upper)):
        c = cand & w
        key = tile[w] * 64 + np.minimum(seg[w], 63)                   # tile x bounce: the stand-in for a window
        rays = np.bincount(key, minlength=n_tiles * 64).astype(np.float64)
        cands = np.bincount(key, weights=c[w].astype(np.float64), minlength=n_tiles * 64)
        share = np.divide(cands, rays, out=np.zeros_like(rays), where=rays > 0)
        beyond = np.maximum(0.0, cands - 0.5 * rays).sum()
        out[name] = {"candidate_share_of_segments": float(c.sum() / max(1, w.sum())),
                     "camera_rays_that_are_candidates": float((c & (seg == 0)).sum() / max(1, (w & (seg == 0)).sum())),
                     "segments_in_windows_above_half": float(rays[share > 0.5].sum() / max(1.0, rays.sum())),
                     "rays_beyond_half_of_their_window_of_all_rays": float(beyond / max(1.0, rays.sum())),
                     "rays_beyond_half_of_their_window_of_candidates": float(beyond / max(1.0, cands.sum())),
                     "window_share_histogram_by_segments": [float(rays[(share >= a / 10.0) & ((share < (a + 1) / 10.0) | (a == 9))].sum() / max(1.0, rays.sum()))
                                                            for a in range(10)]}
    sc.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps(estimate(a.width, a.spp, a.seed)))
