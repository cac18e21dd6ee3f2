"""tools/k2_candidate_share.py — the CPU estimate of K2's candidate-list load on scene 6 (profiles/r27_k2_split.md) — runs
without a device and its figures are sane: shares in [0, 1], the lower bound at or below the upper, and the sample-level model of the sky
and short-path passes leaves about the third of the samples the GPU's statistics report for the path pool (0.33)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARES = ("candidate_share_of_segments", "camera_rays_that_are_candidates", "segments_in_windows_above_half",
          "rays_beyond_half_of_their_window_of_all_rays", "rays_beyond_half_of_their_window_of_candidates")


def test_candidate_share_of_scene6(orc):
    spec = importlib.util.spec_from_file_location("k2_candidate_share", os.path.join(ROOT, "tools", "k2_candidate_share.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.estimate(width=96, spp=1, seed=1)
    print(out)
    assert out["width"] == 96 and out["height"] == 54 and out["samples"] == 96 * 54
    for bound in ("lower", "upper"):
        for k in SHARES:
            assert 0.0 <= out[bound][k] <= 1.0, (bound, k)
        assert abs(sum(out[bound]["window_share_histogram_by_segments"]) - 1.0) < 1e-9
    for k in SHARES[:4]:                                                  # (the last is a ratio of two bounds: not ordered)
        assert out["lower"][k] <= out["upper"][k], k
    assert 0.0 < out["wavefront_share_of_samples"] <= 1.0 and abs(out["wavefront_share_of_samples"] - 0.33) <= 0.15
    assert out["segments_per_wavefront_sample"] >= 1.0
