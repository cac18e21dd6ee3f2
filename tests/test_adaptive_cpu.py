"""Adaptive sampling, host side (no GPU): the round schedule of pt_render_adaptive and its argument checks."""
import ctypes

import pytest


def schedule_py(m, n):
    """include/pt_amd.h: b_0 = 0, b_1 = m/2, b_2 = m, b_{i+1} = min(N, b_i + max(m/2, b_i/2)), integer divisions."""
    b = [0, m // 2, m]
    while b[-1] < n:
        b.append(min(n, b[-1] + max(m // 2, b[-1] // 2)))
    return b


@pytest.mark.parametrize("m,n", [(2, 2), (2, 9), (16, 4000), (64, 100), (7, 7)])
def test_schedule_matches_the_stated_rule(pt, m, n):
    got = pt.adaptive_schedule(m, n)
    assert got == schedule_py(m, n)
    assert got[0] == 0 and got[-1] == n and all(a < b for a, b in zip(got, got[1:]))


def test_schedule_of_the_headline_frame_has_sixteen_rounds(pt):
    assert len(pt.adaptive_schedule(16, 4000)) - 1 == 16


def test_schedule_cap_writes_a_prefix_and_returns_the_full_count(pt):
    full = schedule_py(16, 4000)
    buf = (ctypes.c_uint32 * 5)()
    assert pt.lib.pt_adaptive_schedule(16, 4000, buf, 5) == len(full)
    assert list(buf) == full[:5]
    assert pt.lib.pt_adaptive_schedule(16, 4000, None, 0) == len(full)


@pytest.mark.parametrize("m,n,what", [(1, 8, "min_spp"), (0, 8, "min_spp"), (8, 7, "max_spp")])
def test_schedule_rejects_bad_arguments(pt, m, n, what):
    assert pt.lib.pt_adaptive_schedule(m, n, None, 0) == -1
    assert what in pt.lib.pt_last_error().decode()
    with pytest.raises(pt.PtError, match=what):
        pt.adaptive_schedule(m, n)


def test_adaptive_entry_points_are_declared_and_bound(pt):
    for name in ("pt_render_pixels", "pt_adaptive_schedule", "pt_render_adaptive", "pt_resolve_u8_counts"):
        assert name in pt.ABI_SYMBOLS and hasattr(pt.lib, name)
    # the options struct as the header lays it out: two u32, a double, two u32, a pointer
    assert ctypes.sizeof(pt.AdaptiveOpts) == 32 and pt.AdaptiveOpts.threshold.offset == 8 and pt.AdaptiveOpts.stream.offset == 24
