"""Host side of cross-faded long-form separation (lass_amd/longform.py): the invariants of
plan_windows_faded, the fade ramps bit for bit, the 5-tuple check, the unchanged 3-tuple planners and the ABI.  No GPU."""
import os
import re

import numpy as np
import pytest

from lass_amd import longform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOTALS = lambda W, context: (W + 1, W + context, 2 * W, 20011, 72011, 9_600_000)  # noqa: E731
# (window, context, fade): a small fade, fade = 2 * context, fade = window - 2 * context (the even number below it for the odd
# window), both bounds at once, and the smallest fade
SHAPES = [(4000, 500, 400), (4000, 500, 1000), (4000, 1500, 1000), (4000, 1000, 2000), (4000, 640, 2),
          (7777, 1111, 1234), (7777, 1111, 2222), (7777, 3000, 1776), (7777, 1000, 2),
          (160000, 16000, 8000), (160000, 16000, 32000), (160000, 40000, 80000)]


def _regions(plan, fade):
    """(begin, end, kind) of every region of the plan in recording coordinates: kind 0 stored, 1 fade-in, 2 fade-out."""
    out = []
    for start, lo, hi, fin, fout in plan:
        in_end, out_begin = longform.fade_regions(lo, hi, fin, fout, fade)
        out += [(start + a, start + b, kind) for a, b, kind in ((lo, in_end, 1), (in_end, out_begin, 0), (out_begin, hi, 2)) if a < b]
    return sorted(out)


@pytest.mark.parametrize("window,context,fade", SHAPES)
def test_plan_invariants(window, context, fade):
    for total in TOTALS(window, context):
        what = (total, window, context, fade)
        plan = longform.plan_windows_faded(total, window, context, fade)
        base = longform.plan_windows(total, window, context)
        assert [p[0] for p in plan] == [p[0] for p in base], what                 # the starts are plan_windows'
        if total <= window:
            assert plan == [(0, 0, total, 0, 0)], what
            continue
        h = fade // 2
        for i, ((start, lo, hi, fin, fout), (_, lo0, hi0)) in enumerate(zip(plan, base)):
            assert 0 <= start <= total - window and 0 <= lo < hi <= window, what   # inside the recording, inside the window
            assert (fin, fout) == (int(i > 0), int(i < len(plan) - 1)), what
            assert (lo, hi) == (lo0 - h * fin, hi0 + h * fout), what               # each seam p became [p - F/2, p + F/2)
            assert hi - lo >= fade * (fin + fout), what                            # the keep holds its fades, uncut
            # real context, away from the recording's ends (this bounds every kept sample, the faded ones among them)
            assert start == 0 or lo >= context - h, what
            assert start + window == total or window - hi >= context - h, what
        # every sample is reached by ONE stored range, or by one fade-out and one fade-in over the SAME `fade` samples: the
        # fade-in reads ramp[n - a], the fade-out ramp[b - 1 - n] = ramp[fade - 1 - (n - a)]
        at, reg, k, zones = 0, _regions(plan, fade), 0, 0
        while k < len(reg):
            a, b, kind = reg[k]
            assert a == at, (what, reg[k])
            if kind == 0:
                k += 1
            else:
                assert (a, b, 2) == reg[k + 1] and kind == 1 and b - a == fade, (what, reg[k], reg[k + 1])
                k, zones = k + 2, zones + 1
            at = b
        assert at == total and zones == len(plan) - 1, what
        longform.check_keeps_faded(plan, window, total, fade)
        for group in longform.group_windows_faded(plan, 16):
            longform.check_keeps_faded(group, window, total, fade)


def test_plan_refuses_bad_fades():
    for fade, word in ((401, "even"), (0, "positive"), (-2, "positive"), (1002, "context"), (3002, "context")):
        with pytest.raises(ValueError, match=word):
            longform.plan_windows_faded(20011, 4000, 500, fade)
    with pytest.raises(ValueError, match="fit"):
        longform.plan_windows_faded(20011, 4000, 1600, 802)     # window - 2 * context = 800
    with pytest.raises(ValueError, match="fit"):
        longform.plan_windows_faded(3000, 4000, 1600, 802)      # ... also where the plan would be a single window
    longform.plan_windows_faded(20011, 4000, 1600, 800)
    with pytest.raises(ValueError):                             # plan_windows' own refusals still come through
        longform.plan_windows_faded(512, 4000, 500, 400)


@pytest.mark.parametrize("fade", [1, 2, 3, 400, 1234, 2048, 8000, 32000])
def test_fade_ramp(fade):
    i = np.arange(fade)
    lin = longform.fade_ramp(fade, "linear")
    want = np.array([np.float32(2 * k + 1) / np.float32(2 * fade) for k in range(fade)], dtype=np.float32)
    assert lin.dtype == np.float32 and lin.shape == (fade,) and lin.tobytes() == want.tobytes()
    exact = (2 * i + 1) / (2.0 * fade)                          # (the quotient of two exact integers, rounded once)
    assert np.array_equal(lin, exact.astype(np.float32))
    han = longform.fade_ramp(fade, "hann")
    want = (np.sin(np.pi * (2 * i + 1).astype(np.float64) / (4.0 * fade)) ** 2).astype(np.float32)
    assert han.dtype == np.float32 and han.shape == (fade,) and han.tobytes() == want.tobytes()
    for name, r in (("linear", lin), ("hann", han)):
        # Strictly inside (0, 1) and strictly increasing wherever float32 can show it.  The Hann ramp's last weights are
        # 1 - (pi (2k + 1) / (4 fade))^2: their distance from 1 and from each other drops below half an ulp of 1 (2^-25)
        # beyond fade ~ 4 500, where the table ends in weights that round to 1.0 - so above 2048 only the order is asserted.
        strict = name == "linear" or fade <= 2048
        assert r[0] > 0 and (r[-1] < 1 if strict else r[-1] <= 1), (name, fade)
        d = np.diff(r.astype(np.float64))
        assert (d > 0).all() if strict else (d >= 0).all(), (name, fade)
        total = r.astype(np.float64) + r[::-1].astype(np.float64)  # complementary about the zone's centre
        assert np.abs(total - 1).max() <= np.spacing(np.float32(1)), (name, fade, np.abs(total - 1).max())
    with pytest.raises(ValueError):
        longform.fade_ramp(fade, "cosine")


def test_fade_ramp_refuses_empty():
    with pytest.raises(ValueError):
        longform.fade_ramp(0)


def test_check_keeps_faded():
    W, total, F = 4000, 20011, 400
    plan = longform.plan_windows_faded(total, W, 500, F)
    assert plan[:2] == [(0, 0, 3700, 0, 1), (3000, 300, 3700, 1, 1)] and plan[-1] == (16011, 2289, 4000, 1, 0)
    longform.check_keeps_faded(plan, W, total, F)
    longform.check_keeps_faded(plan[::2], W, total, F)                                  # gaps are fine
    longform.check_keeps_faded([(0, 0, 0, 1, 1), (0, 0, 0, 0, 0)], W, total, F)         # empty keeps meet nothing
    bad = {
        "two stored ranges": [(0, 0, 3000, 0, 0), (2000, 999, 2000, 0, 0)],
        "a stored range over a fade-in": [(0, 0, 3100, 0, 0), (3000, 0, 1000, 1, 0)],
        "a stored range over a zone": [plan[0], plan[1], (3000, 350, 360, 0, 0)],
        "a third fade-in on a zone": [plan[0], plan[1], (3000, 300, 700, 1, 0)],
        "a third fade-out on a zone": [plan[0], plan[1], (0, 3300, 3700, 0, 1)],
        "two fade-ins": [(3000, 300, 3700, 1, 0), (3000, 300, 700, 1, 0)],
        "a zone of two fade-outs": [(0, 0, 3700, 0, 1), (1000, 2300, 2700, 0, 1)],
        "fades that meet without coinciding": [plan[0], (3000, 301, 3700, 1, 1)],
        "a cut fade-out beside a fade-in": [(0, 3400, 3700, 0, 1), (3000, 400, 3700, 1, 0)],
    }
    for what, rows in bad.items():
        with pytest.raises(ValueError, match="overlap"):
            longform.check_keeps_faded(rows, W, total, F)
        for row in rows:                                                                # (each row alone is fine)
            longform.check_keeps_faded([row], W, total, F)
    with pytest.raises(ValueError, match="start"):
        longform.check_keeps_faded([(total - W + 1, 0, 10, 0, 0)], W, total, F)
    with pytest.raises(ValueError, match="keep"):
        longform.check_keeps_faded([(0, 10, W + 1, 1, 0)], W, total, F)
    for F_bad in (0, W + 1):
        with pytest.raises(ValueError, match="fade length"):
            longform.check_keeps_faded(plan, W, total, F_bad)


def test_fade_regions_are_the_documented_clamp():
    assert longform.fade_regions(100, 900, 1, 1, 300) == (400, 600)
    assert longform.fade_regions(100, 900, 0, 1, 300) == (100, 600)
    assert longform.fade_regions(100, 900, 5, 0, 300) == (400, 900)       # any non-zero flag is set
    assert longform.fade_regions(100, 300, 1, 1, 300) == (300, 300)       # hi - lo < F: the fade-in takes it all
    assert longform.fade_regions(100, 500, 1, 1, 300) == (400, 400)       # ... and cuts the fade-out to the last 100 samples
    assert longform.fade_regions(100, 100, 1, 1, 300) == (100, 100)


def test_group_windows_faded_pads_with_empty_rows():
    plan = longform.plan_windows_faded(20011, 4000, 500, 400)
    groups = longform.group_windows_faded(plan, 4)
    assert [len(g) for g in groups] == [4, 4] and sum(groups, [])[:7] == plan and groups[-1][-1] == (16011, 0, 0, 0, 0)
    assert longform.group_windows_faded(plan, 7) == [plan] and longform.group_windows_faded([], 4) == []
    with pytest.raises(ValueError):
        longform.group_windows_faded(plan, 0)


def test_three_tuple_planners_are_unchanged():
    """Literal outputs of plan_windows / group_windows as they were before the faded siblings existed."""
    a = [(0, 0, 3360), (2720, 640, 3360), (5440, 640, 3360), (8160, 640, 3360), (10880, 640, 3360), (13600, 640, 3360),
         (16011, 949, 4000)]
    assert longform.plan_windows(20011, 4000, 640) == a
    assert longform.group_windows(a, 4) == [a[:4], a[4:] + [(16011, 0, 0)]]
    b = [(0, 0, 6777), (2223, 4554, 7777)]
    assert longform.plan_windows(10000, 7777, 1000, 2048) == b
    assert longform.group_windows(b, 3) == [b + [(2223, 0, 0)]]
    assert longform.plan_windows(3000, 4000, 640) == [(0, 0, 3000)]
    longform.check_keeps(a, 4000, 20011)
    with pytest.raises(ValueError, match="overlap"):
        longform.check_keeps([(0, 0, 3360), (2720, 639, 3360)], 4000, 20011)


def test_header_declares_the_faded_symbols():
    """As tests/test_geometry_cpu.py checks the ABI: declared in the header, bound in _lib.SYMBOLS, exported by the library."""
    import __graft_entry__ as g
    g.build()
    from lass_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    declared = set(re.findall(r"\b(lass_[a-z_0-9]+)\s*\(", hdr))
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name in ("lass_separate_windows_faded", "lass_istft_windows_faded"):
        assert name in declared and name in bound and hasattr(lib, name), name
    # each takes its unfaded sibling's arguments plus fade, ramp and F
    assert len(bound["lass_separate_windows_faded"]) == len(bound["lass_separate_windows"]) + 3
    assert len(bound["lass_istft_windows_faded"]) == len(bound["lass_istft_windows"]) + 3
    assert lib.lass_version() >= 10700
    assert lib.lass_separate_windows_faded(None, None, 0, None, None, None, None, 0, None, None, 0, 0, None, 0, None) < 0
    assert lib.lass_istft_windows_faded(None, None, None, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, None, None) < 0
