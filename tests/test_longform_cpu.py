"""Host-side planning of long-form separation (lass_amd/longform.py): the properties of plan_windows and group_windows, and
reference_plan against the reference loop's own ordered writes.  No GPU."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from lass_amd import longform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _triples():
    """200 seeded (total, window, context), with totals just below, at and just above the window and at window + 1."""
    rng = random.Random(4321)
    out = []
    while len(out) < 200:
        window = rng.randint(600, 9000)
        context = rng.randint(0, (window - 1) // 2)
        kind = len(out) % 5
        if kind == 0:
            total = window + rng.choice([-1, 0, 1])
        elif kind == 1:
            total = window + 1
        elif kind == 2:
            total = window + rng.randint(2, 2 * window)
        else:
            total = rng.randint(513, 40 * window)
        if total > 512:
            out.append((total, window, context))
    return out


TRIPLES = _triples()


def test_import_needs_no_torch():
    code = "import sys; import lass_amd.longform; assert 'torch' not in sys.modules, 'torch imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_triples_cover_the_edges():
    assert len(TRIPLES) == 200
    deltas = {t - w for t, w, _ in TRIPLES}
    assert {-1, 0, 1} <= deltas and sum(t == w + 1 for t, w, _ in TRIPLES) >= 40


def test_plan_windows_properties():
    for total, window, context in TRIPLES:
        plan = longform.plan_windows(total, window, context)
        what = (total, window, context)
        if total <= window:
            assert plan == [(0, 0, total)], what
            continue
        assert len(plan) >= 2, what
        cover = np.zeros(total, dtype=np.int32)
        for start, lo, hi in plan:
            assert 0 <= start and start + window <= total, what            # equal length, inside the recording
            assert 0 <= lo < hi <= window, what
            cover[start + lo:start + hi] += 1
            # context: real audio on each side that is not an end of the recording
            assert lo >= context or start + lo == 0, what
            assert window - hi >= context or start + hi == total, what
        assert (cover == 1).all(), what                                   # the keeps tile [0, total) exactly once
        assert [p[0] for p in plan] == sorted({p[0] for p in plan}), what   # distinct, ascending starts
        assert plan[-1][0] == total - window and plan[-1][2] == window and plan[-1][1] >= context, what
        assert plan[0][:2] == (0, 0), what
        hop = window - 2 * context
        assert all(p[0] == k * hop for k, p in enumerate(plan[:-1])), what


def test_plan_windows_window_plus_one():
    assert longform.plan_windows(4001, 4000, 640) == [(0, 0, 3360), (1, 3359, 4000)]
    assert longform.plan_windows(4000, 4000, 640) == [(0, 0, 4000)]
    assert longform.plan_windows(600, 4000, 640) == [(0, 0, 600)]


@pytest.mark.parametrize("max_batch", [1, 2, 8, 16])
def test_group_windows_properties(max_batch):
    for total, window, context in TRIPLES[::4]:
        plan = longform.plan_windows(total, window, context)
        groups = longform.group_windows(plan, max_batch)
        assert len(groups) == -(-len(plan) // max_batch)
        assert all(len(g) == max_batch for g in groups)                   # every group has max_batch rows
        rows = [w for g in groups for w in g]
        assert rows[:len(plan)] == list(plan)                            # the plan, in order ...
        last = plan[-1][0]
        assert all(w[0] == last and w[1] == w[2] for w in rows[len(plan):])   # ... then padding rows with empty keeps
        kept = sorted((s + lo, s + hi) for s, lo, hi in rows if lo < hi)
        assert kept == sorted((s + lo, s + hi) for s, lo, hi in plan)    # the union of keeps is unchanged
        longform.check_keeps(rows, window if total > window else total, total)
    with pytest.raises(ValueError):
        longform.group_windows([(0, 0, 10)], 0)


@pytest.mark.parametrize("length", [160001, 400000, 416000, 1000003])
def test_reference_plan_is_what_the_ordered_writes_leave(length):
    nl, nc, nr = 32000, 96000, 32000
    writes, ranges = longform.reference_plan(length, nl, nc, nr)
    segs = sorted({w[0] for w in writes})
    owner = np.full(length, -1, dtype=np.int64)     # which window wrote here last
    source = np.full(length, -1, dtype=np.int64)    # ... and from which of its samples
    for seg, a, b, src in writes:                   # the reference's writes, in its order
        owner[a:b] = segs.index(seg)
        source[a:b] = np.arange(src, src + b - a)
    want_owner = np.full(length, -1, dtype=np.int64)
    want_source = np.full(length, -1, dtype=np.int64)
    for a, b, lo, hi in ranges:
        assert (want_owner[a + lo:a + hi] == -1).all()   # disjoint
        assert 0 <= lo < hi <= b - a and b <= length
        want_owner[a + lo:a + hi] = segs.index((a, b))
        want_source[a + lo:a + hi] = np.arange(lo, hi)
    assert np.array_equal(owner, want_owner) and np.array_equal(source, want_source)
    assert len(ranges) == len(segs)                      # one contiguous range per distinct window
    assert [r[0] for r in ranges] == sorted(r[0] for r in ranges)
    assert all(b - a == nl + nc + nr for a, b, _, _ in ranges[:-1])   # only the last window may be shorter


def test_reference_plan_geometry_of_the_golden_input():
    _, ranges = longform.reference_plan(400000, 32000, 96000, 32000)
    assert ranges == [(0, 160000, 0, 128000), (96000, 256000, 32000, 128000), (192000, 352000, 32000, 128000),
                      (288000, 400000, 32000, 112000)]


@pytest.mark.parametrize("length", [600, 159999, 160000])
def test_reference_plan_short_input_writes_nothing(length):
    assert longform.reference_plan(length, 32000, 96000, 32000) == ([], [])


def test_value_errors():
    with pytest.raises(ValueError):
        longform.plan_windows(20000, 4000, 2000)       # window <= 2 * context
    with pytest.raises(ValueError):
        longform.plan_windows(20000, 3999, 2000)
    with pytest.raises(ValueError):
        longform.plan_windows(20000, 4000, -1)         # context < 0
    with pytest.raises(ValueError):
        longform.plan_windows(512, 4000, 640)          # total <= n_fft / 2
    with pytest.raises(ValueError):
        longform.plan_windows(1024, 4000, 640, n_fft=2048)
    assert longform.plan_windows(513, 4000, 640) == [(0, 0, 513)]
    assert longform.plan_windows(1025, 4000, 640, n_fft=2048) == [(0, 0, 1025)]


def test_check_keeps():
    longform.check_keeps([(0, 0, 100), (50, 50, 100), (50, 7, 7)], 100, 150)
    with pytest.raises(ValueError, match="overlap"):
        longform.check_keeps([(0, 0, 100), (50, 49, 100)], 100, 150)
    with pytest.raises(ValueError, match="start"):
        longform.check_keeps([(51, 0, 100)], 100, 150)
    with pytest.raises(ValueError, match="keep"):
        longform.check_keeps([(0, 60, 50)], 100, 150)
    with pytest.raises(ValueError, match="keep"):
        longform.check_keeps([(0, 0, 101)], 100, 150)
