"""Host-side planning of ragged batches (lass_amd/ragged.py): bucket arithmetic and the properties of plan_batches.  No GPU."""
import os
import random
import re
import subprocess
import sys

import pytest

from lass_amd import ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [513, 5119, 5120, 10239, 10240]


def _length_lists():
    rng = random.Random(1234)
    lists = [EDGES, EDGES[::-1], EDGES * 5, [513], [10240] * 7]
    for _ in range(20):
        n = rng.randint(1, 60)
        lists.append([rng.choice(EDGES) if rng.random() < 0.25 else rng.randint(513, 60000) for _ in range(n)])
    return lists


def test_import_needs_no_torch():
    code = "import sys; import lass_amd.ragged; assert 'torch' not in sys.modules, 'torch imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_bucket_of_is_the_padded_frame_count():
    for L in range(513, 20481):
        assert ragged.bucket_of(L) == 32 * -(-(1 + L // 160) // 32), L
    assert ragged.bucket_of(5119) != ragged.bucket_of(5120) and ragged.bucket_of(10239) != ragged.bucket_of(10240)
    assert ragged.bucket_of(1025, n_fft=2048) == 32


def test_bucket_range_matches_the_header_formula():
    for L in EDGES + [800, 7777, 160000]:
        lo, hi = ragged.bucket_range(L)
        tp = ragged.bucket_of(L)
        assert (lo, hi) == (max(160 * (tp - 32), 513), L)
        assert ragged.bucket_of(lo) == tp and (lo == 513 or ragged.bucket_of(lo - 1) != tp)
    assert ragged.bucket_range(4000, n_fft=2048) == (1025, 4000)


@pytest.mark.parametrize("max_batch", [1, 3, 16])
def test_plan_batches_properties(max_batch):
    for lengths in _length_lists():
        plan = ragged.plan_batches(lengths, max_batch)
        seen = [i for idx, _ in plan for i in idx]
        assert sorted(seen) == list(range(len(lengths)))               # every index exactly once
        first_of_bucket = []
        for idx, row in plan:
            assert 1 <= len(idx) <= max_batch                          # batches respect max_batch
            assert len({ragged.bucket_of(lengths[i]) for i in idx}) == 1   # one bucket per batch
            assert row == max(lengths[i] for i in idx)                 # row_length == max
            assert idx == sorted(idx)                                  # stable inside a batch
            lo, hi = ragged.bucket_range(row)
            assert all(lo <= lengths[i] <= hi for i in idx)
            first_of_bucket.append((ragged.bucket_of(row), idx[0]))
        # stable across batches: a bucket's batches are consecutive and ascend; buckets come in order of their first clip
        per_bucket = {}
        for b, i0 in first_of_bucket:
            per_bucket.setdefault(b, []).append(i0)
        assert [b for b, _ in first_of_bucket] == [b for b in per_bucket for _ in per_bucket[b]]
        assert all(v == sorted(v) for v in per_bucket.values())
        heads = [v[0] for v in per_bucket.values()]
        assert heads == sorted(heads)
        # only a bucket's last batch may be short
        for b in per_bucket:
            sizes = [len(idx) for idx, row in plan if ragged.bucket_of(row) == b]
            assert all(s == max_batch for s in sizes[:-1])


def test_short_clips_raise():
    for L in (0, 1, 512):
        with pytest.raises(ValueError):
            ragged.bucket_of(L)
        with pytest.raises(ValueError):
            ragged.plan_batches([4000, L], 4)
    with pytest.raises(ValueError):
        ragged.bucket_of(1024, n_fft=2048)
    with pytest.raises(ValueError):
        ragged.plan_batches([4000, 1024], 4, n_fft=2048)
    with pytest.raises(ValueError):
        ragged.plan_batches([4000], 0)
    assert ragged.plan_batches([], 4) == []


def test_ragged_entry_points_declared_and_bound():
    """The four new entry points are in the header and in _lib.SYMBOLS with matching argument counts."""
    from lass_amd import _lib
    header = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    bound = {name: args for name, _res, args in _lib.SYMBOLS}
    for name in ("lass_separate_ragged", "lass_front_end_ragged", "lass_istft_ragged", "lass_ragged_bucket"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(bound[name]), name
