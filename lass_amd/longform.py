"""Host-side planning of long-form separation: which windows of one long recording run through `lass_separate_windows`, and
which part of each window's output is kept.

A recording longer than one forward is cut into overlapping windows of equal length; each window is separated as a clip of its
own (reflect padding at its own two ends) and only its inner part is kept, so that every kept sample has `context` samples of
real audio on each side that is not an end of the recording - overlap-discard, as the reference's chunk_inference does
(models/resunet.py:655-714).  The kept parts tile the recording exactly once, so the windows can be stored straight into one
long output row by the kernels.  No torch, no device: plain integer arithmetic."""
from __future__ import annotations

from typing import List, Sequence, Tuple

Window = Tuple[int, int, int]  # (start, lo, hi): recording[start : start + W], of whose output [lo, hi) is kept


def plan_windows(total: int, window: int, context: int, n_fft: int = 1024) -> List[Window]:
    """[(start, lo, hi)] for a recording of `total` samples: windows of `window` samples, hop = window - 2 * context apart
    while start + window < total, and a last one right-aligned at total - window.  The first keeps [0, window - context), the
    middle ones [context, window - context), the last from where the previous keep ended to its end (lo >= context).  All
    windows have the same length and lie inside the recording; the kept ranges tile [0, total) exactly once.
    total <= window: the single window (0, 0, total), of length `total`."""
    total, window, context = int(total), int(window), int(context)
    if context < 0:
        raise ValueError("context must not be negative")
    if window <= 2 * context:
        raise ValueError(f"a window of {window} samples keeps nothing with {context} samples of context on each side")
    if total <= n_fft // 2:
        raise ValueError(f"a recording of {total} samples is not longer than the reflect padding (n_fft/2 = {n_fft // 2})")
    if total <= window:
        return [(0, 0, total)]
    hop = window - 2 * context
    plan: List[Window] = []
    start = 0
    while start + window < total:
        plan.append((start, context if start else 0, window - context))
        start += hop
    kept = plan[-1][0] + plan[-1][2]  # where the previous keep ended
    last = total - window
    plan.append((last, kept - last, window))
    return plan


def group_windows(plan: Sequence[Window], max_batch: int) -> List[List[Window]]:
    """Groups of exactly `max_batch` windows, in order; the last group is padded by repeating its last window with an empty
    keep (lo == hi: such a row stores nothing), so every group of a recording has one shape - and one graph key."""
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    groups = [list(plan[at:at + max_batch]) for at in range(0, len(plan), max_batch)]
    if groups:
        start = groups[-1][-1][0]
        groups[-1] += [(start, 0, 0)] * (max_batch - len(groups[-1]))
    return groups


def check_keeps(windows: Sequence[Window], window: int, total: int) -> None:
    """ValueError unless every window lies inside the recording, every keep inside its window, and the kept ranges of the
    call are disjoint (the two half-batches store from two streams)."""
    spans = []
    for start, lo, hi in windows:
        if not (0 <= start <= total - window):
            raise ValueError(f"window start {start} leaves [0, {total - window}]")
        if not (0 <= lo <= hi <= window):
            raise ValueError(f"keep ({lo}, {hi}) is no range inside a window of {window} samples")
        if lo < hi:
            spans.append((start + lo, start + hi))
    spans.sort()
    for (_, e0), (s1, _) in zip(spans, spans[1:]):
        if s1 < e0:
            raise ValueError(f"kept ranges overlap at sample {s1}")


def reference_plan(length: int, nl: int, nc: int, nr: int):
    """The reference's chunk loop (models/resunet.py:655-714) for an input of `length` samples with nl / nc / nr samples of left
    context, centre and right context.  Returns (writes, ranges):
      writes - the loop's writes in its own order: ((seg_start, seg_stop), dst_start, dst_stop, src_start), meaning
               out[dst_start:dst_stop] = separate(input[seg_start:seg_stop])[src_start : src_start + dst_stop - dst_start];
      ranges - the same list reduced to what survives (a later write wins): (seg_start, seg_stop, lo, hi), disjoint, ascending,
               meaning out[seg_start + lo : seg_start + hi] = separate(input[seg_start:seg_stop])[lo:hi].
    Every distinct window ends up with ONE contiguous range (asserted).  length <= nl + nc + nr: no writes."""
    length, nl, nc, nr = int(length), int(nl), int(nc), int(nr)
    window = nl + nc + nr
    writes = []
    idx = 0
    while idx + window < length:
        seg = (idx, idx + window)
        if idx == 0:
            writes.append((seg, idx, idx + window - nr, 0))
        else:
            writes.append((seg, idx + nl, idx + window - nr, nl))
        idx += nc
        if idx < length:
            seg = (idx, min(idx + window, length))
            writes.append((seg, idx + nl, seg[1], nl))
    pieces: list = []  # disjoint (a, b, seg)
    for seg, a, b, src in writes:
        assert src == a - seg[0] and seg[0] <= a <= b <= seg[1]
        cut = []
        for x, y, s in pieces:
            if x < min(y, a):
                cut.append((x, min(y, a), s))
            if max(x, b) < y:
                cut.append((max(x, b), y, s))
        if a < b:
            cut.append((a, b, seg))
        pieces = cut
    pieces.sort()
    merged: list = []
    for a, b, seg in pieces:
        if merged and merged[-1][2] == seg and merged[-1][1] == a:
            merged[-1] = (merged[-1][0], b, seg)
        else:
            merged.append((a, b, seg))
    assert len({seg for _, _, seg in merged}) == len(merged), "a window's surviving writes are not one contiguous range"
    ranges = [(seg[0], seg[1], a - seg[0], b - seg[0]) for a, b, seg in merged]
    return writes, ranges
