"""Host-side planning of long-form separation: which windows of one long recording run through `lass_separate_windows`, and
which part of each window's output is kept.

A recording longer than one forward is cut into overlapping windows of equal length; each window is separated as a clip of its
own (reflect padding at its own two ends) and only its inner part is kept, so that every kept sample has `context` samples of
real audio on each side that is not an end of the recording - overlap-discard, as the reference's chunk_inference does
(models/resunet.py:655-714).  The kept parts tile the recording exactly once, so the windows can be stored straight into one
long output row by the kernels.  The `_faded` siblings blend neighbouring windows over a zone around
each seam instead of switching between them (section 14b).  No torch, no device: plain integer arithmetic."""
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


FadedWindow = Tuple[int, int, int, int, int]  # (start, lo, hi, fade_in, fade_out): a Window whose keep may begin / end with a fade


def fade_regions(lo: int, hi: int, fade_in, fade_out, fade: int) -> Tuple[int, int]:
    """(in_end, out_begin) of a kept range [lo, hi), as lass_separate_windows_faded cuts them: [lo, in_end) fades in with
    ramp[n - lo], [out_begin, hi) fades out with ramp[hi - 1 - n], what lies between is stored plainly."""
    in_end = min(lo + fade, hi) if fade_in else lo
    out_begin = max(hi - fade, in_end) if fade_out else hi
    return in_end, out_begin


def plan_windows_faded(total: int, window: int, context: int, fade: int, n_fft: int = 1024) -> List[FadedWindow]:
    """`plan_windows` with cross-faded seams: [(start, lo, hi, fade_in, fade_out)] with the same starts.  Every seam p, where one
    keep ended and the next began, becomes the zone [p - fade/2, p + fade/2): the left window's hi grows by fade/2 and it fades
    out over its last `fade` kept samples, the right window's lo shrinks by fade/2 and it fades in over its first `fade`.
    ValueError unless fade is even, 0 < fade <= 2 * context (a zone stays inside both windows) and fade <= window - 2 * context
    (a keep holds both of its fades; consecutive zones, one hop apart, do not meet).  That suffices for the last, right-aligned
    window too: a window is appended only while start + window < total, so the last zone ends before `total`, inside the last
    window, whose keep is longer than context + fade/2.  Every faded sample keeps context - fade/2 samples of real audio on each
    side that is not an end of the recording.  total <= window: the single window, no fades."""
    fade, window, context = int(fade), int(window), int(context)
    if fade <= 0 or fade % 2:
        raise ValueError(f"the fade length must be even and positive, not {fade}")
    if fade > 2 * context:
        raise ValueError(f"a fade of {fade} samples reaches beyond the {context} samples of context on each side of a seam")
    if fade > window - 2 * context:
        raise ValueError(f"a fade of {fade} samples does not fit twice into a keep of {window} - 2 * {context} + {fade} samples")
    plan = plan_windows(total, window, context, n_fft)
    h, last = fade // 2, len(plan) - 1
    return [(start, lo - (h if i > 0 else 0), hi + (h if i < last else 0), int(i > 0), int(i < last))
            for i, (start, lo, hi) in enumerate(plan)]


def fade_ramp(fade: int, shape: str = "linear"):
    """The fade-in weights of a zone of `fade` samples, float32, ascending, sampled at the centres of the samples so that
    ramp[i] + ramp[fade - 1 - i] = 1 up to rounding (the fade-out reads the table backwards): amplitude-complementary about
    the zone's centre.
      "linear": float32(2i + 1) / float32(2 fade), one correctly rounded division;
      "hann":   sin^2(pi (2i + 1) / (4 fade)), evaluated in float64 and rounded once.  (Its last weights differ from 1 by about
                (pi / (4 fade))^2: beyond some 4 500 samples that is below float32's resolution and the table ends in 1.0.)"""
    import numpy as np
    fade = int(fade)
    if fade < 1:
        raise ValueError("the fade length must be positive")
    odd = 2 * np.arange(fade, dtype=np.int64) + 1
    if shape == "linear":
        return odd.astype(np.float32) / np.float32(2 * fade)
    if shape == "hann":
        return (np.sin(np.pi * odd.astype(np.float64) / (4.0 * fade)) ** 2).astype(np.float32)
    raise ValueError(f'fade shape must be "linear" or "hann", not {shape!r}')


def group_windows_faded(plan: Sequence[FadedWindow], max_batch: int) -> List[List[FadedWindow]]:
    """`group_windows` for 5-tuples: padding rows are (start, 0, 0, 0, 0)."""
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    groups = [list(plan[at:at + max_batch]) for at in range(0, len(plan), max_batch)]
    if groups:
        start = groups[-1][-1][0]
        groups[-1] += [(start, 0, 0, 0, 0)] * (max_batch - len(groups[-1]))
    return groups


def check_keeps_faded(windows: Sequence[FadedWindow], window: int, total: int, fade: int) -> None:
    """`check_keeps` for 5-tuples - of one call, or of all the calls that stitch one output.  ValueError unless every window lies
    inside the recording, every keep inside its window, 1 <= fade <= window, and: the plainly stored ranges overlap nothing,
    and two fade regions either are disjoint or are ONE zone - the same samples, a fade-out and a fade-in of full length, so
    that their ramp indices are i and fade - 1 - i - which no third region meets."""
    fade = int(fade)
    if not 1 <= fade <= window:
        raise ValueError(f"the fade length {fade} leaves [1, {window}]")
    spans = []  # (begin, end, kind): kind 0 plain, 1 fade-in, 2 fade-out
    for start, lo, hi, fin, fout in windows:
        if not (0 <= start <= total - window):
            raise ValueError(f"window start {start} leaves [0, {total - window}]")
        if not (0 <= lo <= hi <= window):
            raise ValueError(f"keep ({lo}, {hi}) is no range inside a window of {window} samples")
        in_end, out_begin = fade_regions(lo, hi, fin, fout, fade)
        for a, b, kind in ((lo, in_end, 1), (in_end, out_begin, 0), (out_begin, hi, 2)):
            if a < b:
                spans.append((start + a, start + b, kind))
    spans.sort()
    at = 0
    while at < len(spans):
        a, b, kind = spans[at]
        zone = at + 1 < len(spans) and spans[at + 1][:2] == (a, b) and {kind, spans[at + 1][2]} == {1, 2} and b - a == fade
        at += 2 if zone else 1
        if at < len(spans) and spans[at][0] < b:
            what = "a cross-fade zone" if zone else "a fade region" if kind else "a plainly stored range"
            raise ValueError(f"kept ranges overlap at sample {spans[at][0]}: {what} [{a}, {b}) meets another range there")


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
