"""Host-side planning of ragged batches: which clips of different lengths may share one `lass_separate_ragged` call.

A clip of L samples has T = 1 + L // hop frames, zero-padded after bn0 to Tp = 32 * ceil(T / 32) (resunet.py:543-548); the
U-Net only ever sees a (Tp, n_fft/2) image.  Clips with the same Tp - the same BUCKET, 32 * hop samples wide: 5120 at hop 160,
10240 at hop 320 - differ only at the two ends of the network (STFT reflection, real rows of x0, kept mask rows, iSTFT trim),
which the per-clip-length kernels handle; so they can share every launch and come out exactly as if separated alone (DESIGN.md
section 13).  Clips of different buckets cannot, and are sorted into separate batches here.  `n_fft` and `hop` are the STFT
geometry of the model that will run the batches (Engine.n_fft, Engine.hop); the defaults are the reference's 16 kHz layout.  No
torch, no device: plain integer arithmetic."""
from __future__ import annotations

from typing import List, Sequence, Tuple

HOP = 160
T_DOWN = 32
BUCKET_SAMPLES = HOP * T_DOWN  # 5120: the default geometry's


def bucket_of(length: int, n_fft: int = 1024, hop: int = HOP) -> int:
    """The bucket of a clip of `length` samples, named by its padded frame count Tp = 32 * ceil((1 + length // hop) / 32)
    = 32 * (length // (32 * hop) + 1).  Lengths <= n_fft / 2 (shorter than the STFT's reflect padding) raise ValueError."""
    length = int(length)
    if length <= n_fft // 2:
        raise ValueError(f"a clip of {length} samples is not longer than the reflect padding (n_fft/2 = {n_fft // 2})")
    return T_DOWN * (length // (int(hop) * T_DOWN) + 1)


def bucket_range(row_length: int, n_fft: int = 1024, hop: int = HOP) -> Tuple[int, int]:
    """(lo, hi): the closed interval of lengths that may share a call whose rows are `row_length` samples long
    (lass_ragged_bucket): lo = max(hop * (Tp - 32), n_fft/2 + 1), hi = row_length."""
    tp = bucket_of(row_length, n_fft, hop)
    return max(int(hop) * (tp - T_DOWN), n_fft // 2 + 1), int(row_length)


def plan_batches(lengths: Sequence[int], max_batch: int, n_fft: int = 1024, hop: int = HOP) -> List[Tuple[List[int], int]]:
    """[(indices, row_length)]: every index of `lengths` exactly once, each batch holding clips of ONE bucket, at most
    `max_batch` of them, row_length = the longest clip of the batch.  Stable: indices ascend inside a batch, a bucket's
    batches follow each other in input order, and buckets come in the order of their first clip."""
    if int(max_batch) < 1:
        raise ValueError("max_batch must be at least 1")
    by_bucket: dict = {}
    for i, n in enumerate(lengths):
        by_bucket.setdefault(bucket_of(n, n_fft, hop), []).append(i)
    plan = []
    for idx in by_bucket.values():
        for at in range(0, len(idx), int(max_batch)):
            part = idx[at:at + int(max_batch)]
            plan.append((part, max(int(lengths[i]) for i in part)))
    return plan
