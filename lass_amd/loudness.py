"""Programme loudness, host side: the K-weighting filter design, the float64 definition of the gated ITU-R BS.1770-4 integrated
loudness that the device meter (csrc/loudness.hip) is held to, and the scalar gain rule of the levelled export.

Nothing of this is ported: the reference measures with `pyloudnorm` (data/waveform_mixers.py) and applies `utils.loudness`'s
gain by hand; the meter here is written from the recommendation.  Its pins are the EBU Tech 3341 tones (tests/test_loudness_cpu.py)
and, for the kernels, this module.

K-weighting is two biquads: a high shelf (+4 dB above 1.5 kHz) and a high-pass (the RLB curve, 38 Hz).  The recommendation
tabulates them at 48 kHz only; `k_weighting` redesigns both for the rate asked from the analogue prototypes behind that table,
with the audio-EQ-cookbook bilinear forms (shelf: G = 4 dB, Q = 1/sqrt 2, fc = 1500 Hz; high-pass: Q = 0.5, fc = 38 Hz).  At
48 kHz they differ from the table in the fourth digit, which is 0.04 LU on the EBU tones.

The cascade runs in direct form II transposed with zero initial state,

    y1 = b0 x + z1;  z1 = b1 x - a1 y1 + z2;  z2 = b2 x - a2 y1          (stage 1, then the same on y1 for stage 2)

which is a 4-state affine recurrence s[n+1] = M s[n] + v x[n].  Both this module and the kernels cut the time axis into chunks,
run every chunk from a zero state, carry the true states over the chunk ends with a power of M, and add each chunk's response
to its true initial state - here with numpy over all chunks at once, because a Python loop over millions of samples is not an
option.  In float64 the split changes the result by rounding only (1e-15 relative).

The second half of the module is what an EBU R 128 delivery is checked against beside the integrated loudness, again written
from the recommendations (BS.1770-4 Annex 2, EBU Tech 3341 and 3342) and pinned by their test signals (tests/test_r128_cpu.py):
`true_peak` with its `oversampling`, `short_term_powers`, `loudness_range`, `max_momentary` and `max_short_term` - the float64
definitions of `lass_resample_true_peak` (csrc/export.hip) and `lass_loudness_stats` (csrc/loudness.hip); DESIGN.md section 19.

The last part is the look-ahead limiter of the levelled export (`limit` and its pieces: `limiter_envelope`, `limiter_window`,
`reach`), the float64 definition of `lass_limit` (csrc/limiter.hip): one gain curve per recording, linked across the channels,
that holds gain x envelope under the ceiling so that the ceiling stops costing loudness; DESIGN.md section 20.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

ABSOLUTE_GATE = -70.0     # LUFS
RELATIVE_GATE = -10.0     # LU under the absolute-gated loudness
OFFSET = -0.691


def k_weighting(rate: int):
    """((b, a) of the high shelf, (b, a) of the high-pass) for `rate`, float64 arrays of 3 with a[0] == 1."""
    rate = int(rate)
    if rate % 10 != 0 or rate < 8000:
        raise ValueError("the meter needs a rate of at least 8000 Hz that is a multiple of 10 (100 ms hops of whole samples)")

    def shelf(gain_db, q, fc):
        A = 10.0 ** (gain_db / 40.0)
        w0 = 2.0 * np.pi * fc / rate
        alpha, c = np.sin(w0) / (2.0 * q), np.cos(w0)
        s = 2.0 * np.sqrt(A) * alpha
        b = np.array([A * ((A + 1) + (A - 1) * c + s), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - s)])
        a = np.array([(A + 1) - (A - 1) * c + s, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - s])
        return b / a[0], a / a[0]

    def highpass(q, fc):
        w0 = 2.0 * np.pi * fc / rate
        alpha, c = np.sin(w0) / (2.0 * q), np.cos(w0)
        b = np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2])
        a = np.array([1 + alpha, -2 * c, 1 - alpha])
        return b / a[0], a / a[0]

    return shelf(4.0, 1.0 / np.sqrt(2.0), 1500.0), highpass(0.5, 38.0)


def coefficients(rate: int) -> np.ndarray:
    """`k_weighting(rate)` as the ten float64 the C-ABI takes: b0 b1 b2 a1 a2 of stage 1, then of stage 2."""
    (b1, a1), (b2, a2) = k_weighting(rate)
    return np.array([b1[0], b1[1], b1[2], a1[1], a1[2], b2[0], b2[1], b2[2], a2[1], a2[2]], dtype=np.float64)


def _biquad(x: np.ndarray, b, a, chunk: int) -> np.ndarray:
    """One stage over the last axis of x (P, N), in x's dtype, the time axis cut into chunks of `chunk` samples."""
    dt = x.dtype.type
    b0, b1, b2, a1, a2 = dt(b[0]), dt(b[1]), dt(b[2]), dt(a[1]), dt(a[2])
    P, N = x.shape
    K = max(1, min(int(chunk), N))
    nc = -(-N // K)
    xp = np.zeros((P, nc * K), dtype=x.dtype)
    xp[:, :N] = x
    xp = xp.reshape(P, nc, K)
    y = np.empty_like(xp)
    z1, z2 = np.zeros((P, nc), dtype=x.dtype), np.zeros((P, nc), dtype=x.dtype)
    for k in range(K):                                  # every chunk from a zero state, all chunks at once
        xk = xp[:, :, k]
        yk = b0 * xk + z1
        z1 = b1 * xk - a1 * yk + z2
        z2 = b2 * xk - a2 * yk
        y[:, :, k] = yk
    if nc > 1:
        # the response of a chunk to its initial state: outputs R (K, 2) and end state E (2, 2), from the unit states
        R, u1, u2 = np.empty((K, 2), dtype=x.dtype), np.array([1, 0], dtype=x.dtype), np.array([0, 1], dtype=x.dtype)
        for k in range(K):
            R[k] = u1
            u1, u2 = -a1 * R[k] + u2, -a2 * R[k]
        E = np.stack([u1, u2])
        s = np.zeros((P, 2), dtype=x.dtype)
        S0 = np.empty((P, nc, 2), dtype=x.dtype)
        for j in range(nc):                             # the carry: one short serial pass
            S0[:, j] = s
            s = s @ E.T + np.stack([z1[:, j], z2[:, j]], axis=1)
        y += np.einsum("pjs,ks->pjk", S0, R)
    return y.reshape(P, nc * K)[:, :N]


def k_weighted(x, rate: int, dtype=np.float64, chunk: Optional[int] = None) -> np.ndarray:
    """The K-weighted signal of x (C, N) or (N,), zero initial state, evaluated in `dtype` (signal, coefficients, state).  chunk:
    samples per chunk of the split evaluation (module docstring); the default is about sqrt(N) in float64 and the whole signal -
    the plain sample-by-sample recurrence - in any other dtype."""
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=dtype)
    one = x.ndim == 1
    y = np.atleast_2d(x)
    if y.shape[1] == 0:
        return x.copy()
    if chunk is None:
        chunk = max(256, int(np.sqrt(y.shape[1]))) if dtype == np.float64 else y.shape[1]
    for b, a in k_weighting(rate):
        y = _biquad(y, b, a, chunk)
    return y[0] if one else y


def n_blocks(n: int, rate: int) -> int:
    """Whole 400 ms blocks, 100 ms apart, in n samples."""
    H = int(rate) // 10
    return (int(n) - 4 * H) // H + 1 if n >= 4 * H else 0


def powers_of_weighted(y, rate: int, weights=None, dtype=np.float64) -> np.ndarray:
    """(nb,) channel-weighted mean squares of an already K-weighted y (C, N) over blocks of T = 4H samples, H = rate // 10 apart,
    whole blocks only."""
    y = np.atleast_2d(np.asarray(y, dtype=dtype))
    C, N = y.shape
    H = int(rate) // 10
    nb = n_blocks(N, rate)
    w = np.ones(C, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype).reshape(C)
    p = np.zeros(nb, dtype=dtype)
    if nb:
        idx = np.arange(nb)[:, None] * H + np.arange(4 * H)[None, :]
        for c in range(C):
            p += w[c] * np.mean(np.square(y[c][idx]), axis=1, dtype=dtype)
    return p


def block_powers(x, rate: int, weights=None, dtype=np.float64) -> np.ndarray:
    """(nb,) block powers of x (C, N): `powers_of_weighted` of `k_weighted(x)`, everything in `dtype`."""
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    k_weighting(rate)                                   # (the refusals, also for a signal too short to be filtered)
    if n_blocks(x.shape[1], rate) == 0:
        return np.zeros(0, dtype=dtype)
    return powers_of_weighted(k_weighted(x, rate, dtype), rate, weights, dtype)


def gate(p: np.ndarray) -> Tuple[float, int]:
    """(integrated loudness, blocks that pass both gates) of block powers p; (-inf, 0) when none passes."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = OFFSET + 10.0 * np.log10(p)
        keep = l > ABSOLUTE_GATE
        if not keep.any():
            return float("-inf"), 0
        rel = OFFSET + 10.0 * np.log10(np.mean(p[keep])) + RELATIVE_GATE
        keep &= l > rel
        if not keep.any():
            return float("-inf"), 0
        return float(OFFSET + 10.0 * np.log10(np.mean(p[keep]))), int(np.count_nonzero(keep))


def integrated_loudness(x, rate: int, weights=None) -> float:
    """Gated integrated loudness of x (C, N) in LUFS (BS.1770-4: 400 ms blocks at 75 % overlap, absolute gate -70 LUFS, relative
    gate -10 LU); -inf when no block survives (shorter than one block, silent)."""
    return gate(block_powers(x, rate, weights))[0]


# ---- EBU R 128: true peak, short-term and momentary maxima, loudness range -----------------------------
RANGE_GATE = -20.0        # LU under the absolute-gated short-term loudness (EBU Tech 3342)
SHORT_TERM_BINS = 30      # a 3 s short-term block in 100 ms hop bins


def oversampling(rate: int) -> int:
    """The true-peak meter's oversampling factor: 4 up to 48 kHz, 2 at 88.2 and 96 kHz, 1 (the sample peak) from 176.4 kHz
    (BS.1770-4 Annex 2 asks 4x at 48 kHz and proportionally less above; an N x meter's under-read depends on f/fs alone)."""
    return max(1, min(4, 192000 // int(rate)))


def true_peak(y, rate: int, dtype=np.float64) -> float:
    """The true peak (linear) of y (C, N) or (N,): with os = oversampling(rate), the larger of the sample peak and the peak of the
    os - 1 interpolated phases of `resample.resample_host(y_c, os, 1, dtype)`, over the channels.  Phase 0 is the samples
    themselves, not the filtered samples, so a true peak is never under the sample peak.  NaNs are skipped."""
    from . import resample as rs
    dtype = np.dtype(dtype)
    y = np.atleast_2d(np.asarray(y, dtype=dtype))
    os_ = oversampling(rate)
    peak = 0.0
    for c in range(y.shape[0]):
        if y.shape[1] == 0:
            continue
        a = np.abs(y[c])
        if os_ > 1:
            with np.errstate(invalid="ignore"):
                z = np.abs(rs.resample_host(y[c], os_, 1, dtype)).reshape(-1, os_)[:, 1:]
            a = np.concatenate([a, z.reshape(-1)])
        a = a[~np.isnan(a)]
        if a.size:
            peak = max(peak, float(a.max()))
    return peak


def n_short_term(n: int, rate: int) -> int:
    """Whole 3 s blocks, 100 ms apart, in n samples."""
    bins = int(n) // (int(rate) // 10)
    return bins - (SHORT_TERM_BINS - 1) if bins >= SHORT_TERM_BINS else 0


def short_term_powers_of_weighted(y, rate: int, weights=None, dtype=np.float64) -> np.ndarray:
    """(ns,) short-term powers of an already K-weighted y (C, N): with H = rate // 10 and S_c[i] the sum of the squares of bin i
    (summed as `powers_of_weighted` sums a block), q_j = sum_c G_c * (S_c[j] + ... + S_c[j+29]) / (30 H), added left to right."""
    dtype = np.dtype(dtype)
    y = np.atleast_2d(np.asarray(y, dtype=dtype))
    C, N = y.shape
    H = int(rate) // 10
    ns = n_short_term(N, rate)
    w = np.ones(C, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype).reshape(C)
    q = np.zeros(ns, dtype=dtype)
    if ns:
        bins = N // H
        for c in range(C):
            S = np.sum(np.square(y[c, :bins * H]).reshape(bins, H), axis=1, dtype=dtype)
            acc = S[0:ns].copy()
            for i in range(1, SHORT_TERM_BINS):
                acc += S[i:i + ns]
            q += w[c] * (acc / dtype.type(SHORT_TERM_BINS * H))
    return q


def short_term_powers(x, rate: int, weights=None, dtype=np.float64) -> np.ndarray:
    """(ns,) short-term powers of x (C, N): `short_term_powers_of_weighted` of `k_weighted(x)`, everything in `dtype`."""
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    k_weighting(rate)
    if n_short_term(x.shape[1], rate) == 0:
        return np.zeros(0, dtype=dtype)
    return short_term_powers_of_weighted(k_weighted(x, rate, dtype), rate, weights, dtype)


def loudness_range(q) -> Tuple[float, float, float, int]:
    """(LRA in LU, p10, p95, blocks kept) of short-term powers q (EBU Tech 3342): absolute gate l > -70 LUFS, relative gate
    l > (loudness of the mean of the abs-gated q) - 20; of the n survivors sorted ascending, p10 = v[floor((n-1) * 0.10 + 0.5)],
    p95 = v[floor((n-1) * 0.95 + 0.5)], LRA = 10 log10(p95 / p10).  (0, 0, 0, 0) when none survives."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = OFFSET + 10.0 * np.log10(q)
        keep = l > ABSOLUTE_GATE
        if not keep.any():
            return 0.0, 0.0, 0.0, 0
        keep &= l > OFFSET + 10.0 * np.log10(np.mean(q[keep])) + RANGE_GATE
    v = np.sort(q[keep])
    n = v.shape[0]
    if n == 0:
        return 0.0, 0.0, 0.0, 0
    p10 = float(v[int(np.floor((n - 1) * 0.10 + 0.5))])
    p95 = float(v[int(np.floor((n - 1) * 0.95 + 0.5))])
    return float(10.0 * np.log10(p95 / p10)), p10, p95, n


def _max_loudness(p) -> float:
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    if p.size == 0:
        return float("-inf")
    with np.errstate(divide="ignore"):
        return float(OFFSET + 10.0 * np.log10(np.max(p)))


def max_momentary(p) -> float:
    """The maximum momentary loudness (LUFS, ungated) of the 400 ms block powers p; -inf for none."""
    return _max_loudness(p)


def max_short_term(q) -> float:
    """The maximum short-term loudness (LUFS, ungated) of the 3 s block powers q; -inf for none."""
    return _max_loudness(q)


def gain_for(loudness: float, peak: Optional[float], target: Optional[float], ceiling: Optional[float]) -> Tuple[np.float32, bool]:
    """(float32 gain, whether the ceiling bit): lass_loudness_gain's rule.  g = 10^((target - loudness) / 20), computed in float64
    and rounded to float32, if a target is given and the loudness is finite, else 1; with a ceiling (linear, > 0) and a float32
    peak with fl(g * peak) > ceiling, g = fl(ceiling / peak), stepped down one float32 ulp while fl(g * peak) > ceiling.  Since
    x -> fl(g * x) is monotone in |x|, no sample at or under the peak then lands over the ceiling."""
    g = np.float32(1.0)
    if target is not None and not np.isnan(target) and np.isfinite(loudness):
        with np.errstate(over="ignore"):
            g = np.float32(10.0 ** ((float(target) - float(loudness)) / 20.0))
    limited = False
    if ceiling is not None and ceiling > 0 and peak is not None:
        pk, ce = np.float32(peak), np.float32(ceiling)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if g * pk > ce:
                limited = True
                g = np.float32(ce / pk)
                while g * pk > ce:
                    g = np.nextafter(g, np.float32(0.0))
    return g, limited


def ceiling_for(peak_ceiling_db: Optional[float], encoding: str) -> Optional[np.float32]:
    """The linear float32 ceiling of a level in dBFS (<= 0), capped at the largest value `encoding` holds without clipping:
    32767/32768 for "pcm16", the largest float32 below 1 for "pcm32"; None for None."""
    if peak_ceiling_db is None:
        return None
    c = np.float32(10.0 ** (float(peak_ceiling_db) / 20.0))
    cap = {"pcm16": np.float32(32767.0 / 32768.0), "pcm32": np.nextafter(np.float32(1.0), np.float32(0.0))}.get(encoding)
    return c if cap is None else min(c, cap)


def check_level_args(loudness, peak_ceiling_db) -> None:
    """ValueError for a target that is not a finite number or a ceiling that is not a number <= 0 dBFS."""
    for name, v in (("loudness", loudness), ("peak_ceiling_db", peak_ceiling_db)):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{name} must be a finite number or None")
    if peak_ceiling_db is not None and peak_ceiling_db > 0:
        raise ValueError("peak_ceiling_db must be <= 0 dBFS")


# ---- the look-ahead limiter ------------------------------------------------------------------------
LIMITER_MAX_REACH = 512   # include/lass_hip.h: LASS_LIMITER_MAX_H


def reach(lookahead_ms: float, rate: int) -> int:
    """The limiter's reach H in frames for a look-ahead in milliseconds: max(1, round(lookahead_ms * rate / 1000))."""
    if isinstance(lookahead_ms, bool) or not isinstance(lookahead_ms, (int, float, np.integer, np.floating)) \
            or not np.isfinite(lookahead_ms) or lookahead_ms < 0:
        raise ValueError("lookahead_ms must be a finite number >= 0")
    return max(1, int(round(float(lookahead_ms) * int(rate) / 1000.0)))


def limiter_window(H: int) -> np.ndarray:
    """The 2H + 1 float32 smoothing taps: np.hanning(2H + 3) without its two zero ends, normalised in float64, then cast."""
    H = int(H)
    if H < 1:
        raise ValueError("H must be at least 1")
    w = np.hanning(2 * H + 3)[1:-1].astype(np.float64)
    return (w / w.sum()).astype(np.float32)


def limiter_envelope(x, rate: int, true: bool = True, dtype=np.float64) -> np.ndarray:
    """(L,) e[n] = max over the channels of x (C, L) or (L,) of max(|x_c[n]|, |z_c[n*os + p]| for p = 1 ... os-1), with
    z_c = `resample.resample_host(x_c, os, 1, dtype)` as `true_peak` forms it and os = oversampling(rate) with `true`, else 1.
    A NaN counts as 0; max_n e[n] is `true_peak(x, rate)`."""
    from . import resample as rs
    dtype = np.dtype(dtype)
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    os_ = oversampling(rate) if true else 1
    e = np.zeros(x.shape[1], dtype=dtype)
    for c in range(x.shape[0]):
        a = np.abs(x[c])
        if os_ > 1 and x.shape[1]:
            with np.errstate(invalid="ignore"):
                z = np.abs(rs.resample_host(x[c], os_, 1, dtype)).reshape(-1, os_)[:, 1:]
            z = np.where(np.isnan(z), dtype.type(0), z)
            a = np.maximum(np.where(np.isnan(a), dtype.type(0), a), z.max(axis=1))
        e = np.maximum(e, np.where(np.isnan(a), dtype.type(0), a))
    return e


def limiter_required(e, gain, ceiling, dtype=np.float64) -> np.ndarray:
    """r[n]: 1 where gain * e[n] <= ceiling, else ceiling / (gain * e[n]); every operation rounded once in `dtype`."""
    dt = np.dtype(dtype).type
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a = dt(gain) * np.asarray(e, dtype=dtype)
        return np.where(a <= dt(ceiling), dt(1), dt(ceiling) / np.where(a <= dt(ceiling), dt(1), a))


def _running_min(r: np.ndarray, H: int, fill) -> np.ndarray:
    """min r[k] over |k - n| <= H, r continued with `fill`: minima of 2^i neighbours doubled up to the largest power of two in
    2H + 1, then two of them overlapped (min is exact: the scheme cannot change a bit)."""
    L, W = r.shape[0], 2 * H + 1
    A = np.concatenate([np.full(H, fill, dtype=r.dtype), r, np.full(H, fill, dtype=r.dtype)])
    p = 1
    while 2 * p <= W:
        A = np.minimum(A[:A.shape[0] - p], A[p:])
        p *= 2
    return np.minimum(A[:L], A[W - p:W - p + L])


def limiter_curve(e, gain, ceiling, H: int, window=None, dtype=np.float64):
    """(G, r, m) of an envelope e (L,): the required gain r (`limiter_required`), its minimum m over |k - n| <= H inside the row,
    and G[n] = sum_{j=-H..H} w[j+H] * m'[n+j] (m' = m inside the row, 1 outside; added in that order) with the two rules that
    make it exact where it matters: G[n] = 1 where every m' in reach is 1, and G[n] := min(G[n], r[n])."""
    dtype = np.dtype(dtype)
    H = int(H)
    if H < 1:
        raise ValueError("H must be at least 1")
    r = limiter_required(e, gain, ceiling, dtype)
    L = r.shape[0]
    one = dtype.type(1)
    m = _running_min(r, H, one)
    w = (limiter_window(H) if window is None else np.asarray(window)).astype(dtype)
    mp = np.concatenate([np.ones(H, dtype=dtype), m, np.ones(H, dtype=dtype)])
    G = np.zeros(L, dtype=dtype)
    for j in range(2 * H + 1):
        G += w[j] * mp[j:j + L]
    G = np.where(_running_min(m, H, one) == one, one, G)
    return np.minimum(G, r), r, m


def limit(x, rate: int, gain, ceiling, H: int, true: bool = True, dtype=np.float64):
    """The look-ahead limiter: (v, G, e) for planes x (C, L) or (L,) - e = `limiter_envelope(x, rate, true)`, G the gain curve of
    `limiter_curve(e, gain, ceiling, H)`, one per recording, and v_c[n] = (gain * G[n]) * x_c[n].  gain * G[n] * e[n] <= ceiling
    up to the rounding of the two products, and a stretch whose envelope needs no reduction within 2H frames is gain * x."""
    dtype = np.dtype(dtype)
    xs = np.asarray(x, dtype=dtype)
    e = limiter_envelope(xs, rate, true, dtype)
    G = limiter_curve(e, gain, ceiling, H, None, dtype)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        v = (dtype.type(gain) * G) * xs
    return v, G, e
