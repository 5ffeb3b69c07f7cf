"""Polyphase resampling, host side: the filter design, a numpy evaluation of the formula the device kernel computes, and the
cache of uploaded taps.

The filter is `scipy.signal.resample_poly`'s default, built with numpy alone (the GPU tests need no scipy):
`firwin(20 * max(up, down) + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up`, i.e. `fc * sinc(fc * k) * kaiser(N, 5)`
normalised to unit sum.  The resampled signal is

    y[n] = sum_m x[m] * h[n * down - m * up + half],   half = (N - 1) / 2,   x = 0 outside the clip,   n < ceil(len(x) * up / down)

which is resample_poly's `padtype="constant"` centring.  `lass_decode_resample` (csrc/resample.hip) evaluates exactly this in
float32; `resample_host` evaluates it in numpy at the dtype asked for and is the yardstick of the device tests.  Parity with
`librosa.load`'s soxr_hq is unpinned, as for `wavio.read_wav`'s scipy path (wavio's docstring).
"""
from __future__ import annotations

from math import gcd
from typing import Dict, Tuple

import numpy as np

MAX_TAPS = 16383     # include/lass_hip.h: LASS_RESAMPLE_MAX_TAPS
ENCODINGS = {"pcm16": 0, "pcm32": 1, "f32": 2}    # include/lass_hip.h: LASS_WAV_*
SAMPLE_BYTES = {"pcm16": 2, "pcm32": 4, "f32": 4}


def ratio(rate_in: int, rate_out: int) -> Tuple[int, int]:
    """(up, down) in lowest terms."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError("sample rates must be positive")
    g = gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def n_taps(up: int, down: int) -> int:
    return 20 * max(int(up), int(down)) + 1


def within_cap(up: int, down: int) -> bool:
    """Whether the device kernel takes this ratio's filter (a filter of this design within the tap cap also fits the kernel's
    polyphase table: up <= n_taps / 20)."""
    return n_taps(up, down) <= MAX_TAPS


LDS_FLOATS = 160 * 256      # csrc/polyphase.h: kLdsFloats, the CU's 160 KiB
OS_TAPS_PER_PHASE = 21      # csrc/export.hip: kOsJ, ceil((20 * os + 1) / os)


def true_peak_fits(up: int, down: int, os: int) -> bool:
    """Whether `lass_resample_true_peak` takes this ratio at oversampling `os`: the ratio is within the tap cap, and a tile of one
    frame - the filter table, the input span of the 21 first-stage outputs one interpolated value reaches, the stage that holds
    them and the second table - fits the CU's LDS (the launcher's formula, csrc/export.hip: true_peak_floats at t = 1)."""
    up, down, os = int(up), int(down), int(os)
    stage = (1 + OS_TAPS_PER_PHASE - 1 + 3) // 4 * 4 + os * (OS_TAPS_PER_PHASE | 1)
    if up == down:
        return True
    if not within_cap(up, down):
        return False
    nt = n_taps(up, down)
    J = -(-nt // up)
    table = up * (J | 1)
    span = ((up - 1) + (1 + OS_TAPS_PER_PHASE - 1 - 1) * down) // up + J
    return (table + span + 3) // 4 * 4 + stage <= LDS_FLOATS


def out_len(frames: int, up: int, down: int) -> int:
    return -(-int(frames) * int(up) // int(down))


def design_taps(up: int, down: int) -> np.ndarray:
    """scipy.signal.resample_poly's default prototype filter times `up`, float64, natural order."""
    m = max(int(up), int(down))
    n = 20 * m + 1
    fc = 1.0 / m
    k = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    h = fc * np.sinc(fc * k) * np.kaiser(n, 5.0)
    h /= h.sum()
    return h * up


def resample_host(x, up: int, down: int, dtype=np.float64) -> np.ndarray:
    """The formula of the module docstring for a 1-D signal, vectorised over the outputs, one tap of every output's phase at a
    time (the order the device kernel accumulates in), with signal, taps, products and sums in `dtype`."""
    dtype = np.dtype(dtype)
    x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    up, down = int(up), int(down)
    if up == down:
        return x.copy()
    h = design_taps(up, down).astype(dtype)
    nt, frames = h.shape[0], x.shape[0]
    t = np.arange(out_len(frames, up, down), dtype=np.int64) * down + (nt - 1) // 2
    m0, p = t // up, t % up
    y = np.zeros(t.shape[0], dtype=dtype)
    zero = dtype.type(0)
    for j in range(-(-nt // up)):
        k, m = p + j * up, m0 - j
        ok = (k < nt) & (m >= 0) & (m < frames)
        y += np.where(ok, x[np.clip(m, 0, frames - 1)] * h[np.minimum(k, nt - 1)], zero)
    return y


_TAPS: Dict[tuple, "object"] = {}


def device_taps(up: int, down: int, device):
    """The float32 taps of (up, down) on `device`, uploaded once."""
    import torch

    device = torch.device(device)
    key = (int(up), int(down), str(device))
    t = _TAPS.get(key)
    if t is None:
        t = _TAPS[key] = torch.from_numpy(design_taps(up, down).astype(np.float32)).to(device)
    return t
