"""The look-ahead limiter without a GPU: `lass_limit` in the ABI, the properties of its float64 definition
(lass_amd/loudness.py: `limit`, `limiter_curve`, `limiter_envelope`, `limiter_window`, `reach`), the claim the feature rests on -
one gain per file misses a loudness target by the whole overshoot once the ceiling binds, the limited planes reach it - and the
pipeline's refusals.

The fixture is the issue's: 6 s at 16 kHz, two channels; 0.02 N(0,1) smoothed by a 4-tap mean plus a 1 kHz tone at 0.05, three
4 ms clicks 0.9 exp(-k/16) sin(2 pi k/4 + pi/4) at 1.0, 2.7 and 4.4 s; the second channel 0.7 x the first, reversed."""
import os
import re

import numpy as np
import pytest

from lass_amd import loudness as ld
from lass_amd import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 16000
H = 24


def _fixture(burst_ms=4.0, tau=16.0):
    L = 6 * RATE
    a = np.convolve(0.02 * np.random.default_rng(0).standard_normal(L), np.ones(4) / 4.0, mode="same")
    a += 0.05 * np.sin(2 * np.pi * 1000.0 * np.arange(L) / RATE)
    k = np.arange(int(burst_ms * RATE / 1000))
    for at in (1.0, 2.7, 4.4):
        s = int(at * RATE)
        a[s:s + k.size] += 0.9 * np.exp(-k / tau) * np.sin(2 * np.pi * k / 4.0 + np.pi / 4.0)
    return np.stack([a, 0.7 * a[::-1]]).astype(np.float32)


@pytest.fixture(scope="module")
def clicks():
    return _fixture()


def _passes(x, target, ceiling, n):
    """The pipeline's loop: the loudness of the limited planes after each of n passes."""
    g = ld.gain_for(ld.integrated_loudness(x, RATE), None, target, None)[0]
    got = []
    for _ in range(n):
        v, G, e = ld.limit(x, RATE, g, ceiling, H)
        got.append((ld.integrated_loudness(v, RATE), v))
        g = np.float32(g * ld.gain_for(got[-1][0], None, target, None)[0])
    return got


def test_symbol_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from lass_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    declared = set(re.findall(r"\b(lass_[a-z_0-9]+)\s*\(", hdr))
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert "lass_limit" in declared and "lass_limit" in bound and hasattr(lib, "lass_limit")
    assert len(bound["lass_limit"]) == 23
    assert re.search(r"#define\s+LASS_LIMITER_MAX_H\s+512\b", hdr) and ld.LIMITER_MAX_REACH == 512
    tile = int(re.search(r"#define\s+LASS_LIMITER_TILE\s+(\d+)", hdr).group(1))
    assert 256 <= tile <= 4096 and tile & (tile - 1) == 0
    assert lib.lass_limit(None, None, 0, 0, 0, 0, 0, 0, None, 0, None, 0.0, 0, None, None, 0, 0, None, None, 0, None, None, None) < 0
    import __graft_entry__ as entry
    assert "limiter.hip" in entry.SOURCES


def test_fixture_is_the_issues(clicks):
    assert abs(ld.integrated_loudness(clicks, RATE) - (-26.27)) < 0.005
    assert abs(20 * np.log10(ld.true_peak(clicks, RATE)) - (-1.38)) < 0.005


@pytest.mark.parametrize("gain_db", [3.0, 10.3, 16.0])
@pytest.mark.parametrize("true", [True, False])
def test_definition_properties(clicks, gain_db, true):
    g, c = np.float32(10.0 ** (gain_db / 20.0)), ld.ceiling_for(-1.0, "f32")
    v, G, e = ld.limit(clicks, RATE, g, c, H, true)
    assert e.max() == (ld.true_peak(clicks, RATE) if true else np.abs(clicks).max())
    G2, r, m = ld.limiter_curve(e, g, c, H)
    assert np.array_equal(G, G2)
    assert np.all(G <= r) and np.all(m <= r) and np.all(G > 0)
    L = e.shape[0]
    free = np.array([np.all(r[max(0, n - 2 * H):n + 2 * H + 1] == 1.0) for n in range(L)])
    assert free.any() and not free.all()
    assert np.all(G[free] == 1.0) and np.all(G[~free] < 1.0)
    assert np.array_equal(v[:, free], (np.float64(g) * clicks.astype(np.float64))[:, free])
    assert np.abs(v).max() <= float(c) * (1 + 2.0 ** -22)
    assert np.all(np.float64(g) * G * e <= float(c) * (1 + 2.0 ** -22))
    # m is the minimum of r over |k - n| <= H inside the row, whatever scheme finds it
    assert np.array_equal(m, np.array([r[max(0, n - H):n + H + 1].min() for n in range(L)]))


def test_quiet_silent_and_nan_rows_come_back_as_g_times_x(clicks):
    g, c = np.float32(2.0), ld.ceiling_for(-1.0, "f32")
    quiet = (0.01 * clicks[:, :4000]).astype(np.float32)
    silent = np.zeros((2, 4000), dtype=np.float32)
    nans = np.full((2, 4000), np.nan, dtype=np.float32)
    for x in (quiet, silent, nans):
        v, G, e = ld.limit(x, RATE, g, c, H)
        _, r, m = ld.limiter_curve(e, g, c, H)
        assert np.all(G == 1.0) and np.count_nonzero(m < 1.0) == 0
        assert np.array_equal(v, np.float64(g) * x.astype(np.float64), equal_nan=True)
    assert np.all(ld.limiter_envelope(nans, RATE) == 0.0)


@pytest.mark.parametrize("target, short, near", [(-23.0, 2.9, 0.01), (-16.0, 9.9, 0.02)])
def test_the_claim(clicks, target, short, near):
    """One gain per file (`gain_for` with the true-peak ceiling) lands `short` LU under the target; two passes of the limiter land
    within `near` LU of it - the issue's table.  The bars are the issue's: at least 2.5 LU short, within 0.1 LU."""
    c = ld.ceiling_for(-1.0, "f32")
    l0 = ld.integrated_loudness(clicks, RATE)
    g1, bit = ld.gain_for(l0, np.float32(ld.true_peak(clicks, RATE)), target, c)
    single = l0 + 20 * np.log10(np.float64(g1))
    (_, _), (l2, v) = _passes(clicks, target, c, 2)
    print(f"target {target}: single gain {single:.2f} LUFS, limited {l2:.2f} LUFS, true peak {20 * np.log10(ld.true_peak(v, RATE)):.3f} dBTP")
    assert bit and target - single >= 2.5 and abs((target - single) - short) < 0.05
    assert abs(l2 - target) <= 0.1 and abs(abs(l2 - target) - near) < 0.01
    assert np.abs(v).max() <= float(c) * (1 + 2.0 ** -22)


def test_divergent_case_moves_closer_each_pass():
    """Where the loud part IS the peaks (30 ms bursts in place of the 4 ms clicks, the decay stretched with them: exp(-k/120)) the
    limiter takes back most of what the gain adds, and two passes stay 0.4 LU short of -16 LUFS; each pass still moves it closer:
    -17.67, -16.39, -16.08, -16.02 LUFS here."""
    x = _fixture(30.0, 120.0)
    c = ld.ceiling_for(-1.0, "f32")
    got = [l for l, _ in _passes(x, -16.0, c, 4)]
    print("bursts, target -16:", " ".join(f"{l:.2f}" for l in got))
    miss = [abs(l + 16.0) for l in got]
    assert all(b < a for a, b in zip(miss, miss[1:]))


def test_reach_and_window():
    assert ld.reach(1.5, 16000) == 24 and ld.reach(1.5, 32000) == 48 and ld.reach(0.0, 16000) == 1 and ld.reach(0.01, 16000) == 1
    assert ld.reach(16.0, 32000) == 512
    for bad in (-1.0, float("nan"), float("inf"), None, "1.5", True):
        with pytest.raises(ValueError):
            ld.reach(bad, 16000)
    for h in (1, 2, 24, 512):
        w = ld.limiter_window(h)
        assert w.dtype == np.float32 and w.shape == (2 * h + 1,)
        assert np.all(w >= 0) and np.array_equal(w, w[::-1]) and w.argmax() == h
        assert abs(w.astype(np.float64).sum() - 1.0) <= 2.0 ** -20
    with pytest.raises(ValueError):
        ld.limiter_window(0)
    with pytest.raises(ValueError):
        ld.limiter_curve(np.zeros(8), 1.0, 0.5, 0)


@pytest.mark.parametrize("kw, match", [
    (dict(limiter=True), "peak_ceiling_db"),
    (dict(limiter=True, loudness=-16.0), "peak_ceiling_db"),
    (dict(limiter=True, peak_ceiling_db=-1.0, limiter_passes=0), "limiter_passes"),
    (dict(limiter=True, peak_ceiling_db=-1.0, limiter_passes=1.5), "limiter_passes"),
    (dict(limiter=True, peak_ceiling_db=-1.0, limiter_lookahead_ms=-1.0), "lookahead_ms"),
    (dict(limiter=True, peak_ceiling_db=-1.0, limiter_lookahead_ms=float("nan")), "lookahead_ms"),
    (dict(limiter=True, peak_ceiling_db=-1.0, limiter_lookahead_ms=40.0), "lookahead_ms"),
])
def test_pipeline_refuses_bad_limiter_arguments_before_any_file_is_opened(kw, match, tmp_path):
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(ValueError, match=match):
        pipeline.separate_files(None, [(missing, "a dog", str(tmp_path / "out.wav"))], 16000, **kw)
    with pytest.raises(ValueError, match=match):
        pipeline.inference(None, missing, "a dog", str(tmp_path / "out.wav"), 16000, **kw)
