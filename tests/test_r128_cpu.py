"""EBU R 128 on the host: the float64 definitions of lass_amd/loudness.py - true peak, short-term powers,
loudness range, the two maxima - against the EBU Tech 3341 / 3342 minimum-requirement signals, the edge cases of the percentile
rule, and the C-ABI's new symbols."""
import os
import re

import numpy as np
import pytest

from lass_amd import loudness as ld
from lass_amd import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stepped_tone(rate, levels_db, seconds, freq=1000.0):
    """A stereo tone at `freq`, `seconds` at each of `levels_db` (dBFS peak), phase running on across the steps."""
    n = int(seconds * rate)
    amp = np.concatenate([np.full(n, 10.0 ** (db / 20.0)) for db in levels_db])
    x = amp * np.sin(2.0 * np.pi * freq * np.arange(amp.shape[0]) / rate)
    return np.stack([x, x])


# ---- loudness range -----------------------------------------------------------------------------------------------------
TECH_3342 = [((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)]


@pytest.mark.parametrize("levels,want", TECH_3342)
def test_ebu_tech_3342_cases(levels, want):
    q = ld.short_term_powers(stepped_tone(16000, levels, 20.0), 16000)
    lra, p10, p95, kept = ld.loudness_range(q)
    print(f"levels {levels}: LRA {lra:.3f} LU, {kept} of {q.shape[0]} blocks kept")
    assert q.shape[0] == ld.n_short_term(len(levels) * 320000, 16000) == len(levels) * 200 - 29
    assert abs(lra - want) <= 1.0
    assert 0 < p10 <= p95 and 0 < kept <= q.shape[0]


def test_a_steady_tone_reads_one_loudness_three_ways():
    x = stepped_tone(16000, (-23,), 10.0)
    p, q = ld.block_powers(x, 16000), ld.short_term_powers(x, 16000)
    i, m, s = ld.gate(p)[0], ld.max_momentary(p), ld.max_short_term(q)
    print(f"integrated {i:.4f}, max momentary {m:.4f}, max short-term {s:.4f} LUFS")
    assert abs(m - i) <= 0.1 and abs(s - i) <= 0.1 and abs(m - s) <= 0.1
    assert abs(i + 23.0) <= 0.1                      # (a stereo 1 kHz sine at -23 dBFS reads -23 LUFS: Tech 3341 case 1)
    assert ld.max_momentary(np.zeros(0)) == float("-inf") == ld.max_short_term([])


def test_short_term_powers_are_thirty_bins():
    """q_j against the definition written out, and the block count at the 3 s edge."""
    rate, H = 16000, 1600
    x = 0.1 * np.random.Generator(np.random.PCG64(3)).standard_normal((2, 52 * H + 17))
    w = np.array([1.0, 0.5])
    y = ld.k_weighted(x, rate)
    q = ld.short_term_powers(x, rate, w)
    assert q.shape == (23,)
    for j in (0, 7, 22):
        want = sum(w[c] * np.sum(np.square(y[c, j * H:(j + 30) * H])) / (30 * H) for c in range(2))
        assert abs(q[j] - want) <= 1e-13 * want
    assert ld.short_term_powers(x[:, :30 * H - 1], rate).shape == (0,) and ld.short_term_powers(x[:, :30 * H], rate).shape == (1,)
    assert [ld.n_short_term(n, rate) for n in (0, 46400, 47999, 48000, 49599, 49600)] == [0, 0, 0, 1, 1, 2]


def test_loudness_range_edge_cases():
    assert ld.loudness_range([]) == (0.0, 0.0, 0.0, 0)
    assert ld.loudness_range([0.0, 1e-9]) == (0.0, 0.0, 0.0, 0)              # nothing over the absolute gate
    assert ld.loudness_range([0.01]) == (0.0, 0.01, 0.01, 1)
    # n = 2: floor(0.1 + 0.5) = 0, floor(0.95 + 0.5) = 1;  n = 3: floor(0.2 + 0.5) = 0, floor(1.9 + 0.5) = 2
    lra, p10, p95, n = ld.loudness_range([0.02, 0.01])
    assert (p10, p95, n) == (0.01, 0.02, 2) and lra == pytest.approx(10 * np.log10(2.0), abs=1e-12)
    lra, p10, p95, n = ld.loudness_range([0.02, 0.01, 0.04])
    assert (p10, p95, n) == (0.01, 0.04, 3) and lra == pytest.approx(10 * np.log10(4.0), abs=1e-12)
    # n = 11: floor(1.0 + 0.5) = 1, floor(9.5 + 0.5) = 10;  n = 21: floor(2.0 + 0.5) = 2, floor(19.0 + 0.5) = 19
    rng = np.random.Generator(np.random.PCG64(4))
    for n, (i10, i95) in ((11, (1, 10)), (21, (2, 19))):
        v = 0.01 * (1.0 + np.arange(n) / n)                                  # within 3 dB: the relative gate keeps all
        _, p10, p95, kept = ld.loudness_range(rng.permutation(v))
        assert (p10, p95, kept) == (v[i10], v[i95], n)
    # the absolute gate is exclusive: a block exactly on it is out, the next double up is in
    # (`on`: the largest double whose loudness, as the rule computes it, is not over the gate; `over`: the next one)
    on = 10.0 ** ((ld.ABSOLUTE_GATE - ld.OFFSET) / 10.0)
    while ld.OFFSET + 10.0 * np.log10(on) > ld.ABSOLUTE_GATE:
        on = np.nextafter(on, 0.0)
    while ld.OFFSET + 10.0 * np.log10(np.nextafter(on, 1.0)) <= ld.ABSOLUTE_GATE:
        on = np.nextafter(on, 1.0)
    over = np.nextafter(on, 1.0)
    assert ld.OFFSET + 10.0 * np.log10(on) == ld.ABSOLUTE_GATE               # such a double exists: -70 is hit exactly
    assert ld.loudness_range([on])[3] == 0
    assert ld.loudness_range([on, over]) == (0.0, over, over, 1)
    # the relative gate drops what lies 20 LU under the abs-gated mean
    assert ld.loudness_range([1e-2, 1e-2, 1e-5])[3] == 2


# ---- true peak ----------------------------------------------------------------------------------------------------------
def test_oversampling():
    assert [ld.oversampling(r) for r in (8000, 16000, 44100, 48000, 88200, 96000, 192000)] == [4, 4, 4, 4, 2, 2, 1]
    assert ld.oversampling(176400) == 1


TONES = [(4.0, 45.0), (6.0, 60.0), (8.0, 67.5), (3.0, 30.0), (2.5, 10.0)]     # (fs / f, phase in degrees)


def faded_tone(rate, div, phase_deg, seconds=0.25, level_db=-6.02, fade=0.02):
    n, k = int(seconds * rate), int(fade * rate)
    x = 10.0 ** (level_db / 20.0) * np.sin(2.0 * np.pi * np.arange(n) / div + np.deg2rad(phase_deg))
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(k) / k)
    x[:k] *= ramp
    x[n - k:] *= ramp[::-1]
    return x


@pytest.mark.parametrize("rate", [16000, 44100, 48000, 96000])
def test_ebu_tech_3341_true_peak_tones(rate):
    for k, (div, ph) in enumerate(TONES):
        x = faded_tone(rate, div, ph)
        tp = 20.0 * np.log10(ld.true_peak(x, rate))
        sp = 20.0 * np.log10(np.max(np.abs(x)))
        print(f"{rate} Hz, fs/{div} at {ph} deg: true peak {tp:.3f} dBTP, sample peak {sp:.3f} dBFS")
        assert -6.02 - 0.4 <= tp <= -6.02 + 0.2
        assert tp >= sp
        if k < 3:
            assert sp <= tp - 0.6
        assert ld.true_peak(np.stack([0.5 * x, x]), rate) == ld.true_peak(x, rate)       # the channels' maximum


def test_true_peak_rules():
    x = faded_tone(16000, 4.0, 45.0)
    assert ld.true_peak(x, 192000) == np.max(np.abs(x))                      # os == 1: the sample peak
    click = np.zeros(100)
    click[50] = 1.0                                                           # phase 0 is the sample, not the filtered sample
    assert ld.true_peak(click, 48000) == 1.0
    hole = x.copy()
    hole[2000] = np.nan                                                       # a NaN is skipped, with all it reaches
    assert 0.4 < ld.true_peak(hole, 16000) <= ld.true_peak(x, 16000)
    assert ld.true_peak(np.zeros((2, 0)), 16000) == 0.0
    a, b = ld.true_peak(x, 16000), ld.true_peak(x, 16000, np.float32)
    assert abs(a - b) <= 1e-6 * a and a != b


# ---- the C-ABI and the pipeline's refusals ------------------------------------------------------------------------------
def test_new_symbols_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from lass_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    declared = set(re.findall(r"\b(lass_[a-z_0-9]+)\s*\(", hdr))
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name in ("lass_resample_true_peak", "lass_loudness_stats"):
        assert name in declared and name in bound and hasattr(lib, name), name
    assert len(bound["lass_resample_true_peak"]) == len(bound["lass_resample_peak"]) + 3 == 17       # os, os_taps, n_os_taps
    assert len(bound["lass_loudness_stats"]) == len(bound["lass_loudness"]) + 2 == 19                # short_term, ns_max
    assert lib.lass_resample_true_peak(None, None, 0, 0, 0, 0, 0, 0, 0, None, 0, 0, 0, None, 0, None, None) < 0
    assert lib.lass_loudness_stats(None, None, 0, 0, 0, 0, 0, None, 0, None, None, None, None, 0, None, 0, None, 0, None) < 0


def test_host_predicate_mirrors_the_launcher():
    from lass_amd import resample as rs
    assert rs.true_peak_fits(1, 1, 4) and rs.true_peak_fits(441, 160, 4) and rs.true_peak_fits(3, 2, 4) and rs.true_peak_fits(1, 2, 2)
    assert rs.within_cap(1, 50000) is False          # (beyond the tap cap anyway)
    assert not rs.true_peak_fits(1, 50000, 4)
    assert rs.within_cap(1, 800) and not rs.true_peak_fits(1, 800, 4)        # inside the tap cap, yet no room for the halo's reach


@pytest.mark.parametrize("kw", [dict(peak="true"), dict(peak="true", loudness=-23.0), dict(peak="rms", peak_ceiling_db=-1.0),
                                dict(peak=None, peak_ceiling_db=-1.0)])
def test_pipeline_refuses_a_bad_peak_before_any_file_is_opened(kw, tmp_path):
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(ValueError, match="peak"):
        pipeline.separate_files(None, [(missing, "a dog", str(tmp_path / "out.wav"))], 16000, **kw)
    with pytest.raises(ValueError, match="peak"):
        pipeline.inference(None, missing, "a dog", str(tmp_path / "out.wav"), 16000, **kw)
