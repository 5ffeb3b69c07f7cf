"""The host definition of the loudness meter and of the export gain (lass_amd/loudness.py), without a device.

Pins: the EBU Tech 3341 tones at EBU's own tolerance of 0.1 LU, the block and gate arithmetic against hand counts, and the gain
rule's guarantee (no gained peak over the ceiling) over awkward float32 peaks.  The device kernels are held to this module in
tests/test_loudness_gpu.py."""
import numpy as np
import pytest

from lass_amd import loudness as ld
from lass_amd import pipeline


def tones(rate: int, segments) -> np.ndarray:
    """In-phase stereo 1 kHz sine, phase-continuous, (peak dBFS, seconds) per segment."""
    n = [int(round(sec * rate)) for _, sec in segments]
    t = np.arange(sum(n)) / rate
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for (db, _), k in zip(segments, n)])
    x = amp * np.sin(2.0 * np.pi * 1000.0 * t)
    return np.stack([x, x])


EBU = [([(-23, 20)], -23.0), ([(-33, 20)], -33.0), ([(-36, 10), (-23, 60), (-36, 10)], -23.0),
       ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0), ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0)]


@pytest.fixture(scope="module")
def at_48k():
    return [ld.integrated_loudness(tones(48000, seg), 48000) for seg, _ in EBU]


def test_ebu_tech_3341_cases_at_48k(at_48k):
    for k, ((_, want), got) in enumerate(zip(EBU, at_48k)):
        print(f"case {k + 1} at 48000 Hz: {got:.3f} LUFS")
        assert abs(got - want) <= 0.1


@pytest.mark.parametrize("rate", [44100, 32000, 16000])
def test_ebu_tech_3341_cases_at_other_rates(at_48k, rate):
    """44 100 Hz is held to EBU's targets like 48 000; 32 000 and 16 000 to their own 48 000 Hz value."""
    for k, ((seg, want), ref) in enumerate(zip(EBU, at_48k)):
        got = ld.integrated_loudness(tones(rate, seg), rate)
        print(f"case {k + 1} at {rate} Hz: {got:.3f} LUFS ({got - ref:+.3f} to 48 kHz)")
        assert abs(got - (want if rate == 44100 else ref)) <= 0.1


def test_block_edges():
    rate, T = 16000, 6400
    long = 0.1 * np.random.Generator(np.random.PCG64(1)).standard_normal((2, 2 * T))
    x = long[:, :T]
    assert ld.block_powers(x[:, :T - 1], rate).shape == (0,) and ld.integrated_loudness(x[:, :T - 1], rate) == float("-inf")
    p = ld.block_powers(x, rate)
    assert p.shape == (1,) and p.dtype == np.float64
    y = ld.k_weighted(x, rate, chunk=T)                       # the plain recurrence
    assert p[0] == pytest.approx(float(np.mean(y[0] ** 2) + np.mean(y[1] ** 2)), rel=1e-12)
    assert ld.integrated_loudness(x, rate) == pytest.approx(-0.691 + 10 * np.log10(p[0]), abs=1e-12)
    assert ld.block_powers(long[:, :T + 1599], rate).shape == (1,) and ld.block_powers(long[:, :T + 1600], rate).shape == (2,)
    assert ld.integrated_loudness(np.zeros((2, 5 * T)), rate) == float("-inf")
    w = ld.block_powers(x, rate, weights=[1.0, 1.41])
    assert w[0] == pytest.approx(float(np.mean(y[0] ** 2) + 1.41 * np.mean(y[1] ** 2)), rel=1e-12)


def test_split_evaluation_equals_the_plain_recurrence():
    x = 0.1 * np.random.Generator(np.random.PCG64(2)).standard_normal((3, 30011))
    plain = ld.k_weighted(x, 32000, chunk=30011)
    for chunk in (1, 7, 256, 30010):
        assert np.max(np.abs(ld.k_weighted(x, 32000, chunk=chunk) - plain)) < 1e-11
    (b1, a1), (b2, a2) = ld.k_weighting(48000)
    for b, a in ((b1, a1), (b2, a2)):
        assert a[0] == 1.0 and b.dtype == np.float64
    # the recommendation's 48 kHz table, to the digits the redesign keeps
    assert np.allclose(b1, [1.53512485958697, -2.69169618940638, 1.19839281085285], atol=2e-4)
    assert np.allclose(a2, [1.0, -1.99004745483398, 0.99007225036621], atol=2e-5)


def test_gates_against_a_hand_count():
    """8 s at 16 kHz: 2 s at -80 dBFS, 3 s at -20, 3 s at -45; 77 blocks of 0.4 s, 0.1 s apart.  Blocks 0 ... 16 lie in the -80
    stretch (two channels of a sine at -80 dBFS peak: about -80 LUFS, under the absolute gate).  Blocks 50 ... 76 lie in the -45
    stretch (about -45 LUFS: over the absolute gate, but the abs-gated mean is about -23 LUFS, so the relative gate at about -33
    drops them).  Blocks 17 ... 49 hold at least 0.1 s of the -20 tone (at worst -26 LUFS) and survive: 33."""
    rate = 16000
    x = tones(rate, [(-80, 2), (-20, 3), (-45, 3)])
    p = ld.block_powers(x, rate)
    l = -0.691 + 10 * np.log10(p)
    assert p.shape == (77,)
    assert np.all(l[:17] < -70) and np.all(l[17:] > -70)
    loud, kept = ld.gate(p)
    assert kept == 33
    assert loud == pytest.approx(-0.691 + 10 * np.log10(np.mean(p[17:50])), abs=1e-12)
    assert -21.0 < loud < -20.0                              # (the full blocks read -20.07; six of the 33 are partial)


def test_k_weighting_refusals():
    for rate in (11025, 4000):
        with pytest.raises(ValueError):
            ld.k_weighting(rate)
        with pytest.raises(ValueError):
            ld.block_powers(np.zeros((1, 100)), rate)


def test_gain_rule():
    f32 = np.float32
    g, bit = ld.gain_for(-30.0, 0.1, -23.0, None)
    assert g == f32(10.0 ** (7.0 / 20.0)) and not bit and g.dtype == np.float32
    g, bit = ld.gain_for(-30.0, 2.0, None, 0.5)
    assert g == f32(0.25) and bit
    assert ld.gain_for(-30.0, 0.4, None, 0.5) == (f32(1.0), False)
    g, bit = ld.gain_for(-30.0, 0.7, -23.0, f32(0.8912509))
    assert bit and f32(g * f32(0.7)) <= f32(0.8912509) and g < f32(10.0 ** (7.0 / 20.0))
    for l in (float("-inf"), float("inf"), float("nan")):
        assert ld.gain_for(l, 0.1, -23.0, 0.9) == (f32(1.0), False)
    assert ld.gain_for(float("-inf"), 3.0, -23.0, 0.75) == (f32(0.25), True)      # the ceiling's gain alone
    # awkward float32 peaks: the gained peak never lands over the ceiling, and where the ceiling bit it is reached within 2 ulps
    rng = np.random.Generator(np.random.PCG64(3))
    peaks = np.concatenate([rng.uniform(0.001, 40.0, 4000).astype(f32), f32(1.0) + np.arange(64, dtype=f32) * f32(2.0 ** -23),
                            np.array([3.0, 1 / 3, 0.1, 0.7, 1e-30, 1e30, 2.0 ** -140, np.inf], dtype=f32)])
    for ce in (ld.ceiling_for(-1.0, "f32"), ld.ceiling_for(0.0, "pcm16"), ld.ceiling_for(0.0, "pcm32"), ld.ceiling_for(-0.1, "pcm16")):
        for pk in peaks:
            for target in (None, -14.0):
                with np.errstate(over="ignore", invalid="ignore"):
                    g, bit = ld.gain_for(-23.0, pk, target, ce)
                    assert g.dtype == np.float32 and not f32(g * pk) > ce
                    if bit and np.isfinite(pk):
                        assert f32(g * pk) >= ce * f32(1.0 - 2.0 ** -22)


def test_ceilings():
    assert ld.ceiling_for(None, "pcm16") is None
    assert ld.ceiling_for(-1.0, "pcm16") == np.float32(10.0 ** (-1 / 20.0)) == ld.ceiling_for(-1.0, "f32")
    assert ld.ceiling_for(0.0, "pcm16") == np.float32(32767.0 / 32768.0) and ld.ceiling_for(0.0, "f32") == np.float32(1.0)
    assert ld.ceiling_for(0.0, "pcm32") == np.nextafter(np.float32(1.0), np.float32(0.0))
    # at the cap nothing clips: the writers' rule on the ceiling itself
    assert pipeline.host_clip_count(np.array([ld.ceiling_for(0.0, "pcm16")] * 2) * [1, -1], "pcm16") == 0
    assert pipeline.host_clip_count(np.array([ld.ceiling_for(0.0, "pcm32")] * 2) * [1, -1], "pcm32") == 0


@pytest.mark.parametrize("kw", [dict(peak_ceiling_db=0.5), dict(loudness="loud"), dict(loudness=float("nan")),
                                dict(peak_ceiling_db=float("inf")), dict(loudness=-23.0, peak_ceiling_db="-1")])
def test_pipeline_refuses_bad_levels_before_any_file_is_opened(kw, tmp_path):
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(ValueError, match="loudness|peak_ceiling_db"):
        pipeline.separate_files(None, [(missing, "a dog", str(tmp_path / "out.wav"))], 16000, **kw)
    with pytest.raises(ValueError, match="loudness|peak_ceiling_db"):
        pipeline.inference(None, missing, "a dog", str(tmp_path / "out.wav"), sampling_rate=16000, **kw)
