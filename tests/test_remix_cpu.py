"""Remix export on the host: the C-ABI declarations, `pipeline.remix_coefficient`, `pipeline.remix_host`
(the numpy float32 restatement of lass_remix_encode's value), `pipeline.check_remix_args`, and what the feature is for, on the
float64 host definition of the resampler (`resample.resample_host`): a remix formed at the file's rate keeps the band above the
model's Nyquist, which the plain down-and-up path loses."""
import ctypes
import os

import numpy as np
import pytest

from lass_amd import pipeline, wavio
from lass_amd import resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C-ABI --------------------------------------------------------------------------------------------------------------
def test_remix_symbols_declared_bound_and_refuse_a_null_context():
    import __graft_entry__ as g
    g.build()
    from lass_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "lass_hip.h")) as f:
        header = f.read()
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert "int lass_remix_encode(lass_ctx* ctx," in header and "int lass_remix_peak(lass_ctx* ctx," in header
    # lass_resample_encode_gain's 18 and the dry source's four; lass_resample_peak's 14 and the same four
    assert len(bound["lass_remix_encode"]) == len(bound["lass_resample_encode_gain"]) + 4 == 22
    assert len(bound["lass_remix_peak"]) == len(bound["lass_resample_peak"]) + 4 == 18
    p = ctypes.c_void_p(0)
    assert lib.lass_remix_encode(None, p, 0, 0, 1, 1, 1, 1, 1, p, 1, p, 0, 0, p, 0, p, p, 0, 1, p, p) == -1      # LASS_ERR_ARG
    assert lib.lass_remix_peak(None, p, 0, 0, 1, 1, 1, 1, 1, p, 1, p, 0, 0, p, 1, p, p) == -1
    assert os.path.exists(os.path.join(g.CSRC, "wav_sample.h"))


# ---- the coefficient ----------------------------------------------------------------------------------------------------
def test_remix_coefficient():
    k = pipeline.remix_coefficient
    assert isinstance(k(-np.inf), np.float32) and k(-np.inf) == np.float32(-1.0) and k(float("-inf")) == -1.0
    assert k(0) == np.float32(0.0) and k(0.0) == 0.0 and k(-0.0) == 0.0
    one = np.float32(1.0)
    assert np.nextafter(one, np.float32(0)) <= k(6.0206) <= np.nextafter(one, np.float32(2))                  # within 1 ulp of 1
    assert k(-12.0) == np.float32(10.0 ** (-12.0 / 20.0) - 1.0) and -1.0 < k(-12.0) < 0.0 < k(6.0)
    for bad in (np.nan, float("nan"), np.inf, float("inf"), 1e5, "loud", None):
        with pytest.raises(ValueError):
            k(bad)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_remix_host_is_two_float32_roundings():
    rng = np.random.Generator(np.random.PCG64(21))
    x = rng.standard_normal(4096).astype(np.float32)
    y = rng.standard_normal(4096).astype(np.float32)
    k = np.float32(0.41)                                       # no power of two: fl(k * y) rounds on nearly every sample
    got = pipeline.remix_host(x, y, k)
    assert got.dtype == np.float32 and got.shape == x.shape
    p = (k * y).astype(np.float32)
    assert np.array_equal(got, (x + p).astype(np.float32))
    # one by one, through float64 with an explicit rounding after each operation (both are exact in float64 before it)
    step = np.float32(np.float64(x) + np.float64(np.float32(np.float64(k) * np.float64(y))))
    assert np.array_equal(got, step)
    once = (x.astype(np.float64) + np.float64(k) * y.astype(np.float64)).astype(np.float32)      # what an fma would give
    differing = int(np.count_nonzero(got != once))
    print(f"two roundings differ from one on {differing} of {x.size} samples")
    assert differing >= 1
    # k = 0 returns x (as values: x + 0), a gain is one more rounding
    assert np.array_equal(pipeline.remix_host(x, y, 0.0), x) and np.array_equal(pipeline.remix_host(x, y, np.float32(0)), x)
    g = np.float32(0.7)
    assert np.array_equal(pipeline.remix_host(x, y, k, gain=g), (g * got).astype(np.float32))
    assert np.array_equal(pipeline.remix_host(x, y, k, gain=np.float32(1)), got)
    # (C, frames) planes as the pipeline hands them over
    assert np.array_equal(pipeline.remix_host(x.reshape(2, -1), y.reshape(2, -1), k), got.reshape(2, -1))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_check_remix_args_refuses_before_the_model_is_touched(tmp_path):
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    wavio.write_wav_pcm16(a, np.zeros((2000, 2), dtype=np.float32), 44100)
    wavio.write_wav_f32(b, np.zeros(2000, dtype=np.float32), 16000)
    jobs = [(a, "a dog", str(tmp_path / "oa.wav")), (b, "rain", str(tmp_path / "ob.wav"))]

    def run(jobs=jobs, **kw):
        return pipeline.separate_files(None, jobs, 16000, **kw)     # the model is None: a refusal must come before its first use

    with pytest.raises(ValueError, match='channels="each"'):
        run(target_gain_db=-6.0, channels="mono")
    with pytest.raises(ValueError, match=r"a\.wav.*own rate \(44100 Hz\).*48000"):
        run(target_gain_db=-6.0, out_rate=48000)
    with pytest.raises(ValueError, match=r"b\.wav.*own rate \(16000 Hz\).*44100"):
        run(target_gain_db=-6.0, out_rate=44100)                    # the first file's own rate is not the second's
    with pytest.raises(ValueError, match="loudness measures the separated planes"):
        run(target_gain_db=-6.0, loudness=-23.0)
    with pytest.raises(ValueError, match="meter measures the separated planes"):
        run(target_gain_db=-6.0, meter=True)
    with pytest.raises(ValueError, match="limiter measures the separated planes"):
        run(target_gain_db=-6.0, limiter=True, peak_ceiling_db=-1.0)
    with pytest.raises(ValueError, match='peak="true" measures the separated planes'):
        run(target_gain_db=-6.0, peak="true", peak_ceiling_db=-1.0)
    with pytest.raises(ValueError, match="2 jobs"):
        run(target_gain_db=[-6.0])
    for bad in (np.nan, np.inf, [0.0, np.nan]):
        with pytest.raises(ValueError, match="target_gain_db"):
            run(target_gain_db=bad)
    four = [j + (str(tmp_path / "r.wav"),) for j in jobs]
    with pytest.raises(ValueError, match="needs a target_gain_db"):
        run(jobs=four)
    with pytest.raises(ValueError, match="a job is"):
        run(jobs=[(a, "a dog")], target_gain_db=0.0)
    # what remix mode does take passes the check - and only then is the model touched
    args = dict(channels="each", out_rate=None, loudness=None, meter=False, limiter=False, peak="sample")
    assert pipeline.check_remix_args(None, jobs, **args) is None
    assert pipeline.check_remix_args(-np.inf, jobs, **args) == [-np.inf, -np.inf]
    assert pipeline.check_remix_args([-12, 6.0], four, **args) == [-12.0, 6.0]
    assert pipeline.check_remix_args(3.0, jobs[:1], **dict(args, out_rate=44100)) == [3.0]
    with pytest.raises(AttributeError):
        run(target_gain_db=-6.0, peak_ceiling_db=-1.0)
    assert not os.path.exists(jobs[0][2])


# ---- what it is for -----------------------------------------------------------------------------------------------------
def _energy_above(x: np.ndarray, rate: int, f_lo: float):
    """(x's energy at frequencies above f_lo, all of it), from its spectrum."""
    p = np.abs(np.fft.rfft(x)) ** 2
    f = np.fft.rfftfreq(x.shape[0], 1.0 / rate)
    return float(p[f > f_lo].sum()), float(p.sum())


@pytest.mark.parametrize("rate,model_rate", [(44100, 16000), (48000, 16000), (48000, 32000), (44100, 32000)])
def test_the_full_band_survives_a_remix(rate, model_rate):
    """All in float64 with `resample.resample_host`, the definition the device kernels are pinned to.  remix - original is
    k x the estimate brought up to the file's rate, so it holds nothing above the model's Nyquist but the filter's stop-band
    leak: its energy above 1.2 x that Nyquist is at most -60 dB of its total (measured: -62.6 to -64.1 dB with seed 0 over the four
    pairs, the spectrum taken over the whole row, rectangular, cut to the file's frame count as the pipeline cuts it), whatever the
    original holds up there.  The plain path, down and up again, returns a tone
    at 0.75 x the model rate under 1e-5 of its amplitude (measured 1.1e-7 ... 2.2e-6 of it; the amplitude at the tone's own
    frequency, taken under a Hann window - what else comes back is the tone folded into the band by the decimation, at the
    filter's stop-band level): the loss the remix avoids."""
    frames = 2 * rate
    up, down = rs.ratio(rate, model_rate)
    rng = np.random.Generator(np.random.PCG64(0))
    estimate = 0.1 * rng.standard_normal(rs.out_len(frames, up, down))          # white noise at the model rate
    t = np.arange(frames) / rate
    # above the model's Nyquist; a cosine, since 0.75 x 32 kHz IS the Nyquist frequency of a 48 kHz file, where a sine vanishes
    # (the amplitude read below is then twice the true one: the bar is held all the same)
    tone = 0.3 * np.cos(2 * np.pi * 0.75 * model_rate * t)
    original = tone + 0.2 * np.sin(2 * np.pi * 440.0 * t)
    wet = rs.resample_host(estimate, down, up)[:frames]
    assert wet.shape[0] == frames
    for db in (-np.inf, -12.0, 6.0):
        k = np.float64(pipeline.remix_coefficient(db))
        remix = original + k * wet
        above, total = _energy_above(remix - original, rate, 1.2 * model_rate / 2)
        leak = 10.0 * np.log10(above / total)
        print(f"{rate} Hz file, {model_rate} Hz model, {db} dB: remix - original holds {leak:.1f} dB above 1.2 x Nyquist")
        assert leak <= -60.0
    # the plain path loses what the remix keeps
    back = rs.resample_host(rs.resample_host(tone, up, down), down, up)[:frames]
    mid = slice(frames // 4, 3 * frames // 4)
    w = np.hanning(frames // 2)
    left = 2.0 * abs(np.sum(w * back[mid] * np.exp(-2j * np.pi * 0.75 * model_rate * t[mid]))) / w.sum() / 0.3
    alias = float(np.max(np.abs(back[mid]))) / 0.3
    print(f"a {0.75 * model_rate:.0f} Hz tone through {rate} -> {model_rate} -> {rate} Hz comes back at {left:.2e} of its amplitude "
          f"(and leaves {alias:.2e} of it elsewhere in the band, folded by the decimation)")
    assert left < 1e-5
    # ... and the remix still holds it: its energy up there is the original's (the leak above is 1e-6 of a weaker signal)
    remix = original + np.float64(pipeline.remix_coefficient(-np.inf)) * wet
    kept, had = _energy_above(remix, rate, 1.2 * model_rate / 2)[0], _energy_above(original, rate, 1.2 * model_rate / 2)[0]
    assert 0.99 * had <= kept <= 1.01 * had
    # at 0 dB the remix is the input
    x32, w32 = original.astype(np.float32), wet.astype(np.float32)
    assert np.array_equal(pipeline.remix_host(x32, w32, pipeline.remix_coefficient(0.0)), x32)
