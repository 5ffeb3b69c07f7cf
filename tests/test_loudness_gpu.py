"""Levelled export on the GPU: the BS.1770 meter (`lass_loudness`), the peak of what the encoder quantises (`lass_resample_peak`),
the gain rule (`lass_loudness_gain`), the encoder with a gain (`lass_resample_encode_gain`) and `pipeline.separate_files` with
`loudness=` / `peak_ceiling_db=`.

Yardsticks: the meter against lass_amd/loudness.py in float64 under the project's usual bar - 4 x the deviation of a float32 host
evaluation of the same cascade from the float64 one, on the same signal; peak, gain and bytes by equality with the pieces they are
built from; the pipeline against the same call's float32 export times the gain the device held."""
import os

import numpy as np
import pytest
import torch

from lass_amd import loudness as ld
from lass_amd import pipeline, wavio
from lass_amd import resample as rs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WRITERS = {"pcm16": wavio.write_wav_pcm16, "pcm32": wavio.write_wav_pcm32, "f32": wavio.write_wav_f32}
DTYPES = {"pcm16": "<i2", "pcm32": "<i4", "f32": "<f4"}
LENGTHS = {16000: [6400, 7999, 8000, 20001, 100003], 32000: [12801, 40007]}


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


@pytest.fixture(scope="module")
def scratch_wav(tmp_path_factory):
    return str(tmp_path_factory.mktemp("loudness") / "host.wav")


def _signal(kind: str, frames: int, rate: int, nch: int, seed):
    """tests/test_export_gpu.py::_signal with the noise at -20 dBFS: seeded noise, or two tones inside every pass band."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "noise":
        return (0.1 * rng.standard_normal((frames, nch))).astype(np.float32)
    t = np.arange(frames)[:, None] / rate
    f1, f2 = 0.011 * rate, 0.12 * rate
    ph = rng.uniform(0, 2 * np.pi, (2, nch))
    return (0.4 * np.sin(2 * np.pi * f1 * t + ph[0]) + 0.3 * np.sin(2 * np.pi * f2 * t + ph[1])).astype(np.float32)


def _host_bytes(scratch, x, enc) -> np.ndarray:
    WRITERS[enc](scratch, x, 16000)
    with open(scratch, "rb") as f:
        return np.frombuffer(f.read()[44:], dtype=np.uint8)


def _gate_case(rate: int) -> np.ndarray:
    """tests/test_loudness_cpu.py's gate case as float32 stereo: 2 s at -80 dBFS, 3 s at -20, 3 s at -45 (33 of 77 blocks survive)."""
    n = [2 * rate, 3 * rate, 3 * rate]
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for db, k in zip((-80, -20, -45), n)])
    x = amp * np.sin(2.0 * np.pi * 1000.0 * np.arange(sum(n)) / rate)
    return np.stack([x, x]).astype(np.float32)


class Case:
    """One (rate, kind, channels): the planes (C, longest length) - a recording of n samples is their first n - with the float64
    and float32 K-weighted planes, each evaluated once."""

    def __init__(self, rate, kind, C):
        self.rate, self.kind, self.C, self.lengths = rate, kind, C, LENGTHS[rate]
        self.x = np.ascontiguousarray(_signal(kind, max(self.lengths), rate, C, [11, rate, C, kind == "noise"]).T)
        self.weights = None if C < 3 else np.array([1.0, 0.5, 1.41], dtype=np.float32)
        self.y32 = None                                               # (the `cases` fixture fills it in)

    def host(self, n):
        """(float64 block powers, the bar: 4 x the largest relative deviation of the float32 evaluation's blocks)."""
        p = ld.block_powers(self.x[:, :n], self.rate, self.weights)
        p32 = ld.powers_of_weighted(self.y32[:, :n], self.rate, self.weights, np.float32)
        return p, 4.0 * float(np.max(np.abs(p32.astype(np.float64) - p) / p))

    def batch(self, order=None, pad=(1, 5)):
        """(planes (B, C, L) behind non-dense strides with noise past every recording's end, lengths) in the given row order."""
        order = list(range(len(self.lengths))) if order is None else order
        L = max(self.lengths)
        big = 0.3 * torch.randn(len(order), self.C + pad[0], L + pad[1], generator=torch.Generator().manual_seed(12))
        for row, k in enumerate(order):
            big[row, :self.C, :self.lengths[k]] = torch.from_numpy(self.x[:, :self.lengths[k]])
        view = big.to(DEV)[:, :self.C, :L]
        assert view.stride(0) == (self.C + pad[0]) * (L + pad[1]) and view.stride(1) == L + pad[1]
        return view, torch.tensor([self.lengths[k] for k in order], dtype=torch.int32)


@pytest.fixture(scope="module")
def cases():
    all_ = [Case(16000, kind, C) for kind in ("noise", "two-tone") for C in (1, 2, 3)] + \
           [Case(32000, kind, 2) for kind in ("noise", "two-tone")]
    for rate in LENGTHS:                 # the plain float32 recurrence, sample by sample: all planes of a rate in one walk
        mine = [cs for cs in all_ if cs.rate == rate]
        y32 = ld.k_weighted(np.concatenate([cs.x for cs in mine]), rate, np.float32)
        at = 0
        for cs in mine:
            cs.y32 = y32[at:at + cs.C]
            at += cs.C
    return all_


# ---- 1. the meter -------------------------------------------------------------------------------------------------------
def test_block_powers_against_the_float64_host(eng, cases):
    """Ragged batches: 6 400 samples is the single block, 7 999 one sample short of a second hop, 8 000 exactly two hops on...,
    100 003 sixty-two carries across hop bins."""
    worst = 0.0
    for cs in cases:
        planes, lengths = cs.batch()
        loud, blocks, counts = eng.loudness(planes, cs.rate, lengths=lengths, weights=cs.weights, return_blocks=True, return_counts=True)
        assert blocks.shape == (len(cs.lengths), ld.n_blocks(max(cs.lengths), cs.rate)) and blocks.dtype == torch.float64
        blocks, counts = blocks.cpu().numpy(), counts.cpu().numpy()
        for row, n in enumerate(cs.lengths):
            p, bar = cs.host(n)
            nb = p.shape[0]
            assert counts[row, 0] == nb == ld.n_blocks(n, cs.rate) and nb >= 1
            err = float(np.max(np.abs(blocks[row, :nb] - p) / p))
            print(f"{cs.rate} Hz {cs.kind} C={cs.C} n={n}: {nb} blocks, worst relative error {err:.3e}, bar {bar:.3e}")
            assert err <= bar and not blocks[row, nb:].any()
            worst = max(worst, err)
    print(f"worst relative block error over all cases {worst:.3e}")


def test_integrated_loudness_against_the_host(eng, cases):
    for cs in cases:
        planes, lengths = cs.batch()
        loud, counts = eng.loudness(planes, cs.rate, lengths=lengths, weights=cs.weights, return_counts=True)
        assert loud.shape == (len(cs.lengths),) and loud.dtype == torch.float64
        for row, n in enumerate(cs.lengths):
            p, bar = cs.host(n)
            _check_gated(p, bar, float(loud[row]), counts[row].cpu().numpy(), f"{cs.rate} Hz {cs.kind} C={cs.C} n={n}")
    # the gate case: both gates drop blocks
    x = _gate_case(16000)
    p = ld.block_powers(x, 16000)
    p32 = ld.powers_of_weighted(ld.k_weighted(x, 16000, np.float32), 16000, None, np.float32)
    bar = 4.0 * float(np.max(np.abs(p32.astype(np.float64) - p) / p))
    loud, counts = eng.loudness(torch.from_numpy(x).to(DEV), 16000, return_counts=True)
    assert ld.gate(p)[1] == 33
    _check_gated(p, bar, float(loud[0]), counts[0].cpu().numpy(), "gate case")


def _check_gated(p, bar, loud, counts, what):
    """The host's gates are not within 1e-3 LU of any block (else the comparison would be a coin toss); then the same count
    and a loudness within what `bar` on every block power allows: 10 log10(1 + bar)."""
    l = ld.OFFSET + 10.0 * np.log10(p)
    absolute = l > ld.ABSOLUTE_GATE
    rel = ld.OFFSET + 10.0 * np.log10(np.mean(p[absolute])) + ld.RELATIVE_GATE
    assert np.min(np.abs(l - ld.ABSOLUTE_GATE)) > 1e-3 and np.min(np.abs(l - rel)) > 1e-3, what
    want, kept = ld.gate(p)
    bar_db = 10.0 * np.log10(1.0 + bar)
    print(f"{what}: host {want:.6f} LUFS, device {loud:.6f}, difference {abs(loud - want):.3e} (bar {bar_db:.3e}), {kept} of {p.shape[0]} blocks")
    assert counts[0] == p.shape[0] and counts[1] == kept
    assert abs(loud - want) <= bar_db


def test_nothing_to_measure_is_minus_infinity(eng):
    x = torch.from_numpy(_signal("noise", 6400, 16000, 2, [13]).T.copy()).to(DEV)
    loud, blocks, counts = eng.loudness(x[:, :6399].contiguous(), 16000, return_blocks=True, return_counts=True)
    assert float(loud[0]) == float("-inf") and counts[0].tolist() == [0.0, 0.0] and blocks.shape == (1, 0)
    loud, counts = eng.loudness(x, 16000, lengths=[6399], return_counts=True)      # the same through `lengths`
    assert float(loud[0]) == float("-inf") and counts[0].tolist() == [0.0, 0.0]
    loud, counts = eng.loudness(torch.zeros(1, 2, 16000, device=DEV), 16000, return_counts=True)
    assert float(loud[0]) == float("-inf") and counts[0].tolist() == [7.0, 0.0]
    both, counts = eng.loudness(torch.stack([torch.zeros_like(x), x]), 16000, return_counts=True)    # silence beside a signal
    assert float(both[0]) == float("-inf") and np.isfinite(float(both[1])) and counts[:, 1].tolist() == [0.0, 1.0]


def test_a_recording_measures_the_same_alone_and_in_a_batch(eng, cases):
    """Each recording alone (dense, L its own length) against its row in a shuffled batch behind other strides, in another call."""
    for cs in cases[1:3] + cases[6:7]:
        order = [3, 0, 4, 2, 1][:len(cs.lengths)] if len(cs.lengths) == 5 else [1, 0]
        planes, lengths = cs.batch(order, pad=(2, 9))
        loud, blocks, counts = eng.loudness(planes, cs.rate, lengths=lengths, weights=cs.weights, return_blocks=True, return_counts=True)
        for row, k in enumerate(order):
            n = cs.lengths[k]
            alone = torch.from_numpy(cs.x[:, :n].copy()).to(DEV)
            l1, b1, c1 = eng.loudness(alone, cs.rate, weights=cs.weights, return_blocks=True, return_counts=True)
            nb = b1.shape[1]
            assert torch.equal(l1[0], loud[row]) and torch.equal(c1[0], counts[row]) and torch.equal(b1[0], blocks[row, :nb]), (cs.kind, n)
            assert np.isfinite(float(l1[0])) and nb == ld.n_blocks(n, cs.rate)


def test_meter_bad_arguments_are_refused(eng):
    from lass_amd import _lib
    x = torch.zeros(1, 2, 16000, device=DEV)
    with pytest.raises(ValueError):
        eng.loudness(x, 11025)
    with pytest.raises(_lib.LassError, match="channels"):
        eng.loudness(torch.zeros(1, 9, 16000, device=DEV), 16000)
    with pytest.raises(_lib.LassError, match="lengths"):
        eng.loudness(x, 16000, lengths=[1, 2])


# ---- 2. the peak --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", [(16000, 16000), (16000, 44100), (32000, 48000)])
def test_resample_peak_is_the_peak_of_the_resampled_planes(eng, rate_in, rate_out):
    B, C, L_in = 3, 2, 4001
    ceiling = rs.out_len(L_in, *rs.ratio(rate_in, rate_out))
    x = torch.from_numpy(np.stack([_signal("noise" if b % 2 else "two-tone", L_in, rate_in, C, [14, b, rate_out]).T for b in range(B)]))
    x[0, 1, L_in - 2] = 3.0                                  # a peak that the shorter frames_out cuts off (rows 0)
    x[2, 0, 17] = -2.5                                       # a negative peak
    big = torch.randn(B, C + 1, L_in + 3)
    big[:, :C, :L_in] = x
    view = big.to(DEV)[:, :C, :L_in]
    for frames_out in (ceiling, ceiling - 7):
        y = torch.stack([eng.resample(view[b].contiguous(), rate_in, rate_out) for b in range(B)])     # (B, C, ceiling)
        want = y[:, :, :frames_out].abs().amax(dim=(1, 2))
        got = eng.resample_peak(view, rate_in, rate_out, frames_out=frames_out)
        assert got.dtype == torch.float32 and torch.equal(got, want), (frames_out, got, want)
        assert torch.equal(eng.resample_peak(view[1], rate_in, rate_out, frames_out=frames_out), want[1:2])     # alone, other call
    assert float(eng.resample_peak(view, rate_in, rate_out)[0]) > float(eng.resample_peak(view, rate_in, rate_out, frames_out=ceiling - 7)[0])
    # a NaN is skipped (with a filter it spreads over the taps' reach, all of which is skipped)
    hole = view.clone()
    hole[1, 0, 2000] = float("nan")
    y = eng.resample(hole[1].contiguous(), rate_in, rate_out)
    assert bool(torch.isnan(y).any())
    got = eng.resample_peak(hole, rate_in, rate_out)
    assert torch.equal(got[1], torch.nan_to_num(y.abs(), nan=0.0).max()) and float(got[1]) > 0.1


# ---- 3. the encoder with a gain -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", [(16000, 16000), (16000, 44100)])
def test_encode_with_gain(eng, scratch_wav, rate_in, rate_out):
    B, C, L_in = 3, 2, 1500
    ceiling = rs.out_len(L_in, *rs.ratio(rate_in, rate_out))
    x = torch.from_numpy(np.ascontiguousarray(np.stack([_signal("two-tone", L_in, rate_in, C, [15, b, rate_out]).T for b in range(B)])))
    x[:, :, 100:110] *= 3.0
    x = x.to(DEV)
    gains = np.array([0.5, 1.7, 3e-3], dtype=np.float32)
    y = torch.stack([eng.resample(x[b], rate_in, rate_out) for b in range(B)]).cpu().numpy()          # (B, C, ceiling)
    for enc in ("pcm16", "pcm32", "f32"):
        for frames_out in (ceiling, ceiling - 4):
            plain_clips, one_clips, clips = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(3))
            plain = eng.resample_encode(x, rate_in, rate_out, enc, frames_out=frames_out, clipped=plain_clips)
            ones = eng.resample_encode(x, rate_in, rate_out, enc, frames_out=frames_out, clipped=one_clips, gain=torch.ones(B, device=DEV))
            assert torch.equal(ones, plain) and torch.equal(one_clips, plain_clips)
            got = eng.resample_encode(x, rate_in, rate_out, enc, frames_out=frames_out, clipped=clips, gain=torch.from_numpy(gains).to(DEV))
            for b in range(B):
                prod = (gains[b] * y[b, :, :frames_out]).astype(np.float32)                         # one float32 rounding
                assert np.array_equal(got[b].cpu().numpy(), _host_bytes(scratch_wav, prod.T, enc)), (enc, frames_out, b)
                assert int(clips[b]) == pipeline.host_clip_count(prod, enc)
            assert int(clips[1]) > 0 or enc == "f32"
    from lass_amd import _lib
    with pytest.raises(_lib.LassError, match="gain"):
        eng.resample_encode(x, rate_in, rate_out, "pcm16", gain=torch.ones(B + 1, device=DEV))


# ---- 4. the gain rule ---------------------------------------------------------------------------------------------------
def test_gain_kernel_equals_the_host_rule(eng):
    rng = np.random.Generator(np.random.PCG64(16))
    loud = np.concatenate([rng.uniform(-60.0, -5.0, 200), [float("-inf"), float("inf"), float("nan"), -23.0, -70.0]])
    peak = np.concatenate([rng.uniform(1e-3, 2.0, 200), [3.0, 0.5, 0.7, 0.8912509, 1e-30]]).astype(np.float32)
    for target, ceiling in [(-23.0, None), (None, ld.ceiling_for(-1.0, "f32")), (-23.0, ld.ceiling_for(-1.0, "f32")),
                            (-14.0, ld.ceiling_for(0.0, "pcm16")), (-14.0, ld.ceiling_for(0.0, "pcm32")), (None, None)]:
        gain, limited = eng.loudness_gain(torch.from_numpy(loud), torch.from_numpy(peak), target, None if ceiling is None else float(ceiling))
        want = [ld.gain_for(l, p, target, ceiling) for l, p in zip(loud, peak)]
        wg, wb = np.array([w[0] for w in want], dtype=np.float32), np.array([w[1] for w in want], dtype=np.int32)
        assert np.array_equal(gain.cpu().numpy().view(np.uint32), wg.view(np.uint32)), (target, ceiling)
        assert np.array_equal(limited.cpu().numpy(), wb)
        if target is not None and ceiling is not None:
            assert 0 < int(wb.sum()) < wb.shape[0]           # peaks that bite and peaks that do not
        if ceiling is not None:
            assert not np.any((wg * peak).astype(np.float32) > ceiling)
    gain, limited = eng.loudness_gain(torch.from_numpy(loud), None, -23.0, None)     # no peak without a ceiling
    assert np.array_equal(gain.cpu().numpy(), np.array([ld.gain_for(l, None, -23.0, None)[0] for l in loud], dtype=np.float32))


# ---- 5. separate_files --------------------------------------------------------------------------------------------------
SR = 16000
TARGET, CEILING_DB = -23.0, -1.0
# |host float64 meter on the written 44.1 kHz float32 file - target|, measured at 0.1575 LU: the meter's rate dependence, 16 kHz
# against 44.1 kHz.  The file is broadband (white noise under the tones), and near the 16 kHz meter's Nyquist frequency the
# bilinear shelf and the resampler's transition band both depart from the 44.1 kHz reading (a 7.5 kHz tone reads 1.6 LU apart on
# the host alone, white noise 0.15 LU; 1 kHz, as in the EBU cases, 0.04 LU).  DESIGN.md section 18.  Asserted at 3 x the value.
MEASURED_MARGIN = 0.1575


def _make_model(sd):
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return AudioSep(ss_model=m.to(DEV).eval().set_compute_dtype("f32"), query_encoder=PrecomputedQueryEncoder())


@pytest.fixture(scope="module")
def holder(synthetic_sd):
    return _make_model(synthetic_sd)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two 1 s files.  clicks.wav, 16 kHz mono PCM16: five clicks on a faint noise floor - a crest factor far over the 22 dB
    between the target and the ceiling, so the ceiling decides its gain.  tones.wav, 44.1 kHz stereo float32: noise and tones with
    a crest factor of some 12 dB, which the ceiling leaves alone."""
    d = tmp_path_factory.mktemp("level")
    clicks = 0.002 * _signal("noise", 16000, 16000, 1, [17])[:, 0]
    clicks[[1500, 4700, 8100, 11000, 14300]] = [0.9, -0.8, 0.9, 0.7, -0.9]
    tones = 0.6 * _signal("noise", 44100, 44100, 2, [18]) + 0.5 * _signal("two-tone", 44100, 44100, 2, [18, 1])
    paths = [str(d / "clicks.wav"), str(d / "tones.wav")]
    wavio.write_wav_pcm16(paths[0], clicks, 16000)
    wavio.write_wav_f32(paths[1], tones, 44100)
    return d, paths


def _payload(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()[44:]


def test_separate_files_at_a_level(holder, scratch_wav, files):
    d, paths = files
    caps = ["a dog barking", "rain on a roof"]
    flat = [str(d / f"flat{k}.wav") for k in range(2)]
    outs = [str(d / f"level{k}.wav") for k in range(2)]
    pipeline.separate_files(holder, list(zip(paths, caps, flat)), SR, encoding="f32")
    recs = pipeline.separate_files(holder, list(zip(paths, caps, outs)), SR, loudness=TARGET, peak_ceiling_db=CEILING_DB)
    ceiling = ld.ceiling_for(CEILING_DB, "f32")
    for k, (enc, nch, rate, frames) in enumerate([("pcm16", 1, 16000, 16000), ("f32", 2, 44100, 44100)]):
        rec = recs[k]
        assert wavio.wav_info(outs[k]) == (enc, nch, rate, frames, 44) and rec["path"] == "device" and rec["clipped"] == 0
        x = np.frombuffer(_payload(flat[k]), dtype="<f4").reshape(frames, nch)
        g = np.float32(rec["gain"])
        assert float(g) == rec["gain"] and rec["gain_db"] == pytest.approx(20 * np.log10(float(g)), abs=1e-9)
        prod = (g * x).astype(np.float32)
        assert _payload(outs[k]) == _host_bytes(scratch_wav, prod if nch > 1 else prod[:, 0], enc).tobytes(), paths[k]
        assert float(np.max(np.abs(prod))) <= ceiling
        # the gain is the host rule's on the device's own measurements
        peak = np.float32(np.max(np.abs(x)))
        assert ld.gain_for(rec["loudness_out"], peak, TARGET, ceiling) == (g, rec["peak_limited"])
        print(f"{os.path.basename(paths[k])}: loudness_out {rec['loudness_out']:.3f} LUFS, gain {rec['gain_db']:.3f} dB, peak {peak:.4f}, "
              f"limited {rec['peak_limited']}")
    assert [r["peak_limited"] for r in recs] == [True, False]
    assert float(np.max(np.abs(np.float32(recs[0]["gain"]) * np.frombuffer(_payload(flat[0]), dtype="<f4")))) > 0.99 * ceiling
    # the unlimited file, measured by the float64 host meter at its own rate
    y = np.frombuffer(_payload(outs[1]), dtype="<f4").reshape(44100, 2).T
    off = abs(ld.integrated_loudness(y, 44100) - TARGET)
    print(f"tones.wav written: host meter at 44 100 Hz is {off:.4f} LU off the target (asserted at {3 * MEASURED_MARGIN:.4f})")
    assert off <= 3 * MEASURED_MARGIN
    # without the ceiling the gain is the whole distance to the target, to float32 rounding
    assert abs(recs[1]["loudness_out"] + recs[1]["gain_db"] - TARGET) < 1e-5


@pytest.mark.filterwarnings("ignore:.*parity with the reference is unpinned.*:UserWarning")
def test_host_route_file_at_a_level(holder, scratch_wav, files):
    """44 101 Hz is over the tap cap both ways: decode, meter (lass_amd/loudness.py), gain rule and export run on the host."""
    d, _ = files
    odd, frames = str(d / "odd.wav"), 30000
    wavio.write_wav_pcm16(odd, 0.5 * _signal("two-tone", frames, 44101, 2, [19]), 44101)
    flat, out = str(d / "odd_flat.wav"), str(d / "odd_level.wav")
    pipeline.separate_files(holder, [(odd, "rain on a roof", flat)], SR, encoding="f32")
    rec = pipeline.separate_files(holder, [(odd, "rain on a roof", out)], SR, loudness=TARGET, peak_ceiling_db=CEILING_DB)[0]
    assert rec["path"] == "host" and rec["clipped"] == 0 and wavio.wav_info(out) == ("pcm16", 2, 44101, frames, 44)
    x = np.frombuffer(_payload(flat), dtype="<f4").reshape(frames, 2)
    g, ceiling = np.float32(rec["gain"]), ld.ceiling_for(CEILING_DB, "pcm16")
    prod = (g * x).astype(np.float32)
    assert _payload(out) == _host_bytes(scratch_wav, prod, "pcm16").tobytes()
    assert float(np.max(np.abs(prod))) <= ceiling and np.isfinite(rec["loudness_out"])
    assert ld.gain_for(rec["loudness_out"], np.float32(np.max(np.abs(x))), TARGET, ceiling) == (g, rec["peak_limited"])
    print(f"host route: loudness_out {rec['loudness_out']:.3f} LUFS, gain {rec['gain_db']:.3f} dB, limited {rec['peak_limited']}")


def test_without_a_level_nothing_changes(holder, eng, scratch_wav, files):
    """Both arguments None: the records have the parent's keys and the bytes are those of the pieces composed by hand
    (tests/test_export_gpu.py::_by_hand, for these two short files)."""
    d, paths = files
    caps = ["a dog barking", "rain on a roof"]
    outs = [str(d / f"none{k}.wav") for k in range(2)]
    recs = pipeline.separate_files(holder, list(zip(paths, caps, outs)), SR, loudness=None, peak_ceiling_db=None)
    assert all(sorted(r) == ["channels", "clipped", "frames", "path", "rate"] for r in recs)
    planes, conds, metas = [], [], []
    for p, cap in zip(paths, caps):
        enc, nch, rate, frames, _ = info = wavio.wav_info(p)
        row = np.zeros(frames * nch * rs.SAMPLE_BYTES[enc], dtype=np.uint8)
        assert wavio.read_wav_raw_into(p, info, row)
        chans = np.frombuffer(row.tobytes(), dtype=DTYPES[enc]).reshape(frames, nch)
        for c in range(nch):
            raw = np.frombuffer(np.ascontiguousarray(chans[:, c]).tobytes(), dtype=np.uint8)
            planes.append(eng.decode_resample(torch.from_numpy(raw.copy()).to(DEV), frames, 1, enc, rate, SR)[0])
            conds.append(holder.query_encoder.get_query_embed(modality="text", text=[cap], device=DEV)[0])
        metas.append((enc, rate, frames, nch))
    seps = holder.ss_model.separate_long_list(planes, torch.stack(conds), window=160000, context=16000, fade=0)
    at = 0
    for k, (enc, rate, frames, n) in enumerate(metas):
        y = np.stack([eng.resample(s, SR, rate)[:frames].cpu().numpy() for s in seps[at:at + n]], axis=1)
        at += n
        assert _payload(outs[k]) == _host_bytes(scratch_wav, y if n > 1 else y[:, 0], enc).tobytes(), paths[k]
