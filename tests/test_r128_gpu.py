"""EBU R 128 on the GPU: the true peak of what the encoder quantises (`lass_resample_true_peak`), the
loudness range and the two maxima beside the integrated loudness (`lass_loudness_stats`), and `pipeline.separate_files` with
`peak="true"` / `meter=True`.

Yardsticks: the true peak by equality with the composition of the public pieces (`Engine.resample` of `Engine.resample`'s output)
and against lass_amd/loudness.py in float64 under the project's usual bar - 4 x the deviation of a float32 host evaluation of
the same chain from the float64 one; the short-term powers under the same bar; the order statistics by equality with numpy's sort
of the device's own powers; the pipeline against the same call's float32 export times the gain the device held, and the written
file against a bound derived from the rounding of the gain and the quantisation (section 19)."""
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


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


@pytest.fixture(scope="module")
def scratch_wav(tmp_path_factory):
    return str(tmp_path_factory.mktemp("r128") / "host.wav")


# ---- 1. the true peak ---------------------------------------------------------------------------------------------------
FRAMES = 13230                   # 0.3 s at 44.1 kHz: seven tiles of 2048, the largest the plan chooses
L_IN = {(16000, 16000): 13230, (16000, 44100): 4800, (32000, 48000): 8820}
RATES = sorted(L_IN)
# where a row's one feature sits, as the output frame its pair of equal samples ends on: the seams of every power-of-two tile up
# to 2048 and beyond, the row's first two frames and its last two
FEATURES = [(1024, 2048, 4096), (1, FRAMES - 1, 12288)]


def _pair_rows(rate_in, rate_out, C, features, seed):
    """(B, C, L_in) float32: noise at 1e-3 and, in channel b % C of row b, two equal adjacent samples of 0.5 placed so that the
    peak of the reconstructed signal lies between the output frames feature - 1 and feature (at 1 : 1 exactly there and 2.1 dB
    over the samples; with a filter as near as the input grid allows)."""
    up, down = rs.ratio(rate_in, rate_out)
    L = L_IN[(rate_in, rate_out)]
    assert rs.out_len(L, up, down) == FRAMES
    x = 1e-3 * np.random.Generator(np.random.PCG64([21, rate_out, C, seed])).standard_normal((len(features), C, L))
    for b, s in enumerate(features):
        m = min(max(int(round((s - 0.5) * down / up - 0.5)), 0), L - 2)
        x[b, b % C, m:m + 2] = 0.5
    return x.astype(np.float32)


def _padded(x):
    """x (B, C, L) on the device behind padded row and plane strides."""
    B, C, L = x.shape
    big = torch.randn(B, C + 1, L + 3, generator=torch.Generator().manual_seed(22))
    big[:, :C, :L] = torch.from_numpy(x)
    view = big.to(DEV)[:, :C, :L]
    assert view.stride(0) == (C + 1) * (L + 3) and view.stride(1) == L + 3
    return view


def _composed(eng, view, rate_in, rate_out, frames_out):
    """(true peak, sample peak), (B,) each, from the public pieces: y = resample(plane)[:frames_out], z = resample(y) at (os, 1),
    the larger of max |y| and max |z| off phase 0, over the channels.  NaNs are skipped."""
    os_ = ld.oversampling(rate_out)
    B, C, _ = view.shape
    true, sample = [], []
    for b in range(B):
        y = eng.resample(view[b].contiguous(), rate_in, rate_out)[:, :frames_out].contiguous()
        z = eng.resample(y, rate_out, os_ * rate_out)
        assert z.shape == (C, os_ * frames_out)
        sp = torch.nan_to_num(y.abs(), nan=0.0).max()
        between = torch.nan_to_num(z.view(C, frames_out, os_)[:, :, 1:].abs(), nan=0.0).max()
        sample.append(sp)
        true.append(torch.maximum(sp, between))
    return torch.stack(true), torch.stack(sample)


@pytest.mark.parametrize("rate_in,rate_out", RATES)
def test_true_peak_equals_the_composition_of_public_pieces(eng, rate_in, rate_out):
    """A tile that forgets its halo, or takes it short, loses the interpolated values next to its seams: every row's peak is one
    of those, on one seam each (or at the row's first or last two frames, where the halo is the zeros outside the row)."""
    for C in (1, 2, 3):
        for features in FEATURES:
            x = _pair_rows(rate_in, rate_out, C, features, 0)
            view = _padded(x)
            for frames_out in (FRAMES, FRAMES - 7):
                want, sample = _composed(eng, view, rate_in, rate_out, frames_out)
                got = eng.resample_true_peak(view, rate_in, rate_out, frames_out=frames_out)
                assert got.dtype == torch.float32 and got.shape == (3,)
                assert torch.equal(got, want), (C, features, frames_out, got, want)
                assert torch.equal(sample, eng.resample_peak(view, rate_in, rate_out, frames_out=frames_out))
                over = 20.0 * torch.log10(want / sample).cpu().numpy()
                print(f"{rate_in} -> {rate_out}, C={C}, features {features}, frames_out {frames_out}: true peak over sample peak by {over} dB")
                cut = [s > frames_out for s in features]              # (the truncated count cuts the last frames' pair off)
                assert all(o >= 0.0 for o in over)
                if rate_in == rate_out:
                    # the host's word on it: the peak lies between the samples, more than 1 dB over them
                    for b, s in enumerate(features):
                        if not cut[b]:
                            tp, sp = ld.true_peak(x[b, :, :frames_out], rate_out), float(np.abs(x[b, :, :frames_out]).max())
                            assert 20.0 * np.log10(tp / sp) > 1.0 and sp == 0.5
                            assert float(sample[b]) == 0.5 and 0.6 < float(want[b]) < 0.68


def _chain(x, up, down, frames_out, os_, dtype):
    """Every value the true peak of plane x is taken over - the resampled samples and the interpolated phases - evaluated on
    the host in `dtype`."""
    y = rs.resample_host(x, up, down, dtype)[:frames_out]
    z = rs.resample_host(y, os_, 1, dtype).reshape(-1, os_)[:, 1:]
    return np.concatenate([y, z.reshape(-1)])


@pytest.mark.parametrize("rate_in,rate_out", RATES)
def test_true_peak_against_the_float64_host(eng, rate_in, rate_out):
    """|max|a| - max|b|| <= max|a - b|: the bar is 4 x the largest deviation of the float32 host evaluation of the chain from the
    float64 one, over the signal, relative to the peak."""
    up, down = rs.ratio(rate_in, rate_out)
    os_ = ld.oversampling(rate_out)
    x = _pair_rows(rate_in, rate_out, 2, FEATURES[0], 1)
    x += (0.2 * np.random.Generator(np.random.PCG64([23, rate_out])).standard_normal(x.shape)).astype(np.float32)
    got = eng.resample_true_peak(torch.from_numpy(x).to(DEV), rate_in, rate_out).cpu().numpy().astype(np.float64)
    for b in range(x.shape[0]):
        c64 = [_chain(x[b, c].astype(np.float64), up, down, FRAMES, os_, np.float64) for c in range(2)]
        c32 = [_chain(x[b, c], up, down, FRAMES, os_, np.float32) for c in range(2)]
        want = max(float(np.abs(c).max()) for c in c64)
        y64 = np.stack([rs.resample_host(x[b, c].astype(np.float64), up, down)[:FRAMES] for c in range(2)])
        assert want == ld.true_peak(y64, rate_out)
        bar = 4.0 * max(float(np.abs(a.astype(np.float64) - d).max()) for a, d in zip(c32, c64)) / want
        err = abs(got[b] - want) / want
        print(f"{rate_in} -> {rate_out} row {b}: true peak {want:.6f}, device off by {err:.3e} relative, bar {bar:.3e}")
        assert err <= bar


def test_true_peak_alone_and_in_a_batch_and_with_a_nan(eng):
    rate_in, rate_out = 16000, 44100
    x = _pair_rows(rate_in, rate_out, 2, FEATURES[0], 2)
    view = _padded(x)
    batch = eng.resample_true_peak(view, rate_in, rate_out)
    for b in (2, 0, 1):
        alone = eng.resample_true_peak(torch.from_numpy(x[b]).to(DEV), rate_in, rate_out)             # dense, another call
        assert torch.equal(alone, batch[b:b + 1])
    assert torch.equal(eng.resample_true_peak(view.flip(0), rate_in, rate_out), batch.flip(0))       # another row
    hole = view.clone()
    hole[1, 1, 2000] = float("nan")                                  # it spreads over both filters' reach, all of it skipped
    want, _ = _composed(eng, hole, rate_in, rate_out, FRAMES)
    got = eng.resample_true_peak(hole, rate_in, rate_out)
    assert torch.equal(got, want) and float(got[1]) > 0.4 and not bool(torch.isnan(got).any())
    # os == 1: the sample peak
    assert torch.equal(eng.resample_true_peak(view, rate_in, 192000), eng.resample_peak(view, rate_in, 192000))


def test_true_peak_refusals(eng):
    from lass_amd import _lib
    from lass_amd.engine import _ptr, _stream
    x = torch.zeros(1, 1, 4800, device=DEV)
    peak = torch.zeros(1, device=DEV)
    taps, os_taps = rs.device_taps(441, 160, DEV), rs.device_taps(4, 1, DEV)

    def call(up=441, down=160, t=taps, n_taps=None, frames_out=13230, os_=4, n_os=81):
        rc = eng.lib.lass_resample_true_peak(eng.ctx, _ptr(x), 4800, 4800, 1, 1, 4800, up, down, _ptr(t), t.numel() if n_taps is None else n_taps,
                                             frames_out, os_, _ptr(os_taps), n_os, _ptr(peak), _stream(eng.device))
        return rc, (eng.lib.lass_last_error(eng.ctx) or b"").decode()

    assert call()[0] == 0
    for kw, word in ((dict(os_=3), "os must be"), (dict(os_=1), "os must be"), (dict(n_os=80), "n_os_taps"), (dict(os_=2), "n_os_taps"),
                     (dict(frames_out=13231), "frames_out"), (dict(up=1, down=50000, n_taps=1000001, frames_out=1), "taps"),
                     (dict(up=1, down=800, t=rs.device_taps(1, 800, DEV), frames_out=6), "LDS")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("lass_resample_true_peak: ") and word in msg, (kw, rc, msg)
    # the host predicate is the launcher's formula: the ratios on either side of the edge
    edge = max(d for d in range(400, 800) if rs.true_peak_fits(1, d, 4))
    assert call(up=1, down=edge, t=rs.device_taps(1, edge, DEV), frames_out=1)[0] == 0
    assert call(up=1, down=edge + 1, t=rs.device_taps(1, edge + 1, DEV), frames_out=1)[0] == -1
    with pytest.raises(_lib.LassError, match="frames_out"):
        eng.resample_true_peak(x, 16000, 44100, frames_out=13231)
    assert pipeline.route(("pcm16", 1, 16000, 16000, 44), 16000, 20, true_peak=True) == "host"
    assert pipeline.route(("pcm16", 1, 16000, 16000, 44), 16000, 20) == "device"


# ---- 2. loudness range and the maxima -----------------------------------------------------------------------------------
STATS_LENGTHS = {16000: [46400, 48000, 49600, 196800, 480000], 32000: [112000, 198400]}
STEPS_DB = [-20, -30, -80, -80, -26, -47, -20, -38, -52, -52, -23, -32, -29, -44, -24]    # one level per 2 s


class StatsCase:
    """Stereo (plus a weighted third channel at 32 kHz) 1 kHz tone over faint noise, its level stepped every 2 s so that both
    gates drop short-term blocks; a recording of n samples is the first n.  The float64 and float32 K-weighted planes are
    evaluated once (the float32 one in hop-long chunks, as the device cuts the recurrence)."""

    def __init__(self, rate):
        self.rate, self.lengths = rate, STATS_LENGTHS[rate]
        self.C = 2 if rate == 16000 else 3
        self.weights = None if self.C == 2 else np.array([1.0, 0.5, 1.41], dtype=np.float32)
        N = max(self.lengths)
        amp = np.repeat(10.0 ** (np.array(STEPS_DB) / 20.0), 2 * rate)[:N]
        rng = np.random.Generator(np.random.PCG64([24, rate]))
        t = np.arange(N) / rate
        ph = rng.uniform(0, 2 * np.pi, self.C)[:, None]
        self.x = (amp * (np.sin(2 * np.pi * 1000.0 * t + ph) + 0.05 * rng.standard_normal((self.C, N)))).astype(np.float32)
        self.y64 = ld.k_weighted(self.x, rate)
        self.y32 = ld.k_weighted(self.x, rate, np.float32, chunk=rate // 10)

    def host(self, n):
        """(block powers, short-term powers, the bar: 4 x the largest relative deviation of the float32 evaluation's short-term
        powers), all of the float64 host."""
        p = ld.powers_of_weighted(self.y64[:, :n], self.rate, self.weights)
        q = ld.short_term_powers_of_weighted(self.y64[:, :n], self.rate, self.weights)
        q32 = ld.short_term_powers_of_weighted(self.y32[:, :n], self.rate, self.weights, np.float32)
        bar = 4.0 * float(np.max(np.abs(q32.astype(np.float64) - q) / q)) if q.size else 0.0
        return p, q, bar

    def batch(self, order=None, pad=(1, 5)):
        order = list(range(len(self.lengths))) if order is None else order
        L = max(self.lengths)
        big = 0.3 * torch.randn(len(order), self.C + pad[0], L + pad[1], generator=torch.Generator().manual_seed(25))
        for row, k in enumerate(order):
            big[row, :self.C, :self.lengths[k]] = torch.from_numpy(self.x[:, :self.lengths[k]])
        view = big.to(DEV)[:, :self.C, :L]
        assert view.stride(1) == L + pad[1]
        return view, torch.tensor([self.lengths[k] for k in order], dtype=torch.int32)


@pytest.fixture(scope="module")
def stats_cases():
    return [StatsCase(16000), StatsCase(32000)]


def _clear_of_the_gates(q):
    """No short-term block within 1e-6 LU of either gate, so that the device's gated set cannot differ from the host's."""
    l = ld.OFFSET + 10.0 * np.log10(q)
    absolute = l > ld.ABSOLUTE_GATE
    rel = ld.OFFSET + 10.0 * np.log10(np.mean(q[absolute])) + ld.RANGE_GATE
    return float(min(np.min(np.abs(l - ld.ABSOLUTE_GATE)), np.min(np.abs(l - rel)))) > 1e-6, int(np.count_nonzero(~absolute)), \
        int(np.count_nonzero(absolute & ~(l > rel)))


def test_loudness_stats_against_the_host(eng, stats_cases):
    for cs in stats_cases:
        planes, lengths = cs.batch()
        st = eng.loudness_stats(planes, cs.rate, lengths=lengths, weights=cs.weights, return_short_term=True)
        loud, blocks, counts = eng.loudness(planes, cs.rate, lengths=lengths, weights=cs.weights, return_blocks=True, return_counts=True)
        assert st["all"].shape == (len(cs.lengths), 10) and st["all"].dtype == torch.float64
        assert torch.equal(st["all"][:, 0], loud) and torch.equal(st["all"][:, 1:3], counts)         # columns 0 ... 2, bit for bit
        assert st["short_term"].shape == (len(cs.lengths), ld.n_short_term(max(cs.lengths), cs.rate))
        ten, short, blocks = st["all"].cpu().numpy(), st["short_term"].cpu().numpy(), blocks.cpu().numpy()
        for row, n in enumerate(cs.lengths):
            what = f"{cs.rate} Hz n={n}"
            p, q, bar = cs.host(n)
            ns = q.shape[0]
            assert ten[row, 6] == ns == ld.n_short_term(n, cs.rate) and not short[row, ns:].any(), what
            mine, mine_p = short[row, :ns], blocks[row, :p.shape[0]]
            assert ten[row, 3] == pytest.approx(ld.max_momentary(mine_p), abs=1e-12), what
            assert abs(ten[row, 3] - ld.max_momentary(p)) <= 10.0 * np.log10(1.0 + bar) + 1e-12 or ns == 0, what
            if ns == 0:                                               # 2.9 s: no short-term block
                assert ten[row, 4] == float("-inf") and ten[row, 5:].tolist() == [0.0] * 5 and np.isfinite(ten[row, 3]), what
                continue
            err = float(np.max(np.abs(mine - q) / q))
            clear, under_abs, under_rel = _clear_of_the_gates(q)
            lra, p10, p95, kept = ld.loudness_range(q)
            print(f"{what}: {ns} short-term blocks, worst relative error {err:.3e} (bar {bar:.3e}); {under_abs} under the absolute gate, "
                  f"{under_rel} under the relative one, {kept} kept; LRA {lra:.6f} LU, device {ten[row, 5]:.6f}")
            assert err <= bar, what
            assert clear and ten[row, 7] == kept, what
            # the selection is exact: the elements numpy's sort and the index rule pick from the device's own powers
            lra_d, p10_d, p95_d, kept_d = ld.loudness_range(mine)
            assert kept_d == kept and ten[row, 8] == p10_d and ten[row, 9] == p95_d, what
            assert ten[row, 5] == pytest.approx(lra_d, abs=1e-12) and ten[row, 4] == pytest.approx(ld.max_short_term(mine), abs=1e-12), what
            # against the all-host float64 value: an order statistic moves by at most the largest perturbation
            assert abs(ten[row, 5] - lra) <= 2.0 * (10.0 / np.log(10.0)) * bar, what
            assert abs(ten[row, 4] - ld.max_short_term(q)) <= (10.0 / np.log(10.0)) * bar, what
        if cs.rate == 16000:
            clear, under_abs, under_rel = _clear_of_the_gates(cs.host(480000)[1])
            assert under_abs > 0 and under_rel > 0 and ld.n_short_term(480000, 16000) == 271          # both gates bite, > 256 blocks


def test_loudness_stats_alone_and_in_a_batch(eng, stats_cases):
    for cs in stats_cases:
        order = [3, 0, 4, 2, 1] if len(cs.lengths) == 5 else [1, 0]
        planes, lengths = cs.batch(order, pad=(2, 9))
        st = eng.loudness_stats(planes, cs.rate, lengths=lengths, weights=cs.weights, return_short_term=True)
        for row, k in enumerate(order):
            n = cs.lengths[k]
            alone = eng.loudness_stats(torch.from_numpy(cs.x[:, :n].copy()).to(DEV), cs.rate, weights=cs.weights, return_short_term=True)
            ns = alone["short_term"].shape[1]
            assert torch.equal(alone["all"][0], st["all"][row]), (cs.rate, n, alone["all"][0], st["all"][row])
            assert torch.equal(alone["short_term"][0], st["short_term"][row, :ns]) and ns == ld.n_short_term(n, cs.rate)


def test_loudness_stats_with_nothing_to_measure(eng):
    inf = float("inf")
    x = 0.1 * torch.randn(1, 2, 6399, generator=torch.Generator().manual_seed(26)).to(DEV)
    assert eng.loudness_stats(x, 16000)["all"][0].tolist() == [-inf, 0.0, 0.0, -inf, -inf, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert eng.loudness_stats(x[:, :, :100], 16000)["all"][0].tolist() == [-inf, 0.0, 0.0, -inf, -inf, 0.0, 0.0, 0.0, 0.0, 0.0]
    st = eng.loudness_stats(torch.zeros(1, 2, 56000, device=DEV), 16000, return_short_term=True)      # 3.5 s of silence
    assert st["all"][0].tolist() == [-inf, 32.0, 0.0, -inf, -inf, 0.0, 6.0, 0.0, 0.0, 0.0] and not bool(st["short_term"].any())
    one = eng.loudness_stats(0.1 * torch.ones(1, 1, 48000, device=DEV).cumsum(2).sin(), 16000)        # one short-term block
    assert one["short_term_blocks"].tolist() == [1.0] and one["short_term_kept"].tolist() == [1.0]
    assert one["loudness_range"].tolist() == [0.0] and float(one["p10"]) == float(one["p95"]) > 0.0
    from lass_amd import _lib
    with pytest.raises(_lib.LassError, match="lengths"):
        eng.loudness_stats(x, 16000, lengths=[1, 2])


# ---- 3. separate_files --------------------------------------------------------------------------------------------------
SR = 16000
TARGET, CEILING_DB = -23.0, -1.0
KW = dict(loudness=TARGET, peak_ceiling_db=CEILING_DB)
CAPS = ["a dog barking", "rain on a roof", "a bell"]
METER_KEYS = ["loudness_range", "max_momentary", "max_short_term"]


def _make_model(sd):
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return AudioSep(ss_model=m.to(DEV).eval().set_compute_dtype("f32"), query_encoder=PrecomputedQueryEncoder())


@pytest.fixture(scope="module")
def holder(synthetic_sd):
    return _make_model(synthetic_sd)


def _bursts(frames, rate, nch, seed, period, length, div, phase_deg, floor=2e-4):
    """Bursts of the tone at rate / div - `length` frames every `period`, faded in and out over a quarter of their length - on a
    faint noise floor.  The duty cycle sets the crest factor, which decides whether the ceiling bites; div and phase set how far
    the samples lie under the tone's peak (div 4 at 45 degrees: 3.01 dB; div 6 at 60 degrees: 1.25 dB)."""
    rng = np.random.Generator(np.random.PCG64([27, seed]))
    x = floor * rng.standard_normal((frames, nch))
    n = np.arange(frames)
    tone = 0.5 * np.sin(2.0 * np.pi * n / div + np.deg2rad(phase_deg))
    at = n % period
    k = max(length // 4, 1)
    env = np.clip(np.minimum(at + 1, length - at) / k, 0.0, 1.0)
    x += (tone * env)[:, None]
    return x.astype(np.float32)


# Frames per burst and per period, chosen once from the separated output of the synthetic model: a level of -23 LUFS under a -1 dB
# ceiling leaves a peak 22 dB over the loudness.  a.wav comes back with its sample peak 23.5 dB and its true peak 23.6 dB over its
# loudness (both ceilings bite); c.wav's bursts of 16 frames every 3 000 come back at 22.0 and 24.0 dB, every 4 000 at 23.3 and
# 25.4 dB: every 2 400 puts the 22 dB between its two peaks, a decibel from either.
BURST_A, PERIOD_A, BURST_C, PERIOD_C = 300, 22050, 16, 2400


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """3.5 s each (six short-term blocks).  a.wav, 44.1 kHz stereo PCM16: bursts of a 7 350 Hz tone, under the model's 8 kHz and six
    samples per period at the file's rate; b.wav, 44.1 kHz stereo float32: a steady tone over noise, which no ceiling touches;
    c.wav, 16 kHz mono PCM16: bursts of the fs/4 tone."""
    d = tmp_path_factory.mktemp("r128files")
    n44, n16 = 154350, 56000
    t = np.arange(n44)[:, None] / 44100.0
    rng = np.random.Generator(np.random.PCG64(28))
    a = _bursts(n44, 44100, 2, 1, PERIOD_A, BURST_A, 6.0, 60.0)
    b = (0.05 * rng.standard_normal((n44, 2)) + 0.3 * np.sin(2 * np.pi * 1000.0 * t + np.array([0.0, 0.5]))).astype(np.float32)
    c = _bursts(n16, 16000, 1, 0, PERIOD_C, BURST_C, 4.0, 45.0)[:, 0]
    paths = [str(d / "a.wav"), str(d / "b.wav"), str(d / "c.wav")]
    wavio.write_wav_pcm16(paths[0], a, 44100)
    wavio.write_wav_f32(paths[1], b, 44100)
    wavio.write_wav_pcm16(paths[2], c, 16000)
    return d, paths


def _payload(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()[44:]


def _host_bytes(scratch, x, enc) -> bytes:
    WRITERS[enc](scratch, x, 16000)
    return _payload(scratch)


def _written(path):
    """(planes (C, frames) float64 as a player decodes them, encoding, rate)"""
    enc, nch, rate, frames, _ = wavio.wav_info(path)
    raw = np.frombuffer(_payload(path), dtype={"pcm16": "<i2", "pcm32": "<i4", "f32": "<f4"}[enc]).reshape(frames, nch).T
    return raw.astype(np.float64) / {"pcm16": 32768.0, "pcm32": 2147483648.0, "f32": 1.0}[enc], enc, rate


def true_peak_bound(ceiling, enc, rate):
    """What the float64 true peak of a written file can reach when the float32 true peak of its gained float32 samples was held to
    `ceiling`: with A the largest absolute tap sum of a phase of the interpolator, each sample the file
    holds is off its gained value fl(g y) by at most q/2 (q the encoding's LSB), fl(g y) is off g y by one float32 rounding, and
    the device's interpolated value by at most J2 = 21 more roundings, all of values not over the ceiling:
    ceiling + A * (q/2 + (J2 + 3) * 2^-24 * ceiling)."""
    os_ = ld.oversampling(rate)
    g = rs.design_taps(os_, 1)
    A = max(float(np.abs(g[p::os_]).sum()) for p in range(os_))
    q = {"pcm16": 2.0 ** -15, "pcm32": 2.0 ** -31, "f32": 0.0}[enc]
    return float(ceiling) + A * (q / 2.0 + (21 + 3) * 2.0 ** -24 * float(ceiling)), A


def _device_figures(eng, planes, rate_in, rate_out, frames_out):
    """(the ten numbers of Engine.loudness_stats, the float32 true peak) of separated planes (C, L) float32 on the host."""
    t = torch.from_numpy(np.array(planes, order="C")).to(DEV)
    return eng.loudness_stats(t, rate_in)["all"][0].cpu().numpy(), np.float32(eng.resample_true_peak(t, rate_in, rate_out, frames_out=frames_out)[0].item())


SHAPES = [("pcm16", 2, 44100, 154350), ("f32", 2, 44100, 154350), ("pcm16", 1, 16000, 56000)]


def test_separate_files_to_r128(holder, eng, scratch_wav, files):
    d, paths = files
    flat, model, true, samp = ([str(d / f"{name}{k}.wav") for k in range(3)] for name in ("flat", "model", "true", "samp"))
    pipeline.separate_files(holder, list(zip(paths, CAPS, flat)), SR, encoding="f32")                  # the samples before the gain
    pipeline.separate_files(holder, list(zip(paths, CAPS, model)), SR, encoding="f32", out_rate=SR)    # the separated planes themselves
    recs = pipeline.separate_files(holder, list(zip(paths, CAPS, true)), SR, peak="true", meter=True, **KW)
    recs_s = pipeline.separate_files(holder, list(zip(paths, CAPS, samp)), SR, peak="sample", **KW)
    assert true_peak_bound(1.0, "f32", 44100)[1] == pytest.approx(2.2414, abs=1e-4)
    level_keys = ["rate", "channels", "frames", "path", "clipped", "loudness_out", "gain", "gain_db", "peak_limited"]
    dbtp_true, dbtp_samp = [], []
    for k, (enc, nch, rate, frames) in enumerate(SHAPES):
        rec = recs[k]
        assert wavio.wav_info(true[k]) == (enc, nch, rate, frames, 44) and rec["path"] == "device" and rec["clipped"] == 0
        assert sorted(rec) == sorted(level_keys + ["true_peak_db"] + METER_KEYS) and sorted(recs_s[k]) == sorted(level_keys)
        x = np.frombuffer(_payload(flat[k]), dtype="<f4").reshape(frames, nch)
        g, ceiling = np.float32(rec["gain"]), ld.ceiling_for(CEILING_DB, enc)
        prod = (g * x).astype(np.float32)
        assert _payload(true[k]) == _host_bytes(scratch_wav, prod if nch > 1 else prod[:, 0], enc), paths[k]
        # the record's figures are the kernels' on the separated planes, and the gain the host rule's on them
        planes = np.frombuffer(_payload(model[k]), dtype="<f4").reshape(-1, nch).T
        ten, tp32 = _device_figures(eng, planes, SR, rate, frames)
        assert [rec["loudness_out"], rec["max_momentary"], rec["max_short_term"], rec["loudness_range"]] == [ten[0], ten[3], ten[4], ten[5]]
        assert ld.gain_for(rec["loudness_out"], tp32, TARGET, ceiling) == (g, rec["peak_limited"])
        assert rec["true_peak_db"] == pytest.approx(20.0 * np.log10(float(g) * float(tp32)), abs=1e-9)
        assert float(np.float32(g * tp32)) <= float(ceiling) and rec["loudness_out"] == recs_s[k]["loudness_out"]
        host_tp = ld.true_peak(x.T, rate)
        assert abs(float(tp32) - host_tp) <= 1e-5 * host_tp
        # the file as written, on the float64 host meter
        bound, _ = true_peak_bound(ceiling, enc, rate)
        tp = ld.true_peak(_written(true[k])[0], rate)
        dbtp_true.append(20.0 * np.log10(tp))
        dbtp_samp.append(20.0 * np.log10(ld.true_peak(_written(samp[k])[0], rate)))
        print(f"{os.path.basename(paths[k])}: loudness_out {rec['loudness_out']:.3f} LUFS, LRA {rec['loudness_range']:.3f} LU, max M "
              f"{rec['max_momentary']:.3f}, max S {rec['max_short_term']:.3f}; gain {rec['gain_db']:.3f} dB (sample: {recs_s[k]['gain_db']:.3f}), "
              f"limited {rec['peak_limited']} (sample: {recs_s[k]['peak_limited']}); written {dbtp_true[-1]:.4f} dBTP "
              f"(sample: {dbtp_samp[-1]:.4f}), bound {20 * np.log10(bound):.4f}, record {rec['true_peak_db']:.4f}; sample peak of the flat "
              f"export {20 * np.log10(np.abs(x).max()):.3f} dBFS, true peak {20 * np.log10(host_tp):.3f} dBTP")
        assert tp <= bound
    # the defect fixed: under the sample-peak ceiling the limited files read over -1 dBTP, under the true-peak ceiling none does
    limited = [k for k in range(3) if recs[k]["peak_limited"]]
    assert limited and all(dbtp_samp[k] > CEILING_DB + 0.01 for k in limited)
    assert all(v <= CEILING_DB + 0.01 for v in dbtp_true)
    # ... and one of them the sample-peak ceiling had not even touched
    assert any(recs[k]["peak_limited"] and not recs_s[k]["peak_limited"] for k in range(3))


def test_meter_alone_and_defaults(holder, eng, files):
    d, paths = files
    jobs = [(paths[2], CAPS[2], str(d / "meter.wav"))]
    plain = pipeline.separate_files(holder, [(paths[2], CAPS[2], str(d / "plain.wav"))], SR)[0]
    rec = pipeline.separate_files(holder, jobs, SR, meter=True)[0]
    assert sorted(plain) == ["channels", "clipped", "frames", "path", "rate"]
    assert sorted(rec) == sorted(["channels", "clipped", "frames", "path", "rate"] + METER_KEYS)
    assert _payload(jobs[0][2]) == _payload(str(d / "plain.wav"))                     # a meter changes no byte
    both = pipeline.inference(holder, paths[2], CAPS[2], str(d / "both.wav"), SR, peak="true", meter=True, **KW)
    assert [both[k] for k in METER_KEYS] == [rec[k] for k in METER_KEYS] and all(np.isfinite(rec[k]) for k in METER_KEYS)
    assert "true_peak_db" in both and "true_peak_db" not in pipeline.inference(holder, paths[2], CAPS[2], str(d / "s.wav"), SR, **KW)


@pytest.mark.filterwarnings("ignore:.*parity with the reference is unpinned.*:UserWarning")
def test_host_route_file_to_r128(holder, scratch_wav, files):
    """44 101 Hz is over the tap cap both ways: decode, meters, true peak (lass_amd/loudness.py), gain rule and export run on the
    host.  The payload within 1 LSB of the host writer of gain x the flat export, as tests/test_export_gpu.py allows the route."""
    d, _ = files
    odd, frames = str(d / "odd.wav"), 154354
    wavio.write_wav_pcm16(odd, _bursts(frames, 44101, 2, 2, PERIOD_A, BURST_A, 6.0, 60.0), 44101)
    flat, model, out = str(d / "odd_flat.wav"), str(d / "odd_model.wav"), str(d / "odd_true.wav")
    pipeline.separate_files(holder, [(odd, CAPS[0], flat)], SR, encoding="f32")
    pipeline.separate_files(holder, [(odd, CAPS[0], model)], SR, encoding="f32", out_rate=SR)
    rec = pipeline.separate_files(holder, [(odd, CAPS[0], out)], SR, peak="true", meter=True, **KW)[0]
    assert rec["path"] == "host" and rec["clipped"] == 0 and wavio.wav_info(out) == ("pcm16", 2, 44101, frames, 44)
    y = np.frombuffer(_payload(flat), dtype="<f4").reshape(frames, 2)
    x = np.frombuffer(_payload(model), dtype="<f4").reshape(-1, 2).T
    g, ceiling = np.float32(rec["gain"]), ld.ceiling_for(CEILING_DB, "pcm16")
    # section 1's functions on the separated planes and on the samples before the gain
    p, q = ld.block_powers(x, SR), ld.short_term_powers(x, SR)
    assert rec["loudness_out"] == ld.gate(p)[0] and np.isfinite(rec["loudness_out"])
    assert [rec[k] for k in METER_KEYS] == [ld.loudness_range(q)[0], ld.max_momentary(p), ld.max_short_term(q)]
    tp = np.float32(ld.true_peak(y.T, 44101))
    assert ld.gain_for(rec["loudness_out"], tp, TARGET, ceiling) == (g, rec["peak_limited"])
    assert rec["true_peak_db"] == pytest.approx(20.0 * np.log10(float(g) * float(tp)), abs=1e-9)
    want = np.frombuffer(_host_bytes(scratch_wav, (g * y).astype(np.float32), "pcm16"), dtype="<i2").astype(np.int64)
    got = np.frombuffer(_payload(out), dtype="<i2").astype(np.int64)
    assert int(np.abs(got - want).max()) <= 1
    written = ld.true_peak(_written(out)[0], 44101)
    print(f"host route: loudness_out {rec['loudness_out']:.3f} LUFS, LRA {rec['loudness_range']:.3f} LU, gain {rec['gain_db']:.3f} dB, "
          f"limited {rec['peak_limited']}, written {20 * np.log10(written):.4f} dBTP")
    assert written <= true_peak_bound(ceiling, "pcm16", 44101)[0]
