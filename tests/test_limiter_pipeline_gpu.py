"""`pipeline.separate_files(limiter=True)` on the GPU: three 2 s files - mono 16 kHz PCM16, stereo 44.1 kHz
PCM16 and one the device kernels do not take (44 101 Hz, the host route) - to a loud target (-10 LUFS) under a -6 dBTP ceiling, so
that the limiter is certain to bite: the ceiling leaves a crest of 4 dB, which no material but a square wave has.

Yardsticks: the files byte for byte what the public pieces give by hand (`Engine.loudness`, `Engine.loudness_gain`, `Engine.limit`,
`Engine.resample_true_peak`, `Engine.resample_encode`) on the separated planes of a plain float32 export of the same jobs; the
written true peak under section 19's bound, which the level stage behind the limiter still owes; the written loudness
(loudness_out + gain_db) against the same jobs without the limiter."""
import numpy as np
import pytest
import torch

from lass_amd import loudness as ld
from lass_amd import pipeline, wavio
from lass_amd import resample as rs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 16000
TARGET, CEILING_DB = -10.0, -6.0
KW = dict(loudness=TARGET, peak_ceiling_db=CEILING_DB, peak="true")
CAPS = ["a dog barking", "a door slamming", "a bell"]
LEVEL_KEYS = ["rate", "channels", "frames", "path", "clipped", "loudness_out", "gain", "gain_db", "peak_limited", "true_peak_db"]
LIMITER_KEYS = ["loudness_in", "limiter_gain_db", "limiter_reduction_db", "limiter_frames"]
METER_KEYS = ["loudness_range", "max_momentary", "max_short_term"]
SHAPES = [("pcm16", 1, 16000, 32000), ("pcm16", 2, 44100, 88200), ("pcm16", 2, 44101, 88202)]


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


@pytest.fixture(scope="module")
def holder(synthetic_sd):
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    return AudioSep(ss_model=m.to(DEV).eval().set_compute_dtype("f32"), query_encoder=PrecomputedQueryEncoder())


def _events(frames, rate, nch, seed):
    """A bed of noise and a 440 Hz tone with a 5 ms click of a 2 kHz tone every 0.45 s: sound events over a quiet bed."""
    rng = np.random.Generator(np.random.PCG64([33, seed]))
    n = np.arange(frames)
    x = 0.01 * rng.standard_normal((frames, nch)) + 0.03 * np.sin(2 * np.pi * 440.0 * n / rate)[:, None]
    k = np.arange(int(0.005 * rate))
    for s in range(int(0.2 * rate), frames - k.size, int(0.45 * rate)):
        x[s:s + k.size] += (0.8 * np.exp(-k / (0.001 * rate)) * np.sin(2 * np.pi * 2000.0 * k / rate + 0.7))[:, None]
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("limiterfiles")
    paths = []
    for k, (enc, nch, rate, frames) in enumerate(SHAPES):
        paths.append(str(d / f"in{k}.wav"))
        x = _events(frames, rate, nch, k)
        wavio.write_wav_pcm16(paths[-1], x if nch > 1 else x[:, 0], rate)
    return d, paths


def _payload(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()[44:]


def _written(path):
    enc, nch, rate, frames, _ = wavio.wav_info(path)
    raw = np.frombuffer(_payload(path), dtype="<i2").reshape(frames, nch).T
    return raw.astype(np.float64) / 32768.0


def true_peak_bound(ceiling, enc, rate):
    """ceiling + A * (q/2 + (J2 + 3) * 2^-24 * ceiling), A the largest absolute tap sum of a phase of the
    interpolator, q the encoding's LSB, J2 = 21."""
    os_ = ld.oversampling(rate)
    g = rs.design_taps(os_, 1)
    A = max(float(np.abs(g[p::os_]).sum()) for p in range(os_))
    q = {"pcm16": 2.0 ** -15, "pcm32": 2.0 ** -31, "f32": 0.0}[enc]
    return float(ceiling) + A * (q / 2.0 + (21 + 3) * 2.0 ** -24 * float(ceiling))


@pytest.fixture(scope="module")
def runs(holder, files):
    """The same jobs five times: the separated planes (a float32 export at the model rate), with the limiter, with the limiter and
    the meter, with limiter=False and without the argument."""
    d, paths = files
    model, lim, met, off, bare = ([str(d / f"{name}{k}.wav") for k in range(3)] for name in ("model", "lim", "met", "off", "bare"))
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*parity with the reference is unpinned.*", category=UserWarning)
        pipeline.separate_files(holder, list(zip(paths, CAPS, model)), SR, encoding="f32", out_rate=SR)
        recs = pipeline.separate_files(holder, list(zip(paths, CAPS, lim)), SR, limiter=True, **KW)
        recs_met = pipeline.separate_files(holder, list(zip(paths, CAPS, met)), SR, limiter=True, meter=True, **KW)
        recs_off = pipeline.separate_files(holder, list(zip(paths, CAPS, off)), SR, limiter=False, **KW)
        recs_bare = pipeline.separate_files(holder, list(zip(paths, CAPS, bare)), SR, **KW)
    return dict(model=model, lim=lim, met=met, off=off, bare=bare, recs=recs, recs_met=recs_met, recs_off=recs_off, recs_bare=recs_bare)


def test_records_and_ceiling(runs):
    recs = runs["recs"]
    assert [r["path"] for r in recs] == ["device", "device", "host"]
    assert sum(r["limiter_frames"] > 0 for r in recs) >= 2
    for k, (enc, nch, rate, frames) in enumerate(SHAPES):
        rec = recs[k]
        assert sorted(rec) == sorted(LEVEL_KEYS + LIMITER_KEYS), rec
        assert wavio.wav_info(runs["lim"][k]) == (enc, nch, rate, frames, 44) and rec["clipped"] == 0
        assert np.isfinite(rec["loudness_in"]) and rec["limiter_reduction_db"] < 0.0 and rec["limiter_frames"] > 0
        ceiling = ld.ceiling_for(CEILING_DB, enc)
        tp = ld.true_peak(_written(runs["lim"][k]), rate)
        print(f"file {k}: in {rec['loudness_in']:.2f} LUFS, limiter gain {rec['limiter_gain_db']:.2f} dB, reduction "
              f"{rec['limiter_reduction_db']:.2f} dB on {rec['limiter_frames']} frames, limited planes {rec['loudness_out']:.2f} LUFS, trim "
              f"{rec['gain_db']:.4f} dB, written {rec['loudness_out'] + rec['gain_db']:.2f} LUFS at {20 * np.log10(tp):.4f} dBTP "
              f"(without the limiter {runs['recs_off'][k]['loudness_out'] + runs['recs_off'][k]['gain_db']:.2f} LUFS)")
        assert tp <= true_peak_bound(ceiling, enc, rate)


def _device_by_hand(eng, runs, k):
    """File k's separated planes through the public pieces: (limited planes, loudness in, the last pass's gain, its info)."""
    enc, nch, rate, frames = SHAPES[k]
    x = torch.from_numpy(np.frombuffer(_payload(runs["model"][k]), dtype="<f4").reshape(-1, nch).T.copy()).to(DEV)
    ceiling, H = ld.ceiling_for(CEILING_DB, enc), ld.reach(1.5, SR)
    loud_in = eng.loudness(x, SR)
    g = eng.loudness_gain(loud_in, None, TARGET, None)[0]
    v, info = eng.limit(x, SR, g, ceiling, H, "true")
    g = g * eng.loudness_gain(eng.loudness(v, SR), None, TARGET, None)[0]
    v, info = eng.limit(x, SR, g, ceiling, H, "true")
    return v[0], loud_in, g, info


def _host_by_hand(runs):
    """The host file's separated planes through `lass_amd.loudness`: (limited planes, loudness in, gain, curve, envelope)."""
    enc, nch, rate, frames = SHAPES[2]
    x = np.frombuffer(_payload(runs["model"][2]), dtype="<f4").reshape(-1, nch).T
    ceiling, H = ld.ceiling_for(CEILING_DB, enc), ld.reach(1.5, SR)
    l_in = ld.integrated_loudness(x, SR)
    g = ld.gain_for(l_in, None, TARGET, None)[0]
    v = ld.limit(x, SR, g, ceiling, H)[0].astype(np.float32)
    g = np.float32(g * ld.gain_for(ld.integrated_loudness(v, SR), None, TARGET, None)[0])
    v, G, e = ld.limit(x, SR, g, ceiling, H)
    return v.astype(np.float32), l_in, g, G, e


def _limiter_values_by_hand(rec, loud_in, g, info):
    assert rec["loudness_in"] == float(loud_in[0])
    assert rec["limiter_gain_db"] == 20.0 * np.log10(np.float64(np.float32(g[0].item())))
    assert rec["limiter_reduction_db"] == 20.0 * np.log10(np.float64(np.float32(info["min_gain"][0].item())))
    assert rec["limiter_frames"] == int(info["frames"][0])


def test_device_files_are_the_public_pieces_by_hand(eng, runs):
    for k, (enc, nch, rate, frames) in enumerate(SHAPES[:2]):
        rec = runs["recs"][k]
        v, loud_in, g, info = _device_by_hand(eng, runs, k)
        ceiling = ld.ceiling_for(CEILING_DB, enc)
        measured = eng.loudness(v, SR)
        pk = eng.resample_true_peak(v, SR, rate, frames_out=frames)
        trim, bit = eng.loudness_gain(measured, pk, TARGET, ceiling)
        clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
        payload = eng.resample_encode(v, SR, rate, enc, frames_out=frames, clipped=clipped, gain=trim)
        assert bytes(payload[0].cpu().numpy()) == _payload(runs["lim"][k]), k
        assert int(clipped[0]) == 0 == rec["clipped"]
        assert rec["loudness_out"] == float(measured[0])
        assert rec["gain"] == float(trim[0]) and rec["peak_limited"] == bool(bit[0])
        _limiter_values_by_hand(rec, loud_in, g, info)


def test_host_route_runs_the_definition(runs):
    enc, nch, rate, frames = SHAPES[2]
    rec = runs["recs"][2]
    ceiling, H = ld.ceiling_for(CEILING_DB, enc), ld.reach(1.5, SR)
    v, l_in, g, G, e = _host_by_hand(runs)
    assert rec["loudness_in"] == l_in and rec["loudness_out"] == ld.integrated_loudness(v, SR)
    assert rec["limiter_gain_db"] == 20.0 * np.log10(np.float64(g)) and rec["limiter_reduction_db"] == 20.0 * np.log10(G.min())
    assert rec["limiter_frames"] == int(np.count_nonzero(ld.limiter_curve(e, g, ceiling, H)[2] < 1.0))


def test_meter_beside_the_limiter(eng, runs):
    """limiter=True with meter=True, the largest set of numbers a file sends to the host behind its payload: the meter writes
    nothing into a file, each record is the limiter run's plus the three meter figures, and those are the figures of the LIMITED
    planes - `Engine.loudness_stats` of them by hand on the device files, `lass_amd.loudness` on the host file."""
    for k in range(3):
        rec, met = runs["recs"][k], runs["recs_met"][k]
        assert _payload(runs["met"][k]) == _payload(runs["lim"][k]), k
        assert sorted(met) == sorted(LEVEL_KEYS + LIMITER_KEYS + METER_KEYS), met
        assert {key: val for key, val in met.items() if key not in METER_KEYS} == rec
    for k in range(2):
        met = runs["recs_met"][k]
        v, loud_in, g, info = _device_by_hand(eng, runs, k)
        ten = dict(zip(eng.STATS_COLUMNS, eng.loudness_stats(v, SR)["all"][0].tolist()))
        assert [met[key] for key in METER_KEYS] == [ten[key] for key in METER_KEYS], (k, met, ten)
        _limiter_values_by_hand(met, loud_in, g, info)
    v = _host_by_hand(runs)[0]
    p, q = ld.block_powers(v, SR), ld.short_term_powers(v, SR)
    assert [runs["recs_met"][2][key] for key in METER_KEYS] == [ld.loudness_range(q)[0], ld.max_momentary(p), ld.max_short_term(q)]


def test_limiter_brings_device_files_closer_to_the_target(runs):
    for k in range(2):
        on, off = runs["recs"][k], runs["recs_off"][k]
        assert off["peak_limited"]                           # the single gain was held down by the ceiling
        assert abs(on["loudness_out"] + on["gain_db"] - TARGET) < abs(off["loudness_out"] + off["gain_db"] - TARGET)


def test_limiter_false_is_the_call_without_the_argument(runs):
    assert runs["recs_off"] == runs["recs_bare"]
    for k in range(3):
        assert sorted(runs["recs_off"][k]) == sorted(LEVEL_KEYS)
        assert _payload(runs["off"][k]) == _payload(runs["bare"][k])
