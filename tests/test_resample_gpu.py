"""Device load path on the GPU: `lass_decode_resample` (PCM decode + mono down-mix + polyphase FIR in one launch) against the
host's own arithmetic, and the evaluator's `device_decode` route.

Yardsticks: decoding is compared bit for bit with `wavio.read_wav`; resampling with `resample.resample_host` in float64 on
the decoded clip.  The resampling bar follows DESIGN.md section 11's convention: 4 x the largest deviation of the SAME
formula evaluated in float32 on the host (`resample_host(dtype=float32)`) from the float64 yardstick, on the same clip,
computed in the test and printed next to the device's deviation.  Neither scipy nor the reference is needed here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lass_amd import resample as rs
from lass_amd import synthetic, wavio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATE_TABLE = [(32000, 16000), (48000, 16000), (44100, 16000), (22050, 16000), (24000, 16000), (8000, 16000), (11025, 16000),
              (44100, 32000)]
WRITERS = {"pcm16": wavio.write_wav_pcm16, "pcm32": wavio.write_wav_pcm32, "f32": wavio.write_wav_f32}


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


@pytest.fixture(scope="module")
def model(synthetic_sd):
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    return m.to(DEV).eval()


def _raw_row(path, pad: int = 0):
    """(wav_info, the file's data chunk as a uint8 row padded to a multiple of 4 bytes + `pad`)."""
    info = wavio.wav_info(path)
    assert info is not None, path
    nbytes = info[3] * info[1] * rs.SAMPLE_BYTES[info[0]]
    row = np.zeros((nbytes + 3) // 4 * 4 + pad, dtype=np.uint8)
    assert wavio.read_wav_raw_into(path, info, row)
    return info, row


def _device(eng, path, rate_out):
    info, row = _raw_row(path)
    enc, nch, rate, frames, _ = info
    y = eng.decode_resample(torch.from_numpy(row).to(DEV), frames, nch, enc, rate, rate_out)
    assert y.shape == (1, rs.out_len(frames, *rs.ratio(rate, rate_out))) and y.dtype == torch.float32
    return y[0].cpu().numpy()


def _signal(kind: str, frames: int, rate: int, nch: int, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "noise":
        return (0.25 * rng.standard_normal((frames, nch))).astype(np.float32)
    t = np.arange(frames)[:, None] / rate
    f1, f2 = 0.011 * rate, 0.12 * rate      # both tones inside the pass band of every pair of the table
    ph = rng.uniform(0, 2 * np.pi, (2, nch))
    return (0.4 * np.sin(2 * np.pi * f1 * t + ph[0]) + 0.3 * np.sin(2 * np.pi * f2 * t + ph[1])).astype(np.float32)


def _prime_near(n: int) -> int:
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


def _bar_and_ref(x, up, down, sl=slice(None)):
    """(float64 yardstick, bar = 4 x max |float32 host evaluation - yardstick|) over the outputs `sl` of clip x."""
    ref = rs.resample_host(x, up, down)[sl]
    host32 = rs.resample_host(x, up, down, dtype=np.float32)[sl]
    return ref, 4.0 * float(np.max(np.abs(host32.astype(np.float64) - ref)))


# ---- decode only --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["pcm16", "pcm32", "f32"])
@pytest.mark.parametrize("nch", [1, 2, 3, 6])
def test_decode_only_equals_read_wav(tmp_path, eng, enc, nch):
    """up == down == 1: PCM16 / PCM32 / float32 decode and the mono down-mix reproduce read_wav's values - bit for bit with 1
    and 2 channels (a sum of two floats and a halving round once), within 1 ulp with 3 and 6 (numpy's mean adds the channels in
    its own order; the kernel adds them in ascending order)."""
    frames = 4099
    x = _signal("noise", frames, 16000, nch, [1, nch])
    x[:8] = np.array([1.0, -1.0, 0.999999, -0.999999, 1e-9, -3e-5, 0.5, 0.0], dtype=np.float32)[:, None]
    p = str(tmp_path / "a.wav")
    WRITERS[enc](p, x if nch > 1 else x[:, 0], 16000)
    want, _ = wavio.read_wav(p, 16000)
    got = _device(eng, p, 16000)
    assert got.shape == want.shape == (frames,)
    if nch <= 2:
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want))
    else:
        ulp = np.spacing(np.abs(want).astype(np.float32))
        worst = float(np.max(np.abs(got.astype(np.float64) - want) / ulp))
        print(f"decode {enc} x{nch}: worst deviation {worst:.2f} ulp")
        assert worst <= 1.0


# ---- resampling ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", RATE_TABLE)
@pytest.mark.parametrize("enc,nch", [("pcm16", 1), ("f32", 2)])
def test_resample_matches_host_formula(tmp_path, eng, rate_in, rate_out, enc, nch):
    up, down = rs.ratio(rate_in, rate_out)
    p = str(tmp_path / "a.wav")
    for kind in ("noise", "two-tone"):
        for frames in (1, 37, _prime_near(10 * rate_in)):
            x = _signal(kind, frames, rate_in, nch, [rate_in, rate_out, frames])
            WRITERS[enc](p, x if nch > 1 else x[:, 0], rate_in)
            decoded, _ = wavio.read_wav(p, rate_in)
            ref, bar = _bar_and_ref(decoded, up, down)
            got = _device(eng, p, rate_out)
            assert got.shape == ref.shape == (rs.out_len(frames, up, down),)
            err = float(np.max(np.abs(got.astype(np.float64) - ref)))
            print(f"{rate_in}->{rate_out} {enc} x{nch} {kind} frames={frames}: device {err:.3e}  bar (4 x host f32) {bar:.3e}")
            assert err <= bar, (kind, frames, err, bar)


@pytest.mark.parametrize("up,down,frames", [(1, 819, 200001), (819, 1, 301), (7, 5, 50021)])
def test_resample_other_ratios(eng, up, down, frames):
    """Ratios outside the table, through `Engine.resample`: the two largest filters under the tap cap (16 381 taps: all in one
    phase, and 21 per phase over 819 phases) and a small one."""
    x = _signal("noise", frames, 16000, 1, [up, down])[:, 0]
    ref, bar = _bar_and_ref(x, up, down)
    got = eng.resample(torch.from_numpy(x).to(DEV), 16000 * down, 16000 * up).cpu().numpy()
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"up={up} down={down}: device {err:.3e}  bar {bar:.3e}")
    assert got.shape == ref.shape and err <= bar


KAISER5_RIPPLE = 10.0 ** (-(5.0 / 0.1102 + 8.7) / 20.0)   # Kaiser's design formula: beta = 0.1102 (A - 8.7) -> A = 54.1 dB, 2.0e-3


@pytest.mark.parametrize("rate_in,rate_out", RATE_TABLE)
def test_closed_forms(eng, rate_in, rate_out):
    """A constant stays that constant, a 1 kHz sine keeps amplitude and phase, a tone above the output Nyquist is suppressed.
    `Away from the edges` = more than one filter length from either end.  What the FILTER contributes is measured on the float64
    yardstick in the test, never fixed: the device must sit within the bar of the yardstick, and the yardstick within the
    design's own limits - a phase's taps sum to 1 exactly only when up == 1 (the prototype has unit sum; with up > 1 each of
    the up phases sums to 1 up to the stop-band leakage at the image frequencies), and the pass band of a Kaiser(5) design
    ripples by 2.0e-3 (KAISER5_RIPPLE); the filter is symmetric, so it shifts no phase."""
    up, down = rs.ratio(rate_in, rate_out)
    frames = rate_in * 2
    edge = -(-rs.n_taps(up, down) // down) + 1
    mid = slice(edge, rs.out_len(frames, up, down) - edge)
    dev = lambda x: eng.resample(torch.from_numpy(x).to(DEV), rate_in, rate_out).cpu().numpy().astype(np.float64)  # noqa: E731

    x = np.full(frames, 0.5, dtype=np.float32)
    ref, bar = _bar_and_ref(x, up, down, mid)
    got = dev(x)[mid]
    ripple = float(np.max(np.abs(ref - 0.5)))
    print(f"{rate_in}->{rate_out} constant: device-yardstick {np.max(np.abs(got - ref)):.3e} bar {bar:.3e}; yardstick-0.5 {ripple:.3e}")
    assert np.max(np.abs(got - ref)) <= bar
    assert np.max(np.abs(got - 0.5)) <= bar + ripple
    if up == 1:
        assert ripple <= 1e-14 and np.max(np.abs(got - 0.5)) <= bar + 1e-14
    assert ripple <= KAISER5_RIPPLE

    t_in, t_out = np.arange(frames) / rate_in, np.arange(rs.out_len(frames, up, down))[mid] / rate_out
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * t_in + 0.3)).astype(np.float32)
    ref, bar = _bar_and_ref(x, up, down, mid)
    got = dev(x)[mid]
    basis = np.stack([np.sin(2 * np.pi * 1000.0 * t_out), np.cos(2 * np.pi * 1000.0 * t_out)], axis=1)
    fit = lambda y: np.linalg.lstsq(basis, y, rcond=None)[0]  # noqa: E731
    (a_d, b_d), (a_r, b_r) = fit(got), fit(ref)
    amp_d, amp_r, ph_d, ph_r = np.hypot(a_d, b_d), np.hypot(a_r, b_r), np.arctan2(b_d, a_d), np.arctan2(b_r, a_r)
    print(f"{rate_in}->{rate_out} 1 kHz: amplitude device {amp_d:.7f} yardstick {amp_r:.7f}; phase device {ph_d:.7f} yardstick {ph_r:.7f}; "
          f"device-yardstick {np.max(np.abs(got - ref)):.3e} bar {bar:.3e}")
    assert np.max(np.abs(got - ref)) <= bar
    assert abs(amp_d - amp_r) <= bar and abs(ph_d - ph_r) <= bar / 0.5
    assert abs(amp_d - 0.5) <= 0.5 * KAISER5_RIPPLE + bar and abs(ph_d - 0.3) <= 1e-5

    if rate_in > rate_out:   # (an input below the output rate holds nothing above the output Nyquist)
        f_stop = 0.5 * rate_out + 0.45 * (0.5 * rate_in - 0.5 * rate_out)
        x = (0.5 * np.sin(2 * np.pi * f_stop * t_in + 0.1)).astype(np.float32)     # -6 dB
        ref, bar = _bar_and_ref(x, up, down, mid)
        got = dev(x)[mid]
        level_r, level_d = float(np.max(np.abs(ref))), float(np.max(np.abs(got)))
        print(f"{rate_in}->{rate_out} tone at {f_stop:.0f} Hz, -6 dB in: yardstick {20 * np.log10(level_r):.1f} dB, device "
              f"{20 * np.log10(max(level_d, 1e-30)):.1f} dB (bar {bar:.3e})")
        assert level_d <= level_r + bar


# ---- invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,enc,nch", [(44100, "pcm16", 1), (48000, "f32", 2), (16000, "pcm32", 2)])
def test_bitwise_invariance(tmp_path, eng, rate_in, enc, nch):
    """One clip gives the same bits alone, as row 7 of a shuffled batch of 16, behind a wider row stride, and on a second call."""
    frames, rate_out = 30011, 16000
    paths = []
    for i in range(16):
        x = _signal("noise" if i % 2 else "two-tone", frames, rate_in, nch, [77, i])
        paths.append(str(tmp_path / f"c{i}.wav"))
        WRITERS[enc](paths[-1], x if nch > 1 else x[:, 0], rate_in)
    info, row = _raw_row(paths[0])
    alone = eng.decode_resample(torch.from_numpy(row).to(DEV), frames, nch, enc, rate_in, rate_out)
    again = eng.decode_resample(torch.from_numpy(row).to(DEV), frames, nch, enc, rate_in, rate_out)
    assert torch.equal(alone, again)
    order = list(np.random.Generator(np.random.PCG64(5)).permutation(np.arange(1, 16)))
    order.insert(7, 0)
    for pad in (0, 128):
        batch = np.stack([_raw_row(paths[i], pad)[1] for i in order])
        raw = torch.from_numpy(batch).to(DEV)
        assert raw.stride(0) == row.shape[0] + pad
        out = eng.decode_resample(raw, frames, nch, enc, rate_in, rate_out)
        assert torch.equal(out[7], alone[0]), pad
        assert not torch.equal(out[6], alone[0])
    out2 = torch.empty_like(out)
    assert eng.decode_resample(raw, frames, nch, enc, rate_in, rate_out, out=out2) is out2 and torch.equal(out2, out)


def test_long_clip_64bit_indexing(tmp_path, eng):
    """320 s at 44 100 -> 16 000 Hz: frames * up = 2.26e9 > 2^31.  The first and the last 2 000 outputs against the host formula
    on a head / tail slice (a slice that starts at a multiple of `down` frames maps onto whole outputs: n0 * down == m0 * up)."""
    rate_in, rate_out, frames = 44100, 16000, 320 * 44100
    up, down = rs.ratio(rate_in, rate_out)
    assert frames * up > 2 ** 31
    x = _signal("noise", frames, rate_in, 1, [320])[:, 0]
    p = str(tmp_path / "long.wav")
    wavio.write_wav_pcm16(p, x, rate_in)
    decoded, _ = wavio.read_wav(p, rate_in)
    got = _device(eng, p, rate_out).astype(np.float64)
    L_out = rs.out_len(frames, up, down)
    assert got.shape == (L_out,) and L_out == 5120000
    # head: outputs 0 ... 1999 read frames below (1999 * 441 + 4410) / 160 < 8000
    ref, bar = _bar_and_ref(decoded[:8000], up, down, slice(0, 2000))
    err = float(np.max(np.abs(got[:2000] - ref)))
    print(f"head: device {err:.3e} bar {bar:.3e}")
    assert err <= bar
    m0 = (frames - 8000) // down * down
    n0 = m0 * up // down
    assert n0 * down == m0 * up
    lo = L_out - 2000 - n0
    assert lo > rs.n_taps(up, down) // down + 1     # beyond the reach of the slice's missing left context
    ref, bar = _bar_and_ref(decoded[m0:], up, down, slice(lo, lo + 2000))
    err = float(np.max(np.abs(got[-2000:] - ref)))
    print(f"tail: device {err:.3e} bar {bar:.3e}")
    assert ref.shape == (2000,) and err <= bar
    assert np.max(np.abs(got[-2000:])) > 0.1


# ---- error paths --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_launch(eng):
    from lass_amd import _lib
    frames, nch, up, down = 1000, 2, 160, 441
    L_out = rs.out_len(frames, up, down)
    raw = torch.zeros(2, frames * nch * 2 + 8, dtype=torch.uint8, device=DEV)
    taps = torch.zeros(rs.MAX_TAPS + 2, dtype=torch.float32, device=DEV)
    out = torch.full((2, L_out + 1), -7.25, dtype=torch.float32, device=DEV)
    good = dict(raw=raw.data_ptr(), stride=raw.stride(0), B=2, frames=frames, ch=nch, enc=rs.ENCODINGS["pcm16"], up=up, down=down,
                taps=taps.data_ptr(), n_taps=rs.n_taps(up, down), out=out.data_ptr(), L_out=L_out)

    def call(**kw):
        a = dict(good, **kw)
        rc = eng.lib.lass_decode_resample(eng.ctx, ctypes.c_void_p(a["raw"]), a["stride"], a["B"], a["frames"], a["ch"], a["enc"],
                                          a["up"], a["down"], ctypes.c_void_p(a["taps"]), a["n_taps"], ctypes.c_void_p(a["out"]),
                                          a["L_out"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, eng.lib.lass_last_error(eng.ctx).decode()

    bad = [dict(enc=3), dict(enc=-1), dict(ch=0), dict(ch=9), dict(up=0), dict(down=0), dict(up=-3), dict(n_taps=8820),
           dict(n_taps=rs.MAX_TAPS + 2), dict(n_taps=0), dict(L_out=L_out + 1), dict(L_out=L_out - 1),
           dict(stride=frames * nch * 2 - 4), dict(stride=frames * nch * 2 + 2), dict(raw=0), dict(out=0), dict(taps=0), dict(B=0),
           dict(frames=0), dict(raw=raw.data_ptr() + 2), dict(up=1, down=7, n_taps=3, L_out=rs.out_len(frames, 1, 7), enc=5)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("lass_decode_resample:"), (kw, rc, msg)   # LASS_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    # a polyphase table beyond the kernel's LDS budget, and the Python layer's own refusal of a ratio over the tap cap
    rc, msg = call(up=30000, down=1, n_taps=3, L_out=frames * 30000)
    assert rc == -1 and msg.startswith("lass_decode_resample:")
    with pytest.raises(_lib.LassError, match="cap"):
        eng.resample(torch.zeros(100, device=DEV), 44101, 16000)
    rc, msg = call()
    torch.cuda.synchronize()
    flat = out.reshape(-1)   # the good call does run (zeros in, zeros out), dense (B, L_out) and not a float further
    assert rc == 0 and bool((flat[: 2 * L_out] == 0).all()) and bool((flat[2 * L_out:] == -7.25).all())


# ---- evaluator ----------------------------------------------------------------------------------------------------------
def _evaluators(tmp_path, batch_size=16, length=24000, **fmt):
    from lass_amd.evaluator import DCASEEvaluator
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=40, length=length, **fmt)
    adir = os.path.join(str(tmp_path), "lass_validation")
    on = DCASEEvaluator(16000, csv_path, adir, batch_size=batch_size, device_decode=True)
    off = DCASEEvaluator(16000, csv_path, adir, batch_size=batch_size)
    return on, off, adir


@pytest.mark.filterwarnings("ignore:.*parity with the reference is unpinned.*:UserWarning")
def test_evaluator_other_rate_set_stays_resident(tmp_path, model, synthetic_sd):
    """40 items as 32 kHz PCM16 stereo, evaluated at 16 kHz, batch 16: with device_decode every batch is a resident one and the
    per-clip rows sit within the project's 0.01 dB metric bar of device_decode=False (the unchanged host route: scipy in
    float64, generic path).  Graph replay: lass_separate captures a (pointers, shape) key at its THIRD sighting and replays
    it from the fourth; three batches over two slots show every key once per call, so with batch 16 the replays start in
    call 4 - and in call 2 with batch 8 (five batches: slot 0's key shows three times in call 1), which is checked as well,
    on a second separator so that its keys meet an empty graph table."""
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    pl_model = AudioSep(ss_model=model, query_encoder=PrecomputedQueryEncoder())
    on, off, adir = _evaluators(tmp_path, file_rate=32000, channels=2, encoding="pcm16")
    ref = off(pl_model)
    assert off.last_path == "resident" and off.resident_batches == 0 and off.generic_batches == 3   # today: every batch falls out
    reps = []
    for call in range(5):
        got = on(pl_model)
        assert on.last_path == "resident" and on.resident_batches == 3 and on.generic_batches == 0, call
        worst = float(np.max(np.abs(on.last_rows - off.last_rows)))
        print(f"call {call}: worst per-clip difference to device_decode=False {worst:.2e} dB")
        assert worst <= 0.01 and got == pytest.approx(ref, abs=0.01)
        reps.append(model.engine.graph_stats()[2])
    assert reps[3] > reps[2] and reps[4] > reps[3], reps
    # batch 8 on a separator of its own: a context keeps four graphs and gives a new key the least recently used entry WITHOUT a
    # graph, so behind the three graphs captured above the two batch-8 keys would evict each other and never reach a third sighting
    from lass_amd.evaluator import DCASEEvaluator
    from lass_amd.resunet import ResUNet30
    model8 = ResUNet30(1, 1, 512)
    model8.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    pl8 = AudioSep(ss_model=model8.to(DEV).eval(), query_encoder=PrecomputedQueryEncoder())
    on8 = DCASEEvaluator(16000, os.path.join(str(tmp_path), "lass_synthetic_validation.csv"), adir, batch_size=8, device_decode=True)
    on8(pl8)
    assert on8.last_path == "resident" and on8.resident_batches == 5 and on8.generic_batches == 0
    r1 = model8.engine.graph_stats()[2]
    on8(pl8)
    r2 = model8.engine.graph_stats()[2]
    print(f"batch 8: replays after call 1 {r1}, after call 2 {r2}")
    assert r2 > r1, (r1, r2)     # replays from the second call on
    assert float(np.max(np.abs(on8.last_rows - off.last_rows))) <= 0.01


def test_evaluator_native_set_is_unchanged(tmp_path, model):
    """Mono float32 at the evaluator's rate: device_decode=True takes today's code path; the rows are equal, bit for bit.  (Clips
    of 4 000 samples: the power and SDR sums of a clip up to 4 096 samples are made by ONE workgroup, so no order of f64 atomics
    is left open between two runs - tests/test_gpu_parity.py allows 1e-9 dB between runs of longer clips for that reason.)"""
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    pl_model = AudioSep(ss_model=model, query_encoder=PrecomputedQueryEncoder())
    on, off, _ = _evaluators(tmp_path, length=4000)
    a, b = on(pl_model), off(pl_model)
    assert on.last_path == off.last_path == "resident" and on.resident_batches == off.resident_batches == 3
    assert on.generic_batches == off.generic_batches == 0
    print(f"native set: worst difference {np.max(np.abs(on.last_rows - off.last_rows)):.3e} dB")
    assert np.array_equal(on.last_rows, off.last_rows) and a == b
    assert all(not hasattr(s, "raw_src") for slots in on._slots.values() for s in slots)


@pytest.mark.filterwarnings("ignore:.*parity with the reference is unpinned.*:UserWarning")
def test_evaluator_mixed_set_sends_one_batch_generic(tmp_path, model):
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    pl_model = AudioSep(ss_model=model, query_encoder=PrecomputedQueryEncoder())
    on, off, adir = _evaluators(tmp_path, file_rate=32000, channels=2, encoding="pcm16")
    p = os.path.join(adir, "noise_0020.wav")       # one mono file among the stereo ones (batch 1 of 0 ... 2)
    x, _ = wavio.read_wav(p, 32000)
    wavio.write_wav_pcm16(p, x, 32000)
    on(pl_model)
    off(pl_model)
    assert on.last_path == "resident" and on.resident_batches == 2 and on.generic_batches == 1
    assert float(np.max(np.abs(on.last_rows - off.last_rows))) <= 0.01


@pytest.mark.filterwarnings("ignore:.*parity with the reference is unpinned.*:UserWarning")
def test_evaluator_odd_rate_runs_generic_without_slots(tmp_path, model):
    """44 101 Hz -> 16 000 Hz is 16000/44101 in lowest terms: 882 021 taps, far over the cap.  The call runs generic (host
    resampling) and no slot was allocated on the way."""
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.evaluator import DCASEEvaluator
    pl_model = AudioSep(ss_model=model, query_encoder=PrecomputedQueryEncoder())
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=3, length=8000, file_rate=44101)
    adir = os.path.join(str(tmp_path), "lass_validation")
    assert not rs.within_cap(*rs.ratio(44101, 16000))
    on = DCASEEvaluator(16000, csv_path, adir, batch_size=2, device_decode=True)
    off = DCASEEvaluator(16000, csv_path, adir, batch_size=2, resident=False)
    on(pl_model)
    assert on.last_path == "generic" and on._slots == {} and on.resident_batches == 0
    off(pl_model)
    np.testing.assert_allclose(on.last_rows, off.last_rows, rtol=0, atol=1e-9)
