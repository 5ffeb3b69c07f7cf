"""Remix export on the GPU: `lass_remix_encode` and `lass_remix_peak` - the export kernels with a dry
source - and `pipeline.separate_files(target_gain_db=)` on top of them.

Yardsticks, all equality unless a bar is stated: the host writers (`wavio.write_wav_*`) applied to `pipeline.remix_host` - the
numpy float32 restatement v = fl(x + fl(k * y)) - of the host-decoded dry payload x and `Engine.resample` of each plane y (which
tests/test_export_gpu.py and tests/test_resample_gpu.py pin to the float64 formula); the pipeline against the same public pieces
composed by hand."""
import ctypes
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
ENCS = ("pcm16", "pcm32", "f32")
KS = (np.float32(-1.0), np.float32(0.0), np.float32(0.41), pipeline.remix_coefficient(6))


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


@pytest.fixture(scope="module")
def scratch_wav(tmp_path_factory):
    return str(tmp_path_factory.mktemp("remix") / "host.wav")


def _signal(kind: str, frames: int, rate: int, nch: int, seed):
    """tests/test_export_gpu.py::_signal: seeded noise, or two tones inside every pass band."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "noise":
        return (0.25 * rng.standard_normal((frames, nch))).astype(np.float32)
    t = np.arange(frames)[:, None] / rate
    f1, f2 = 0.011 * rate, 0.12 * rate
    ph = rng.uniform(0, 2 * np.pi, (2, nch))
    return (0.4 * np.sin(2 * np.pi * f1 * t + ph[0]) + 0.3 * np.sin(2 * np.pi * f2 * t + ph[1])).astype(np.float32)


def _host_bytes(scratch, x, enc) -> np.ndarray:
    """The data chunk `wavio.write_wav_*` writes for x ((frames,) or (frames, channels))."""
    WRITERS[enc](scratch, x, 16000)
    with open(scratch, "rb") as f:
        return np.frombuffer(f.read()[44:], dtype=np.uint8)


def _planes_bytes(scratch, v, enc) -> np.ndarray:
    """The same for (C, frames) planes."""
    return _host_bytes(scratch, v.T if v.shape[0] > 1 else v[0], enc)


def _padded(row: np.ndarray, pad: int = 0) -> np.ndarray:
    out = np.zeros((row.shape[0] + 3) // 4 * 4 + pad, dtype=np.uint8)
    out[:row.shape[0]] = row
    return out


def _decode(row: np.ndarray, enc: str, frames: int, nch: int) -> np.ndarray:
    """(C, frames) float32 of a payload row by `wavio.read_wav`'s rules, the device's `sample_at`."""
    s = np.frombuffer(row[:frames * nch * rs.SAMPLE_BYTES[enc]].tobytes(), dtype=DTYPES[enc])
    if enc == "pcm16":
        x = s.astype(np.float32) / np.float32(32768.0)
    elif enc == "pcm32":
        x = (s.astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        x = s.astype(np.float32)
    return np.ascontiguousarray(x.reshape(frames, nch).T)


def _dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _amount(*ks) -> torch.Tensor:
    return torch.tensor([float(k) for k in ks], dtype=torch.float32, device=DEV)


def _case(scratch, rate_in, rate_out, L_in, C, seed):
    """Planes at rate_in with some samples scaled to clip, their `Engine.resample` comes from the caller; a dry signal of the
    ceiling's frame count at rate_out, some of it beyond full scale (a float32 payload holds that)."""
    ceiling = rs.out_len(L_in, *rs.ratio(rate_in, rate_out))
    x = _signal("two-tone", L_in, rate_in, C, [31, C, rate_out, seed])
    x[100:110] *= 3.0
    d = 1.6 * _signal("noise", ceiling, rate_out, C, [32, C, rate_out, seed])
    d[5:9] = np.array([1.0, -1.0, 1.75, -1.75], dtype=np.float32)[:, None]
    return x, d, ceiling


# ---- 1. the encoder against the host writers on the host restatement ------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", [(16000, 44100), (32000, 48000), (16000, 11025), (16000, 16000)])
def test_remix_encode_equals_the_host_writers_on_the_restatement(eng, scratch_wav, rate_in, rate_out):
    """L_in = 1500: three tiles at 16 -> 44.1 kHz, the > 64 KiB LDS route at 16 -> 11.025 kHz, k_encode at 16 -> 16 kHz (two
    tiles).  Every pair of dry and output encoding, frames_out at the ceiling and 4 under it, four amounts; alone, a second
    time, and as row 1 of B = 3 with other amounts, strides and a wider dry and output row."""
    L_in, clips_seen = 1500, 0
    for C in (1, 3):
        x, d, ceiling = _case(scratch_wav, rate_in, rate_out, L_in, C, 0)
        planes = _dev(x.T)
        y = eng.resample(planes, rate_in, rate_out).cpu().numpy()
        assert y.shape == (C, ceiling)
        big = torch.randn(3, C + 1, L_in + 5, device=DEV)
        big[1, :C, :L_in] = planes
        view = big[:, :C, :L_in]
        assert view.stride(0) == (C + 1) * (L_in + 5) and view.stride(1) == L_in + 5
        for dry_enc in ENCS:
            row = _host_bytes(scratch_wav, d if C > 1 else d[:, 0], dry_enc)
            xd = _decode(row, dry_enc, ceiling, C)
            dry = _dev(_padded(row))[None]
            rows3 = torch.randint(0, 120, (3, dry.shape[1] + 16), dtype=torch.uint8, device=DEV)      # (float32 rows of small finite values)
            rows3[1, :dry.shape[1]] = dry[0]
            for enc in ENCS:
                for frames_out in (ceiling, ceiling - 4):
                    for k in KS:
                        v = pipeline.remix_host(xd[:, :frames_out], y[:, :frames_out], k)
                        want = _planes_bytes(scratch_wav, v, enc)
                        clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
                        alone = eng.remix_encode(planes, rate_in, rate_out, enc, dry, dry_enc, _amount(k), frames_out=frames_out,
                                                 clipped=clipped)
                        what = (C, dry_enc, enc, frames_out, float(k))
                        assert alone.shape == (1, want.shape[0]) and np.array_equal(alone[0].cpu().numpy(), want), what
                        clips = pipeline.host_clip_count(v, enc)
                        assert int(clipped[0]) == clips, what
                        clips_seen += clips
                        again = eng.remix_encode(planes, rate_in, rate_out, enc, dry, dry_enc, _amount(k), frames_out=frames_out)
                        assert torch.equal(again, alone), what
                        out = torch.full((3, (want.shape[0] + 3) // 4 * 4 + 12), 0xA5, dtype=torch.uint8, device=DEV)
                        counts = torch.zeros(3, dtype=torch.int32, device=DEV)
                        rows = eng.remix_encode(view, rate_in, rate_out, enc, rows3, dry_enc, _amount(0.3, k, -0.7),
                                                frames_out=frames_out, out=out, clipped=counts)
                        assert rows.shape == (3, want.shape[0]) and torch.equal(rows[1], alone[0]), what
                        assert not torch.equal(rows[0], alone[0]) and bool((out[:, want.shape[0]:] == 0xA5).all()), what
                        assert int(counts[1]) == clips, what
    assert clips_seen > 100


@pytest.mark.parametrize("rate_in,rate_out", [(16000, 44100), (16000, 16000)])
def test_remix_encode_with_a_gain(eng, scratch_wav, rate_in, rate_out):
    L_in, C = 1500, 3
    x, d, ceiling = _case(scratch_wav, rate_in, rate_out, L_in, C, 1)
    planes = _dev(x.T)
    y = eng.resample(planes, rate_in, rate_out).cpu().numpy()
    row = _host_bytes(scratch_wav, d, "pcm32")
    xd, dry = _decode(row, "pcm32", ceiling, C), _dev(_padded(row))[None]
    k = np.float32(0.41)
    for enc in ENCS:
        for g in (np.float32(0.37), np.float32(1.9)):
            v = pipeline.remix_host(xd, y, k, gain=g)
            clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
            got = eng.remix_encode(planes, rate_in, rate_out, enc, dry, "pcm32", _amount(k), clipped=clipped, gain=_amount(g))
            assert np.array_equal(got[0].cpu().numpy(), _planes_bytes(scratch_wav, v, enc)), (enc, float(g))
            assert int(clipped[0]) == pipeline.host_clip_count(v, enc)
        plain = eng.remix_encode(planes, rate_in, rate_out, enc, dry, "pcm32", _amount(k))
        assert torch.equal(eng.remix_encode(planes, rate_in, rate_out, enc, dry, "pcm32", _amount(k), gain=_amount(1.0)), plain)
    from lass_amd import _lib
    with pytest.raises(_lib.LassError, match="gain"):
        eng.remix_encode(planes, rate_in, rate_out, "pcm16", dry, "pcm32", _amount(k), gain=_amount(1.0, 1.0))
    with pytest.raises(_lib.LassError, match="amount"):
        eng.remix_encode(planes, rate_in, rate_out, "pcm16", dry, "pcm32", _amount(k, k))
    with pytest.raises(_lib.LassError, match="dry must be"):
        eng.remix_encode(planes, rate_in, rate_out, "pcm16", dry[:, :-8], "pcm32", _amount(k))
    with pytest.raises(_lib.LassError, match="dry_encoding"):
        eng.remix_encode(planes, rate_in, rate_out, "pcm16", dry, "pcm24", _amount(k))


# ---- 2. the peak ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", [(16000, 44100), (32000, 48000), (16000, 11025), (16000, 16000)])
def test_remix_peak_is_the_peak_of_what_the_encoder_quantises(eng, scratch_wav, rate_in, rate_out):
    L_in = 1500
    for C in (1, 3):
        x, d, ceiling = _case(scratch_wav, rate_in, rate_out, L_in, C, 2)
        planes = _dev(x.T)
        y = eng.resample(planes, rate_in, rate_out).cpu().numpy()
        big = torch.randn(3, C + 1, L_in + 5, device=DEV)
        big[1, :C, :L_in] = planes
        for dry_enc in ENCS:
            row = _host_bytes(scratch_wav, d if C > 1 else d[:, 0], dry_enc)
            xd, dry = _decode(row, dry_enc, ceiling, C), _dev(_padded(row))[None]
            rows3 = torch.randint(0, 120, (3, dry.shape[1] + 16), dtype=torch.uint8, device=DEV)
            rows3[1, :dry.shape[1]] = dry[0]
            for frames_out in (ceiling, ceiling - 4):
                for k in KS:
                    v = pipeline.remix_host(xd[:, :frames_out], y[:, :frames_out], k)
                    want = torch.tensor([np.max(np.abs(v))], dtype=torch.float32, device=DEV)
                    got = eng.remix_peak(planes, rate_in, rate_out, dry, dry_enc, _amount(k), frames_out=frames_out)
                    assert torch.equal(got, want), (C, dry_enc, frames_out, float(k), got, want)
                    three = eng.remix_peak(big[:, :C, :L_in], rate_in, rate_out, rows3, dry_enc, _amount(0.3, k, -0.7), frames_out=frames_out)
                    assert torch.equal(three[1:2], want)
    # a NaN in the planes is skipped: every output it reaches is, the rest still count
    hole = planes.clone()
    hole[C - 1, 700] = float("nan")
    yh = eng.resample(hole, rate_in, rate_out).cpu().numpy()
    v = pipeline.remix_host(xd, yh, KS[2])
    assert np.isnan(v).any() and not np.isnan(v).all()
    got = eng.remix_peak(hole, rate_in, rate_out, dry, dry_enc, _amount(KS[2]))
    assert torch.equal(got, torch.tensor([np.nanmax(np.abs(v))], dtype=torch.float32, device=DEV))


# ---- 3. the identities ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", [(16000, 16000), (16000, 44100)])
def test_amount_zero_returns_the_pcm16_payload_byte_for_byte(eng, rate_in, rate_out):
    C, frames = 3, 4097
    q = np.random.Generator(np.random.PCG64(33)).integers(-32768, 32768, (frames, C)).astype("<i2")
    q[:4] = np.array([-32768, 32767, 0, -1], dtype="<i2")[:, None]
    payload = _padded(np.frombuffer(q.tobytes(), dtype=np.uint8))
    L_in = rs.out_len(frames, *rs.ratio(rate_out, rate_in))
    assert rs.out_len(L_in, *rs.ratio(rate_in, rate_out)) >= frames
    planes = 5.0 * torch.randn(C, L_in, generator=torch.Generator().manual_seed(34)).to(DEV)         # finite, loud: 0 * y is +-0
    clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = eng.remix_encode(planes, rate_in, rate_out, "pcm16", _dev(payload)[None], "pcm16", _amount(0.0), frames_out=frames,
                           clipped=clipped)
    assert np.array_equal(got[0].cpu().numpy(), payload[:frames * C * 2]) and int(clipped[0]) == 0


@pytest.mark.parametrize("rate_in,rate_out", [(16000, 16000), (16000, 44100)])
def test_a_silent_dry_payload_gives_the_plain_export(eng, rate_in, rate_out):
    C, L_in = 2, 1500
    x = _signal("two-tone", L_in, rate_in, C, [35, rate_out])
    x[200:210] *= 3.0
    planes = _dev(x.T)
    ceiling = rs.out_len(L_in, *rs.ratio(rate_in, rate_out))
    dry = torch.zeros(1, ceiling * C * 4, dtype=torch.uint8, device=DEV)
    for enc in ("pcm16", "pcm32"):
        a, b = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        got = eng.remix_encode(planes, rate_in, rate_out, enc, dry, "f32", _amount(1.0), clipped=a)
        assert torch.equal(got, eng.resample_encode(planes, rate_in, rate_out, enc, clipped=b)) and int(a[0]) == int(b[0]) > 0


# ---- 4. one-frame tiles, 64-bit indices -------------------------------------------------------------------------------
def test_one_frame_tiles_with_a_dry_source(eng):
    """tests/test_export_gpu.py::test_one_frame_tiles_start_off_the_dword with a PCM16 dry payload and amount -1: up = 1, down =
    50 000 leaves tiles of ONE frame, and the dry source must not cost that plan its frame."""
    down, frames_out = 50000, 5
    L_in = (frames_out - 1) * down + 1
    x = np.zeros(L_in, dtype=np.float32)
    y = np.array([0.25, -0.5, 0.125, 0.75, -1.0], dtype=np.float32)
    x[::down] = y
    x[1::down] = 0.9                                          # neighbours that must not leak in
    q = np.array([16384, 8192, -4096, -8192, 16385], dtype="<i2")
    v = pipeline.remix_host(q.astype(np.float32) / np.float32(32768.0), y, -1.0)        # 0.25, 0.75, -0.25, -1, 1.5 + 1/32768
    planes, taps = torch.from_numpy(x).to(DEV), torch.tensor([0.0, 1.0, 0.0], device=DEV)
    dry = _dev(_padded(np.frombuffer(q.tobytes(), dtype=np.uint8)))
    amount, clipped = _amount(-1.0), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((16,), 0xA5, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = eng.lib.lass_remix_encode(eng.ctx, p(planes), L_in, L_in, 1, 1, L_in, 1, down, p(taps), 3, p(dry), 12, rs.ENCODINGS["pcm16"],
                                   p(amount), rs.ENCODINGS["pcm16"], ctypes.c_void_p(0), p(out), 12, frames_out, p(clipped),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.lass_last_error(eng.ctx).decode()
    got = out.cpu().numpy()
    assert np.array_equal(got[:10].view("<i2"), np.clip(np.round(v.astype(np.float64) * 32768), -32768, 32767).astype("<i2"))
    assert bool((got[10:] == 0xA5).all()) and int(clipped[0]) == 1
    peak = torch.full((1,), -7.25, device=DEV)
    rc = eng.lib.lass_remix_peak(eng.ctx, p(planes), L_in, L_in, 1, 1, L_in, 1, down, p(taps), 3, p(dry), 12, rs.ENCODINGS["pcm16"],
                                 p(amount), frames_out, p(peak), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and float(peak[0]) == float(np.max(np.abs(v)))


def test_long_plane_64bit_indexing_with_a_dry_source(eng, scratch_wav):
    """tests/test_export_gpu.py::test_long_plane_64bit_indexing's shape (310 s, 16 000 -> 44 100 Hz: n * down passes 2^31) with a
    mono PCM16 dry row; the last 4 096 frames against the host composition."""
    rate_in, rate_out, L_in = 16000, 44100, 310 * 16000
    frames_out = rs.out_len(L_in, *rs.ratio(rate_in, rate_out))
    plane = (0.25 * torch.randn(L_in, generator=torch.Generator().manual_seed(36))).to(DEV)
    q = torch.randint(-20000, 20000, (frames_out + 1,), dtype=torch.int16, generator=torch.Generator().manual_seed(37)).to(DEV)
    k = KS[2]
    clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = eng.remix_encode(plane[None], rate_in, rate_out, "pcm16", q.view(torch.uint8)[None], "pcm16", _amount(k), clipped=clipped)
    assert got.shape == (1, frames_out * 2)
    tail = eng.resample(plane, rate_in, rate_out)[-4096:].cpu().numpy()
    xd = q[frames_out - 4096:frames_out].cpu().numpy().astype(np.float32) / np.float32(32768.0)
    want = _host_bytes(scratch_wav, pipeline.remix_host(xd, tail, k), "pcm16")
    assert np.array_equal(got[0, -8192:].cpu().numpy(), want)
    assert np.max(np.abs(want.view("<i2").astype(np.int64))) > 3000
    pk = eng.remix_peak(plane[None], rate_in, rate_out, q.view(torch.uint8)[None], "pcm16", _amount(k))
    assert float(pk[0]) >= float(np.max(np.abs(pipeline.remix_host(xd, tail, k))))


# ---- 5. error paths ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_launch(eng):
    B, C, L_in, up, down = 2, 2, 1000, 441, 160
    ceiling = rs.out_len(L_in, up, down)
    planes = torch.zeros(B, C, L_in + 3, device=DEV)
    taps = torch.zeros(rs.MAX_TAPS + 2, dtype=torch.float32, device=DEV)
    row, dry_row = ceiling * C * 2, ceiling * C * 4
    out = torch.full((B, row + 8), 0x5A, dtype=torch.uint8, device=DEV)
    dry = torch.zeros(B, dry_row + 8, dtype=torch.uint8, device=DEV)
    amount, gain = torch.zeros(B, device=DEV), torch.ones(B, device=DEV)
    clipped = torch.zeros(B, dtype=torch.int32, device=DEV)
    peak = torch.full((B,), -7.25, device=DEV)
    good = dict(planes=planes.data_ptr(), row_stride=planes.stride(0), plane_stride=planes.stride(1), B=B, ch=C, L_in=L_in, up=up,
                down=down, taps=taps.data_ptr(), n_taps=rs.n_taps(up, down), dry=dry.data_ptr(), dry_stride=dry.stride(0),
                dry_enc=rs.ENCODINGS["pcm32"], amount=amount.data_ptr(), enc=rs.ENCODINGS["pcm16"], gain=0, out=out.data_ptr(),
                out_stride=out.stride(0), frames_out=ceiling, clipped=clipped.data_ptr(), peak=peak.data_ptr())
    vp, stream = ctypes.c_void_p, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def encode(**kw):
        a = dict(good, **kw)
        rc = eng.lib.lass_remix_encode(eng.ctx, vp(a["planes"]), a["row_stride"], a["plane_stride"], a["B"], a["ch"], a["L_in"], a["up"],
                                       a["down"], vp(a["taps"]), a["n_taps"], vp(a["dry"]), a["dry_stride"], a["dry_enc"], vp(a["amount"]),
                                       a["enc"], vp(a["gain"]), vp(a["out"]), a["out_stride"], a["frames_out"], vp(a["clipped"]), stream)
        return rc, eng.lib.lass_last_error(eng.ctx).decode()

    def peak_of(**kw):
        a = dict(good, **kw)
        rc = eng.lib.lass_remix_peak(eng.ctx, vp(a["planes"]), a["row_stride"], a["plane_stride"], a["B"], a["ch"], a["L_in"], a["up"],
                                     a["down"], vp(a["taps"]), a["n_taps"], vp(a["dry"]), a["dry_stride"], a["dry_enc"], vp(a["amount"]),
                                     a["frames_out"], vp(a["peak"]), stream)
        return rc, eng.lib.lass_last_error(eng.ctx).decode()

    new = [dict(dry=0), dict(dry=dry.data_ptr() + 2), dict(dry_enc=3), dict(dry_enc=-1), dict(dry_stride=dry_row - 4),
           dict(dry_stride=dry_row + 2), dict(dry_enc=rs.ENCODINGS["pcm16"], dry_stride=row - 4), dict(amount=0),
           dict(amount=amount.data_ptr() + 2)]
    inherited = [dict(frames_out=ceiling + 1), dict(frames_out=0), dict(ch=9), dict(plane_stride=L_in - 1), dict(n_taps=8820),
                 dict(up=0), dict(taps=0), dict(planes=0), dict(B=0), dict(L_in=0)]
    for kw in new + inherited + [dict(out=0), dict(out=out.data_ptr() + 2), dict(out_stride=row + 2), dict(out_stride=row - 4),
                                 dict(enc=3), dict(gain=gain.data_ptr() + 2)]:
        rc, msg = encode(**kw)
        assert rc == -1 and msg.startswith("lass_remix_encode:"), (kw, rc, msg)      # LASS_ERR_ARG
    for kw in new + inherited + [dict(peak=0), dict(peak=peak.data_ptr() + 2)]:
        rc, msg = peak_of(**kw)
        assert rc == -1 and msg.startswith("lass_remix_peak:"), (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and int(clipped.sum()) == 0 and bool((peak == -7.25).all())
    # the good calls do run: a silent remix
    rc, msg = encode()
    assert rc == 0, msg
    rc, msg = encode(gain=gain.data_ptr())
    assert rc == 0, msg
    rc, msg = peak_of()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert bool((out[:, :row] == 0).all()) and bool((out[:, row:] == 0x5A).all()) and bool((peak == 0).all())


# ---- 6. separate_files ------------------------------------------------------------------------------------------------
SR, WINDOW, CONTEXT = 16000, 32000, 3200
CAPTIONS = ["a dog barking", "rain on a roof", "a dog barking"]
DBS = [-np.inf, -12.0, 6.0]
KW = dict(window=WINDOW, context=CONTEXT)


@pytest.fixture(scope="module")
def holder(synthetic_sd):
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    return AudioSep(ss_model=m.to(DEV).eval().set_compute_dtype("f32"), query_encoder=PrecomputedQueryEncoder())


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """44.1 kHz stereo PCM16 of 3.1 s, 16 kHz mono f32 of 0.5 s, 32 kHz 3-channel PCM32 of 2.3 s."""
    d = tmp_path_factory.mktemp("files")
    specs = [("a.wav", "pcm16", 44100, 2, 136710), ("b.wav", "f32", 16000, 1, 8000), ("c.wav", "pcm32", 32000, 3, 73600)]
    paths = []
    for i, (name, enc, rate, nch, frames) in enumerate(specs):
        x = 0.6 * _signal("noise", frames, rate, nch, [38, i]) + 0.5 * _signal("two-tone", frames, rate, nch, [38, i, 1])
        paths.append(str(d / name))
        WRITERS[enc](paths[-1], x if nch > 1 else x[:, 0], rate)
    return d, paths


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _raw_row(path):
    info = wavio.wav_info(path)
    enc, nch, rate, frames, _ = info
    row = np.zeros(frames * nch * rs.SAMPLE_BYTES[enc], dtype=np.uint8)
    assert wavio.read_wav_raw_into(path, info, row)
    return row, enc, nch, rate, frames


def _separate_by_hand(holder, eng, paths, captions):
    """Per file (its separated planes at the model rate, on the device; its raw row; encoding, channels, rate, frames): every
    channel decoded on its own and separated in one `separate_long_list` call, as the pass does."""
    planes, conds, metas = [], [], []
    for p, cap in zip(paths, captions):
        row, enc, nch, rate, frames = _raw_row(p)
        chans = np.frombuffer(row.tobytes(), dtype=DTYPES[enc]).reshape(frames, nch)
        mine = [eng.decode_resample(_dev(_padded(np.frombuffer(np.ascontiguousarray(chans[:, c]).tobytes(), dtype=np.uint8))),
                                    frames, 1, enc, rate, SR)[0] for c in range(nch)]
        cond = holder.query_encoder.get_query_embed(modality="text", text=[cap], device=DEV)[0]
        planes += mine
        conds += [cond] * nch
        metas.append((row, enc, nch, rate, frames))
    seps = holder.ss_model.separate_long_list(planes, torch.stack(conds), **KW)
    out, at = [], 0
    for m in metas:
        out.append((seps[at:at + m[2]],) + m)
        at += m[2]
    return out


@pytest.fixture(scope="module")
def by_hand(holder, eng, files):
    return _separate_by_hand(holder, eng, files[1], CAPTIONS)


@pytest.fixture(scope="module")
def plain_run(holder, files):
    d, paths = files
    outs = [str(d / f"plain_{k}.wav") for k in range(3)]
    return outs, pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs)), SR, **KW)


@pytest.fixture(scope="module")
def remix_run(holder, files):
    d, paths = files
    outs = [str(d / f"remix_{k}.wav") for k in range(3)]
    return outs, pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs)), SR, target_gain_db=DBS, **KW)


def test_separate_files_remix_equals_the_pieces_by_hand(eng, files, by_hand, remix_run):
    d, paths = files
    outs, recs = remix_run
    for p, o, rec, db, (seps, row, enc, nch, rate, frames) in zip(paths, outs, recs, DBS, by_hand):
        y = np.stack([eng.resample(s, SR, rate)[:frames].cpu().numpy() for s in seps])
        v = pipeline.remix_host(_decode(row, enc, frames, nch), y, pipeline.remix_coefficient(db))
        hand = str(d / "hand.wav")
        WRITERS[enc](hand, v.T if nch > 1 else v[0], rate)
        assert wavio.wav_info(o) == wavio.wav_info(p) == (enc, nch, rate, frames, 44)      # the input's header
        assert _read(o) == _read(hand), (p, db)
        assert rec == dict(rate=rate, channels=nch, frames=frames, path="device", clipped=pipeline.host_clip_count(v, enc),
                           target_gain_db=db), rec
    # removing the target took something out, the boost put something in: neither file is the input, both are close to it
    assert _read(outs[0])[44:] != _read(paths[0])[44:]


def test_at_0_db_the_file_comes_back(holder, files):
    d, paths = files
    outs = [str(d / f"zero_{k}.wav") for k in range(3)]
    recs = pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs)), SR, target_gain_db=0.0, **KW)
    assert _read(outs[0])[44:] == _read(paths[0])[44:]                                   # PCM16: byte for byte
    assert np.array_equal(np.frombuffer(_read(outs[1])[44:], dtype="<f4"), np.frombuffer(_read(paths[1])[44:], dtype="<f4"))
    # PCM32 comes back as its float32 rounding: 24 of 31 bits kept, at most 2^6 away
    a, b = (np.frombuffer(_read(f)[44:], dtype="<i4").astype(np.int64) for f in (outs[2], paths[2]))
    assert int(np.max(np.abs(a - b))) <= 64
    assert [r["clipped"] for r in recs] == [0, 0, 0] and all(r["target_gain_db"] == 0.0 for r in recs)


def test_jobs_of_four_write_both_stems_from_one_separation(holder, files, plain_run, remix_run, monkeypatch):
    d, paths = files
    outs = [str(d / f"both_t_{k}.wav") for k in range(3)]
    remixes = [str(d / f"both_r_{k}.wav") for k in range(3)]
    calls, sep = [], holder.ss_model.separate_long_list
    with monkeypatch.context() as mp:
        mp.setattr(holder.ss_model, "separate_long_list", lambda *a, **kw: (calls.append(len(a[0])), sep(*a, **kw))[1])
        recs = pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs, remixes)), SR, target_gain_db=DBS, **KW)
    assert calls == [6]                                                      # one pass, one separation of the six planes
    for k in range(3):
        assert _read(outs[k]) == _read(plain_run[0][k]) and _read(remixes[k]) == _read(remix_run[0][k]), k
        rec = dict(recs[k])
        assert rec.pop("remix") == remix_run[1][k] and rec == plain_run[1][k]


def test_target_gain_db_none_is_the_call_without_it(holder, files, plain_run):
    d, paths = files
    outs = [str(d / f"none_{k}.wav") for k in range(3)]
    recs = pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs)), SR, target_gain_db=None, **KW)
    assert recs == plain_run[1] and all("target_gain_db" not in r and "remix" not in r for r in recs)
    assert [_read(o) for o in outs] == [_read(o) for o in plain_run[0]]


def test_a_ceiling_keeps_a_boost_from_clipping(holder, eng, files):
    d, _ = files
    loud, frames, rate = str(d / "loud.wav"), 52000, 44100
    x = 0.6 * _signal("noise", frames, rate, 2, [39]) + 0.5 * _signal("two-tone", frames, rate, 2, [39, 1])
    wavio.write_wav_pcm16(loud, (0.999 / np.max(np.abs(x))) * x, rate)
    free, held = str(d / "loud_free.wav"), str(d / "loud_held.wav")
    (seps, row, enc, nch, _, _), = _separate_by_hand(holder, eng, [loud], ["a dog barking"])
    stacked, dry, amount = torch.stack(seps), _dev(_padded(row))[None], _amount(pipeline.remix_coefficient(12))
    y = eng.resample(stacked, SR, rate)[:, :frames].cpu().numpy()
    v = pipeline.remix_host(_decode(row, enc, frames, nch), y, pipeline.remix_coefficient(12))
    # without a ceiling the boost clips, and the record says how often
    rec = pipeline.separate_files(holder, [(loud, "a dog barking", free)], SR, target_gain_db=12, encoding="pcm16", **KW)[0]
    assert rec["clipped"] == pipeline.host_clip_count(v, "pcm16") > 0 and "gain" not in rec
    # with one: remix_peak -> loudness_gain (the ceiling's gain alone) -> remix_encode(gain=)
    rec = pipeline.separate_files(holder, [(loud, "a dog barking", held)], SR, target_gain_db=12, encoding="pcm16",
                                  peak_ceiling_db=-1.0, **KW)[0]
    ceiling = ld.ceiling_for(-1.0, "pcm16")
    pk = eng.remix_peak(stacked, SR, rate, dry, enc, amount, frames_out=frames)
    assert float(pk[0]) == float(np.max(np.abs(v))) > 1.0
    gain, limited = eng.loudness_gain(torch.full((1,), -np.inf, dtype=torch.float64, device=DEV), pk, None, ceiling)
    clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    want = eng.remix_encode(stacked, SR, rate, "pcm16", dry, enc, amount, frames_out=frames, clipped=clipped, gain=gain)
    assert _read(held)[44:] == want[0].cpu().numpy().tobytes() and int(clipped[0]) == 0 and int(limited[0]) == 1
    assert rec["clipped"] == 0 and rec["peak_limited"] is True and "loudness_out" not in rec
    assert rec["gain"] == float(gain[0]) == float(ld.gain_for(-np.inf, np.float32(pk[0].item()), None, ceiling)[0]) < 1.0
    assert rec["gain_db"] == pytest.approx(20.0 * np.log10(rec["gain"])) and rec["target_gain_db"] == 12.0
    q = np.frombuffer(_read(held)[44:], dtype="<i2").astype(np.int64)
    assert np.max(np.abs(q)) <= np.rint(np.float64(ceiling) * 32768.0) and np.max(np.abs(q)) >= 0.98 * ceiling * 32768.0


@pytest.mark.filterwarnings("ignore:.*parity with the reference is unpinned.*:UserWarning")
def test_odd_rate_file_takes_the_host_route(holder, files):
    """44 101 Hz <-> 16 000 Hz is over the tap cap both ways: decode, remix and export run on the host (`remix_host`), within
    1 LSB of the same composition made by hand (the bar of tests/test_export_gpu.py's host-route test: the separation is the
    device's, the rest float32 numpy on both sides)."""
    d, _ = files
    odd, out, frames = str(d / "odd.wav"), str(d / "odd_out.wav"), 30000
    wavio.write_wav_pcm16(odd, 0.5 * _signal("two-tone", frames, 44101, 2, [40]), 44101)
    rec = pipeline.separate_files(holder, [(odd, "rain on a roof", out)], SR, target_gain_db=-12.0, peak_ceiling_db=-12.0, **KW)[0]
    assert rec["path"] == "host" and rec["target_gain_db"] == -12.0 and rec["frames"] == frames and rec["clipped"] == 0
    assert wavio.wav_info(out) == ("pcm16", 2, 44101, frames, 44)
    decoded = np.frombuffer(_read(odd)[44:], dtype="<i2").reshape(frames, 2).astype(np.float32) / np.float32(32768.0)
    planes = [torch.from_numpy(wavio._resample(decoded[:, c], 44101, SR)).to(DEV) for c in range(2)]
    cond = holder.query_encoder.get_query_embed(modality="text", text=["rain on a roof"], device=DEV)[0]
    seps = holder.ss_model.separate_long_list(planes, torch.stack([cond, cond]), **KW)
    y = np.stack([wavio._resample(s.cpu().numpy(), SR, 44101)[:frames] for s in seps])
    v = pipeline.remix_host(decoded.T, y, pipeline.remix_coefficient(-12.0))
    g, bit = ld.gain_for(-np.inf, np.float32(np.max(np.abs(v))), None, ld.ceiling_for(-12.0, "pcm16"))
    assert rec["peak_limited"] == bit and rec["gain"] == pytest.approx(float(g), rel=1e-4)
    want = np.clip(np.round((g * v).astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64)
    got = np.frombuffer(_read(out)[44:], dtype="<i2").reshape(frames, 2).T.astype(np.int64)
    worst = int(np.max(np.abs(got - want)))
    print(f"host route: worst difference to the hand-made host remix {worst} LSB")
    assert worst <= 1 and np.max(np.abs(got)) > 3000
