"""Export path on the GPU: `lass_decode_resample_planar` (per-channel decode), `lass_resample_encode` (resample back + PCM
encode + interleave) and the file pipeline on top of them (lass_amd/pipeline.py).

Yardsticks: the planar decode is compared bit for bit with `Engine.decode_resample` of each channel alone; the encoder with the
host writers (`wavio.write_wav_*`, whose float64 rule tests/test_pipeline_cpu.py shows equal to the device's float32 rule) applied
to `Engine.resample` of each plane; the resampled values themselves with `resample.resample_host` in float64 under
tests/test_resample_gpu.py's bar (4 x the float32 host evaluation's own deviation); the pipeline with the same public pieces
composed by hand.  Everything is equality unless a bar is stated."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lass_amd import pipeline, wavio
from lass_amd import resample as rs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WRITERS = {"pcm16": wavio.write_wav_pcm16, "pcm32": wavio.write_wav_pcm32, "f32": wavio.write_wav_f32}
DTYPES = {"pcm16": "<i2", "pcm32": "<i4", "f32": "<f4"}


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


@pytest.fixture(scope="module")
def scratch_wav(tmp_path_factory):
    return str(tmp_path_factory.mktemp("export") / "host.wav")


def _signal(kind: str, frames: int, rate: int, nch: int, seed):
    """tests/test_resample_gpu.py::_signal: seeded noise, or two tones inside every pass band."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "noise":
        return (0.25 * rng.standard_normal((frames, nch))).astype(np.float32)
    t = np.arange(frames)[:, None] / rate
    f1, f2 = 0.011 * rate, 0.12 * rate
    ph = rng.uniform(0, 2 * np.pi, (2, nch))
    return (0.4 * np.sin(2 * np.pi * f1 * t + ph[0]) + 0.3 * np.sin(2 * np.pi * f2 * t + ph[1])).astype(np.float32)


def _host_bytes(scratch, x, enc) -> np.ndarray:
    """The data chunk `wavio.write_wav_*` writes for x ((frames,) or (frames, channels)): the host's quantise + interleave."""
    WRITERS[enc](scratch, x, 16000)
    with open(scratch, "rb") as f:
        return np.frombuffer(f.read()[44:], dtype=np.uint8)


def _padded(row: np.ndarray, pad: int = 0) -> np.ndarray:
    out = np.zeros((row.shape[0] + 3) // 4 * 4 + pad, dtype=np.uint8)
    out[:row.shape[0]] = row
    return out


def _edge_values() -> np.ndarray:
    """The kinds of tests/test_pipeline_cpu.py's quantisation test: ties of both scales, +-1, just in and out of range, huge,
    denormal."""
    k = np.arange(-40, 40, dtype=np.float64)
    v = np.concatenate([(k + 0.5) / 32768.0, np.array([32766.5, 32767.5, -32767.5, -32768.5, 32767.49, -32768.51]) / 32768.0,
                        (np.arange(-20, 20, dtype=np.float64) * 2.0 + 1.0) * 2.0 ** -32,
                        [1.0, -1.0, 1.5, -1.5, 0.99999994, -0.99999994, 1.0000001, -1.0000001, 3e38, -3e38, 1e-40, -1e-40, 1.4e-45,
                         0.0, -0.0, 2.0 ** -31, -2.0 ** -31, 0.5, 2147483520.0 / 2.0 ** 31]])
    return v.astype(np.float32)


# ---- 1. planar decode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["pcm16", "pcm32", "f32"])
@pytest.mark.parametrize("nch", [1, 2, 3, 8])
def test_planar_decode_equals_mono_decode_of_each_channel(eng, scratch_wav, enc, nch):
    """frames = 4099: L_out crosses a 2 048-output tile for every pair; B = 3 behind a padded row stride."""
    frames, B = 4099, 3
    for rate_in, rate_out in [(16000, 16000), (32000, 16000), (44100, 16000), (16000, 44100), (8000, 16000)]:
        xs = [_signal("noise" if b % 2 else "two-tone", frames, rate_in, nch, [1, b, nch, rate_in]) for b in range(B)]
        for x in xs:
            x[:4] = np.array([1.0, -1.0, 0.999999, -3e-5], dtype=np.float32)[:, None]
        raw = torch.from_numpy(np.stack([_padded(_host_bytes(scratch_wav, x if nch > 1 else x[:, 0], enc), 128) for x in xs])).to(DEV)
        assert raw.stride(0) >= frames * nch * rs.SAMPLE_BYTES[enc] + 128
        got = eng.decode_resample_planar(raw, frames, nch, enc, rate_in, rate_out)
        L_out = rs.out_len(frames, *rs.ratio(rate_in, rate_out))
        assert got.shape == (B, nch, L_out) and got.dtype == torch.float32 and got.is_contiguous()
        for c in range(nch):
            mono = torch.from_numpy(np.stack([_padded(_host_bytes(scratch_wav, x[:, c], enc)) for x in xs])).to(DEV)
            want = eng.decode_resample(mono, frames, 1, enc, rate_in, rate_out)
            assert torch.equal(got[:, c], want), (rate_in, rate_out, c)
        assert float(got.abs().max()) > 0.1
        alone = eng.decode_resample_planar(raw[1:2].contiguous(), frames, nch, enc, rate_in, rate_out)
        assert torch.equal(alone[0], got[1])
        out = torch.empty_like(got)
        assert eng.decode_resample_planar(raw, frames, nch, enc, rate_in, rate_out, out=out) is out and torch.equal(out, got)


# ---- 2. encode without resampling ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["pcm16", "pcm32", "f32"])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_encode_equals_the_host_writers(eng, scratch_wav, enc, C):
    """L = 4097 (four 1 024-frame tiles and one frame): C * L is odd for C = 1 and 3, so the PCM16 row ends on a 2-byte store."""
    L = 4097
    x = _signal("noise", L, 16000, C, [2, C])
    edge = _edge_values()
    for c in range(C):
        x[5 + c:5 + c + edge.shape[0], c] = edge           # (shifted per channel: the frames mix kinds)
        x[1020 + c:1030 + c, c] *= 40.0                       # clipping across a tile boundary
    x[3000, C - 1] = 0.125                                    # (the NaN's place below: unclipped)
    planes = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = eng.resample_encode(planes, 16000, 16000, enc, clipped=clipped)
    want = _host_bytes(scratch_wav, x if C > 1 else x[:, 0], enc)
    assert got.shape == (1, L * C * rs.SAMPLE_BYTES[enc]) and got.dtype == torch.uint8
    assert np.array_equal(got[0].cpu().numpy(), want)
    host_clips = pipeline.host_clip_count(x, enc)
    assert int(clipped[0]) == host_clips and (host_clips > 10 or enc == "f32")
    # one NaN encodes as PCM 0 (and stays itself as float32), is not counted, and disturbs no neighbour
    planes[C - 1, 3000] = float("nan")
    clipped.zero_()
    got = eng.resample_encode(planes, 16000, 16000, enc, clipped=clipped)[0].cpu().numpy().view(DTYPES[enc]).copy()
    ref = want.view(DTYPES[enc]).copy()
    at = 3000 * C + C - 1
    assert np.isnan(got[at]) if enc == "f32" else got[at] == 0
    got[at] = ref[at]
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)) and int(clipped[0]) == host_clips


# ---- 3. encode with resampling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", [(16000, 44100), (16000, 48000), (32000, 48000), (32000, 44100), (16000, 11025)])
def test_resample_encode_equals_export_of_the_device_resampler(eng, scratch_wav, rate_in, rate_out):
    """16 000 -> 11 025 Hz: 13 671 floats of table + 3 001 of span + the stage pass 64 KiB (the raised dynamic-LDS limit)."""
    L_in = 1500
    up, down = rs.ratio(rate_in, rate_out)
    ceiling = rs.out_len(L_in, up, down)
    for C in (1, 3):
        x = _signal("two-tone", L_in, rate_in, C, [3, C, rate_out])
        x[100:110] *= 3.0                                    # some clipping
        planes = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
        y = eng.resample(planes, rate_in, rate_out).cpu().numpy()           # (C, ceiling)
        assert y.shape == (C, ceiling)
        big = torch.randn(3, C + 1, L_in + 5, device=DEV)
        big[1, :C, :L_in] = planes
        for enc in ("pcm16", "pcm32", "f32"):
            for frames_out in (ceiling, ceiling - 4):
                want = _host_bytes(scratch_wav, y[:, :frames_out].T if C > 1 else y[0, :frames_out], enc)
                clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
                alone = eng.resample_encode(planes, rate_in, rate_out, enc, frames_out=frames_out, clipped=clipped)
                assert np.array_equal(alone[0].cpu().numpy(), want), (C, enc, frames_out)
                assert int(clipped[0]) == pipeline.host_clip_count(y[:, :frames_out], enc)
                assert torch.equal(eng.resample_encode(planes, rate_in, rate_out, enc, frames_out=frames_out), alone)   # second call
                # as row 1 of B = 3 behind non-trivial row and plane strides, into a wider output whose tail stays untouched
                view = big[:, :C, :L_in]
                assert view.stride(0) == (C + 1) * (L_in + 5) and view.stride(1) == L_in + 5
                out = torch.full((3, (want.shape[0] + 3) // 4 * 4 + 12), 0xA5, dtype=torch.uint8, device=DEV)
                counts = torch.zeros(3, dtype=torch.int32, device=DEV)
                rows = eng.resample_encode(view, rate_in, rate_out, enc, frames_out=frames_out, out=out, clipped=counts)
                assert rows.shape == (3, want.shape[0]) and torch.equal(rows[1], alone[0])
                assert not torch.equal(rows[0], alone[0]) and bool((out[:, want.shape[0]:] == 0xA5).all())
                assert int(counts[1]) == int(clipped[0])


def test_one_frame_tiles_start_off_the_dword(eng):
    """A ratio whose one-frame span nearly fills the LDS leaves a tile of ONE frame: with PCM16 mono every odd tile then starts in
    the middle of a dword (the 2-byte head store).  up = 1, down = 50 000, taps (0, 1, 0): y[n] = x[n * down]."""
    down, frames_out = 50000, 5
    L_in = (frames_out - 1) * down + 1
    x = np.zeros(L_in, dtype=np.float32)
    want = np.array([0.25, -0.5, 0.125, 0.75, -1.0], dtype=np.float32)
    x[::down] = want
    x[1::down] = 0.9                                          # neighbours that must not leak in
    planes, taps = torch.from_numpy(x).to(DEV), torch.tensor([0.0, 1.0, 0.0], device=DEV)
    out = torch.full((16,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = eng.lib.lass_resample_encode(eng.ctx, ctypes.c_void_p(planes.data_ptr()), L_in, L_in, 1, 1, L_in, 1, down,
                                      ctypes.c_void_p(taps.data_ptr()), 3, rs.ENCODINGS["pcm16"], ctypes.c_void_p(out.data_ptr()), 12,
                                      frames_out, ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.lass_last_error(eng.ctx).decode()
    got = out.cpu().numpy()
    assert np.array_equal(got[:10].view("<i2"), np.clip(np.round(want.astype(np.float64) * 32768), -32768, 32767).astype("<i2"))
    assert bool((got[10:] == 0xA5).all())


# ---- 4. against the float64 yardstick -----------------------------------------------------------------------------------
def test_export_against_the_float64_yardstick(eng):
    """F32 export within 4 x the float32 host evaluation's own deviation from the float64 formula; PCM16
    within 1 LSB of the float64 formula quantised in float64.  The second is derived, not measured: the float32 evaluation is
    off by < 1e-6 = 0.03 LSB, so a sample can differ only where the exact value sits that close to a rounding boundary."""
    rate_in, rate_out, L_in = 16000, 44100, 6000
    up, down = rs.ratio(rate_in, rate_out)
    for kind in ("noise", "two-tone"):
        x = _signal(kind, L_in, rate_in, 2, [4, kind == "noise"])
        planes = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
        f32 = eng.resample_encode(planes, rate_in, rate_out, "f32")[0].cpu().numpy().view("<f4").reshape(-1, 2)
        q16 = eng.resample_encode(planes, rate_in, rate_out, "pcm16")[0].cpu().numpy().view("<i2").reshape(-1, 2)
        for c in range(2):
            ref = rs.resample_host(x[:, c], up, down)
            host32 = rs.resample_host(x[:, c], up, down, dtype=np.float32)
            bar = 4.0 * float(np.max(np.abs(host32.astype(np.float64) - ref)))
            err = float(np.max(np.abs(f32[:, c].astype(np.float64) - ref)))
            q_ref = np.clip(np.round(ref * 32768.0), -32768, 32767).astype(np.int64)
            lsb = np.abs(q16[:, c].astype(np.int64) - q_ref)
            print(f"{kind} ch{c}: f32 export {err:.3e} bar {bar:.3e}; pcm16 differing samples {np.count_nonzero(lsb)} of {lsb.shape[0]}, "
                  f"worst {int(lsb.max())} LSB")
            assert f32.shape[0] == ref.shape[0] and err <= bar
            assert int(lsb.max()) <= 1


# ---- 5. round trip ------------------------------------------------------------------------------------------------------
def test_pcm16_round_trip_is_the_identity(eng):
    C, L = 3, 4097
    q = np.random.Generator(np.random.PCG64(5)).integers(-32768, 32768, (C, L)).astype(np.int32)
    q[:, :4] = np.array([-32768, 32767, 0, -1])
    x = torch.from_numpy((q / 32768.0).astype(np.float32)).to(DEV)
    clipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    raw = eng.resample_encode(x, 16000, 16000, "pcm16", clipped=clipped)
    assert np.array_equal(raw[0].cpu().numpy().view("<i2").reshape(L, C).T, q.astype("<i2")) and int(clipped[0]) == 0
    back = eng.decode_resample_planar(raw, L, C, "pcm16", 16000, 16000)
    assert torch.equal(back[0], x)


# ---- 6. 64-bit indexing -------------------------------------------------------------------------------------------------
def test_long_plane_64bit_indexing(eng, scratch_wav):
    """310 s at 16 000 -> 44 100 Hz: n * down = 13.67e6 * 160 passes 2^31.  The last 4 096 frames against `Engine.resample`'s
    (the input side's own 64-bit test pins that one to the host formula)."""
    rate_in, rate_out, L_in = 16000, 44100, 310 * 16000
    up, down = rs.ratio(rate_in, rate_out)
    frames_out = rs.out_len(L_in, up, down)
    assert (frames_out - 1) * down > 2 ** 31
    plane = (0.25 * torch.randn(L_in, generator=torch.Generator().manual_seed(6))).to(DEV)
    got = eng.resample_encode(plane[None], rate_in, rate_out, "pcm16")
    assert got.shape == (1, frames_out * 2)
    tail = eng.resample(plane, rate_in, rate_out)[-4096:].cpu().numpy()
    want = _host_bytes(scratch_wav, tail, "pcm16")
    assert np.array_equal(got[0, -8192:].cpu().numpy(), want)
    assert np.max(np.abs(want.view("<i2").astype(np.int64))) > 3000


# ---- 7. error paths -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_launch(eng):
    from lass_amd import _lib
    B, C, L_in, up, down = 2, 2, 1000, 441, 160
    ceiling = rs.out_len(L_in, up, down)
    planes = torch.zeros(B, C, L_in + 3, device=DEV)
    taps = torch.zeros(rs.MAX_TAPS + 2, dtype=torch.float32, device=DEV)
    row = ceiling * C * 2
    out = torch.full((B, row + 8), 0x5A, dtype=torch.uint8, device=DEV)
    clipped = torch.zeros(B, dtype=torch.int32, device=DEV)
    good = dict(planes=planes.data_ptr(), row_stride=planes.stride(0), plane_stride=planes.stride(1), B=B, ch=C, L_in=L_in, up=up,
                down=down, taps=taps.data_ptr(), n_taps=rs.n_taps(up, down), enc=rs.ENCODINGS["pcm16"], out=out.data_ptr(),
                out_stride=out.stride(0), frames_out=ceiling, clipped=clipped.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        rc = eng.lib.lass_resample_encode(eng.ctx, ctypes.c_void_p(a["planes"]), a["row_stride"], a["plane_stride"], a["B"], a["ch"],
                                          a["L_in"], a["up"], a["down"], ctypes.c_void_p(a["taps"]), a["n_taps"], a["enc"],
                                          ctypes.c_void_p(a["out"]), a["out_stride"], a["frames_out"], ctypes.c_void_p(a["clipped"]),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, eng.lib.lass_last_error(eng.ctx).decode()

    bad = [dict(frames_out=ceiling + 1), dict(frames_out=0), dict(ch=9), dict(ch=0), dict(out=out.data_ptr() + 2),
           dict(out_stride=row + 2), dict(out_stride=row - 4), dict(plane_stride=L_in - 1), dict(row_stride=planes.stride(1) + L_in - 1),
           dict(n_taps=8820), dict(n_taps=rs.MAX_TAPS + 2), dict(enc=3), dict(enc=-1), dict(up=0), dict(down=0), dict(taps=0),
           dict(planes=0), dict(out=0), dict(B=0), dict(L_in=0), dict(up=30000, down=1, n_taps=3, frames_out=5)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("lass_resample_encode:"), (kw, rc, msg)   # LASS_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and int(clipped.sum()) == 0
    # the planar decoder shares lass_decode_resample's limits under its own name
    raw = torch.zeros(2, 1000 * 2 * 2 + 8, dtype=torch.uint8, device=DEV)
    dec = torch.full((2, 2, rs.out_len(1000, 160, 441) + 1), -7.25, device=DEV)
    for kw in (dict(ch=9), dict(enc=3), dict(n_taps=8820), dict(L_out=dec.shape[2]), dict(stride=1000 * 2 * 2 - 4)):
        a = dict(dict(ch=2, enc=0, n_taps=rs.n_taps(160, 441), L_out=dec.shape[2] - 1, stride=raw.stride(0)), **kw)
        rc = eng.lib.lass_decode_resample_planar(eng.ctx, ctypes.c_void_p(raw.data_ptr()), a["stride"], 2, 1000, a["ch"], a["enc"], 160, 441,
                                                 ctypes.c_void_p(taps.data_ptr()), a["n_taps"], ctypes.c_void_p(dec.data_ptr()), a["L_out"],
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == -1 and eng.lib.lass_last_error(eng.ctx).decode().startswith("lass_decode_resample_planar:"), kw
    torch.cuda.synchronize()
    assert bool((dec == -7.25).all())
    # the Python layer's own refusals, in decode_resample's words
    with pytest.raises(_lib.LassError, match="cap"):
        eng.resample_encode(torch.zeros(1, 100, device=DEV), 16000, 44101, "pcm16")
    with pytest.raises(_lib.LassError, match="frames_out"):
        eng.resample_encode(torch.zeros(1, 100, device=DEV), 16000, 44100, "pcm16", frames_out=277)
    with pytest.raises(_lib.LassError, match="encoding"):
        eng.resample_encode(torch.zeros(1, 100, device=DEV), 16000, 44100, "pcm24")
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and bool((out[:, :row] == 0).all()) and bool((out[:, row:] == 0x5A).all())   # the good call does run


# ---- 8. separate_files --------------------------------------------------------------------------------------------------
SR, WINDOW, CONTEXT = 16000, 32000, 3200
CAPTIONS = ["a dog barking", "rain on a roof", "a dog barking"]


def _make_model(sd, mode="f32"):
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return AudioSep(ss_model=m.to(DEV).eval().set_compute_dtype(mode), query_encoder=PrecomputedQueryEncoder())


@pytest.fixture(scope="module")
def holder(synthetic_sd):
    return _make_model(synthetic_sd)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """44.1 kHz stereo PCM16 of 3.1 s and 32 kHz 3-channel PCM32 of 2.3 s (several windows each), 16 kHz mono f32 of 0.5 s (one
    short clip: the separate_list branch)."""
    d = tmp_path_factory.mktemp("files")
    specs = [("a.wav", "pcm16", 44100, 2, 136710), ("b.wav", "f32", 16000, 1, 8000), ("c.wav", "pcm32", 32000, 3, 73600)]
    paths = []
    for i, (name, enc, rate, nch, frames) in enumerate(specs):
        x = 0.6 * _signal("noise", frames, rate, nch, [8, i]) + 0.5 * _signal("two-tone", frames, rate, nch, [8, i, 1])
        paths.append(str(d / name))
        WRITERS[enc](paths[-1], x if nch > 1 else x[:, 0], rate)
    return d, paths


def _by_hand(holder, eng, scratch, paths, captions, out_dir, channels="each", fade=0):
    """The pipeline from public pieces: raw row -> decode_resample per extracted channel (or of the whole row: mono) ->
    separate_long_list -> Engine.resample -> [:frames] -> the host writer.  Returns the files' bytes."""
    planes, conds, metas = [], [], []
    for p, cap in zip(paths, captions):
        enc, nch, rate, frames, _ = info = wavio.wav_info(p)
        row = np.zeros(frames * nch * rs.SAMPLE_BYTES[enc], dtype=np.uint8)
        assert wavio.read_wav_raw_into(p, info, row)
        if channels == "each":
            chans = np.frombuffer(row.tobytes(), dtype=DTYPES[enc]).reshape(frames, nch)
            mine = [eng.decode_resample(torch.from_numpy(_padded(np.frombuffer(np.ascontiguousarray(chans[:, c]).tobytes(), dtype=np.uint8))).to(DEV),
                                        frames, 1, enc, rate, SR)[0] for c in range(nch)]
        else:
            mine = [eng.decode_resample(torch.from_numpy(_padded(row)).to(DEV), frames, nch, enc, rate, SR)[0]]
        cond = holder.query_encoder.get_query_embed(modality="text", text=[cap], device=DEV)[0]
        planes += mine
        conds += [cond] * len(mine)
        metas.append((enc, rate, frames, len(mine)))
    seps = holder.ss_model.separate_long_list(planes, torch.stack(conds), window=WINDOW, context=CONTEXT, fade=fade)
    files, at = [], 0
    for k, (enc, rate, frames, n) in enumerate(metas):
        y = np.stack([eng.resample(s, SR, rate)[:frames].cpu().numpy() for s in seps[at:at + n]], axis=1)
        at += n
        out = os.path.join(out_dir, f"hand{k}.wav")
        WRITERS[enc](out, y if n > 1 else y[:, 0], rate)
        with open(out, "rb") as f:
            files.append(f.read())
    return files


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("channels,fade", [("each", 0), ("mono", 0), ("each", 400)])
def test_separate_files_equals_the_pieces_by_hand(holder, eng, scratch_wav, files, monkeypatch, channels, fade):
    d, paths = files
    outs = [str(d / f"out_{channels}_{fade}_{k}.wav") for k in range(3)]
    calls = []
    embed = holder.query_encoder.get_query_embed
    with monkeypatch.context() as mp:
        mp.setattr(holder.query_encoder, "get_query_embed", lambda **kw: (calls.append(list(kw["text"])), embed(**kw))[1])
        recs = pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs)), SR, channels=channels, window=WINDOW, context=CONTEXT,
                                       fade=fade)
    assert calls == [["a dog barking", "rain on a roof"]]                  # one call per pass, each distinct caption once
    want = _by_hand(holder, eng, scratch_wav, paths, CAPTIONS, str(d), channels, fade)
    for p, o, rec, w in zip(paths, outs, recs, want):
        enc, nch, rate, frames, _ = wavio.wav_info(p)
        nch_out = nch if channels == "each" else 1
        assert wavio.wav_info(o) == (enc, nch_out, rate, frames, 44)       # the input's header, the channel count aside for mono
        assert {k: rec[k] for k in ("rate", "channels", "frames", "path")} == dict(rate=rate, channels=nch_out, frames=frames, path="device")
        got = _read(o)
        assert got[:44] == w[:44] and got == w, (p, channels, fade)
        x = wavio.read_wav(o)[0]
        assert rec["clipped"] == 0 and float(np.max(np.abs(x))) > 1e-3     # (a real signal came out)


def test_inference_is_the_one_job_call(holder, files):
    d, paths = files
    a, b = str(d / "inf.wav"), str(d / "one.wav")
    rec = pipeline.inference(holder, paths[0], CAPTIONS[0], a, sampling_rate=SR, window=WINDOW, context=CONTEXT)
    one = pipeline.separate_files(holder, [(paths[0], CAPTIONS[0], b)], SR, window=WINDOW, context=CONTEXT)
    assert [rec] == one and _read(a) == _read(b) and len(_read(a)) == 44 + 136710 * 2 * 2
    # an embedding in place of the caption, and other passes (max_samples below one file: each file a pass of its own)
    e = holder.query_encoder.get_query_embed(modality="text", text=[CAPTIONS[0]])[0].numpy()
    c = str(d / "emb.wav")
    pipeline.separate_files(holder, [(paths[1], "rain on a roof", str(d / "x.wav")), (paths[0], e, c)], SR, window=WINDOW,
                            context=CONTEXT, max_samples=1000)
    assert _read(c) == _read(a)


@pytest.mark.filterwarnings("ignore:.*parity with the reference is unpinned.*:UserWarning")
def test_odd_rate_file_takes_the_host_route(holder, eng, files):
    """44 101 Hz <-> 16 000 Hz is over the tap cap both ways: decode and export run on the host, the separation on the device, in
    the same pass as a device-route file."""
    d, paths = files
    odd, frames = str(d / "odd.wav"), 30000
    x = 0.5 * _signal("two-tone", frames, 44101, 2, [8, 9])
    wavio.write_wav_pcm16(odd, x, 44101)
    outs = [str(d / "odd_out.wav"), str(d / "odd_b.wav")]
    recs = pipeline.separate_files(holder, [(odd, "rain on a roof", outs[0]), (paths[1], "a dog barking", outs[1])], SR,
                                   window=WINDOW, context=CONTEXT)
    assert [r["path"] for r in recs] == ["host", "device"]
    assert wavio.wav_info(outs[0]) == ("pcm16", 2, 44101, frames, 44) and recs[0]["frames"] == frames and recs[0]["channels"] == 2
    decoded = np.frombuffer(_read(odd)[44:], dtype="<i2").reshape(frames, 2).astype(np.float32) / 32768.0
    planes = [torch.from_numpy(wavio._resample(decoded[:, c], 44101, SR)).to(DEV) for c in range(2)]
    cond = holder.query_encoder.get_query_embed(modality="text", text=["rain on a roof"], device=DEV)[0]
    seps = holder.ss_model.separate_long_list(planes, torch.stack([cond, cond]), window=WINDOW, context=CONTEXT)
    y = np.stack([wavio._resample(s.cpu().numpy(), SR, 44101)[:frames] for s in seps], axis=1)
    want = np.clip(np.round(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64)
    got = np.frombuffer(_read(outs[0])[44:], dtype="<i2").reshape(frames, 2).astype(np.int64)
    worst = int(np.max(np.abs(got - want)))
    print(f"host route: worst difference to the hand-made host result {worst} LSB")
    assert worst <= 1 and np.max(np.abs(got)) > 30


def test_short_file_is_refused_by_name(holder, files):
    d, _ = files
    p = str(d / "short.wav")
    wavio.write_wav_pcm16(p, np.zeros(1400, dtype=np.float32), 44100)         # 508 samples at 16 kHz <= n_fft/2 = 512
    with pytest.raises(ValueError, match=r"short\.wav.*not longer than the reflect padding"):
        pipeline.separate_files(holder, [(p, "rain", str(d / "never.wav"))], SR)
    assert not os.path.exists(str(d / "never.wav"))


def test_bf16_run_equals_the_pieces_by_hand(synthetic_sd, eng, scratch_wav, files):
    """The first file in bf16: the same separation calls on the same planes as by hand, so the same bytes."""
    d, paths = files
    bf = _make_model(synthetic_sd, "bf16")
    out = str(d / "bf16.wav")
    pipeline.separate_files(bf, [(paths[0], CAPTIONS[0], out)], SR, window=WINDOW, context=CONTEXT)
    want = _by_hand(bf, eng, scratch_wav, paths[:1], CAPTIONS[:1], str(d))[0]
    got = _read(out)
    lsb = np.abs(np.frombuffer(got[44:], dtype="<i2").astype(np.int64) - np.frombuffer(want[44:], dtype="<i2").astype(np.int64))
    print(f"bf16: {np.count_nonzero(lsb)} differing samples, worst {int(lsb.max())} LSB")
    assert got == want
