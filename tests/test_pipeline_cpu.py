"""Host side of the file pipeline (lass_amd/pipeline.py) and of the export kernel's contract: the WAV header, the two PCM
quantisation rules the device applies in float32 against the host writers' float64 ones, the length algebra that lets a file
come back at its own frame count, job planning, and the two new C-ABI symbols.  No GPU."""
import os
import struct

import numpy as np
import pytest

from lass_amd import pipeline, wavio
from lass_amd import resample as rs

WRITERS = {"pcm16": wavio.write_wav_pcm16, "pcm32": wavio.write_wav_pcm32, "f32": wavio.write_wav_f32}
RATE_PAIRS = [(16000, 44100), (16000, 48000), (32000, 48000), (32000, 44100), (16000, 11025), (32000, 16000), (8000, 16000),
              (16000, 16000)]


def quantise_f32(y: np.ndarray, encoding: str):
    """lass_resample_encode's PCM rules restated in numpy, every step in float32: (samples, how many the clip changed)."""
    y = np.asarray(y, dtype=np.float32)
    scale, lo, hi, dt = (np.float32(32768.0), -32768, 32767, "<i2") if encoding == "pcm16" else (np.float32(2147483648.0), -2147483648,
                                                                                             2147483647, "<i4")
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(y * scale)                      # float32 product (exact: a power of two), ties to even
    assert r.dtype == np.float32
    nan = np.isnan(r)
    r = np.where(nan, np.float32(0), r)
    over, under = r > np.float32(hi), r < np.float32(lo)     # float32(2^31 - 1) == 2^31: r >= 2^31 there, as the kernel tests
    if encoding == "pcm32":
        over = r >= np.float32(2147483648.0)
    q = np.where(over, hi, np.where(under, lo, r.astype(np.float64))).astype(np.int64)
    return q.astype(dt), int(np.count_nonzero(over | under))


def edge_values() -> np.ndarray:
    """Every kind of float32 the quantisers can meet: ties k + 0.5 of both scales, +-1, just inside and outside, huge, denormal."""
    k = np.arange(-40, 40, dtype=np.float64)
    ties16 = (k + 0.5) / 32768.0
    far16 = (np.array([32766.5, 32767.5, -32767.5, -32768.5, 32767.49, -32768.51])) / 32768.0
    ties32 = (np.arange(-20, 20, dtype=np.float64) * 2.0 + 1.0) * 2.0 ** -32     # (k + 0.5) / 2^31: float32 holds them near 0
    rng = np.random.Generator(np.random.PCG64(16))
    v = np.concatenate([ties16, far16, ties32, [1.0, -1.0, 1.5, -1.5, 0.99999994, -0.99999994, 1.0000001, -1.0000001, 3e38, -3e38,
                                                1e-40, -1e-40, 1.4e-45, 0.0, -0.0, 2.0 ** -31, -2.0 ** -31, 0.5, 2147483520.0 / 2.0 ** 31],
                        rng.uniform(-1.2, 1.2, 3000), rng.standard_normal(3000) * 1e-4])
    return v.astype(np.float32)


def _payload(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()[44:]


# ---- header -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("enc", ["pcm16", "pcm32", "f32"])
def test_wav_header_is_the_writers(tmp_path, enc, nch):
    """wav_header equals the first 44 bytes of the writer's file, and the file equals bytes computed here (the writers now call
    wav_header: this holds them to what they wrote before)."""
    frames, rate = 37, 44100
    x = np.random.Generator(np.random.PCG64([3, nch])).uniform(-1.3, 1.3, (frames, nch)).astype(np.float32)
    p = str(tmp_path / "a.wav")
    WRITERS[enc](p, x if nch > 1 else x[:, 0], rate)
    with open(p, "rb") as f:
        data = f.read()
    assert wavio.wav_header(enc, nch, rate, frames) == data[:44]
    if enc == "f32":
        body, tag, size = x.astype("<f4").tobytes(), 3, 4
    elif enc == "pcm16":
        body, tag, size = np.clip(np.round(x.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes(), 1, 2
    else:
        body, tag, size = np.clip(np.round(x.astype(np.float64) * 2147483648.0), -2147483648, 2147483647).astype("<i4").tobytes(), 1, 4
    want = (b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, tag, nch, rate, rate * size * nch,
                                                                                   size * nch, 8 * size)
            + b"data" + struct.pack("<I", len(body)) + body)
    assert data == want
    assert wavio.wav_info(p) == (enc, nch, rate, frames, 44)


def test_wav_header_refuses_nonsense():
    for bad in (dict(encoding="pcm24"), dict(channels=0), dict(rate=0), dict(frames=-1), dict(frames=2 ** 31, channels=2)):
        with pytest.raises(ValueError):
            wavio.wav_header(**dict(dict(encoding="pcm16", channels=1, rate=16000, frames=10), **bad))


# ---- quantisation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["pcm16", "pcm32"])
def test_float32_quantisation_equals_the_writers(tmp_path, enc):
    """The device's float32 rule and the writers' float64 rule give the same samples for every finite float32 tried, and the same
    clip count; a NaN encodes as 0 and is not counted."""
    v = edge_values()
    p = str(tmp_path / "q.wav")
    WRITERS[enc](p, v, 16000)
    want = np.frombuffer(_payload(p), dtype="<i2" if enc == "pcm16" else "<i4")
    got, clips = quantise_f32(v, enc)
    assert np.array_equal(got, want)
    assert clips == pipeline.host_clip_count(v, enc) and clips >= 4
    q, n = quantise_f32(np.array([np.nan, 0.25], dtype=np.float32), enc)
    assert q[0] == 0 and n == 0 and pipeline.host_clip_count(np.array([np.nan]), enc) == 0


# ---- length algebra -----------------------------------------------------------------------------------------------------
def test_original_frame_count_is_always_reachable():
    """A file of F frames at rate r decodes to L = ceil(F * u / d) model-rate samples; coming back, the ceiling ceil(L * d / u)
    is never below F, so frames_out = F is always allowed."""
    for model_rate, file_rate in RATE_PAIRS + [(16000, 22050), (32000, 8000), (16000, 96000)]:
        up, down = rs.ratio(file_rate, model_rate)
        back = rs.ratio(model_rate, file_rate)
        assert back == (down, up)
        for F in list(range(1, 2000)) + [4099, 44100, 136710, 2 ** 24 + 1, 320 * 44100 + 7]:
            L = rs.out_len(F, up, down)
            assert rs.out_len(L, *back) >= F, (model_rate, file_rate, F)


# ---- planning -----------------------------------------------------------------------------------------------------------
def test_passes_respect_max_samples():
    rng = np.random.Generator(np.random.PCG64(9))
    sizes = [int(s) for s in rng.integers(1, 1000, 200)] + [5000, 1, 1]
    for bound in (1, 999, 1000, 2500, 10 ** 6):
        passes = pipeline.plan_passes(sizes, bound)
        assert [i for p in passes for i in p] == list(range(len(sizes)))
        for p in passes:
            assert sum(sizes[i] for i in p) <= bound or len(p) == 1
        for a, b in zip(passes, passes[1:]):   # greedy: the next job would not have fitted
            assert sum(sizes[i] for i in a) + sizes[b[0]] > bound
    assert pipeline.plan_passes([], 10) == []
    with pytest.raises(ValueError):
        pipeline.plan_passes([1], 0)
    assert pipeline.model_samples(2, 44100, 44100, 16000, "each") == (2, 16000)
    assert pipeline.model_samples(2, 44100, 44101, 16000, "mono") == (1, 16001)


def test_captions_are_deduplicated():
    e = np.zeros(512, dtype=np.float32)
    captions, index = pipeline.dedup_captions(["a dog", "rain", "a dog", e, "rain", "wind"])
    assert captions == ["a dog", "rain", "wind"] and index == [0, 1, 0, None, 1, 2]
    assert pipeline.dedup_captions([e]) == ([], [None])


def test_route_decision(tmp_path):
    x = np.zeros((100, 2), dtype=np.float32)
    ok, odd, wide, cut = (str(tmp_path / n) for n in ("ok.wav", "odd.wav", "wide.wav", "cut.wav"))
    wavio.write_wav_pcm16(ok, x, 44100)
    wavio.write_wav_pcm16(odd, x, 44101)
    wavio.write_wav_f32(wide, np.zeros((100, 9), dtype=np.float32), 16000)
    with open(ok, "rb") as f:
        whole = f.read()
    with open(cut, "wb") as f:
        f.write(whole[:40])                          # the header stops inside the data chunk's own header
    assert pipeline.route(wavio.wav_info(ok), 16000) == "device"
    assert pipeline.route(wavio.wav_info(ok), 32000) == "device"
    assert wavio.wav_info(odd) is not None and pipeline.route(wavio.wav_info(odd), 16000) == "host"      # 882 021 taps
    assert wavio.wav_info(wide)[1] == 9 and pipeline.route(wavio.wav_info(wide), 16000) == "host"
    assert wavio.wav_info(cut) is None and pipeline.route(wavio.wav_info(cut), 16000) == "host"
    # the way back counts too: a file the decoder takes, written at a rate the encoder does not
    assert pipeline.route(wavio.wav_info(ok), 16000, out_rate=44101) == "host"
    assert pipeline.route(wavio.wav_info(ok), 16000, out_rate=48000) == "device"
    with open(cut, "wb") as f:
        f.write(whole[:-2])                          # a data chunk longer than the file
    assert wavio.wav_info(cut) is None and pipeline.route(wavio.wav_info(cut), 16000) == "host"


def test_host_decode_keeps_channels(tmp_path):
    """The host route's per-channel decode is read_wav's rule per channel: equal to read_wav of a mono file of that channel."""
    x = np.random.Generator(np.random.PCG64(4)).uniform(-1, 1, (50, 9)).astype(np.float32)
    for enc, w in WRITERS.items():
        p, m = str(tmp_path / "nine.wav"), str(tmp_path / "one.wav")
        w(p, x, 22050)
        got = pipeline._host_decode(p, wavio.wav_info(p), "each")
        assert got.shape == (9, 50) and got.dtype == np.float32
        for c in (0, 8):
            w(m, x[:, c], 22050)
            assert np.array_equal(got[c], wavio.read_wav(m)[0])
        assert np.array_equal(pipeline._host_decode(p, wavio.wav_info(p), "mono")[0], wavio.read_wav(p)[0])


# ---- C-ABI --------------------------------------------------------------------------------------------------------------
def test_new_symbols_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from lass_amd import _lib
    lib = _lib.load()
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    assert len(bound["lass_decode_resample_planar"]) == len(bound["lass_decode_resample"]) == 14
    assert len(bound["lass_resample_encode"]) == 17
    for name in ("lass_decode_resample_planar", "lass_resample_encode"):
        assert hasattr(lib, name), name
    assert "export.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "export.hip"))
