"""Device load path, host side (no GPU): the C-ABI symbol, the numpy filter design and host resampler against scipy, the WAV
header reader / raw reader / multi-channel writers, and the evaluator's `device_decode` keyword."""
import os
import re
import struct

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RATE_TABLE = [(32000, 16000), (48000, 16000), (44100, 16000), (22050, 16000), (24000, 16000), (8000, 16000), (11025, 16000),
              (44100, 32000)]


def test_symbol_in_header_and_bindings():
    from lass_amd import _lib, resample
    hdr = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    assert re.search(r"\bint lass_decode_resample\s*\(", hdr)
    args = [a for n, _, a in _lib.SYMBOLS if n == "lass_decode_resample"]
    assert len(args) == 1 and len(args[0]) == 14
    assert "resample.hip" in __import__("__graft_entry__").SOURCES
    # the Python layer's copies of the header's constants
    defs = dict(re.findall(r"#define (LASS_(?:WAV|RESAMPLE)_[A-Z0-9_]+) (\d+)", hdr))
    assert int(defs["LASS_RESAMPLE_MAX_TAPS"]) == resample.MAX_TAPS
    assert {k: int(defs["LASS_WAV_" + k.upper()]) for k in resample.ENCODINGS} == resample.ENCODINGS


@pytest.mark.parametrize("rate_in,rate_out", RATE_TABLE)
def test_design_taps_equals_scipy_firwin(rate_in, rate_out):
    from scipy.signal import firwin
    from lass_amd import resample
    up, down = resample.ratio(rate_in, rate_out)
    h = resample.design_taps(up, down)
    ref = firwin(20 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert h.dtype == np.float64 and h.shape == ref.shape == (resample.n_taps(up, down),)
    assert np.max(np.abs(h - ref)) <= 1e-15
    assert resample.within_cap(up, down)   # every pair of the table runs on the device


@pytest.mark.parametrize("rate_in,rate_out", RATE_TABLE)
def test_resample_host_equals_scipy_resample_poly(rate_in, rate_out):
    from scipy.signal import resample_poly
    from lass_amd import resample
    up, down = resample.ratio(rate_in, rate_out)
    nt = resample.n_taps(up, down)
    rng = np.random.Generator(np.random.PCG64([rate_in, rate_out]))
    lengths = [1, 37, max(2, nt // (2 * up)), 3 * down + 1, 5003]   # 1; shorter than the filter; not multiples of `down`
    assert lengths[2] * up < nt and all(down == 1 or n % down for n in lengths[3:])
    for n in lengths:
        x = rng.standard_normal(n)
        y = resample.resample_host(x, up, down)
        ref = resample_poly(x, up, down)
        assert y.dtype == np.float64 and y.shape == ref.shape == (-(-n * up // down),), (n, y.shape, ref.shape)
        assert y.shape[0] == resample.out_len(n, up, down)
        assert np.max(np.abs(y - ref)) <= 1e-14, (n, np.max(np.abs(y - ref)))
    y32 = resample.resample_host(x.astype(np.float32), up, down, dtype=np.float32)
    assert y32.dtype == np.float32 and np.max(np.abs(y32 - ref)) < 5e-6


def test_ratio_and_cap():
    from lass_amd import resample
    assert resample.ratio(44100, 16000) == (160, 441) and resample.ratio(16000, 16000) == (1, 1)
    assert resample.n_taps(160, 441) == 8821 and resample.n_taps(640, 441) == 12801
    assert resample.within_cap(1, 819) and not resample.within_cap(1, 820)       # 16 381 / 16 401 taps
    assert not resample.within_cap(*resample.ratio(44101, 16000))
    x = np.arange(5.0)
    assert np.array_equal(resample.resample_host(x, 3, 3), x)


def _write_raw(path, tag, nch, rate, bits, payload, fmt_size=16, extensible_sub=None, riff=b"RIFF", extra_chunk=True):
    block = nch * bits // 8
    fmt = struct.pack("<HHIIHH", tag, nch, rate, rate * block, block, bits)
    if extensible_sub is not None:
        fmt += struct.pack("<HHI", 22, bits, 3) + struct.pack("<H", extensible_sub) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    fmt = fmt[:fmt_size] if fmt_size < 16 else fmt
    body = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if extra_chunk:
        body += b"LIST" + struct.pack("<I", 3) + b"abc\x00"   # an odd-sized chunk in front of the data (padded to even)
    body += b"data" + struct.pack("<I", len(payload)) + payload
    with open(path, "wb") as f:
        f.write(riff + struct.pack("<I", 4 + len(body)) + b"WAVE" + body)


def test_wav_info(tmp_path):
    from lass_amd import wavio
    p = str(tmp_path / "a.wav")
    x = (np.random.default_rng(3).standard_normal((50, 2)) * 0.2).astype(np.float32)
    wavio.write_wav_pcm16(p, x[:, 0], 32000)
    assert wavio.wav_info(p) == ("pcm16", 1, 32000, 50, 44)
    wavio.write_wav_pcm16(p, x, 32000)
    assert wavio.wav_info(p) == ("pcm16", 2, 32000, 50, 44)
    wavio.write_wav_pcm32(p, x, 48000)
    assert wavio.wav_info(p) == ("pcm32", 2, 48000, 50, 44)
    wavio.write_wav_pcm32(p, x[:, 1], 48000)
    assert wavio.wav_info(p) == ("pcm32", 1, 48000, 50, 44)
    wavio.write_wav_f32(p, x[:, 0], 16000)
    assert wavio.wav_info(p) == ("f32", 1, 16000, 50, 44)
    wavio.write_wav_f32(p, x, 44100)
    assert wavio.wav_info(p) == ("f32", 2, 44100, 50, 44)
    # multi-channel files read back as the mean over channels, sample for sample
    y, sr = wavio.read_wav(p, 44100)
    assert sr == 44100 and np.array_equal(y, x.mean(axis=1).astype(np.float32))
    # a chunk in front of the data moves the offset; WAVE_FORMAT_EXTENSIBLE names its encoding in the sub-format
    _write_raw(p, 3, 2, 44100, 32, x.tobytes())
    assert wavio.wav_info(p) == ("f32", 2, 44100, 50, 56)
    _write_raw(p, 0xFFFE, 2, 44100, 32, x.tobytes(), extensible_sub=3)
    assert wavio.wav_info(p) == ("f32", 2, 44100, 50, 80)
    _write_raw(p, 0xFFFE, 2, 44100, 32, x.tobytes(), extensible_sub=1)
    assert wavio.wav_info(p)[0] == "pcm32"
    # what it does not fully understand is None, never an exception
    good = open(p, "rb").read()
    for cut in (0, 3, 11, 12, 19, 20, 30, 47, len(good) - 1):           # truncated header / truncated data
        open(p, "wb").write(good[:cut])
        assert wavio.wav_info(p) is None, cut
    _write_raw(p, 1, 1, 16000, 16, b"\x00" * 20, fmt_size=14)            # a 14-byte fmt chunk
    assert wavio.wav_info(p) is None
    _write_raw(p, 1, 1, 16000, 8, b"\x00" * 20)                          # 8-bit PCM
    assert wavio.wav_info(p) is None
    _write_raw(p, 1, 1, 16000, 24, b"\x00" * 21)                         # 24-bit PCM
    assert wavio.wav_info(p) is None
    _write_raw(p, 1, 2, 16000, 16, b"\x00" * 22)                         # not whole frames
    assert wavio.wav_info(p) is None
    _write_raw(p, 1, 1, 16000, 16, b"")                                  # no samples
    assert wavio.wav_info(p) is None
    _write_raw(p, 1, 1, 16000, 16, b"\x00" * 20, riff=b"RIFX")
    assert wavio.wav_info(p) is None
    assert wavio.wav_info(str(tmp_path / "missing.wav")) is None


def test_read_wav_raw_into(tmp_path):
    from lass_amd import wavio
    p, q = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    x = (np.random.default_rng(4).standard_normal((33, 2)) * 0.2).astype(np.float32)
    wavio.write_wav_pcm16(p, x, 32000)
    info = wavio.wav_info(p)
    row = np.full(33 * 2 * 2 + 4, 0xAB, dtype=np.uint8)
    assert wavio.read_wav_raw_into(p, info, row)
    assert row[:132].tobytes() == open(p, "rb").read()[44:] and np.all(row[132:] == 0xAB)
    # the same payload behind another chunk: the offset is the file's own
    _write_raw(q, 1, 2, 32000, 16, open(p, "rb").read()[44:])
    row2 = np.zeros(132, dtype=np.uint8)
    assert wavio.read_wav_raw_into(q, info, row2) and np.array_equal(row2, row[:132])
    # another encoding, channel count, rate or length; a row that is too short or not bytes; a truncated file
    for write, arr, rate in ((wavio.write_wav_f32, x, 32000), (wavio.write_wav_pcm16, x[:, 0], 32000),
                             (wavio.write_wav_pcm16, x, 16000), (wavio.write_wav_pcm16, x[:32], 32000),
                             (wavio.write_wav_pcm16, np.concatenate([x, x[:1]]), 32000)):
        write(q, arr, rate)
        keep = row.copy()
        assert not wavio.read_wav_raw_into(q, info, row)
        assert np.array_equal(row, keep)
    assert not wavio.read_wav_raw_into(p, info, np.zeros(131, dtype=np.uint8))
    assert not wavio.read_wav_raw_into(p, info, np.zeros(132, dtype=np.int8))
    open(q, "wb").write(open(p, "rb").read()[:-2])
    assert not wavio.read_wav_raw_into(q, info, row)
    assert not wavio.read_wav_raw_into(str(tmp_path / "missing.wav"), info, row)


def test_writers_1d_bytes_unchanged(tmp_path, golden_dir):
    """Mono input writes the bytes it wrote before the writers took (frames, channels) arrays: the expectation was recorded
    with the earlier writers."""
    from lass_amd import wavio
    g = np.load(os.path.join(golden_dir, "wavio_writers_1d.npz"))
    p = str(tmp_path / "a.wav")
    wavio.write_wav_f32(p, g["x"], 22050)
    assert open(p, "rb").read() == g["f32_at_22050"].tobytes()
    wavio.write_wav_pcm16(p, g["x"], 44100)
    assert open(p, "rb").read() == g["pcm16_at_44100"].tobytes()
    # (frames, 1) is the same file; (frames, 2) interleaves
    wavio.write_wav_pcm16(p, g["x"][:, None], 44100)
    assert open(p, "rb").read() == g["pcm16_at_44100"].tobytes()
    wavio.write_wav_f32(p, np.stack([g["x"], -g["x"]], axis=1), 22050)
    raw = open(p, "rb").read()
    assert struct.unpack("<HHIIHH", raw[20:36]) == (3, 2, 22050, 22050 * 8, 8, 32)
    assert np.array_equal(np.frombuffer(raw[44:], dtype="<f4").reshape(-1, 2)[:, 1], -g["x"])
    with pytest.raises(ValueError):
        wavio.write_wav_f32(p, np.zeros((2, 2, 2), dtype=np.float32), 16000)


def test_write_validation_set_formats(tmp_path):
    from lass_amd import synthetic, wavio
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    synthetic.write_validation_set(a, n_clips=2, length=1600)
    s, n, _ = synthetic.make_clip(1, 1600)
    assert wavio.wav_info(os.path.join(a, "lass_validation", "src_0001.wav")) == ("f32", 1, 16000, 1600, 44)
    assert np.array_equal(wavio.read_wav(os.path.join(a, "lass_validation", "noise_0001.wav"), 16000)[0], n)
    csv_b = synthetic.write_validation_set(b, n_clips=2, length=1600, file_rate=32000, channels=2, encoding="pcm16")
    assert open(csv_b).read() == open(os.path.join(a, "lass_synthetic_validation.csv")).read()
    assert wavio.wav_info(os.path.join(b, "lass_validation", "src_0001.wav")) == ("pcm16", 2, 32000, 3200, 44)


def test_evaluator_device_decode_keyword(tmp_path):
    """The keyword exists, defaults to off, and changes nothing about where the evaluator computes: without a GPU a call still
    fails loudly."""
    import inspect
    from lass_amd import synthetic
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.evaluator import DCASEEvaluator
    from lass_amd.resunet import ResUNet30
    assert inspect.signature(DCASEEvaluator.__init__).parameters["device_decode"].default is False
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=2, length=1600, file_rate=32000, channels=2,
                                              encoding="pcm16")
    adir = os.path.join(str(tmp_path), "lass_validation")
    assert DCASEEvaluator(16000, csv_path, adir).device_decode is False
    ev = DCASEEvaluator(16000, csv_path, adir, batch_size=2, device_decode=True)
    assert ev.device_decode is True and ev._slots == {}
    if not torch.cuda.is_available():
        pl_model = AudioSep(ss_model=ResUNet30(1, 1, 512), query_encoder=PrecomputedQueryEncoder())
        with pytest.raises(RuntimeError) as off:   # (LassError is one; which layer refuses first is not this test's business)
            DCASEEvaluator(16000, csv_path, adir, batch_size=2)(pl_model)
        with pytest.raises(RuntimeError) as on:
            ev(pl_model)
        assert type(on.value) is type(off.value) and ev._slots == {}
