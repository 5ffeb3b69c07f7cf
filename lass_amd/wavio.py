"""Minimal RIFF/WAVE reader-writer (PCM16, PCM32, float32), mono down-mix.

`wav_info` / `read_wav_raw_into` serve the evaluator's device load path: header parsing and the raw payload only, the decode,
down-mix and resampling being `lass_decode_resample`'s (lass_amd/resample.py has the filter).  `wav_header` serves the way back
out: the 44 bytes in front of a payload the device encoded (`lass_resample_encode`, lass_amd/pipeline.py).


Stands in for `librosa.load(path, sr=16000, mono=True)` (dcase_evaluator.py:73-74) for files that are ALREADY at the
target rate: the load then reduces to PCM decode + mono down-mix + int->float scaling (x/32768 for int16, as
soundfile/librosa do).  Whether the Zenodo validation audio is at 16 kHz is NOT established from the reference (its
scripts/process_audio.sh converts TRAINING data with `sox -r 16000 -c 1`; the validation set's rate is not stated):
`librosa.load` would resample such files (librosa 0.10: `res_type="soxr_hq"`).  librosa / soxr are absent here, so a file at
another rate is resampled by `scipy.signal.resample_poly` (polyphase FIR, Kaiser window) with a one-time warning: the
result is band-limited correctly but is NOT bit-comparable with librosa's - **parity unpinned** at this boundary (SURVEY
8c; the reference holds no fixture for it).  `read_wav(..., strict_rate=True)` (or LASS_WAV_STRICT_RATE=1) raises instead,
for callers that would rather resample offline (`sox -r 16000 -c 1`, as scripts/process_audio.sh does for training data).
"""
from __future__ import annotations

import struct

import numpy as np


_warned_resample = False


def _resample(x: np.ndarray, rate: int, sr: int) -> np.ndarray:
    """Polyphase resampling rate -> sr (parity unpinned against librosa.load's soxr_hq, see the module docstring)."""
    from math import gcd

    from scipy.signal import resample_poly
    g = gcd(int(rate), int(sr))
    return resample_poly(x.astype(np.float64), sr // g, rate // g).astype(np.float32)


def read_wav(path: str, sr: int | None = None, strict_rate: bool | None = None) -> tuple[np.ndarray, int]:
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, raw = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            raw = body
        pos += 8 + size + (size & 1)
    if fmt is None or raw is None:
        raise ValueError(f"{path}: missing fmt/data chunk")
    tag, ch, rate, _, _, bits = fmt
    if tag == 0xFFFE and len(data) > 0:  # WAVE_FORMAT_EXTENSIBLE: sub-format in the extension; infer from bits
        tag = 3 if bits == 32 and b"\x03\x00\x00\x00\x00\x00\x10\x00" in data[:128] else 1
    if tag == 1 and bits == 16:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif tag == 1 and bits == 32:
        x = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif tag == 3 and bits == 32:
        x = np.frombuffer(raw, dtype="<f4").astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported WAV encoding tag={tag} bits={bits}")
    if ch > 1:
        x = x.reshape(-1, ch).mean(axis=1).astype(np.float32)  # librosa mono=True
    if sr is not None and rate != sr:
        import os
        if strict_rate is None:
            strict_rate = os.environ.get("LASS_WAV_STRICT_RATE", "0") not in ("", "0")
        if strict_rate:
            raise ValueError(f"{path}: sample rate {rate} != {sr}; resample offline (e.g. sox -r {sr} -c 1)")
        global _warned_resample
        if not _warned_resample:
            _warned_resample = True
            import warnings
            warnings.warn(f"{path}: {rate} Hz resampled to {sr} Hz with scipy.signal.resample_poly - librosa.load would use "
                          "soxr_hq; parity with the reference is unpinned for resampled files (further files: no message)")
        x, rate = _resample(x, rate, sr), sr
    return np.ascontiguousarray(x), rate


def read_wav_into(path: str, sr: int, out: np.ndarray) -> bool:
    """Fast path of `read_wav` for the evaluator's resident data path: a mono file ALREADY at `sr` whose sample count equals
    `len(out)` is decoded straight into `out` (a float32 row of a pinned staging buffer): float32 data by one `readinto`
    (file -> pinned memory, no intermediate array), PCM16 / PCM32 with read_wav's own scaling.  Anything else - other rate,
    channels, length, exotic header - returns False and leaves the decision to `read_wav`.  Values are bit-identical to
    `read_wav(path, sr)[0]` whenever it returns True."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            return False
        fmt = None
        while True:
            ch = f.read(8)
            if len(ch) < 8:
                return False
            cid, size = ch[:4], struct.unpack("<I", ch[4:])[0]
            if cid == b"fmt ":
                body = f.read(size + (size & 1))
                if size < 16:
                    return False
                fmt = struct.unpack("<HHIIHH", body[:16])
            elif cid == b"data":
                break
            else:
                f.seek(size + (size & 1), 1)
        if fmt is None:
            return False
        tag, nch, rate, _, _, bits = fmt
        n = out.shape[0]
        if nch != 1 or rate != sr or out.dtype != np.float32 or not out.flags.c_contiguous:
            return False
        if tag == 3 and bits == 32:
            if size != 4 * n:
                return False
            return f.readinto(memoryview(out).cast("B")) == size
        if tag == 1 and bits == 16:
            if size != 2 * n:
                return False
            raw = np.frombuffer(f.read(size), dtype="<i2")
            if raw.shape[0] != n:
                return False
            np.divide(raw.astype(np.float32), np.float32(32768.0), out=out)
            return True
        if tag == 1 and bits == 32:
            if size != 4 * n:
                return False
            raw = np.frombuffer(f.read(size), dtype="<i4")
            if raw.shape[0] != n:
                return False
            out[:] = (raw.astype(np.float64) / 2147483648.0).astype(np.float32)
            return True
    return False


_EXT_PCM, _EXT_FLOAT = b"\x01\x00", b"\x03\x00"
_EXT_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"  # KSDATAFORMAT_SUBTYPE_*: the tag + this


def _parse_header(f):
    """(encoding, channels, rate, frames, data_offset) from an open file positioned at 0, or None."""
    import os
    head = f.read(12)
    if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        return None
    fmt = None
    while True:
        ch = f.read(8)
        if len(ch) < 8:
            return None
        cid, size = ch[:4], struct.unpack("<I", ch[4:])[0]
        if cid == b"fmt ":
            body = f.read(size + (size & 1))
            if size < 16 or len(body) < size:
                return None
            tag, nch, rate, _, block, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE:  # WAVE_FORMAT_EXTENSIBLE: the encoding is the sub-format GUID's first two bytes
                if size < 40 or body[26:40] != _EXT_TAIL:
                    return None
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = (tag, nch, rate, block, bits)
        elif cid == b"data":
            break
        else:
            f.seek(size + (size & 1), 1)
    if fmt is None:
        return None
    tag, nch, rate, block, bits = fmt
    enc = {(1, 16): "pcm16", (1, 32): "pcm32", (3, 32): "f32"}.get((tag, bits))
    offset = f.tell()
    if (enc is None or nch < 1 or rate < 1 or block != nch * bits // 8 or size % block != 0 or size == 0
            or os.fstat(f.fileno()).st_size < offset + size):
        return None
    return enc, nch, rate, size // block, offset


def wav_info(path: str):
    """(encoding, channels, rate, frames, data_offset) of a RIFF/WAVE file from its header alone - encoding "pcm16", "pcm32" or
    "f32", data_offset the first payload byte - or None for any header this module does not fully understand: not RIFF/WAVE,
    truncated, a `fmt ` chunk under 16 bytes, another encoding, a block size that is not channels x sample size, a data
    chunk that is empty, not whole frames, or longer than the file."""
    try:
        with open(path, "rb") as f:
            return _parse_header(f)
    except (OSError, struct.error):
        return None


def read_wav_raw_into(path: str, info, out_u8: np.ndarray) -> bool:
    """The file's data chunk, undecoded, into `out_u8` (a uint8 row of a pinned staging buffer, at least as long as the chunk) in
    one `readinto`; decoding, down-mix and resampling are the device's (`Engine.decode_resample`).  True only if the file's
    encoding, channels, rate and frame count equal `info`'s (a `wav_info` tuple; its data_offset is the file's own) and
    every byte arrived."""
    try:
        with open(path, "rb") as f:
            mine = _parse_header(f)
            if mine is None or tuple(mine[:4]) != tuple(info[:4]):
                return False
            nbytes = mine[3] * mine[1] * (2 if mine[0] == "pcm16" else 4)
            if out_u8.dtype != np.uint8 or out_u8.ndim != 1 or not out_u8.flags.c_contiguous or out_u8.shape[0] < nbytes:
                return False
            return f.readinto(memoryview(out_u8)[:nbytes]) == nbytes
    except (OSError, struct.error):
        return False


def wav_frames(path: str) -> int:
    """Sample frames of a RIFF/WAVE file from its header alone (0 if the header is not understood)."""
    try:
        with open(path, "rb") as f:
            head = f.read(12)
            if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
                return 0
            block = 0
            while True:
                ch = f.read(8)
                if len(ch) < 8:
                    return 0
                cid, size = ch[:4], struct.unpack("<I", ch[4:])[0]
                if cid == b"fmt ":
                    body = f.read(size + (size & 1))
                    block = struct.unpack("<HHIIHH", body[:16])[4]
                elif cid == b"data":
                    return size // block if block else 0
                else:
                    f.seek(size + (size & 1), 1)
    except OSError:
        return 0


def _frames_channels(x: np.ndarray):
    """1-D = mono; 2-D = (frames, channels), written interleaved."""
    if x.ndim == 1:
        return 1
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("a (frames,) or (frames, channels) array expected")
    return x.shape[1]


_WAV_FORMATS = {"pcm16": (1, 2), "pcm32": (1, 4), "f32": (3, 4)}  # encoding -> (format tag, bytes per sample)


def wav_header(encoding: str, channels: int, rate: int, frames: int) -> bytes:
    """The 44-byte RIFF/WAVE header (`fmt ` chunk of 16 bytes, then `data`) in front of `frames` interleaved frames of
    `channels` samples, encoding "pcm16", "pcm32" or "f32": what the three writers below put in front of their payload, for
    callers that hold the payload already (lass_amd.pipeline writes the device's `Engine.resample_encode` rows behind it)."""
    if encoding not in _WAV_FORMATS:
        raise ValueError(f"encoding must be one of {sorted(_WAV_FORMATS)}")
    tag, size = _WAV_FORMATS[encoding]
    channels, rate, frames = int(channels), int(rate), int(frames)
    nbytes = frames * channels * size
    if channels < 1 or rate < 1 or frames < 0 or 36 + nbytes >= 2 ** 32:
        raise ValueError("channels and rate must be positive and the payload must stay below 4 GiB")
    return b"RIFF" + struct.pack("<I", 36 + nbytes) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, tag, channels, rate, rate * size * channels, size * channels, 8 * size) + b"data" + struct.pack("<I", nbytes)


def _write(path: str, encoding: str, q: np.ndarray, sr: int) -> None:
    nch = _frames_channels(q)
    with open(path, "wb") as f:
        f.write(wav_header(encoding, nch, sr, q.shape[0]) + q.tobytes())


def write_wav_f32(path: str, x: np.ndarray, sr: int) -> None:
    _write(path, "f32", np.ascontiguousarray(x, dtype="<f4"), sr)


def write_wav_pcm16(path: str, x: np.ndarray, sr: int) -> None:
    _write(path, "pcm16", np.ascontiguousarray(np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")), sr)


def write_wav_pcm32(path: str, x: np.ndarray, sr: int) -> None:
    _write(path, "pcm32", np.ascontiguousarray(np.clip(np.round(np.asarray(x, dtype=np.float64) * 2147483648.0), -2147483648, 2147483647).astype("<i4")), sr)
