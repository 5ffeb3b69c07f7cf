"""File in, file out: separate WAV files by caption and write WAV files, with everything between the two file accesses on the
device.

Neither `separate_files` nor `inference` exists in the reference in this form: upstream AudioSep's `pipeline.inference(model,
audio_file, text, output_file)` loads one file with librosa at 32 kHz mono, runs one forward (or `chunk_inference`) and writes
int16 with scipy.  What the two functions below do - channel by channel, at the file's own rate, encoding and frame count, many
files per pass, hard or cross-faded seams - is THIS PACKAGE'S SPECIFICATION, pinned by tests/test_export_gpu.py against a
composition of the package's public pieces, not by a reference fixture (as DESIGN.md sections 14 and 15 say of the long-form
calls).

One pass over a group of files:

    WAV bytes -> pinned row -> H2D -> Engine.decode_resample_planar (or decode_resample for channels="mono")
              -> every plane one recording of ResUNet30.separate_long_list, with its file's condition
                 (channels="linked": every FILE one recording of separate_long_list_linked, guided by its mono down-mix)
              -> Engine.resample_encode back to the file's rate, encoding and frame count -> D2H into a pinned row
              -> wavio.wav_header + payload written

Files are read on one thread and written on another while the device works.  Only the encoded payload leaves the device.

With a level asked for (`loudness=` in LUFS, `peak_ceiling_db=` in dBFS) three more launches stand between the separation and
the encoder, per file: `Engine.loudness` over all of the file's planes at the model rate (a gain commutes with the linear
resampler, so no file-rate float plane is made), `Engine.resample_peak` of the samples the encoder is about to quantise, and
`Engine.loudness_gain`, whose one gain per file - the channel balance is kept - stays on the device and goes into
`Engine.resample_encode(gain=)`.  Loudness, gain and the limited flag travel to the host behind the payload, with the clip
counter, in the layout `Tail` alone knows.  Without a level none of this runs: the pass is the one above.

For an EBU R 128 delivery (-23 LUFS, -1 dBTP) `peak="true"` puts `Engine.resample_true_peak` - the peak of the signal between
the samples the encoder is about to quantise - where `Engine.resample_peak` stood, and `meter=True` puts `Engine.loudness_stats`
where `Engine.loudness` stood: loudness range, maximum momentary and maximum short-term loudness travel to the host with the
rest.  At their defaults neither launches anything and no record gains a key.

One gain per file misses its loudness target by the whole overshoot whenever the ceiling binds, which a separated sound event - a
high crest factor - makes the usual case.  `limiter=True` puts `Engine.limit` in front of the level stage: the separated planes
are measured, brought to the target by a gain without a ceiling and limited to the ceiling by a look-ahead gain curve, one per
file, at the model rate, `limiter_passes` times with the gain corrected by the loudness the limited planes measure between the
passes - a fixed count, all on the device.  The limited planes then go through the level stage above unchanged, which still
guarantees the ceiling on what is written; its gain is now a static trim - thousandths of a dB where the limiter takes a few dB
off rare peaks, tenths where it takes 25 dB off most of the file.  DESIGN.md section 20.

With `target_gain_db=` the file written is a REMIX: the original with the target's level changed by that many dB (-inf takes the
target out, -12 ducks it, +6 brings it up), v = original + k * target with k = 10^(dB/20) - 1, formed at the file's own rate
from the original's own samples.  The device copy of a file's raw row is kept until that file's encode, which is
`Engine.remix_encode` with the row as its dry source in the place of `Engine.resample_encode`: one more read stream in the
same launch.  Only the estimate is band-limited to the model's rate; what the model did not touch keeps its full band, and at
0 dB the file comes back as it went in.  A job of four, (in, query, out, remix_out), writes both the target and the remix from
one separation.  DESIGN.md section 21.

A file the device kernels do not take - a header `wavio.wav_info` does not fully understand, more than 8 channels, a rate pair
beyond `resample.within_cap` in either direction - is decoded, resampled and written on the host (`wavio._resample`,
`wavio.write_wav_*`); its separation still runs on the device, in the same pass, and its record says `path == "host"`.

What the arguments and a file's header decide is decided before the first pass, host only: `Options` for the call and one
`FilePlan` per job (`plan_files`).  A pass reads them and calls one function per stage of a file: `_device_level`,
`_device_remix_level`, `_send` and `_collect`, `host_target` and `host_remix` on the host route.  DESIGN.md section 22.
"""
from __future__ import annotations

import threading
import time
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import loudness as ld
from . import resample as rs
from . import wavio

MAX_CHANNELS = 8                     # include/lass_hip.h: lass_decode_resample, lass_resample_encode
DEFAULT_MAX_SAMPLES = 1 << 26        # model-rate samples per pass, all planes counted: 256 MiB per float32 buffer of the pass
_WRITERS = {"pcm16": wavio.write_wav_pcm16, "pcm32": wavio.write_wav_pcm32, "f32": wavio.write_wav_f32}


# ---- planning (host only) ---------------------------------------------------------------------------------------------------
def route(info, sampling_rate: int, out_rate: Optional[int] = None, true_peak: bool = False) -> str:
    """"device" if the two device kernels take the file - `info` a `wavio.wav_info` tuple, at most 8 channels, and both rate
    pairs (file -> model, model -> output) within the kernels' tap cap - else "host".  true_peak: a true peak is asked for, and
    the output pair must also be one `Engine.resample_true_peak` takes (`resample.true_peak_fits`)."""
    if info is None:
        return "host"
    _, nch, rate, _, _ = info
    if nch > MAX_CHANNELS:
        return "host"
    out_rate = rate if out_rate is None else int(out_rate)
    if not rs.within_cap(*rs.ratio(rate, sampling_rate)) or not rs.within_cap(*rs.ratio(sampling_rate, out_rate)):
        return "host"
    if true_peak and not rs.true_peak_fits(*rs.ratio(sampling_rate, out_rate), ld.oversampling(out_rate)):
        return "host"
    return "device"


def model_samples(nch: int, rate: int, frames: int, sampling_rate: int, channels: str) -> Tuple[int, int]:
    """(planes, model-rate samples per plane) a file puts into a pass: its channels ("each", "linked") or 1 ("mono"),
    ceil(frames * up / down)."""
    return (1 if channels == "mono" else nch), rs.out_len(frames, *rs.ratio(rate, sampling_rate))


def pass_rows(n_planes: int, channels: str) -> int:
    """The model-rate rows a file of `n_planes` planes holds in a pass: its planes, and under "linked" its guide as well."""
    return n_planes + 1 if channels == "linked" else n_planes


def group_by_planes(counts: Sequence[int]) -> List[List[int]]:
    """The positions of `counts` grouped by value, groups in the order of their first member and positions ascending inside a
    group: the files of a pass by channel count, one `ResUNet30.separate_long_list_linked` call per group."""
    groups: Dict[int, List[int]] = {}
    for k, n in enumerate(counts):
        groups.setdefault(int(n), []).append(k)
    return list(groups.values())


def plan_passes(samples: Sequence[int], max_samples: int) -> List[List[int]]:
    """Consecutive jobs grouped into passes of at most `max_samples` model-rate samples; a job over the bound on its own is a
    pass of its own.  Every job is in exactly one pass, in input order."""
    max_samples = int(max_samples)
    if max_samples < 1:
        raise ValueError("max_samples must be at least 1")
    passes, cur, held = [], [], 0
    for i, n in enumerate(samples):
        if cur and held + n > max_samples:
            passes.append(cur)
            cur, held = [], 0
        cur.append(i)
        held += int(n)
    if cur:
        passes.append(cur)
    return passes


def dedup_captions(queries) -> Tuple[List[str], List[Optional[int]]]:
    """(the distinct captions in first-seen order, per query its index into them - None for a query that is an embedding)."""
    captions, where, index = [], {}, []
    for q in queries:
        if isinstance(q, str):
            if q not in where:
                where[q] = len(captions)
                captions.append(q)
            index.append(where[q])
        else:
            index.append(None)
    return captions, index


def _host_info(path: str):
    """(encoding or None, channels, rate, frames) of a file `wavio.wav_info` refuses, through `wavio.read_wav`'s own parser (which
    raises ValueError for what it cannot read either); the channel layout is then unknown and the file counts as mono."""
    x, rate = wavio.read_wav(path)
    return None, 1, rate, int(x.shape[0])


@dataclass(frozen=True)
class Options:
    """What a `separate_files` call asks of every file, after its checks."""
    loudness: Optional[float]        # LUFS target
    ceiling_db: Optional[float]      # peak_ceiling_db
    true_peak: bool                  # peak == "true"
    meter: bool
    limiter: bool
    reach: int                       # the limiter's look-ahead in model-rate frames (0 without one)
    passes: int                      # limiter_passes (0 without a limiter)
    remix: bool                      # a target_gain_db was given

    @property
    def level(self) -> bool:
        return self.loudness is not None or self.ceiling_db is not None

    @property
    def extra(self) -> bool:         # whether a target sends anything to the host beside its payload and clip counter
        return self.level or self.meter


@dataclass(frozen=True)
class FilePlan:
    """Everything about one job that its header and the call's arguments decide (`plan_files`); the pass derives none of it."""
    info: Optional[tuple]            # `wavio.wav_info`'s tuple, None for a header it refuses
    meta: tuple                      # (encoding or None, channels, rate, frames) of the input
    how: str                         # `route`: "device" or "host"
    n_planes: int                    # recordings the file puts into a pass, and channels of what is written
    length: int                      # model-rate samples per plane
    enc_o: str
    rate_o: int
    frames_o: int
    ceiling: Optional[np.float32]    # `loudness.ceiling_for`: linear, capped for PCM
    in_path: str
    out_path: Optional[str]          # the separated target's file; None where the job's one file is the remix
    remix_path: Optional[str]
    db: Optional[float]              # the job's target_gain_db
    amount: Optional[np.float32]     # `remix_coefficient(db)`


def plan_files(jobs, dbs, o: Options, sampling_rate: int, n_fft: int, channels: str = "each", encoding: Optional[str] = None,
               out_rate: Optional[int] = None) -> List[FilePlan]:
    """One FilePlan per job, from the files' headers alone.  dbs: `check_remix_args`' list or None.  The output has the input's
    frame count at the input's rate, else ceil(model-rate samples * up / down).  ValueError, with the file's name, for a file not
    longer than the reflect padding n_fft/2 at the model rate (`longform.plan_windows`' refusal, before anything is written), and
    under channels="linked" for a file of more than 8 channels (the linked calls' limit)."""
    sr, plans = int(sampling_rate), []
    for k, job in enumerate(jobs):
        info = wavio.wav_info(job[0])
        how = route(info, sr, out_rate, o.true_peak)
        enc_in, nch, rate, frames = meta = info[:4] if info is not None else _host_info(job[0])
        n_planes, length = model_samples(nch, rate, frames, sr, channels)
        if channels == "linked" and n_planes > MAX_CHANNELS:
            raise ValueError(f'{job[0]}: channels="linked" takes at most {MAX_CHANNELS} channels, the file has {n_planes}')
        if length <= n_fft // 2:
            raise ValueError(f"{job[0]}: a recording of {length} samples is not longer than the reflect padding "
                             f"(n_fft/2 = {n_fft // 2})")
        rate_o, enc_o = rate if out_rate is None else int(out_rate), encoding or enc_in or "f32"
        plans.append(FilePlan(
            info, meta, how, n_planes, length, enc_o, rate_o,
            frames if rate_o == rate else rs.out_len(length, *rs.ratio(sr, rate_o)), ld.ceiling_for(o.ceiling_db, enc_o), job[0],
            job[2] if dbs is None or len(job) == 4 else None, job[-1] if dbs is not None else None,
            None if dbs is None else dbs[k], None if dbs is None else remix_coefficient(dbs[k])))
    return plans


# ---- host route -------------------------------------------------------------------------------------------------------------
def _host_decode(path: str, info, channels: str) -> np.ndarray:
    """(planes, frames) float32 at the file's rate: `wavio.read_wav`'s decode rules, per channel ("each") or down-mixed."""
    if info is None or channels == "mono":
        return wavio.read_wav(path)[0][None]
    enc, nch, _, frames, offset = info
    with open(path, "rb") as f:
        f.seek(offset)
        raw = f.read(frames * nch * rs.SAMPLE_BYTES[enc])
    if enc == "pcm16":
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif enc == "pcm32":
        x = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        x = np.frombuffer(raw, dtype="<f4").astype(np.float32)
    return np.ascontiguousarray(x.reshape(frames, nch).T)


def _host_resample(x: np.ndarray, rate_in: int, rate_out: int) -> np.ndarray:
    return x if rate_in == rate_out else np.stack([wavio._resample(p, rate_in, rate_out) for p in x])


def host_clip_count(x: np.ndarray, encoding: str) -> int:
    """PCM samples of x that `wavio.write_wav_pcm16` / `write_wav_pcm32` clip (0 for "f32"; a NaN is not counted)."""
    if encoding == "f32":
        return 0
    scale, lo, hi = (32768.0, -32768, 32767) if encoding == "pcm16" else (2147483648.0, -2147483648, 2147483647)
    r = np.round(np.asarray(x, dtype=np.float64) * scale)
    return int(np.count_nonzero((r < lo) | (r > hi)))


# ---- remix -------------------------------------------------------------------------------------------
def remix_coefficient(db) -> np.float32:
    """k of `original + k * target` for a change of the target's level by `db` dB: float32(10^(db/20) - 1), formed in float64
    and rounded once.  Exactly -1 for -inf (the target is removed) and exactly 0 for 0 (the file comes back).  ValueError for a
    NaN, for +inf and for a boost beyond float32."""
    try:
        db = float(db)
    except (TypeError, ValueError):
        raise ValueError("target_gain_db must be a number of dB (-inf removes the target)") from None
    if np.isnan(db) or db == np.inf:
        raise ValueError("target_gain_db must be a number of dB below +inf (-inf removes the target)")
    with np.errstate(over="ignore"):
        k = np.float32(np.power(10.0, np.float64(db) / 20.0) - 1.0)
    if not np.isfinite(k):
        raise ValueError(f"target_gain_db = {db} dB is beyond float32")
    return k


def remix_host(x: np.ndarray, y: np.ndarray, k, gain=None) -> np.ndarray:
    """lass_remix_encode's value before quantisation, restated in numpy float32: v = fl(x + fl(k * y)) - two roundings, as the
    kernel makes them - and fl(gain * v) with a gain.  x: the decoded original, y: the estimate resampled to the file's rate."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.float32(k) * y
        v = x + p
        return v if gain is None else np.float32(gain) * v


def check_remix_args(target_gain_db, jobs, channels: str, out_rate, loudness, meter, limiter, peak) -> Optional[List[float]]:
    """The dB of every job, or None without a `target_gain_db`.  ValueError for a job that is no (in, query, out) or (in, query,
    out, remix_out), a job of four without a target_gain_db, a target_gain_db that is neither one number nor one per job
    (`remix_coefficient`'s refusals), and in remix mode for channels="mono" (there is no mono original to mix into), an out_rate
    that differs from a file's own rate (the original exists at its own rate alone), and loudness=, meter=True, limiter=True and
    peak="true": those measure the separated planes at the model rate, which a remix does not write.  Reads the files' headers,
    nothing else: it runs before the model is touched."""
    for j in jobs:
        if len(j) not in (3, 4):
            raise ValueError("a job is (in_path, query, out_path) or (in_path, query, out_path, remix_out_path)")
    if target_gain_db is None:
        if any(len(j) == 4 for j in jobs):
            raise ValueError("a job (in_path, query, out_path, remix_out_path) needs a target_gain_db")
        return None
    if isinstance(target_gain_db, (list, tuple, np.ndarray)):
        dbs = list(target_gain_db)
        if len(dbs) != len(jobs):
            raise ValueError(f"target_gain_db holds {len(dbs)} values for {len(jobs)} jobs")
    else:
        dbs = [target_gain_db] * len(jobs)
    for d in dbs:
        remix_coefficient(d)
    dbs = [float(d) for d in dbs]
    if channels == "mono":
        raise ValueError('target_gain_db needs channels="each": a remix keeps the original\'s channels')
    for name, on in (("loudness", loudness is not None), ("meter", bool(meter)), ("limiter", bool(limiter)), ('peak="true"', peak == "true")):
        if on:
            raise ValueError(f"{name} measures the separated planes at the model rate, which a remix (target_gain_db) does not "
                             "write; peak_ceiling_db with peak=\"sample\" is what a remix takes")
    if out_rate is not None:
        for j in jobs:
            info = wavio.wav_info(j[0])
            rate = info[2] if info is not None else _host_info(j[0])[2]
            if int(out_rate) != rate:
                raise ValueError(f"{j[0]}: a remix is written at the file's own rate ({rate} Hz), not out_rate = {int(out_rate)}")
    return dbs


def _remix_record(rec: dict, db: float, gain=None, limited=None) -> dict:
    rec["target_gain_db"] = float(db)
    if gain is not None:
        with np.errstate(divide="ignore"):
            rec.update({"gain": float(gain), "gain_db": float(20.0 * np.log10(np.float64(gain))), "peak_limited": bool(limited)})
    return rec


# ---- the pass ---------------------------------------------------------------------------------------------------------------
class _Clock:
    """Seconds per stage into `profile` (synchronising the device at each stage's end); nothing at all without one."""

    def __init__(self, profile: Optional[Dict[str, float]], device):
        self.profile, self.device = profile, device

    @contextmanager
    def __call__(self, stage: str):
        if self.profile is None:
            yield
            return
        import torch
        t0 = time.perf_counter()
        yield
        torch.cuda.synchronize(self.device)
        self.profile[stage] = self.profile.get(stage, 0.0) + time.perf_counter() - t0


class _Pinned:
    """Pinned uint8 rows, reused across files and passes instead of page-locking a fresh one per file."""

    def __init__(self):
        self.free: List = []
        self.lock = threading.Lock()     # the reader thread takes rows while the main thread takes and gives

    def take(self, nbytes: int):
        import torch
        with self.lock:
            fit = [b for b in self.free if b.numel() >= nbytes]
            if fit:
                buf = min(fit, key=lambda b: b.numel())
                self.free = [b for b in self.free if b is not buf]   # (list.remove would compare tensors)
                return buf
        return torch.empty(max(4, (nbytes + 3) // 4 * 4), dtype=torch.uint8).pin_memory()

    def give(self, buf) -> None:
        with self.lock:
            self.free.append(buf)


def _read_job(path: str, info, how: str, channels: str, pool: _Pinned, profile):
    """Reader thread: the raw payload in a pinned row (device route) or the decoded planes (host route)."""
    t0 = time.perf_counter()
    if how == "device":
        nbytes = info[3] * info[1] * rs.SAMPLE_BYTES[info[0]]
        buf = pool.take(nbytes)
        if not wavio.read_wav_raw_into(path, info, buf.numpy()[:nbytes]):
            raise OSError(f"{path}: the file changed or could not be read")
        got = buf
    else:
        got = _host_decode(path, info, channels)
    if profile is not None:
        profile["read"] = profile.get("read", 0.0) + time.perf_counter() - t0
    return got


def _write_device(path: str, header: bytes, buf, nbytes: int, event, profile) -> None:
    """Writer thread: the payload has arrived in the pinned row once `event` has passed."""
    event.synchronize()
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(header)
        f.write(memoryview(buf.numpy())[:nbytes])
    if profile is not None:
        profile["write"] = profile.get("write", 0.0) + time.perf_counter() - t0


def _write_host(path: str, encoding: str, x: np.ndarray, rate: int, profile) -> None:
    t0 = time.perf_counter()
    _WRITERS[encoding](path, x.T if x.shape[0] > 1 else x[0], rate)
    if profile is not None:
        profile["write"] = profile.get("write", 0.0) + time.perf_counter() - t0


def _level_record(measured: float, gain, limited: bool, true_peak=None) -> dict:
    """true_peak: the float32 true peak before the gain, with peak="true"."""
    with np.errstate(divide="ignore"):
        rec = {"loudness_out": float(measured), "gain": float(gain), "gain_db": float(20.0 * np.log10(np.float64(gain))),
               "peak_limited": bool(limited)}
        if true_peak is not None:
            rec["true_peak_db"] = float(20.0 * np.log10(np.float64(gain) * np.float64(true_peak)))
    return rec


def _meter_record(loudness_range: float, max_momentary: float, max_short_term: float) -> dict:
    return {"loudness_range": float(loudness_range), "max_momentary": float(max_momentary), "max_short_term": float(max_short_term)}


def _limiter_record(loudness_in: float, gain, min_gain, frames: int) -> dict:
    with np.errstate(divide="ignore"):
        return {"loudness_in": float(loudness_in), "limiter_gain_db": float(20.0 * np.log10(np.float64(gain))),
                "limiter_reduction_db": float(20.0 * np.log10(np.float64(min_gain))), "limiter_frames": int(frames)}


def check_limiter_args(limiter, limiter_lookahead_ms, limiter_passes, peak_ceiling_db, sampling_rate: int) -> None:
    """ValueError for a limiter without a ceiling to hold, a look-ahead that is no finite number >= 0 or reaches further than
    the kernel's `loudness.LIMITER_MAX_REACH` frames at the model rate, or a pass count that is no integer >= 1."""
    if not limiter:
        return
    if peak_ceiling_db is None:
        raise ValueError("limiter=True needs a peak_ceiling_db")
    if isinstance(limiter_passes, bool) or not isinstance(limiter_passes, (int, np.integer)) or limiter_passes < 1:
        raise ValueError("limiter_passes must be an integer >= 1")
    H = ld.reach(limiter_lookahead_ms, sampling_rate)
    if H > ld.LIMITER_MAX_REACH:
        raise ValueError(f"limiter_lookahead_ms reaches {H} frames at {sampling_rate} Hz, over the limiter's {ld.LIMITER_MAX_REACH}")


def _host_limit(x: np.ndarray, rate: int, target: Optional[float], ceiling, H: int, true: bool, passes: int):
    """The device route's limiter loop with lass_amd.loudness and numpy: (limited float32 planes, loudness of x, the gain of the
    last pass, the smallest value of its curve, the frames whose look-ahead minimum is below 1)."""
    l_in = ld.integrated_loudness(x, rate)
    g = ld.gain_for(l_in, None, target, None)[0]
    passes = passes if target is not None else 1
    for k in range(passes):
        e = ld.limiter_envelope(x, rate, true)
        G, _, m = ld.limiter_curve(e, g, ceiling, H)
        v = ((np.float64(g) * G) * x.astype(np.float64)).astype(np.float32)
        if k + 1 < passes:
            g = np.float32(g * ld.gain_for(ld.integrated_loudness(v, rate), None, target, None)[0])
    return v, l_in, g, (float(G.min()) if G.size else 1.0), int(np.count_nonzero(m < 1.0))


def check_peak_arg(peak, peak_ceiling_db) -> None:
    """ValueError for a `peak` that is neither "sample" nor "true", or "true" without a ceiling to hold it to."""
    if peak not in ("sample", "true"):
        raise ValueError('peak must be "sample" or "true"')
    if peak == "true" and peak_ceiling_db is None:
        raise ValueError('peak="true" needs a peak_ceiling_db')


# ---- what travels to the host behind a payload ------------------------------------------------------------------------------
_ITEM = {"uint8": 1, "int32": 4, "float32": 4, "float64": 8}
_LEVEL = (("limited", "int32", 1), ("gain", "float32", 1))
_STATS = {"max_momentary": 3, "max_short_term": 4, "loudness_range": 5}   # columns of Engine.loudness_stats' ten (STATS_COLUMNS)


class Tail:
    """One pinned row's layout: the encoded payload, then the file's numbers as named fields.  The fields start at the payload's
    end rounded up to the largest item among them and each starts on a multiple of its own item size, in the order given.  The
    only place that knows an offset: `size` is what to take from the pinned pool, `put` packs on the device's stream (one copy
    per field), `get` unpacks once the row has arrived."""

    def __init__(self, nbytes: int, fields):
        self.nbytes, self.where = int(nbytes), {"payload": (0, int(nbytes), "uint8")}
        widest = max(_ITEM[dtype] for _, dtype, _ in fields)
        at = (self.nbytes + widest - 1) // widest * widest
        for name, dtype, count in fields:
            at = (at + _ITEM[dtype] - 1) // _ITEM[dtype] * _ITEM[dtype]
            self.where[name] = (at, at + count * _ITEM[dtype], dtype)
            at += count * _ITEM[dtype]
        self.size = at

    @classmethod
    def target(cls, nbytes: int, o: Options) -> "Tail":
        """A separated target's: the clip counter; with a level the limited flag, the gain, the true peak where one is held and
        the loudness; the meter's ten numbers; the limiter's four."""
        fields = [("clipped", "int32", 1)]
        if o.level:
            fields += _LEVEL + ((("peak", "float32", 1),) if o.true_peak else ()) + (("loudness", "float64", 1),)
        if o.meter:
            fields += [("stats", "float64", 10)]
        if o.limiter:
            fields += [("loudness_in", "float64", 1), ("limiter_gain", "float32", 1), ("min_gain", "float32", 1), ("limiter_frames", "int32", 1)]
        return cls(nbytes, fields)

    @classmethod
    def remix(cls, nbytes: int, gained: bool) -> "Tail":
        """A remix's: the clip counter, and under a ceiling the limited flag and the gain."""
        return cls(nbytes, (("clipped", "int32", 1),) + (_LEVEL if gained else ()))

    def __contains__(self, name: str) -> bool:
        return name in self.where

    def _view(self, buf, name: str):
        import torch
        lo, hi, dtype = self.where[name]
        return buf[lo:hi].view(getattr(torch, dtype))

    def put(self, buf, name: str, tensor) -> None:
        self._view(buf, name).copy_(tensor, non_blocking=True)

    def get(self, buf, name: str):
        """The field's value: a Python number for a field of one item, else the view."""
        v = self._view(buf, name)
        return v[0].item() if v.numel() == 1 and name != "payload" else v

    def record(self, buf, rec: dict) -> dict:
        """rec with what the row holds beside the payload, under the record's keys."""
        rec["clipped"] = int(self.get(buf, "clipped"))
        gain, limited = (np.float32(self.get(buf, "gain")), bool(self.get(buf, "limited"))) if "gain" in self else (None, None)
        if "loudness" in self:
            rec.update(_level_record(self.get(buf, "loudness"), gain, limited, np.float32(self.get(buf, "peak")) if "peak" in self else None))
        elif gain is not None:
            _remix_record(rec, rec["target_gain_db"], gain, limited)
        if "stats" in self:
            ten = self.get(buf, "stats")
            rec.update(_meter_record(*(float(ten[_STATS[k]]) for k in ("loudness_range", "max_momentary", "max_short_term"))))
        if "loudness_in" in self:
            rec.update(_limiter_record(self.get(buf, "loudness_in"), np.float32(self.get(buf, "limiter_gain")),
                                       np.float32(self.get(buf, "min_gain")), self.get(buf, "limiter_frames")))
        return rec


# ---- a file's stages ---------------------------------------------------------------------------------
class _Ctx(NamedTuple):
    """What every stage of a call needs beside the file's plan."""
    eng: object
    sr: int
    o: Options
    clock: _Clock
    pool: _Pinned
    writer: ThreadPoolExecutor
    profile: Optional[Dict[str, float]]


def host_target(x: np.ndarray, plan: FilePlan, o: Options, sr: int) -> Tuple[np.ndarray, dict]:
    """The host route's target: x the separated planes at the model rate -> (the samples to write, the record's entries).  The
    device's rule with lass_amd.loudness and numpy."""
    rec = {}
    if o.limiter:
        x, *lim = _host_limit(x, sr, o.loudness, plan.ceiling, o.reach, o.true_peak, o.passes)
        rec.update(_limiter_record(*lim))
    y = _host_resample(x, sr, plan.rate_o)[:, :plan.frames_o]
    if o.extra:
        p = ld.block_powers(x, sr)
    if o.level:
        measured = ld.gate(p)[0]
        if o.true_peak:
            pk = np.float32(ld.true_peak(y, plan.rate_o))
        else:
            pk = float(np.nanmax(np.abs(y))) if y.size else 0.0
        g, bit = ld.gain_for(measured, pk, o.loudness, plan.ceiling)
        y = (g * y.astype(np.float32)).astype(np.float32)
        rec.update(_level_record(measured, g, bit, pk if o.true_peak else None))
    if o.meter:
        q = ld.short_term_powers(x, sr)
        rec.update(_meter_record(ld.loudness_range(q)[0], ld.max_momentary(p), ld.max_short_term(q)))
    rec["clipped"] = host_clip_count(y, plan.enc_o)
    return y, rec


def host_remix(x: np.ndarray, dry: np.ndarray, plan: FilePlan, sr: int) -> Tuple[np.ndarray, dict]:
    """The host route's remix: x the separated planes at the model rate, dry the decoded original -> (samples, entries)."""
    v = remix_host(dry, _host_resample(x, sr, plan.rate_o)[:, :plan.frames_o], plan.amount)
    rec = {}
    if plan.ceiling is not None:
        pk = np.float32(np.nanmax(np.abs(v))) if v.size else np.float32(0.0)
        g, bit = ld.gain_for(-np.inf, pk, None, plan.ceiling)
        v = (g * v).astype(np.float32)
        _remix_record(rec, plan.db, g, bit)
    rec["clipped"] = host_clip_count(v, plan.enc_o)
    return v, rec


def _device_level(eng, o: Options, plan: FilePlan, sr: int, stacked):
    """The limiter loop, the meter or the loudness, the sample or true peak, the gain -> (the planes to encode, the gain or
    None, the tensors of `Tail.target`'s fields).  Everything stays on the device."""
    fields, gain, pk = {}, None, None
    if o.limiter:
        loud_in = eng.loudness(stacked, sr)
        lim_gain = eng.loudness_gain(loud_in, None, o.loudness, None)[0]
        n_pass = o.passes if o.loudness is not None else 1
        for k in range(n_pass):
            held, lim = eng.limit(stacked, sr, lim_gain, plan.ceiling, o.reach, "true" if o.true_peak else "sample")
            if k + 1 < n_pass:
                lim_gain = lim_gain * eng.loudness_gain(eng.loudness(held, sr), None, o.loudness, None)[0]
        stacked = held[0]
        fields.update(loudness_in=loud_in, limiter_gain=lim_gain, min_gain=lim["min_gain"], limiter_frames=lim["frames"])
    if o.meter:
        stats = eng.loudness_stats(stacked, sr)["all"]
        measured, fields["stats"] = stats[:, 0], stats[0]
    else:
        measured = eng.loudness(stacked, sr)
    if o.ceiling_db is not None:
        pk = (eng.resample_true_peak if o.true_peak else eng.resample_peak)(stacked, sr, plan.rate_o, frames_out=plan.frames_o)
    if o.level:
        gain, limited = eng.loudness_gain(measured, pk, o.loudness, plan.ceiling)
        fields.update(limited=limited, gain=gain, loudness=measured, **({"peak": pk} if o.true_peak else {}))
    return stacked, gain, fields


def _device_remix_level(eng, plan: FilePlan, sr: int, stacked, dry, amount):
    """The peak of the remix about to be quantised and the ceiling's gain alone -> (the gain, `Tail.remix`'s fields)."""
    import torch
    pk = eng.remix_peak(stacked, sr, plan.rate_o, dry, plan.meta[0], amount, frames_out=plan.frames_o)
    gain, limited = eng.loudness_gain(torch.full((1,), -np.inf, dtype=torch.float64, device=eng.device), pk, None, plan.ceiling)
    return gain, {"limited": limited, "gain": gain}


def _send(ctx: _Ctx, plan: FilePlan, rec: dict, path: str, stacked, gain, fields: dict, dry=None, amount=None):
    """Encode (`Engine.remix_encode` with a dry source, else `Engine.resample_encode`), copy payload and fields into a pinned row
    and hand the row to the writer thread -> the pass's pending entry (remix?, record, tail, row, the write)."""
    import torch
    eng = ctx.eng
    with ctx.clock("encode"):
        clipped = torch.zeros(1, dtype=torch.int32, device=eng.device)
        if dry is None:
            payload = eng.resample_encode(stacked, ctx.sr, plan.rate_o, plan.enc_o, frames_out=plan.frames_o, clipped=clipped, gain=gain)
        else:
            payload = eng.remix_encode(stacked, ctx.sr, plan.rate_o, plan.enc_o, dry, plan.meta[0], amount, frames_out=plan.frames_o,
                                       clipped=clipped, gain=gain)
    tail = Tail.target(payload.shape[1], ctx.o) if dry is None else Tail.remix(payload.shape[1], gain is not None)
    buf = ctx.pool.take(tail.size)
    with ctx.clock("d2h"):
        values = dict(payload=payload[0], clipped=clipped, **fields)
        assert set(values) == set(tail.where), (sorted(values), sorted(tail.where))
        for name in tail.where:
            tail.put(buf, name, values[name])
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(eng.device))
    header = wavio.wav_header(plan.enc_o, plan.n_planes, plan.rate_o, plan.frames_o)
    return dry is not None, rec, tail, buf, ctx.writer.submit(_write_device, path, header, buf, tail.nbytes, done, ctx.profile)


def _to_host(ctx: _Ctx, mine) -> np.ndarray:
    import torch
    with ctx.clock("d2h"):
        return torch.stack(mine).cpu().numpy()


def _write_target(ctx: _Ctx, plan: FilePlan, rec: dict, mine, stacked):
    """The separated target of one file, levelled as the call asks -> its pending entry; `rec` is complete once collected."""
    if plan.how == "device":
        gain, fields = None, {}
        if ctx.o.extra:
            with ctx.clock("level"):
                stacked, gain, fields = _device_level(ctx.eng, ctx.o, plan, ctx.sr, stacked)
        return _send(ctx, plan, rec, plan.out_path, stacked, gain, fields)
    y, entries = host_target(_to_host(ctx, mine), plan, ctx.o, ctx.sr)
    rec.update(entries)
    return False, rec, None, None, ctx.writer.submit(_write_host, plan.out_path, plan.enc_o, y, plan.rate_o, ctx.profile)


def _write_remix(ctx: _Ctx, plan: FilePlan, rec: dict, mine, stacked, dry, amount):
    """The remix of one file from its separated planes and its original (`dry`: the raw row on the device, the decoded planes on
    the host route) -> its pending entry."""
    if plan.how == "device":
        gain, fields = None, {}
        if plan.ceiling is not None:
            with ctx.clock("level"):
                gain, fields = _device_remix_level(ctx.eng, plan, ctx.sr, stacked, dry, amount)
        return _send(ctx, plan, rec, plan.remix_path, stacked, gain, fields, dry, amount)
    v, entries = host_remix(_to_host(ctx, mine), dry, plan, ctx.sr)
    rec.update(entries)
    return True, rec, None, None, ctx.writer.submit(_write_host, plan.remix_path, plan.enc_o, v, plan.rate_o, ctx.profile)


def _collect(pending, pool: _Pinned) -> None:
    """Wait for every file of the pass, the targets first, and read each device row's numbers into its record before the row
    goes back to the pool."""
    for _, rec, tail, buf, fut in sorted(pending, key=lambda entry: entry[0]):
        fut.result()
        if buf is not None:
            tail.record(buf, rec)
            pool.give(buf)


def _submit_reads(reader, plans, ids, channels: str, pool: _Pinned, profile):
    return [reader.submit(_read_job, plans[i].in_path, plans[i].info, plans[i].how, channels, pool, profile) for i in ids]


def separate_files(model, jobs, sampling_rate: int, channels: str = "each", encoding: Optional[str] = None,
                   out_rate: Optional[int] = None, window: int = 160000, context: int = 16000, fade: int = 0,
                   fade_shape: str = "linear", max_batch: int = 16, max_samples: int = DEFAULT_MAX_SAMPLES,
                   profile: Optional[Dict[str, float]] = None, loudness: Optional[float] = None,
                   peak_ceiling_db: Optional[float] = None, peak: str = "sample", meter: bool = False, limiter: bool = False,
                   limiter_lookahead_ms: float = 1.5, limiter_passes: int = 2, target_gain_db=None) -> List[dict]:
    """Separate WAV files by caption, file in and file out.  model: an `AudioSep`-shaped holder (`.ss_model` a ResUNet30 on the
    device working at `sampling_rate`, `.query_encoder` with `get_query_embed`); jobs: a sequence of (in_path, query, out_path),
    query a caption or a (512,) embedding.  channels "each": every channel of a file is separated on its own with the file's
    query and the output keeps the channel layout; "mono": the channels are averaged first (as `librosa.load(mono=True)` does) and
    the output is mono; "linked": ONE mask per file, estimated from the file's mono down-mix (`Engine.decode_resample` of its raw
    row, the "mono" path's own; on the host route `ResUNet30.downmix` of its model-rate planes) and applied to every channel
    (`ResUNet30.separate_long_list_linked`, the files of a pass grouped by channel count) - the network runs once per file, the
    stereo image of the target stays put, the output keeps the channel layout, everything after the separation (level, limiter,
    remix) sees the C planes of "each", and a record gains "linked": True.  A pass counts C + 1 rows for such a file.  encoding / out_rate None: the input file's own; the output then has the input's frame count, else
    ceil(model-rate samples * up / down).  window, context, fade, fade_shape, max_batch: `ResUNet30.separate_long_list`'s.  Files
    are taken in passes of at most `max_samples` model-rate samples (all planes counted), which bounds the memory; the captions
    of a pass are embedded in one `get_query_embed` call, each distinct caption once.  profile: a dict that receives seconds per
    stage (read, h2d, decode, separate, level, encode, d2h, write), with the device synchronised after each stage - for measurement.
    Returns one record per job, in order: {"rate", "channels", "frames", "clipped", "path"} of the file written - "clipped" the
    number of PCM samples the writer clipped, "path" "device" or "host" (module docstring).
    loudness: the integrated loudness (ITU-R BS.1770-4, LUFS) every file is brought to; peak_ceiling_db: the level in dBFS (<= 0)
    no written sample exceeds - the gain is lowered where it would, and with "pcm16" / "pcm32" the ceiling is capped at the
    largest value that does not clip, so "clipped" is then 0.  One gain per file.  With either, a record also has "loudness_out"
    (measured on the separated planes before the gain; -inf for a file shorter than 400 ms or silent, which gets gain 1 or the
    ceiling's gain alone), "gain" (linear, the float32 applied), "gain_db" and "peak_limited" (whether the ceiling lowered it).
    peak "true" (it needs a peak_ceiling_db): the ceiling holds the true peak - the peak of the written signal between its samples,
    4 x oversampled up to 48 kHz (`loudness.true_peak`, `Engine.resample_true_peak`) - instead of the sample peak, as EBU R 128's
    -1 dBTP asks; a true peak is never under the sample peak, so "clipped" stays 0, and the record gains "true_peak_db", the true
    peak of what was written (20 log10 of gain x true peak).  meter: the record gains "loudness_range" (LU, EBU Tech 3342),
    "max_momentary" and "max_short_term" (LUFS), measured like "loudness_out" on the separated planes at the model rate before
    the gain (`Engine.loudness_stats` in the place of `Engine.loudness`); with or without a level.
    limiter (it needs a peak_ceiling_db): a look-ahead limiter (`Engine.limit`, `loudness.limit`) in front of the level stage, so
    that a ceiling that binds no longer costs the file its loudness: the separated planes are brought to `loudness` by a gain
    without a ceiling (1 without a target) and held under the ceiling by one gain curve per file that reaches
    `limiter_lookahead_ms` to either side of a peak, `limiter_passes` (>= 1) times, the gain corrected between the passes by the
    loudness of the limited planes (one pass without a target).  The record gains "loudness_in" (the separated planes),
    "limiter_gain_db" (the last pass's gain), "limiter_reduction_db" (20 log10 of the curve's smallest value, <= 0) and
    "limiter_frames" (frames the curve was asked to lower); "loudness_out" and the `meter` figures then describe the LIMITED planes,
    "gain" is the static trim the level stage applies to them, and the loudness written is loudness_out + gain_db.
    target_gain_db (None: all of the above, bit for bit): a number of dB (-inf allowed), or one per job, turns on REMIX MODE - the
    file written to out_path is the original with the target's level changed by that many dB, original + k * target with k =
    `remix_coefficient(dB)`, at the file's own rate, channels and frame count (`Engine.remix_encode`; `remix_host` on the host
    route): -inf removes the target, 0 gives the file back.  A job may then be (in_path, query, out_path, remix_out_path): out_path
    is written exactly as without target_gain_db, the separated target, and remix_out_path is the remix, from the same separated
    planes with one more encode launch; the record describes out_path as ever and carries "remix", the remix file's record.  The
    record of a remix has "target_gain_db" beside the five keys.  A boost can clip, so peak_ceiling_db (with peak="sample") holds
    for the remix too: `Engine.remix_peak` of what is about to be quantised, `Engine.loudness_gain` for the ceiling's gain alone,
    `Engine.remix_encode(gain=)`; its record gains "gain", "gain_db" and "peak_limited" (no "loudness_out": nothing is metered),
    and with PCM output "clipped" is 0.  Remix mode refuses (`check_remix_args`, ValueError) channels="mono", an out_rate other than
    a file's own rate, loudness=, meter=True, limiter=True and peak="true".  The raw rows of a pass stay on the device until their
    files are encoded, BESIDE the `max_samples` bound: about 5.5 bytes per model-rate sample for 44.1 kHz PCM16 at a 16 kHz model
    (2 bytes x 44100 / 16000), up to 12 for 48 kHz float32.
    A file not longer than n_fft/2 samples at the model rate raises ValueError before anything is written."""
    import torch

    if channels not in ("each", "mono", "linked"):
        raise ValueError('channels must be "each" or "mono" (or "linked": one mask from the down-mix for every channel)')
    if encoding is not None and encoding not in rs.ENCODINGS:
        raise ValueError(f"encoding must be one of {sorted(rs.ENCODINGS)} or None")
    ld.check_level_args(loudness, peak_ceiling_db)
    check_peak_arg(peak, peak_ceiling_db)
    check_limiter_args(limiter, limiter_lookahead_ms, limiter_passes, peak_ceiling_db, int(sampling_rate))
    jobs = [tuple(j) for j in jobs]
    dbs = check_remix_args(target_gain_db, jobs, channels, out_rate, loudness, bool(meter), bool(limiter), peak)
    o = Options(loudness, peak_ceiling_db, peak == "true", bool(meter), bool(limiter),
                ld.reach(limiter_lookahead_ms, int(sampling_rate)) if limiter else 0, int(limiter_passes) if limiter else 0, dbs is not None)
    ss = model.ss_model
    eng = ss.engine
    dev, sr = eng.device, int(sampling_rate)
    plans = plan_files(jobs, dbs, o, sr, eng.n_fft, channels, encoding, out_rate)

    clock, pool = _Clock(profile, dev), _Pinned()
    records: List[Optional[dict]] = [None] * len(jobs)
    passes = plan_passes([pass_rows(p.n_planes, channels) * p.length for p in plans], max_samples)
    with ThreadPoolExecutor(1) as reader, ThreadPoolExecutor(1) as writer:
        ctx = _Ctx(eng, sr, o, clock, pool, writer, profile)
        reads = _submit_reads(reader, plans, passes[0], channels, pool, profile) if passes else []
        for pi, ids in enumerate(passes):
            # the next pass is read while this one runs
            ahead = _submit_reads(reader, plans, passes[pi + 1], channels, pool, profile) if pi + 1 < len(passes) else []
            captions, cap_of = dedup_captions([jobs[i][1] for i in ids])
            emb = (model.query_encoder.get_query_embed(modality="text", text=captions, device=dev).to(torch.float32)
                   if captions else None)
            planes, conds, uploaded, dry, pending = [], [], [], {}, []
            linked = []                                              # channels="linked": (planes, guide, condition) per file
            amounts = torch.tensor([float(plans[i].amount) for i in ids], dtype=torch.float32).to(dev) if o.remix else None
            for k, (i, fut) in enumerate(zip(ids, reads)):
                plan, got = plans[i], fut.result()
                enc_in, nch, rate, frames = plan.meta
                if plan.how == "device":
                    nbytes = frames * nch * rs.SAMPLE_BYTES[enc_in]
                    with clock("h2d"):
                        raw = got[None, :(nbytes + 3) // 4 * 4].to(dev, non_blocking=True)
                    with clock("decode"):
                        if channels != "mono":
                            mine = list(eng.decode_resample_planar(raw, frames, nch, enc_in, rate, sr)[0])
                        else:
                            mine = [eng.decode_resample(raw, frames, nch, enc_in, rate, sr)[0]]
                        if channels == "linked":                     # the guide is the mono path's own down-mix
                            guide = eng.decode_resample(raw, frames, nch, enc_in, rate, sr)[0]
                    uploaded.append(got)
                else:
                    mine = [torch.from_numpy(p).to(dev) for p in _host_resample(got, rate, sr)]
                    if channels == "linked":
                        guide = ss.downmix(torch.stack(mine))
                if o.remix:
                    dry[i] = raw if plan.how == "device" else got   # kept until the file's encode: the remix's dry source
                cond = emb[cap_of[k]] if cap_of[k] is not None else torch.as_tensor(jobs[i][1]).to(device=dev, dtype=torch.float32).reshape(-1)
                if channels == "linked":
                    linked.append((torch.stack(mine), guide, cond))
                    continue
                planes += mine
                conds += [cond] * len(mine)
            with clock("separate"):
                if channels == "linked":
                    # one network pass per file whatever its channels: the files of the pass by channel count, one call per count
                    done = [None] * len(linked)
                    for group in group_by_planes([f[0].shape[0] for f in linked]):
                        outs = ss.separate_long_list_linked([linked[k][0] for k in group], torch.stack([linked[k][2] for k in group]),
                                                            [linked[k][1] for k in group], window=window, context=context,
                                                            max_batch=max_batch, fade=fade, fade_shape=fade_shape)
                        for k, sep in zip(group, outs):
                            done[k] = sep
                    seps = [row for sep in done for row in sep]      # C planes per file, as under "each", from here on
                else:
                    seps = ss.separate_long_list(planes, torch.stack(conds), window=window, context=context, max_batch=max_batch,
                                                 fade=fade, fade_shape=fade_shape)
            at = 0
            for j, i in enumerate(ids):
                plan, mine = plans[i], seps[at:at + plans[i].n_planes]
                at += plan.n_planes
                if any(int(m.shape[0]) != plan.length for m in mine):
                    raise RuntimeError(f"{plan.in_path}: separated planes of {[int(m.shape[0]) for m in mine]} samples, planned {plan.length}")
                rec = {"rate": plan.rate_o, "channels": plan.n_planes, "frames": plan.frames_o, "path": plan.how}
                if channels == "linked":
                    rec["linked"] = True
                stacked = torch.stack(mine) if plan.how == "device" else None
                if o.remix:
                    remix = _remix_record(dict(rec), plan.db)
                    pending.append(_write_remix(ctx, plan, remix, mine, stacked, dry.pop(i), amounts[j:j + 1]))
                    if plan.out_path is None:                      # the remix is the job's one file
                        records[i] = remix
                        continue
                    rec["remix"] = remix                           # ... or goes beside the target, which is written as ever
                pending.append(_write_target(ctx, plan, rec, mine, stacked))
                records[i] = rec
            reads = ahead
            # the pass's files are on disk (so its uploads are long done) and its numbers read before its pinned rows go back
            _collect(pending, pool)
            for buf in uploaded:
                pool.give(buf)
    return records


def inference(model, audio_file: str, text, output_file: str, sampling_rate: int = 32000, **kw) -> dict:
    """One file through `separate_files`: the single-file shape of upstream AudioSep's `pipeline.inference`.  loudness, peak_ceiling_db,
    peak, meter, limiter, limiter_lookahead_ms, limiter_passes, target_gain_db (with which `output_file` is the remix) and the other
    keywords are `separate_files`'s.  Returns the job's record."""
    return separate_files(model, [(audio_file, text, output_file)], sampling_rate, **kw)[0]
