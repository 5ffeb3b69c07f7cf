"""DCASE-2024 T9 evaluator with the reference's interface (dcase_evaluator.py:27-145).

Same constructor, same `__call__(pl_model) -> (mean_sisdr, mean_sdri, mean_sdr)`, same mixing / declipping / metric
definitions and the same printed line.  Differences are in execution only:
  * clips are separated in batches (`batch_size`, default 16) instead of one by one - eval-mode BatchNorm has no
    cross-clip coupling, so results are unchanged;
  * SDR / SI-SDR reductions run on the device over the resident waveforms (no D2H of audio);
  *  the SNR mixing / declipping runs on the device too (`lass_mix_at_snr`), WAV decoding of the next
    clips is prefetched by a small thread pool while the GPU separates the current batch, a batch goes to the device
    through pinned double buffers on a copy stream (`_Stager`: the host never waits on the GPU inside the loop), and
    caption embeddings are cached per caption (captions repeat; the query encoder is called once per distinct caption);
    `device_mixing=False` restores the reference's host-side numpy mixing (used by the parity tests as the yardstick);
  * (round 5) the RESIDENT path, taken when the separator offers `separate_into` (lass_amd.ResUNet30 does) and mixing is on
    the device: two persistent batch slots - pinned host rows the decode threads fill DIRECTLY (`read_wav_into`: a float32
    file goes file -> pinned memory in one `readinto`), and one set of device tensors (source, noise, SNR, mixture, condition,
    output) each - so that `lass_separate` sees recurring pointers: the full batches replay its captured hipGraph with the two
    overlapping half-batches (include/lass_hip.h) instead of launching ~40 kernels eagerly, and the loop allocates nothing per
    batch.  Any clip that does not fit a slot row (other length, rate, channels) sends its batch through the generic path
    below; results are identical either way (`resident=False` forces the generic path);
  * (opt-in, `device_decode=True`) a validation set that is NOT mono at the evaluator's rate - another sample rate, several
    channels - keeps the resident path: the slots then carry pinned and device BYTE rows, the decode threads only read each
    file's data chunk into them (`read_wav_raw_into`), and PCM decode, mono down-mix and polyphase resampling run on the
    device (`lass_decode_resample`, two launches per batch in front of `lass_mix_at_snr`).  Without it such a set is decoded and
    resampled on the host (`read_wav`: scipy in float64, ~10 ms per clip) and every batch takes the generic path.  The filter
    is the host's (lass_amd/resample.py), evaluated in float32; a set that is mono at the rate runs exactly as without the flag;
  * (opt-in, `ragged=True`) a set whose clips DIFFER in length: the generic path below batches only consecutive clips of
    identical length, so such a set runs as batch-1 launches.  With the flag it decodes a window of clips, sorts them into
    32-frame buckets (lass_amd/ragged.py), stages each batch as zero-padded rows and separates it with one
    `lass_separate_ragged` launch set; mixing and the SDR sums run on the padded rows unchanged (the padding adds exact zeros)
    and the dB figures use each clip's own length.  Waveforms are bit-equal to the clip-by-clip run; rows come back in csv order;
  * under torch.distributed the clip list is block-sharded over ranks and the per-clip metric rows are all-gathered
    once at the end (RCCL when the backend is "nccl").
"""
from __future__ import annotations

import csv
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List

import numpy as np
import torch

from . import _alloc
from . import dist as ldist
from . import resample as rs
from .engine import get_engine
from .metrics import stats_to_db
from .ragged import plan_batches
from .utils import load_ss_model, parse_yaml
from .wavio import read_wav, read_wav_into, read_wav_raw_into, wav_frames, wav_info


def _mix_on_host(source: np.ndarray, noise: np.ndarray, snr_db: int):
    """The evaluator's deterministic mixer (dcase_evaluator.py:77-89) in numpy: the noise is given the gain that puts the
    pair at `snr_db` (power ratio of the two clips), and a mixture that would clip is brought down to a 0.9 peak together
    with its source, so the SDR reference stays consistent with what the separator hears.  Returns (source, mixture);
    `lass_mix_at_snr` is the device-side twin."""
    gain = np.sqrt(np.mean(np.square(source)) / (10 ** (snr_db / 10)) / np.mean(np.square(noise)))
    mixture = source + noise * gain
    peak = np.max(np.abs(mixture))
    if peak > 1:
        source, mixture = source * (0.9 / peak), mixture * (0.9 / peak)
    return source, mixture


class _Stager:
    """Host -> device staging of one batch off the compute stream: the decoded clips are stacked straight into PINNED host
    buffers (two slots, reused) and copied by a side stream, which the compute stream only waits on.  With
    `torch.from_numpy(np.stack(...)).to(device)` the copy is pageable: it queues behind the previous batch's kernels on the
    compute stream and holds the host until it is done, so nothing of the next batch is prepared while the GPU works."""

    def __init__(self, device, slots: int = 2):
        self.device = device
        self.stream = torch.cuda.Stream(device)
        self.slots = [{"bufs": {}, "done": None} for _ in range(slots)]
        self.n = 0

    def put(self, columns: List[List[np.ndarray]]) -> List[torch.Tensor]:
        """columns: per output tensor, the B equal-shape float32 arrays to stack -> the (B, ...) device tensors."""
        slot = self.slots[self.n % len(self.slots)]
        self.n += 1
        if slot["done"] is not None:
            slot["done"].synchronize()  # the copy that last read these pinned buffers (two batches ago)
        compute = torch.cuda.current_stream(self.device)
        outs = []
        with torch.cuda.stream(self.stream):
            for k, arrays in enumerate(columns):
                shape = (len(arrays),) + tuple(arrays[0].shape)
                pin = slot["bufs"].get(k)
                if pin is None or pin.shape[1:] != shape[1:] or pin.shape[0] < shape[0]:
                    pin = slot["bufs"][k] = torch.empty(shape, dtype=torch.float32).pin_memory()
                view = pin[: shape[0]]
                np.stack(arrays, out=view.numpy())
                dev = torch.empty(shape, dtype=torch.float32, device=self.device)
                dev.copy_(view, non_blocking=True)
                dev.record_stream(compute)
                outs.append(dev)
            slot["done"] = torch.cuda.Event()
            slot["done"].record(self.stream)
        compute.wait_event(slot["done"])
        return outs


class _Slot:
    """One resident batch: pinned host rows for the decode threads and the device tensors lass_separate sees again and again."""

    def __init__(self, B: int, L: int, device, raw_bytes: int = 0):
        """raw_bytes > 0 (device_decode on a set that is not mono at the rate): the pinned rows hold the files' data chunks,
        `raw_bytes` bytes each, next to device copies of them; the float32 rows exist on the device only."""
        pin = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype).pin_memory()  # noqa: E731
        dev = lambda *shape, dtype=torch.float32: _alloc.empty(shape, dtype=dtype, device=device)  # noqa: E731
        self.pin_snr = pin(B)
        self.np_snr = self.pin_snr.numpy()
        if raw_bytes:
            self.pin_src, self.pin_noise = pin(B, raw_bytes, dtype=torch.uint8), pin(B, raw_bytes, dtype=torch.uint8)
            self.raw_src, self.raw_noise = dev(B, raw_bytes, dtype=torch.uint8), dev(B, raw_bytes, dtype=torch.uint8)
        else:
            self.pin_src, self.pin_noise = pin(B, L), pin(B, L)
        self.np_src, self.np_noise = self.pin_src.numpy(), self.pin_noise.numpy()
        self.src, self.noise, self.snr, self.mix, self.out = dev(B, L), dev(B, L), dev(B), dev(B, L), dev(B, L)
        self.cond = dev(B, 512)
        self.scratch = dev(B, 4, dtype=torch.float64)
        self.h2d_done = None      # the copy that last read the pinned rows
        self.compute_done = None  # the kernels that last read / wrote the device tensors


class DCASEEvaluator:
    def __init__(self, sampling_rate=16000, eval_indexes="lass_synthetic_validation.csv", audio_dir="lass_validation",
                 batch_size: int = 16, device_mixing: bool = True, io_workers: int = 2, resident: bool = True,
                 device_decode: bool = False, ragged: bool = False) -> None:
        r"""DCASE T9 LASS evaluator (dcase_evaluator.py:28-47)."""
        self.sampling_rate = sampling_rate
        with open(eval_indexes) as csv_file:
            csv_reader = csv.reader(csv_file, delimiter=",")
            eval_list = [row for row in csv_reader][1:]
        self.eval_list = eval_list
        self.audio_dir = audio_dir
        self.batch_size = batch_size
        self.device_mixing = device_mixing
        self.io_workers = max(1, io_workers)
        self.last_rows = None  # (N,3) per-clip [sdr, sdri, sisdr] of the last call (all ranks)
        self._embed_cache: Dict[str, torch.Tensor] = {}
        self.resident = resident
        self.device_decode = device_decode  # module docstring: decode / down-mix / resample on the device (resident path only)
        self.ragged = ragged   # module docstring: bucketed batches of clips of different lengths (generic path only)
        if ragged and not device_mixing:
            raise ValueError("ragged=True mixes on the device (zero-padded rows): it needs device_mixing=True")
        self._slots = {}       # (B, L, device, file format) -> [two _Slot]: kept across calls, so later calls replay graphs from their first batch
        self.last_path = None  # "resident" / "generic": which data path the last call took (tests, bench)
        self.resident_batches = self.generic_batches = 0

    def _read_pair(self, eval_data):
        """dcase_evaluator.py:67-74 for one csv row: decode the two clips only -> (source, noise, snr, caption)."""
        source, noise, snr, caption = eval_data
        source, _ = read_wav(os.path.join(self.audio_dir, f"{source}.wav"), self.sampling_rate)
        noise, _ = read_wav(os.path.join(self.audio_dir, f"{noise}.wav"), self.sampling_rate)
        return source.astype(np.float32, copy=False), noise.astype(np.float32, copy=False), int(snr), caption

    def _conditions(self, pl_model, captions: List[str], device) -> torch.Tensor:
        """One query-encoder call per DISTINCT caption not seen before (dcase_evaluator.py:93-97 calls it per clip)."""
        missing = [c for c in dict.fromkeys(captions) if c not in self._embed_cache]
        if missing:
            emb = pl_model.query_encoder.get_query_embed(modality="text", text=missing, device=device)
            for c, e in zip(missing, emb):
                self._embed_cache[c] = e.detach().to(device=device, dtype=torch.float32)
        return torch.stack([self._embed_cache[c] for c in captions])

    def _load_clip(self, eval_data):
        """Host-side variant of the data path (`device_mixing=False`): decode one csv row's pair and mix it on the CPU
        -> (source, mixture, caption), float32.  Semantics of dcase_evaluator.py:67-89."""
        source, noise, snr_db, caption = self._read_pair(eval_data)
        source, mixture = _mix_on_host(source, noise, snr_db)
        return source.astype(np.float32, copy=False), mixture.astype(np.float32, copy=False), caption

    def __call__(self, pl_model) -> tuple:
        r"""Evaluate (dcase_evaluator.py:49-122)."""
        rank, ws = ldist.world()
        if rank == 0:
            print("Evaluation on DCASE T9 synthetic validation set.")
        pl_model.eval()
        device = pl_model.device
        eng = get_engine(device)
        n_total = len(self.eval_list)
        lo, hi = ldist.shard_range(n_total, rank, ws)
        rows: List[np.ndarray] = []
        self._embed_cache.clear()  # embeddings belong to this pl_model's query encoder
        self.resident_batches = self.generic_batches = 0
        use_resident = (self.resident and self.device_mixing and hasattr(pl_model.ss_model, "separate_into") and hi > lo)
        self.last_path = "resident" if use_resident else "generic"
        if use_resident:
            rows = self._run_resident(pl_model, eng, device, lo, hi)
        else:
            rows = self._run_generic(pl_model, eng, device, self.eval_list[lo:hi])
        local = np.concatenate(rows, axis=0) if rows else np.zeros((0, 3))
        allrows = ldist.gather_rows(local, n_total, device)
        self.last_rows = allrows
        mean_sdr, mean_sdri, mean_sisdr = (float(np.mean(allrows[:, k])) for k in range(3))
        return mean_sisdr, mean_sdri, mean_sdr

    @staticmethod
    def _rows_from_stats(pending_stats) -> List[np.ndarray]:
        rows = []
        if not pending_stats:
            return rows
        # ONE device-to-host copy for all batches (each .cpu() is a synchronising call: 2 x 17 of them cost ~1 ms per evaluation)
        flat = torch.cat([t for st_sep, st_mix, _ in pending_stats for t in (st_sep, st_mix)]).cpu().numpy()
        at = 0
        for st_sep, _st_mix, length in pending_stats:
            m = st_sep.shape[0]
            sdr, sisdr = stats_to_db(flat[at:at + m], length)
            sdr_no_sep, _ = stats_to_db(flat[at + m:at + 2 * m], length)
            at += 2 * m
            rows.append(np.stack([sdr, sdr - sdr_no_sep, sisdr], axis=1))
        return rows

    def _run_resident(self, pl_model, eng, device, lo: int, hi: int) -> List[np.ndarray]:
        """The resident data path (module docstring): clip k of this rank's shard lives in row k % B of slot (k // B) % 2."""
        B = self.batch_size
        items = self.eval_list[lo:hi]
        n = len(items)
        first = os.path.join(self.audio_dir, f"{items[0][0]}.wav")
        sr = self.sampling_rate
        fmt, raw_bytes = None, 0  # fmt: the (encoding, channels, rate, frames) every file must have for the device to decode it
        if self.device_decode:
            info = wav_info(first)
            if info is not None and not (info[1] == 1 and info[2] == sr):
                enc, nch, rate, frames = fmt = info[:4]
                if nch > 8 or not rs.within_cap(*rs.ratio(rate, sr)):
                    info = None
            if info is None:  # nothing the device path takes: decided before any slot exists
                self.last_path = "generic"
                return self._run_generic(pl_model, eng, device, items)
        if fmt is None:
            L = wav_frames(first)
            if L <= 0:
                return self._run_generic(pl_model, eng, device, items)
        else:
            L = rs.out_len(frames, *rs.ratio(rate, sr))
            raw_bytes = (frames * nch * rs.SAMPLE_BYTES[enc] + 3) // 4 * 4
        key = (B, L, str(device)) + ((fmt,) if fmt else ())
        slots = self._slots.get(key)
        if slots is None:
            self._slots.clear()  # one shape at a time: 2 x (2 pinned + 5 device) x B x L floats
            slots = self._slots[key] = [_Slot(B, L, device, raw_bytes), _Slot(B, L, device, raw_bytes)]
        nb = (n + B - 1) // B
        compute = torch.cuda.current_stream(device)
        copy_stream = torch.cuda.Stream(device)

        def decode(k: int):
            """-> None when both files went straight into the slot rows, else the generic loader's tuple for this clip."""
            source, noise, snr, _caption = items[k]
            slot, r = slots[(k // B) % 2], k % B
            if fmt is not None:
                if (read_wav_raw_into(os.path.join(self.audio_dir, f"{source}.wav"), fmt, slot.np_src[r])
                        and read_wav_raw_into(os.path.join(self.audio_dir, f"{noise}.wav"), fmt, slot.np_noise[r])):
                    slot.np_snr[r] = float(int(snr))
                    return None
                return self._read_pair(items[k])
            if (read_wav_into(os.path.join(self.audio_dir, f"{source}.wav"), sr, slot.np_src[r])
                    and read_wav_into(os.path.join(self.audio_dir, f"{noise}.wav"), sr, slot.np_noise[r])):
                slot.np_snr[r] = float(int(snr))
                return None
            return self._read_pair(items[k])

        pending_stats, rows_out = [], []
        # (a burst of 8 / 16 decode threads for the first two batches - the GPU idles until batch 0 is on it - was measured SLOWER
        # than the steady two: 0.946 / 0.940 vs 0.955 of the separator, same process; the extra threads contend with the launching
        # thread and the HIP runtime's own)
        with torch.no_grad(), ThreadPoolExecutor(max_workers=self.io_workers) as pool:
            futures = {}
            submitted = 0  # batches whose decode jobs are out

            def submit_ready(upto: int):
                nonlocal submitted
                while submitted < min(nb, upto):
                    slot = slots[submitted % 2]
                    if slot.h2d_done is not None:
                        slot.h2d_done.synchronize()  # the copy of batch `submitted - 2` out of these pinned rows (long done)
                        slot.h2d_done = None
                    for k in range(submitted * B, min(n, (submitted + 1) * B)):
                        futures[k] = pool.submit(decode, k)
                    submitted += 1

            submit_ready(2)
            for j in range(nb):
                k0, k1 = j * B, min(n, (j + 1) * B)
                res = [futures.pop(k).result() for k in range(k0, k1)]
                slot, m = slots[j % 2], k1 - k0
                captions = [items[k][3] for k in range(k0, k1)]
                if all(r is None for r in res):
                    self.resident_batches += 1
                    with torch.cuda.stream(copy_stream):
                        if slot.compute_done is not None:
                            copy_stream.wait_event(slot.compute_done)  # batch j - 2 has finished with these device tensors
                        (slot.src if fmt is None else slot.raw_src)[:m].copy_(slot.pin_src[:m], non_blocking=True)
                        (slot.noise if fmt is None else slot.raw_noise)[:m].copy_(slot.pin_noise[:m], non_blocking=True)
                        slot.snr[:m].copy_(slot.pin_snr[:m], non_blocking=True)
                        slot.h2d_done = torch.cuda.Event()
                        slot.h2d_done.record(copy_stream)
                    compute.wait_event(slot.h2d_done)
                    src, mix, cond, out = slot.src[:m], slot.mix[:m], slot.cond[:m], slot.out[:m]
                    if fmt is not None:
                        eng.decode_resample(slot.raw_src[:m], frames, nch, enc, rate, sr, out=src)
                        eng.decode_resample(slot.raw_noise[:m], frames, nch, enc, rate, sr, out=slot.noise[:m])
                    eng.mix_at_snr(src, slot.noise[:m], slot.snr[:m], out=mix, scratch=slot.scratch)
                    cond.copy_(self._conditions(pl_model, captions, device))
                    pl_model.ss_model.separate_into(mix, cond, out)
                    pending_stats.append((eng.sdr_stats(src, out), eng.sdr_stats(src, mix), L))
                    slot.compute_done = torch.cuda.Event()
                    slot.compute_done.record(compute)
                    # batch j + 2 reuses THIS slot's pinned rows: its decode jobs go out once the copy above has left them
                    # (submit_ready waits for that copy; the GPU already holds this batch's kernels, so the host can afford to)
                    submit_ready(j + 3)
                else:
                    # some clip of this batch does not fit a slot row: the whole batch takes the generic route (rows that did
                    # land in the slot are read back out of it), in order, with the statistics kept in sequence
                    self.generic_batches += 1
                    group = []
                    for r_, k in zip(res, range(k0, k1)):
                        if r_ is None and fmt is not None:
                            r_ = self._read_pair(items[k])  # (the slot row holds the file's bytes, not samples)
                        elif r_ is None:
                            r_ = (slot.np_src[k % B].copy(), slot.np_noise[k % B].copy(), int(items[k][2]), items[k][3])
                        group.append(r_)
                    submit_ready(j + 3)
                    rows_out.extend(self._rows_from_stats(pending_stats))
                    pending_stats = []
                    rows_out.extend(self._run_generic(pl_model, eng, device, None, decoded=group))
            rows_out.extend(self._rows_from_stats(pending_stats))
        return rows_out

    def _run_generic(self, pl_model, eng, device, items, decoded=None) -> List[np.ndarray]:
        """The generic data path: clips of any length, grouped into batches of consecutive equal-length clips, fresh device
        tensors per batch (eager launches).  `decoded`: already decoded (source, noise, snr, caption) tuples instead of csv rows."""
        if self.ragged:
            return self._run_ragged(pl_model, eng, device, items, decoded)
        rows: List[np.ndarray] = []
        loader = self._read_pair if self.device_mixing else self._load_clip
        if decoded is not None:
            assert self.device_mixing
            items, loader = decoded, (lambda t: t)
        lo, hi = 0, len(items)
        with torch.no_grad(), ThreadPoolExecutor(max_workers=self.io_workers) as pool:
            # sliding window of decode jobs: at most two batches ahead of the one on the GPU
            pending = deque()
            pending_stats = []
            stager = _Stager(device)
            nxt = lo

            def refill():
                nonlocal nxt
                while nxt < hi and len(pending) < 2 * self.batch_size:
                    pending.append(pool.submit(loader, items[nxt]))
                    nxt += 1

            refill()
            while pending:
                group = [pending.popleft().result()]
                # batch consecutive clips of identical length (DCASE clips are all 10 s)
                while pending and len(group) < self.batch_size:
                    cand = pending[0].result()
                    if cand[0].shape != group[0][0].shape:
                        break
                    group.append(cand)
                    pending.popleft()
                refill()
                if self.device_mixing:
                    snr_col = [np.full(1, float(g[2]), dtype=np.float32) for g in group]
                    src, noise, snr = stager.put([[g[0] for g in group], [g[1] for g in group], snr_col])
                    mix = eng.mix_at_snr(src, noise, snr[:, 0])  # src is rescaled in place where the mixture clipped
                    captions = [g[3] for g in group]
                else:
                    src, mix = stager.put([[g[0] for g in group], [g[1] for g in group]])
                    captions = [g[2] for g in group]
                conditions = self._conditions(pl_model, captions, device)
                input_dict = {"mixture": mix[:, None, :], "condition": conditions}
                sep = pl_model.ss_model(input_dict)["waveform"][:, 0, :]
                # the (B,6) f64 statistics stay on the device: no host synchronisation inside the loop, so decoding /
                # staging of the next batch overlaps this batch's kernels; they are fetched once after the loop
                pending_stats.append((eng.sdr_stats(src, sep.contiguous()), eng.sdr_stats(src, mix), src.shape[1]))
            rows.extend(self._rows_from_stats(pending_stats))
        return rows


    def _run_ragged(self, pl_model, eng, device, items, decoded=None) -> List[np.ndarray]:
        """`ragged=True` (module docstring): windows of 4 batches' worth of clips, each planned into one-bucket batches."""
        ss = pl_model.ss_model
        if not hasattr(ss, "separate_ragged"):
            raise TypeError("ragged=True needs a separator with separate_ragged (lass_amd.ResUNet30)")
        loader = self._read_pair
        if decoded is not None:
            items, loader = decoded, (lambda t: t)
        n = len(items)
        n_fft = getattr(getattr(ss, "engine", None), "n_fft", 1024)
        hop = getattr(getattr(ss, "engine", None), "hop", 160)
        window = 4 * self.batch_size
        order: List[int] = []
        pending_stats = []
        with torch.no_grad(), ThreadPoolExecutor(max_workers=self.io_workers) as pool:
            stager = _Stager(device)
            jobs = deque(pool.submit(loader, items[k]) for k in range(min(n, window)))
            submitted = len(jobs)
            for w0 in range(0, n, window):
                clips = [jobs.popleft().result() for _ in range(min(window, n - w0))]
                while submitted < min(n, w0 + 2 * window):  # the next window decodes while this one is on the GPU
                    jobs.append(pool.submit(loader, items[submitted]))
                    submitted += 1
                lengths = [int(c[0].shape[0]) for c in clips]
                if any(c[1].shape[0] != m for c, m in zip(clips, lengths)):
                    raise ValueError("a source and its noise clip differ in length")
                for idx, row in plan_batches(lengths, self.batch_size, n_fft, hop):
                    pad = lambda x: np.pad(x, (0, row - x.shape[0]))  # noqa: E731
                    snr_col = [np.full(1, float(clips[i][2]), dtype=np.float32) for i in idx]
                    src, noise, snr = stager.put([[pad(clips[i][0]) for i in idx], [pad(clips[i][1]) for i in idx], snr_col])
                    mix = eng.mix_at_snr(src, noise, snr[:, 0])  # zero tails stay zero; the two means share their 1/row
                    cond = self._conditions(pl_model, [clips[i][3] for i in idx], device)
                    lens = np.asarray([lengths[i] for i in idx], dtype=np.int64)
                    sep = ss.separate_ragged(mix, lens, cond)
                    pending_stats.append((eng.sdr_stats(src, sep), eng.sdr_stats(src, mix), lens))
                    order.extend(w0 + i for i in idx)
        rows = self._rows_from_stats(pending_stats)
        if not rows:
            return rows
        out = np.empty((n, 3))
        out[np.asarray(order)] = np.concatenate(rows, axis=0)
        return [out]


def eval(evaluator, checkpoint_path, config_yaml="config/audiosep_base.yaml", device="cuda", query_encoder=None):
    """dcase_evaluator.py:126-145.  `query_encoder` defaults to the precomputed-embedding stand-in (CLAP itself stays
    on PyTorch-ROCm and needs its own checkpoint; pass a CLAP_Encoder-compatible object to use it)."""
    from .audiosep import PrecomputedQueryEncoder

    configs = parse_yaml(config_yaml)
    if query_encoder is None:
        query_encoder = PrecomputedQueryEncoder()
    pl_model = load_ss_model(configs=configs, checkpoint_path=checkpoint_path, query_encoder=query_encoder).to(device)
    print("-------  Start Evaluation  -------")
    SISDR, SDRi, SDR = evaluator(pl_model)
    msg_clotho = "SDR: {:.3f}, SDRi: {:.3f}, SISDR: {:.3f}".format(SDR, SDRi, SISDR)
    print(msg_clotho)
    print("-------------------------  Done  ---------------------------")
    return SDR, SDRi, SISDR
