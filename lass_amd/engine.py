"""Thin torch-tensor front end over the C-ABI: owns one `lass_ctx`, hands device pointers and the current HIP stream
to liblass_hip.  torch is plumbing here (device memory, streams); every number is produced by the HIP kernels."""
from __future__ import annotations

from collections import namedtuple
from ctypes import byref, c_char_p, c_double, c_int, c_int64, c_size_t, c_void_p
from typing import Dict, Optional

import numpy as np
import torch

from . import _alloc, _lib, arch, longform


def _ptr(t: Optional[torch.Tensor]):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _stream(device) -> c_void_p:
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


# The leading arguments of every export entry of the C layer, and the dry source's of the two remix entries, in the order of
# include/lass_hip.h under its names: built by keyword, handed over with *.
_ExportHead = namedtuple("_ExportHead", "planes row_stride plane_stride B channels L_in up down taps n_taps")
_DryArgs = namedtuple("_DryArgs", "dry dry_row_stride_bytes dry_encoding amount")


class Engine:
    """One context per (process, device)."""

    def __init__(self, device="cuda:0", multistft=None, stft=None):
        """multistft: None = ResUNet30 (models/resunet.py); (n_fft, win_lengths, mask_window) = the multi-resolution-STFT
        separator (lass_create_multistft).  stft: ResUNet30's STFT geometry (n_fft, hop) - None or (1024, 160) = the reference's
        16 kHz layout, (2048, 320) = the same network at 32 kHz (lass_create_stft; arch.STFT_GEOMETRIES).  Every method takes
        its frame counts, bucket and length limits from it (`n_fft`, `hop`)."""
        if stft is not None:
            if multistft is not None:
                raise ValueError("stft=(n_fft, hop) is ResUNet30's geometry: the multi-STFT model has its own (n_fft, hop 160)")
            stft = arch.check_stft(*stft)
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LassError("lass_amd computes on an MI355X only (device must be a cuda/HIP device)")
        if not torch.cuda.is_available():
            raise _lib.LassError("no HIP device visible to torch; lass_amd has no CPU fallback")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        h = c_void_p()
        self.multistft = None
        if multistft is None:
            rc = self.lib.lass_create(byref(h), idx) if stft is None else self.lib.lass_create_stft(byref(h), idx, stft[0], stft[1])
        else:
            n_fft, wins, mask_window = int(multistft[0]), [int(w) for w in multistft[1]], int(multistft[2])
            rc = self.lib.lass_create_multistft(byref(h), idx, n_fft, len(wins), (c_int * len(wins))(*wins), mask_window)
            self.multistft = (n_fft, tuple(wins), mask_window)
        if rc < 0:
            raise _lib.LassError(f"lass_create failed ({rc}): {self.lib.lass_last_error(None).decode()}")
        self.ctx = h
        n_fft, hop = c_int(), c_int()
        _lib.check(self.ctx, self.lib.lass_stft_geometry(self.ctx, byref(n_fft), byref(hop)), "lass_stft_geometry")
        self.n_fft, self.hop = n_fft.value, hop.value  # the context's word: (1024, 160), (2048, 320), or the multi-STFT model's
        self._stage_n_fft = self.n_fft if multistft is None else arch.N_FFT  # stft_magphase / istft (lass_stft_magphase)
        self.n_branches = 1 if multistft is None else len(self.multistft[1])
        self._ws_buf: Optional[torch.Tensor] = None  # ONE workspace, as large as the largest (B, L) seen so far
        self._ws_last = None                         # (B, L) of the last call that used it (its intermediates live there)
        self.ws_allocations = 0
        self._fade_bufs: Dict[int, torch.Tensor] = {}  # B -> fade flags int32 (B,2), beside _win_bufs
        self._win_bufs: Dict[int, tuple] = {}        # B -> (starts int64 (B), keep int32 (B,2), condition (B,512)): persistent
        self.finalized = False

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.lass_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ---- weights ---------------------------------------------------------------------------------------------
    def set_param(self, name: str, t) -> int:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        t = t.detach()
        if not t.is_floating_point():
            return 1  # num_batches_tracked & co: not used by inference
        t = t.to(torch.float32).contiguous()
        shape = (c_int64 * max(1, t.dim()))(*t.shape)
        if t.is_cuda:  # lass_set_param copies synchronously on the NULL stream: the source must be complete first
            torch.cuda.current_stream(t.device).synchronize()
        rc = self.lib.lass_set_param(self.ctx, name.encode(), _ptr(t), shape, t.dim(), 0)
        self.finalized = False
        return _lib.check(self.ctx, rc, f"lass_set_param({name})")

    COMPUTE_MODES = {"f32": 0, "bf16": 1, "bf16x3": 2}  # include/lass_hip.h: LASS_COMPUTE_*

    def load_state_dict(self, sd: Dict[str, object], compute_dtype: str = "f32"):
        for k, v in sd.items():
            self.set_param(k, v)
        self.finalize(compute_dtype)

    def finalize(self, compute_dtype: str = "f32"):
        """compute_dtype 'f32' (default; exact-f32 MFMA arithmetic) or 'bf16' (BASELINE configs[2]: 3x3 convs on the
        bf16 MFMA, f32 accumulate - reduced precision)."""
        mode = self.COMPUTE_MODES[compute_dtype]
        _lib.check(self.ctx, self.lib.lass_finalize(self.ctx, mode), "lass_finalize")
        self.finalized = True
        self.compute_dtype = compute_dtype

    # ---- hot path --------------------------------------------------------------------------------------------
    def workspace_bytes(self, B: int, L: int) -> int:
        n = c_size_t()
        _lib.check(self.ctx, self.lib.lass_workspace_bytes(self.ctx, B, L, byref(n)), "lass_workspace_bytes")
        return n.value

    def _workspace(self, B: int, L: int) -> torch.Tensor:
        """One buffer keyed on capacity: any (B, L) whose lass_workspace_bytes fits reuses it (lass_separate only needs
        workspace_bytes >= its plan), so the evaluator's ragged last batch neither frees and re-allocates gigabytes nor
        changes the workspace pointer the captured graph of the common batch is keyed on.  It grows when a larger shape
        arrives (the old buffer is released first: workspaces are GBs)."""
        need = self.workspace_bytes(B, L)
        if self._ws_buf is None or self._ws_buf.numel() < need:
            self._ws_buf = None
            self._ws_buf = _alloc.empty(need, dtype=torch.uint8, device=self.device)
            self.ws_allocations += 1
        else:
            _alloc.refill(self._ws_buf)  # under poison only, on the call's stream: a replayed graph meets fresh poison too
        self._ws_last = (B, L)
        return self._ws_buf

    def separate(self, mixture: torch.Tensor, condition: torch.Tensor, out: Optional[torch.Tensor] = None):
        """mixture (B,L) f32, condition (B,512) f32 on this device -> (B,L) f32."""
        assert mixture.dim() == 2 and condition.dim() == 2 and condition.shape == (mixture.shape[0], arch_cond())
        mixture = self._dev(mixture)
        condition = self._dev(condition)
        B, L = mixture.shape
        if out is None:
            out = _alloc.empty_like(mixture)
        elif (out.shape != mixture.shape or out.dtype != torch.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise _lib.LassError(f"out must be a contiguous float32 {tuple(mixture.shape)} tensor on {self.device}")
        ws = self._workspace(B, L)
        rc = self.lib.lass_separate(self.ctx, _ptr(mixture), _ptr(condition), _ptr(out), B, L, _ptr(ws), ws.numel(),
                                    _stream(self.device))
        _lib.check(self.ctx, rc, "lass_separate")
        return out

    def ragged_bucket(self, L: int):
        """(lo, hi): the lengths that may share a `separate_ragged` call with rows of L samples (lass_ragged_bucket)."""
        lo, hi = c_int(), c_int()
        if self.lib.lass_ragged_bucket(self.ctx, int(L), byref(lo), byref(hi)) < 0:
            raise _lib.LassError(f"lass_ragged_bucket: L = {L} is not longer than the reflect padding ({self.n_fft // 2})")
        return lo.value, hi.value

    def _ragged_lengths(self, lengths, B: int, L: int, checked: bool, what: str) -> torch.Tensor:
        """The lengths of a ragged call as a device int32 (B) tensor.  A Python sequence, numpy array or CPU tensor is checked
        against the bucket of L here and uploaded; a device tensor is taken as it is, and only with `checked=True` - the
        caller's word that it did the check (the library never reads the array; the kernels clamp)."""
        if torch.is_tensor(lengths) and lengths.is_cuda:
            if not checked:
                raise _lib.LassError(f"{what}: device lengths cannot be checked without a copy to the host: pass host "
                                     "lengths, or checked=True once you have checked them (Engine.ragged_bucket)")
            if lengths.device != self.device or lengths.dtype != torch.int32 or lengths.shape != (B,) or not lengths.is_contiguous():
                raise _lib.LassError(f"{what}: device lengths must be a contiguous int32 ({B},) tensor on {self.device}")
            return lengths
        host = np.asarray(lengths.numpy() if torch.is_tensor(lengths) else lengths)
        if host.shape != (B,) or not np.issubdtype(host.dtype, np.integer):
            raise _lib.LassError(f"{what}: lengths must be {B} integers")
        lo, hi = self.ragged_bucket(L)
        if host.min() < lo or host.max() > hi:
            raise _lib.LassError(f"{what}: lengths {int(host.min())} .. {int(host.max())} leave the bucket [{lo}, {hi}] of rows "
                                 f"of {L} samples: sort the clips into buckets first (lass_amd.ragged.plan_batches)")
        return torch.from_numpy(host.astype(np.int32)).to(self.device)

    def separate_ragged(self, mixture: torch.Tensor, lengths, condition: torch.Tensor, out: Optional[torch.Tensor] = None,
                        checked: bool = False):
        """Clips of different lengths in one call: mixture (B,L) f32 with clip b in mixture[b, :lengths[b]] (the rest of the
        row is never read), condition (B,512) -> (B,L) f32 with out[b, :lengths[b]] what `separate` gives for the clip alone
        and out[b, lengths[b]:] zero.  All lengths must lie in the bucket of L (`ragged_bucket`); see `_ragged_lengths` for
        how they are checked."""
        assert mixture.dim() == 2 and condition.dim() == 2 and condition.shape == (mixture.shape[0], arch_cond())
        mixture = self._dev(mixture)
        condition = self._dev(condition)
        B, L = mixture.shape
        lens = self._ragged_lengths(lengths, B, L, checked, "separate_ragged")
        if out is None:
            out = _alloc.empty_like(mixture)
        elif (out.shape != mixture.shape or out.dtype != torch.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise _lib.LassError(f"out must be a contiguous float32 {tuple(mixture.shape)} tensor on {self.device}")
        ws = self._workspace(B, L)
        rc = self.lib.lass_separate_ragged(self.ctx, _ptr(mixture), _ptr(lens), _ptr(condition), _ptr(out), B, L, _ptr(ws),
                                           ws.numel(), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_separate_ragged")
        return out

    # ---- long recordings: windows of one long row ----------------------------------------------------------------
    def window_buffers(self, B: int):
        """The engine's persistent index and condition buffers of a B-window call: (starts int64 (B), keep int32 (B,2),
        condition f32 (B,512)).  `separate_windows` stages host indices and a single condition here, so consecutive calls present
        the same pointers (and reach graph replay); a caller may also fill them itself with stream-ordered copies."""
        B = int(B)
        if B not in self._win_bufs:
            self._win_bufs[B] = (torch.zeros(B, dtype=torch.int64, device=self.device),
                                 torch.zeros(B, 2, dtype=torch.int32, device=self.device),
                                 torch.zeros(B, arch_cond(), dtype=torch.float32, device=self.device))
        return self._win_bufs[B]

    def fade_buffer(self, B: int) -> torch.Tensor:
        """The engine's persistent fade flags of a B-window call, int32 (B,2), beside `window_buffers`: groups that stage their
        flags here present the same pointer."""
        B = int(B)
        if B not in self._fade_bufs:
            self._fade_bufs[B] = torch.zeros(B, 2, dtype=torch.int32, device=self.device)
        return self._fade_bufs[B]

    def _fade_ramp(self, fade, ramp, W: int, what: str) -> torch.Tensor:
        """The ramp of a faded window call on the device, f32 (F) with 1 <= F <= W.  Keep it there between calls: a fresh upload
        is a fresh pointer, and no graph replay."""
        if fade is None or ramp is None:
            raise ValueError(f"{what}: fade and ramp go together")
        ramp = self._dev(torch.as_tensor(ramp))
        if ramp.dtype != torch.float32 or ramp.dim() != 1 or not ramp.is_contiguous() or not 1 <= ramp.numel() <= W:
            raise ValueError(f"{what}: ramp must be a contiguous 1-D float32 table of 1 to {W} weights")
        return ramp

    def _window_index(self, starts, keep, total: int, W: int, checked: bool, what: str, fade=None, F: int = 0):
        """starts / keep of a window call as device tensors (int64 (B), int32 (B,2)).  Python sequences (or numpy arrays, CPU
        tensors) are checked here - every window inside the recording, every keep inside its window, kept ranges disjoint
        (ValueError) - and staged into the engine's persistent buffers; device tensors are taken as they are, and only with
        `checked=True` (the library never reads them; the kernels clamp).  keep None (the front end keeps nothing): empty keeps.
        fade (a faded call with a ramp of F weights): B (fade_in, fade_out) pairs, given the way starts and keep are and returned
        as a third tensor, int32 (B,2); host flags are checked with the keeps (lass_amd.longform.check_keeps_faded: fade regions
        may meet in pairs) and staged into `fade_buffer`."""
        if keep is None:
            on_device = torch.is_tensor(starts) and starts.is_cuda
            keep = torch.zeros(len(starts), 2, dtype=torch.int32, device=self.device) if on_device else [(0, 0)] * len(starts)
        dev_s, dev_k = torch.is_tensor(starts) and starts.is_cuda, torch.is_tensor(keep) and keep.is_cuda
        dev_f = torch.is_tensor(fade) and fade.is_cuda
        if dev_s or dev_k or dev_f:
            if not (dev_s and dev_k and (dev_f or fade is None)):
                raise _lib.LassError(f"{what}: starts and keep (and fade) must all be device tensors or all host sequences")
            if not checked:
                raise _lib.LassError(f"{what}: device indices cannot be checked without a copy to the host: pass host "
                                     "sequences, or checked=True once you have checked them (lass_amd.longform.check_keeps)")
            B = starts.numel()
            if (starts.device != self.device or starts.dtype != torch.int64 or starts.dim() != 1 or not starts.is_contiguous()
                    or keep.device != self.device or keep.dtype != torch.int32 or keep.numel() != 2 * B or not keep.is_contiguous()):
                raise _lib.LassError(f"{what}: device indices must be contiguous int64 (B,) starts and int32 (B,2) keeps on "
                                     f"{self.device}")
            if fade is None:
                return starts, keep
            if fade.device != self.device or fade.dtype != torch.int32 or fade.numel() != 2 * B or not fade.is_contiguous():
                raise _lib.LassError(f"{what}: device fade flags must be a contiguous int32 (B,2) tensor on {self.device}")
            return starts, keep, fade
        hs = np.asarray(starts.numpy() if torch.is_tensor(starts) else starts)
        hk = np.asarray(keep.numpy() if torch.is_tensor(keep) else keep)
        B = hs.shape[0] if hs.ndim == 1 else 0
        if B < 1 or hk.size != 2 * B or not np.issubdtype(hs.dtype, np.integer) or not np.issubdtype(hk.dtype, np.integer):
            raise ValueError(f"{what}: starts must be B >= 1 integers and keep B (lo, hi) pairs of integers")
        hk = hk.reshape(B, 2)
        if fade is None:
            longform.check_keeps([(int(a), int(lo), int(hi)) for a, (lo, hi) in zip(hs, hk)], W, total)
        else:
            hf = np.asarray(fade.numpy() if torch.is_tensor(fade) else fade)
            if hf.size != 2 * B or not (np.issubdtype(hf.dtype, np.integer) or hf.dtype == np.bool_):
                raise ValueError(f"{what}: fade must be B (fade_in, fade_out) pairs of integers")
            hf = hf.reshape(B, 2).astype(np.int32)
            longform.check_keeps_faded([(int(a), int(lo), int(hi), int(fi), int(fo)) for a, (lo, hi), (fi, fo) in zip(hs, hk, hf)],
                                       W, total, F)
        buf_s, buf_k, _ = self.window_buffers(B)
        buf_s.copy_(torch.from_numpy(hs.astype(np.int64)))
        buf_k.copy_(torch.from_numpy(hk.astype(np.int32)))
        if fade is None:
            return buf_s, buf_k
        buf_f = self.fade_buffer(B)
        buf_f.copy_(torch.from_numpy(hf))
        return buf_s, buf_k, buf_f

    def separate_windows(self, recording: torch.Tensor, starts, keep, condition: torch.Tensor, window: int,
                         out: Optional[torch.Tensor] = None, checked: bool = False, fade=None, ramp=None) -> torch.Tensor:
        """B windows of ONE recording in one call (lass_separate_windows): recording (total,) f32; window b is
        recording[starts[b] : starts[b] + window], separated as that clip alone, and of its output only [lo_b, hi_b) =
        keep[b] is stored, at out[starts[b] + lo_b : starts[b] + hi_b].  Nothing else of `out` (total,) is touched: a fresh `out`
        is zero-filled, one passed in keeps its other samples.  condition (B,512), or (1,512) / (512,) for all windows (expanded
        into a persistent buffer).  See `_window_index` for how starts / keep are checked.
        fade, ramp (both or neither; lass_separate_windows_faded): B (fade_in, fade_out) flag pairs and the F ascending fade-in
        weights (`_window_index`, `_fade_ramp`).  The first F kept samples of a window that fades in and the last F of one that fades out are
        not stored but weighted and ADDED to `out`, which must hold 0 there before the first window reaches them (a fresh `out`
        does); everything else is stored as without fades, bit for bit."""
        if recording.dim() != 1:
            raise ValueError("separate_windows takes a 1-D recording")
        recording = self._dev(recording)
        total, W = recording.shape[0], int(window)
        faded = fade is not None or ramp is not None
        if faded:
            ramp = self._fade_ramp(fade, ramp, W, "separate_windows")
            idx_s, idx_k, idx_f = self._window_index(starts, keep, total, W, checked, "separate_windows", fade, ramp.numel())
        else:
            idx_s, idx_k = self._window_index(starts, keep, total, W, checked, "separate_windows")
        B = idx_s.numel()
        condition = self._dev(condition)
        if condition.numel() == arch_cond() and (B > 1 or condition.dim() == 1):
            cond = self.window_buffers(B)[2]
            cond.copy_(condition.reshape(1, -1).expand(B, -1))
        elif condition.shape == (B, arch_cond()):
            cond = condition
        else:
            raise ValueError(f"condition must be ({B}, {arch_cond()}), (1, {arch_cond()}) or ({arch_cond()},)")
        if out is None:
            out = torch.zeros_like(recording)
        elif (out.shape != recording.shape or out.dtype != torch.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise _lib.LassError(f"out must be a contiguous float32 {tuple(recording.shape)} tensor on {self.device}")
        ws = self._workspace(B, W)
        if faded:
            rc = self.lib.lass_separate_windows_faded(self.ctx, _ptr(recording), total, _ptr(idx_s), _ptr(idx_k), _ptr(idx_f), _ptr(ramp),
                                                      ramp.numel(), _ptr(cond), _ptr(out), B, W, _ptr(ws), ws.numel(),
                                                      _stream(self.device))
            _lib.check(self.ctx, rc, "lass_separate_windows_faded")
            return out
        rc = self.lib.lass_separate_windows(self.ctx, _ptr(recording), total, _ptr(idx_s), _ptr(idx_k), _ptr(cond), _ptr(out), B, W,
                                            _ptr(ws), ws.numel(), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_separate_windows")
        return out

    # ---- linked channels: one mask from a guide, applied to every plane ---------------------------
    MAX_LINKED_CHANNELS = 8  # include/lass_hip.h: LASS_MAX_LINKED_CHANNELS

    def _linked_io(self, guide: torch.Tensor, planes: torch.Tensor, out: Optional[torch.Tensor], zero: bool, what: str):
        """planes (C,) + guide.shape and the output of the same shape (a fresh one zero-filled where `zero`), both contiguous
        float32 on the engine's device, 1 <= C <= 8."""
        planes = self._dev(planes)
        if planes.dim() != guide.dim() + 1 or planes.shape[1:] != guide.shape or not 1 <= planes.shape[0] <= self.MAX_LINKED_CHANNELS:
            raise ValueError(f"{what}: planes must be (C,) + {tuple(guide.shape)} with 1 <= C <= {self.MAX_LINKED_CHANNELS}")
        if out is None:
            out = torch.zeros_like(planes) if zero else _alloc.empty_like(planes)
        elif (out.shape != planes.shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous()):
            raise _lib.LassError(f"out must be a contiguous float32 {tuple(planes.shape)} tensor on {self.device}")
        return planes, out

    def separate_ragged_linked(self, guide: torch.Tensor, lengths, planes: torch.Tensor, condition: torch.Tensor,
                               out: Optional[torch.Tensor] = None, checked: bool = False) -> torch.Tensor:
        """`separate_ragged` with linked channels (lass_separate_ragged_linked): guide (B,L) decides one mask per clip, which is
        applied to every plane of planes (C,B,L) -> (C,B,L); plane c does not depend on the others.  lengths as for
        `separate_ragged` (`_ragged_lengths`), or None: every clip is L samples long.  condition (B,512)."""
        assert guide.dim() == 2 and condition.dim() == 2 and condition.shape == (guide.shape[0], arch_cond())
        guide, condition = self._dev(guide), self._dev(condition)
        B, L = guide.shape
        lens = None if lengths is None else self._ragged_lengths(lengths, B, L, checked, "separate_ragged_linked")
        planes, out = self._linked_io(guide, planes, out, False, "separate_ragged_linked")
        ws = self._workspace(B, L)
        rc = self.lib.lass_separate_ragged_linked(self.ctx, _ptr(guide), _ptr(lens), _ptr(planes), B * L, planes.shape[0],
                                                  _ptr(condition), _ptr(out), B * L, B, L, _ptr(ws), ws.numel(), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_separate_ragged_linked")
        return out

    def separate_windows_linked(self, guide: torch.Tensor, planes: torch.Tensor, starts, keep, condition: torch.Tensor, window: int,
                                out: Optional[torch.Tensor] = None, checked: bool = False, fade=None, ramp=None) -> torch.Tensor:
        """`separate_windows` with linked channels (lass_separate_windows_linked): guide (total,) decides one mask per window,
        which is applied to that window of every row of planes (C,total) -> out (C,total).  starts, keep, condition, fade and
        ramp are `separate_windows`'s, the same for every plane; nothing of `out` outside the kept ranges is touched (a fresh
        `out` is zero-filled, which the fade regions need)."""
        if guide.dim() != 1:
            raise ValueError("separate_windows_linked takes a 1-D guide")
        guide = self._dev(guide)
        total, W = guide.shape[0], int(window)
        faded = fade is not None or ramp is not None
        idx_f = None
        if faded:
            ramp = self._fade_ramp(fade, ramp, W, "separate_windows_linked")
            idx_s, idx_k, idx_f = self._window_index(starts, keep, total, W, checked, "separate_windows_linked", fade, ramp.numel())
        else:
            idx_s, idx_k = self._window_index(starts, keep, total, W, checked, "separate_windows_linked")
        B = idx_s.numel()
        condition = self._dev(condition)
        if condition.numel() == arch_cond() and (B > 1 or condition.dim() == 1):
            cond = self.window_buffers(B)[2]
            cond.copy_(condition.reshape(1, -1).expand(B, -1))
        elif condition.shape == (B, arch_cond()):
            cond = condition
        else:
            raise ValueError(f"condition must be ({B}, {arch_cond()}), (1, {arch_cond()}) or ({arch_cond()},)")
        planes, out = self._linked_io(guide, planes, out, True, "separate_windows_linked")
        ws = self._workspace(B, W)
        rc = self.lib.lass_separate_windows_linked(self.ctx, _ptr(guide), total, _ptr(idx_s), _ptr(idx_k), _ptr(idx_f),
                                                   _ptr(ramp if faded else None), ramp.numel() if faded else 0, _ptr(planes), total,
                                                   planes.shape[0], _ptr(cond), _ptr(out), total, B, W, _ptr(ws), ws.numel(),
                                                   _stream(self.device))
        _lib.check(self.ctx, rc, "lass_separate_windows_linked")
        return out

    def _mask_pair(self, m_re: torch.Tensor, m_im: torch.Tensor, B: int, L: int, what: str):
        m_re, m_im = self._dev(m_re), self._dev(m_im)
        shape = (B, arch.frames_for(L, self.hop), self.n_fft // 2 + 1)
        if tuple(m_re.shape) != shape or tuple(m_im.shape) != shape:
            raise ValueError(f"{what}: the mask must be two {shape} tensors")
        return m_re, m_im, _alloc.empty(shape, dtype=torch.float32, device=self.device), _alloc.empty(shape, dtype=torch.float32, device=self.device)

    def masked_stft(self, plane: torch.Tensor, m_re: torch.Tensor, m_im: torch.Tensor, lengths=None, checked: bool = False):
        """The per-channel stage of the linked calls (lass_masked_stft): plane (B,L) and the complex mask m_re, m_im
        (B,T,n_fft/2+1) -> (y_re, y_im), Y = STFT(plane) * M as four float32 products and two sums, each rounded once.  lengths:
        as for `front_end_ragged`, or None (dense); rows beyond a ragged clip's own frames are zero."""
        plane = self._dev(plane)
        B, L = plane.shape
        lens = None if lengths is None else self._ragged_lengths(lengths, B, L, checked, "masked_stft")
        m_re, m_im, y_re, y_im = self._mask_pair(m_re, m_im, B, L, "masked_stft")
        rc = self.lib.lass_masked_stft(self.ctx, _ptr(plane), _ptr(lens), B, L, _ptr(m_re), _ptr(m_im), _ptr(y_re), _ptr(y_im),
                                       _stream(self.device))
        _lib.check(self.ctx, rc, "lass_masked_stft")
        return y_re, y_im

    def masked_stft_windows(self, recording: torch.Tensor, starts, window: int, m_re: torch.Tensor, m_im: torch.Tensor,
                            checked: bool = False):
        """`masked_stft` of the windows recording[starts[b] : starts[b] + window] of a 1-D recording (lass_masked_stft_windows)."""
        recording = self._dev(recording)
        total, W = recording.shape[0], int(window)
        idx_s, _ = self._window_index(starts, None, total, W, checked, "masked_stft_windows")
        B = idx_s.numel()
        m_re, m_im, y_re, y_im = self._mask_pair(m_re, m_im, B, W, "masked_stft_windows")
        rc = self.lib.lass_masked_stft_windows(self.ctx, _ptr(recording), total, _ptr(idx_s), B, W, _ptr(m_re), _ptr(m_im), _ptr(y_re),
                                               _ptr(y_im), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_masked_stft_windows")
        return y_re, y_im

    def _dev(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self.device:
            raise _lib.LassError(f"tensor on {t.device}, engine on {self.device}")
        if t.dtype != torch.float32:
            raise _lib.LassError("float32 tensors only")
        return t.contiguous()

    # ---- stage entry points (parity tests) -------------------------------------------------------------------
    def stft_magphase(self, wav: torch.Tensor, want_complex: bool = False):
        wav = self._dev(wav)
        B, L = wav.shape
        T = arch.frames_for(L, self.hop)
        mk = lambda: _alloc.empty(B, T, self._stage_n_fft // 2 + 1, dtype=torch.float32, device=self.device)  # noqa: E731
        mag, cos, sin = mk(), mk(), mk()
        re, im = (mk(), mk()) if want_complex else (None, None)
        rc = self.lib.lass_stft_magphase(self.ctx, _ptr(wav), B, L, _ptr(mag), _ptr(cos), _ptr(sin), _ptr(re),
                                         _ptr(im), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_stft_magphase")
        return (mag, cos, sin, re, im) if want_complex else (mag, cos, sin)

    def multi_stft(self, wav: torch.Tensor, win_lengths, hop: int = arch.HOP):
        """(B,L) -> {win: (mag, cos, sin)} each (B,1,T,win//2+1): every analysis window in ONE launch."""
        wav = self._dev(wav)
        B, L = wav.shape
        T = 1 + L // hop
        wins = [int(w) for w in win_lengths]
        n = len(wins)
        outs = {w: tuple(_alloc.empty(B, 1, T, w // 2 + 1, dtype=torch.float32, device=self.device) for _ in range(3))
                for w in wins}
        arr = lambda i: (c_void_p * n)(*[outs[w][i].data_ptr() for w in wins])  # noqa: E731
        rc = self.lib.lass_multi_stft(self.ctx, _ptr(wav), B, L, hop, n, (c_int * n)(*wins), arr(0), arr(1), arr(2),
                                      _stream(self.device))
        _lib.check(self.ctx, rc, "lass_multi_stft")
        return outs

    def istft(self, real: torch.Tensor, imag: torch.Tensor, length: int):
        real, imag = self._dev(real), self._dev(imag)
        B, T, F = real.shape
        assert F == self._stage_n_fft // 2 + 1 and imag.shape == real.shape
        wav = _alloc.empty(B, length, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_istft(self.ctx, _ptr(real), _ptr(imag), B, T, length, _ptr(wav), None, _stream(self.device))
        _lib.check(self.ctx, rc, "lass_istft")
        return wav

    def film_width(self) -> int:
        return self.lib.lass_film_width(self.ctx)

    def film_offset(self, site: str) -> int:
        return self.lib.lass_film_offset(self.ctx, site.encode())

    def film(self, cond: torch.Tensor, raw: bool = False) -> torch.Tensor:
        cond = self._dev(cond)
        B = cond.shape[0]
        out = _alloc.empty(B, self.film_width(), dtype=torch.float32, device=self.device)
        fn = self.lib.lass_film_raw if raw else self.lib.lass_film
        _lib.check(self.ctx, fn(self.ctx, _ptr(cond), B, _ptr(out), _stream(self.device)), "lass_film")
        return out

    def convblock(self, prefix: str, x: torch.Tensor, shift: torch.Tensor, cout: int) -> torch.Tensor:
        x = self._dev(x)
        B, _cin, H, W = x.shape
        y = _alloc.empty(B, cout, H, W, dtype=torch.float32, device=self.device)
        scratch = _alloc.empty_like(y)
        rc = self.lib.lass_convblock(self.ctx, prefix.encode(), _ptr(x), B, H, W, _ptr(shift), _ptr(y), _ptr(scratch),
                                     _stream(self.device))
        _lib.check(self.ctx, rc, "lass_convblock")
        return y

    def encoder_block(self, name: str, x: torch.Tensor, shift: torch.Tensor, cout: int, down):
        """One encoder block incl. its (fused) avg-pool: x (B,Cin,H,W) -> (y (B,Cout,H,W), pool or None)."""
        x = self._dev(x)
        B, _cin, H, W = x.shape
        y = _alloc.empty(B, cout, H, W, dtype=torch.float32, device=self.device)
        pool = (_alloc.empty(B, cout, H // down[0], W // down[1], dtype=torch.float32, device=self.device)
                if tuple(down) != (1, 1) else None)
        scratch = _alloc.empty_like(y)
        rc = self.lib.lass_encoder_block(self.ctx, name.encode(), _ptr(x), B, H, W, _ptr(shift), _ptr(y), _ptr(pool),
                                         _ptr(scratch), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_encoder_block")
        return y, pool

    def front_end(self, wav: torch.Tensor, out=None):
        """(B,L) -> (mag, cos, sin (B,T,n_fft/2+1), x0): STFT + bn0 + T-pad + F-crop (resunet.py:533-552).
        x0 is (B,Tpad,n_fft/2) for ResUNet30 (512 bins, 1024 at the (2048, 320) geometry) and (n_windows,B,Tpad,1024) for the multi-STFT model (mag/cos/sin are then the
        mask window's).  `out` = a (mag, cos, sin, x0) tuple of an earlier call to write into (no allocation in this call)."""
        wav = self._dev(wav)
        B, L = wav.shape
        T = arch.frames_for(L, self.hop)
        nb = self.n_fft // 2 + 1
        shape = (B, arch.padded_frames(T), nb - 1)
        x0_shape = (self.n_branches,) + shape if self.multistft else shape
        if out is not None:
            mag, cos, sin, x0 = (self._dev(t) for t in out)
            if not (mag.shape == cos.shape == sin.shape == (B, T, nb) and tuple(x0.shape) == tuple(x0_shape)
                    and all(t.dtype == torch.float32 and t.is_contiguous() for t in (mag, cos, sin, x0))):
                raise ValueError("front_end: `out` does not match this input's shapes")
        else:
            mk = lambda: _alloc.empty(B, T, nb, dtype=torch.float32, device=self.device)  # noqa: E731
            mag, cos, sin = mk(), mk(), mk()
            x0 = _alloc.empty(x0_shape, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_front_end(self.ctx, _ptr(wav), B, L, _ptr(mag), _ptr(cos), _ptr(sin), _ptr(x0),
                                     _stream(self.device))
        _lib.check(self.ctx, rc, "lass_front_end")
        return mag, cos, sin, x0

    def front_end_ragged(self, wav: torch.Tensor, lengths, checked: bool = False):
        """`front_end` with a length per clip (lass_front_end_ragged): same shapes as for B clips of L samples; beyond clip b's
        own 1 + lengths[b] // hop frames x0 and mag / cos / sin are zero."""
        wav = self._dev(wav)
        B, L = wav.shape
        lens = self._ragged_lengths(lengths, B, L, checked, "front_end_ragged")
        T = arch.frames_for(L, self.hop)
        nb = self.n_fft // 2 + 1
        shape = (B, arch.padded_frames(T), nb - 1)
        mk = lambda: _alloc.empty(B, T, nb, dtype=torch.float32, device=self.device)  # noqa: E731
        mag, cos, sin = mk(), mk(), mk()
        x0 = _alloc.empty((self.n_branches,) + shape if self.multistft else shape, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_front_end_ragged(self.ctx, _ptr(wav), _ptr(lens), B, L, _ptr(mag), _ptr(cos), _ptr(sin), _ptr(x0),
                                            _stream(self.device))
        _lib.check(self.ctx, rc, "lass_front_end_ragged")
        return mag, cos, sin, x0

    def istft_ragged(self, real: torch.Tensor, imag: torch.Tensor, lengths, length: int, n_fft: Optional[int] = None,
                     win_length: Optional[int] = None, checked: bool = False):
        """`istft_nfft` with a length per clip (lass_istft_ragged): real, imag (B, 1 + length // hop, n_fft/2+1) -> (B, length),
        clip b from its own first 1 + lengths[b] // hop frames, zero from lengths[b] on."""
        real, imag = self._dev(real), self._dev(imag)
        n_fft = self.n_fft if n_fft is None else int(n_fft)
        win_length = n_fft if win_length is None else int(win_length)
        B, T, F = real.shape
        assert F == n_fft // 2 + 1 and imag.shape == real.shape
        if n_fft != self.n_fft:
            raise _lib.LassError("istft_ragged: the bucket is the context's (n_fft must be the engine's)")
        lens = self._ragged_lengths(lengths, B, length, checked, "istft_ragged")
        wav = _alloc.empty(B, length, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_istft_ragged(self.ctx, _ptr(real), _ptr(imag), _ptr(lens), B, T, length, n_fft, win_length, _ptr(wav),
                                        _stream(self.device))
        _lib.check(self.ctx, rc, "lass_istft_ragged")
        return wav

    def front_end_windows(self, recording: torch.Tensor, starts, window: int, checked: bool = False):
        """`front_end` of the windows recording[starts[b] : starts[b] + window] of a 1-D recording (lass_front_end_windows):
        shapes as for B clips of `window` samples, row b what `front_end` gives for the gathered window."""
        recording = self._dev(recording)
        total, W = recording.shape[0], int(window)
        B = len(starts)
        idx_s, _ = self._window_index(starts, None, total, W, checked, "front_end_windows")
        T = arch.frames_for(W, self.hop)
        nb = self.n_fft // 2 + 1
        shape = (B, arch.padded_frames(T), nb - 1)
        mk = lambda: _alloc.empty(B, T, nb, dtype=torch.float32, device=self.device)  # noqa: E731
        mag, cos, sin = mk(), mk(), mk()
        x0 = _alloc.empty((self.n_branches,) + shape if self.multistft else shape, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_front_end_windows(self.ctx, _ptr(recording), total, _ptr(idx_s), B, W, _ptr(mag), _ptr(cos), _ptr(sin),
                                             _ptr(x0), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_front_end_windows")
        return mag, cos, sin, x0

    def istft_windows(self, real: torch.Tensor, imag: torch.Tensor, starts, keep, window: int, out: torch.Tensor,
                      n_fft: Optional[int] = None, win_length: Optional[int] = None, checked: bool = False, fade=None,
                      ramp=None) -> torch.Tensor:
        """`istft_nfft` for windows (lass_istft_windows): real, imag (B, 1 + window // hop, n_fft/2+1); of window b's `window`
        samples only keep[b] = [lo, hi) is stored, at out[starts[b] + lo : starts[b] + hi] of the 1-D `out`.  fade, ramp: as for
        `separate_windows` (lass_istft_windows_faded); `out` holds 0 in the fade regions beforehand."""
        real, imag, out = self._dev(real), self._dev(imag), self._dev(out)
        n_fft = self.n_fft if n_fft is None else int(n_fft)
        win_length = n_fft if win_length is None else int(win_length)
        B, T, F = real.shape
        assert F == n_fft // 2 + 1 and imag.shape == real.shape and out.dim() == 1
        total, W = out.shape[0], int(window)
        faded = fade is not None or ramp is not None
        if faded:
            ramp = self._fade_ramp(fade, ramp, W, "istft_windows")
            idx_s, idx_k, idx_f = self._window_index(starts, keep, total, W, checked, "istft_windows", fade, ramp.numel())
        else:
            idx_s, idx_k = self._window_index(starts, keep, total, W, checked, "istft_windows")
        if idx_s.numel() != B:
            raise ValueError(f"istft_windows: {B} spectra, {idx_s.numel()} windows")
        if faded:
            rc = self.lib.lass_istft_windows_faded(self.ctx, _ptr(real), _ptr(imag), _ptr(idx_s), _ptr(idx_k), _ptr(idx_f), _ptr(ramp),
                                                   ramp.numel(), total, B, T, W, n_fft, win_length, _ptr(out), _stream(self.device))
            _lib.check(self.ctx, rc, "lass_istft_windows_faded")
            return out
        rc = self.lib.lass_istft_windows(self.ctx, _ptr(real), _ptr(imag), _ptr(idx_s), _ptr(idx_k), total, B, T, W, n_fft,
                                         win_length, _ptr(out), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_istft_windows")
        return out

    def stft_components(self, wav: torch.Tensor, n_fft: int, win_lengths, hop: int = arch.HOP):
        """(B,L) -> {win: (mag, cos, sin)} each (B,1,T,n_fft//2+1): `calculate_stft_components` at a COMMON n_fft for
        every win_length (zero-padded windows), one launch."""
        wav = self._dev(wav)
        B, L = wav.shape
        T = 1 + L // hop
        wins = [int(w) for w in win_lengths]
        n = len(wins)
        outs = {w: tuple(_alloc.empty(B, 1, T, n_fft // 2 + 1, dtype=torch.float32, device=self.device) for _ in range(3))
                for w in wins}
        arr = lambda i: (c_void_p * n)(*[outs[w][i].data_ptr() for w in wins])  # noqa: E731
        rc = self.lib.lass_stft_components(self.ctx, _ptr(wav), B, L, n_fft, hop, n, (c_int * n)(*wins), arr(0), arr(1),
                                           arr(2), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_stft_components")
        return outs

    def istft_nfft(self, real: torch.Tensor, imag: torch.Tensor, length: int, n_fft: int, win_length: int):
        real, imag = self._dev(real), self._dev(imag)
        B, T, F = real.shape
        assert F == n_fft // 2 + 1 and imag.shape == real.shape
        wav = _alloc.empty(B, length, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_istft_nfft(self.ctx, _ptr(real), _ptr(imag), B, T, length, n_fft, win_length, _ptr(wav),
                                      _stream(self.device))
        _lib.check(self.ctx, rc, "lass_istft_nfft")
        return wav

    def separate_components(self, mags, cos_mask: torch.Tensor, sin_mask: torch.Tensor, condition: torch.Tensor,
                            length: int) -> torch.Tensor:
        """Precomputed analysis in (the multi-STFT wrapper's input form): mags = [ (B,T,F) per analysis window in the
        context's order ], cos / sin of the mask window -> waveform (B, length)."""
        mags = [self._dev(m) for m in mags]
        cos_mask, sin_mask, condition = self._dev(cos_mask), self._dev(sin_mask), self._dev(condition)
        B, T, F = mags[0].shape
        if len(mags) != self.n_branches or any(m.shape != (B, T, F) for m in mags) or F != self.n_fft // 2 + 1 \
                or cos_mask.shape != (B, T, F) or sin_mask.shape != (B, T, F) or T != arch.frames_for(length, self.hop) \
                or condition.shape != (B, arch_cond()):
            raise _lib.LassError("separate_components: inconsistent shapes")
        out = _alloc.empty(B, length, dtype=torch.float32, device=self.device)
        ws = self._workspace(B, length)
        arr = (c_void_p * len(mags))(*[m.data_ptr() for m in mags])
        rc = self.lib.lass_separate_components(self.ctx, arr, _ptr(cos_mask), _ptr(sin_mask), _ptr(condition), _ptr(out),
                                               B, length, _ptr(ws), ws.numel(), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_separate_components")
        return out

    def workspace_tensor(self, name: str, B: int, L: int) -> torch.Tensor:
        """View of a named intermediate that the last `separate` of shape (B, L) left in the workspace (f32 mode)."""
        off = c_size_t()
        shape, strides = (c_int64 * 4)(), (c_int64 * 4)()
        rc = self.lib.lass_workspace_tensor(self.ctx, B, L, name.encode(), byref(off), shape, strides)
        if rc == -3:  # LASS_ERR_STATE
            raise _lib.LassError(f"lass_workspace_tensor: the last separation of {B} clips ran as two half-batches (the workspace "
                                 "holds two half-batch layouts): tap after an eager call (set_graph_replay(False)), with "
                                 "LASS_SPLIT=0, or with a batch below 8")
        if rc < 0:
            raise _lib.LassError(f"lass_workspace_tensor: unknown tensor '{name}' or bad shape")
        ws = self._ws_buf if self._ws_last == (B, L) else None
        if ws is None:
            raise _lib.LassError("the workspace does not hold a run of that shape: call separate(B, L) first")
        assert off.value % 4 == 0
        flat = ws.view(torch.float32)
        return flat.as_strided(tuple(shape), tuple(strides), off.value // 4)

    def upconv(self, name: str, x: torch.Tensor, shift: torch.Tensor, cout: int, up) -> torch.Tensor:
        x = self._dev(x)
        B, _cin, h, w = x.shape
        y = _alloc.empty(B, cout, h * up[0], w * up[1], dtype=torch.float32, device=self.device)
        rc = self.lib.lass_upconv(self.ctx, name.encode(), _ptr(x), B, h, w, _ptr(shift), _ptr(y),
                                  _stream(self.device))
        _lib.check(self.ctx, rc, "lass_upconv")
        return y

    def mask_apply(self, x12, mag, cos, sin):
        x12, mag, cos, sin = map(self._dev, (x12, mag, cos, sin))
        B, C, Tp, F = x12.shape
        T = mag.shape[1]
        assert C == 32 and F == self.n_fft // 2
        o_re = _alloc.empty_like(mag)
        o_im = _alloc.empty_like(mag)
        rc = self.lib.lass_mask_apply(self.ctx, _ptr(x12), _ptr(mag), _ptr(cos), _ptr(sin), B, T, Tp, _ptr(o_re),
                                      _ptr(o_im), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_mask_apply")
        return o_re, o_im

    def sdr_stats(self, ref: torch.Tensor, est: torch.Tensor) -> torch.Tensor:
        """(B,L),(B,L) f32 -> (B,6) f64 sums (see include/lass_hip.h)."""
        ref, est = self._dev(ref), self._dev(est)
        B, L = ref.shape
        stats = _alloc.empty(B, 6, dtype=torch.float64, device=self.device)
        rc = self.lib.lass_sdr_stats(self.ctx, _ptr(ref), _ptr(est), B, L, _ptr(stats), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_sdr_stats")
        return stats

    def mix_at_snr(self, source: torch.Tensor, noise: torch.Tensor, snr_db: torch.Tensor, out: Optional[torch.Tensor] = None,
                   scratch: Optional[torch.Tensor] = None):
        """dcase_evaluator.py:77-89 on the device.  source (B,L) is scaled IN PLACE when the mixture needs declipping;
        returns the mixture (B,L) (`out` / `scratch` (B,4) f64: caller-kept buffers, nothing allocated here)."""
        source, noise, snr_db = self._dev(source), self._dev(noise), self._dev(snr_db)
        B, L = source.shape
        assert noise.shape == source.shape and snr_db.shape == (B,)
        mixture = _alloc.empty_like(source) if out is None else self._dev(out)
        assert mixture.shape == source.shape and mixture.is_contiguous() and mixture.dtype == torch.float32
        if scratch is None:
            scratch = _alloc.empty(B, 4, dtype=torch.float64, device=self.device)
        assert scratch.dtype == torch.float64 and scratch.numel() >= 4 * B and scratch.is_contiguous()
        rc = self.lib.lass_mix_at_snr(self.ctx, _ptr(source), _ptr(noise), _ptr(snr_db), _ptr(mixture), B, L,
                                      _ptr(scratch), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_mix_at_snr")
        return mixture

    def decode_resample(self, raw_u8: torch.Tensor, frames: int, channels: int, encoding: str, rate_in: int, rate_out: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """librosa.load(path, sr=rate_out, mono=True) behind the file read (dcase_evaluator.py:73-74), on the device: raw_u8
        (B, row bytes) uint8 - each row a WAV data chunk of `frames` frames x `channels` samples, encoding "pcm16" / "pcm32" /
        "f32", rows a multiple of 4 bytes apart - -> (B, ceil(frames * up / down)) float32 mono at rate_out (`out`: written
        in place).  The filter is lass_amd.resample.design_taps; a ratio beyond the kernel's tap cap raises LassError
        (resample.within_cap tells beforehand)."""
        return self._decode_resample(raw_u8, frames, channels, encoding, rate_in, rate_out, out, False)

    def decode_resample_planar(self, raw_u8: torch.Tensor, frames: int, channels: int, encoding: str, rate_in: int, rate_out: int,
                               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`decode_resample` without the down-mix: -> (B, channels, ceil(frames * up / down)) float32, plane c of row b bit-identical
        to `decode_resample` of a mono payload holding that channel alone (lass_decode_resample_planar)."""
        return self._decode_resample(raw_u8, frames, channels, encoding, rate_in, rate_out, out, True)

    def _decode_resample(self, raw_u8, frames, channels, encoding, rate_in, rate_out, out, planar: bool) -> torch.Tensor:
        from . import resample as rs
        if raw_u8.dim() == 1:
            raw_u8 = raw_u8[None]
        if raw_u8.device != self.device or raw_u8.dtype != torch.uint8 or raw_u8.dim() != 2 or raw_u8.stride(1) != 1:
            raise _lib.LassError(f"raw_u8 must be a (B, bytes) uint8 tensor on {self.device} with contiguous rows")
        if encoding not in rs.ENCODINGS:
            raise _lib.LassError(f"encoding must be one of {sorted(rs.ENCODINGS)}")
        B = raw_u8.shape[0]
        if raw_u8.shape[1] < int(frames) * int(channels) * rs.SAMPLE_BYTES[encoding]:
            raise _lib.LassError("raw_u8 rows are shorter than frames x channels samples")
        up, down = rs.ratio(rate_in, rate_out)
        L_out = rs.out_len(frames, up, down)
        taps = self._taps(rate_in, rate_out, "wavio.read_wav")
        shape = (B, int(channels), L_out) if planar else (B, L_out)
        if out is None:
            out = _alloc.empty(shape, dtype=torch.float32, device=self.device)
        elif (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise _lib.LassError(f"out must be a contiguous float32 {shape} tensor on {self.device}")
        stride = raw_u8.stride(0) if B > 1 else (raw_u8.shape[1] + 3) // 4 * 4  # (one row: no stride to honour)
        name = "lass_decode_resample_planar" if planar else "lass_decode_resample"
        rc = getattr(self.lib, name)(self.ctx, _ptr(raw_u8), stride, B, int(frames), int(channels), rs.ENCODINGS[encoding], up, down,
                                     _ptr(taps), 1 if taps is None else taps.numel(), _ptr(out), L_out, _stream(self.device))
        _lib.check(self.ctx, rc, name)
        return out

    def _taps(self, rate_in: int, rate_out: int, host: str):
        """The filter of the ratio on the device, None where there is none; a ratio beyond the kernel's tap cap raises LassError,
        which names `host`, the host function to use instead."""
        from . import resample as rs
        up, down = rs.ratio(rate_in, rate_out)
        if (up, down) == (1, 1):
            return None
        if not rs.within_cap(up, down):
            raise _lib.LassError(f"resampling {rate_in} -> {rate_out} Hz needs {rs.n_taps(up, down)} taps, over the device "
                                 f"kernel's cap of {rs.MAX_TAPS}: resample on the host ({host})")
        return rs.device_taps(up, down, self.device)

    def resample(self, x: torch.Tensor, rate_in: int, rate_out: int) -> torch.Tensor:
        """(B, L) or (L,) float32 at rate_in -> float32 at rate_out: the mono float32 case of `decode_resample`."""
        x = self._dev(x)
        one = x.dim() == 1
        x = x[None] if one else x
        y = self.decode_resample(x.view(torch.uint8), x.shape[1], 1, "f32", rate_in, rate_out)
        return y[0] if one else y

    def _planes(self, planes: torch.Tensor):
        """(planes as (B, C, L), row stride, plane stride) of a (B, C, L) or (C, L) float32 tensor with contiguous samples."""
        if planes.dim() == 2:
            planes = planes[None]
        if planes.device != self.device or planes.dtype != torch.float32 or planes.dim() != 3 or planes.stride(2) != 1:
            raise _lib.LassError(f"planes must be a (B, C, L) or (C, L) float32 tensor on {self.device} with contiguous samples")
        B, C, L = planes.shape
        plane_stride = planes.stride(1) if C > 1 else L                      # (one plane, one row: no stride to honour)
        row_stride = planes.stride(0) if B > 1 else (C - 1) * plane_stride + L
        return planes, row_stride, plane_stride

    def _export_plan(self, planes, rate_in: int, rate_out: int, frames_out, encoding: Optional[str] = None):
        """What the export methods share, with their refusals in their order: (head, B, C, frames_out) - head the leading arguments
        of every export entry of the C layer (planes, row stride, plane stride, B, C, L, up, down, taps, n_taps; taps NULL and 1
        without a filter), frames_out defaulted to its ceiling ceil(L * up / down) and held under it."""
        from . import resample as rs
        planes, row_stride, plane_stride = self._planes(planes)
        if encoding is not None and encoding not in rs.ENCODINGS:
            raise _lib.LassError(f"encoding must be one of {sorted(rs.ENCODINGS)}")
        B, C, L = planes.shape
        up, down = rs.ratio(rate_in, rate_out)
        ceiling = rs.out_len(L, up, down)
        frames_out = ceiling if frames_out is None else int(frames_out)
        if not 1 <= frames_out <= ceiling:
            raise _lib.LassError(f"frames_out must lie in 1 ... ceil(L * up / down) = {ceiling}")
        taps = self._taps(rate_in, rate_out, "wavio.write_wav_*")
        head = _ExportHead(planes=_ptr(planes), row_stride=row_stride, plane_stride=plane_stride, B=B, channels=C, L_in=L, up=up,
                           down=down, taps=_ptr(taps), n_taps=1 if taps is None else taps.numel())
        return head, B, C, frames_out

    def _per_row(self, name: str, t: torch.Tensor, B: int, dtype) -> None:
        """Refuse `name` unless it is a contiguous (B,) tensor of dtype on the device."""
        if tuple(t.shape) != (B,) or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise _lib.LassError(f"{name} must be a contiguous {str(dtype).split('.')[-1]} ({B},) tensor on {self.device}")

    def _payload_rows(self, name: str, t: torch.Tensor, B: int, row_bytes: int) -> int:
        """Refuse `name` unless it is a (B, >= row_bytes) uint8 tensor on the device with contiguous rows; its row stride in bytes."""
        if (t.dim() != 2 or t.shape[0] != B or t.shape[1] < row_bytes or t.dtype != torch.uint8 or t.device != self.device
                or t.stride(1) != 1):
            raise _lib.LassError(f"{name} must be a ({B}, >= {row_bytes}) uint8 tensor on {self.device} with contiguous rows")
        return t.stride(0) if B > 1 else (row_bytes + 3) // 4 * 4            # (one row: no stride to honour)

    def _encode_tail(self, B: int, row_bytes: int, out, clipped, gain):
        """The trailing arguments of the encode entries, checked: (out, allocated if None; its row stride)."""
        if out is None:
            out = _alloc.empty(B, (row_bytes + 3) // 4 * 4, dtype=torch.uint8, device=self.device)
        out_stride = self._payload_rows("out", out, B, row_bytes)
        if clipped is not None:
            self._per_row("clipped", clipped, B, torch.int32)
        if gain is not None:
            self._per_row("gain", gain, B, torch.float32)
        return out, out_stride

    def resample_encode(self, planes: torch.Tensor, rate_in: int, rate_out: int, encoding: str, frames_out: Optional[int] = None,
                        out: Optional[torch.Tensor] = None, clipped: Optional[torch.Tensor] = None,
                        gain: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The export side of `decode_resample_planar`, on the device: planes (B, C, L) or (C, L) float32 at rate_in (any strides
        with contiguous samples; C 1 ... 8) -> (B, frames_out * C * sample bytes) uint8, each row a WAV data chunk at rate_out
        ("pcm16" / "pcm32" / "f32", frames interleaved) as wavio.write_wav_* would write the resampled planes.  frames_out (default
        and at most ceil(L * up / down)) truncates.  `out`: a (B, >= row bytes) uint8 tensor written in place, rows a multiple of 4
        bytes apart, bytes past a row's end left alone; `clipped`: (B,) int32 counters, zero-filled by the caller, that receive
        the number of PCM samples the clip changed.  `gain`: (B,) float32 on the device; every resampled sample of row b is
        multiplied by gain[b] (one float32 rounding) before it is quantised (lass_resample_encode_gain; without it
        lass_resample_encode, as ever).  The filter is lass_amd.resample.design_taps; a ratio beyond the kernel's tap cap raises
        LassError (resample.within_cap tells beforehand)."""
        from . import resample as rs
        head, B, C, frames_out = self._export_plan(planes, rate_in, rate_out, frames_out, encoding)
        row_bytes = frames_out * C * rs.SAMPLE_BYTES[encoding]
        out, out_stride = self._encode_tail(B, row_bytes, out, clipped, gain)
        tail = (_ptr(out), out_stride, frames_out, _ptr(clipped), _stream(self.device))
        if gain is not None:
            rc = self.lib.lass_resample_encode_gain(self.ctx, *head, rs.ENCODINGS[encoding], _ptr(gain), *tail)
            _lib.check(self.ctx, rc, "lass_resample_encode_gain")
        else:
            rc = self.lib.lass_resample_encode(self.ctx, *head, rs.ENCODINGS[encoding], *tail)
            _lib.check(self.ctx, rc, "lass_resample_encode")
        return out[:, :row_bytes]

    def resample_peak(self, planes: torch.Tensor, rate_in: int, rate_out: int, frames_out: Optional[int] = None) -> torch.Tensor:
        """(B,) float32: max |y| over the channels and the first frames_out frames of each recording, y the very float32 values
        `resample_encode` of the same arguments quantises (lass_resample_peak); a NaN is skipped."""
        head, B, _, frames_out = self._export_plan(planes, rate_in, rate_out, frames_out)
        peak = _alloc.empty(B, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_resample_peak(self.ctx, *head, frames_out, _ptr(peak), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_resample_peak")
        return peak

    def _remix_args(self, planes, rate_in, rate_out, dry, dry_encoding, amount, frames_out):
        """What `remix_encode` and `remix_peak` share: `_export_plan`'s result and the dry source's arguments (dry, row stride,
        encoding, amount), with `resample_encode`'s refusals and those of the dry source."""
        from . import resample as rs
        head, B, C, frames_out = self._export_plan(planes, rate_in, rate_out, frames_out)
        if dry_encoding not in rs.ENCODINGS:
            raise _lib.LassError(f"dry_encoding must be one of {sorted(rs.ENCODINGS)}")
        if dry.dim() == 1:
            dry = dry[None]
        dry_stride = self._payload_rows("dry", dry, B, frames_out * C * rs.SAMPLE_BYTES[dry_encoding])
        self._per_row("amount", amount, B, torch.float32)
        dry_args = _DryArgs(dry=_ptr(dry), dry_row_stride_bytes=dry_stride, dry_encoding=rs.ENCODINGS[dry_encoding], amount=_ptr(amount))
        return head, B, C, frames_out, dry_args

    def remix_encode(self, planes: torch.Tensor, rate_in: int, rate_out: int, encoding: str, dry: torch.Tensor, dry_encoding: str,
                     amount: torch.Tensor, frames_out: Optional[int] = None, out: Optional[torch.Tensor] = None,
                     clipped: Optional[torch.Tensor] = None, gain: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`resample_encode` of a remix, on the device (lass_remix_encode): what is quantised for frame n, channel c of row b is
        v = fl(x + fl(amount[b] * y)) - times gain[b], rounded once more, with a `gain` - where y is the float32 `resample_encode`
        quantises (bit-identical to `resample` of the plane) and x sample n * C + c of row b of `dry`, decoded as
        `decode_resample_planar` decodes it.  dry: a (B, >= frames_out * C * sample bytes) uint8 tensor on the device, each row a
        WAV data chunk at rate_out ("pcm16" / "pcm32" / "f32", whatever `encoding` is), rows a multiple of 4 bytes apart; amount:
        (B,) float32 on the device (`pipeline.remix_coefficient`: -1 removes the target, 0 gives the original back).  The other
        arguments, the result and the refusals are `resample_encode`'s; `pipeline.remix_host` is the numpy restatement of v."""
        from . import resample as rs
        if encoding not in rs.ENCODINGS:
            raise _lib.LassError(f"encoding must be one of {sorted(rs.ENCODINGS)}")
        head, B, C, frames_out, dry_args = self._remix_args(planes, rate_in, rate_out, dry, dry_encoding, amount, frames_out)
        row_bytes = frames_out * C * rs.SAMPLE_BYTES[encoding]
        out, out_stride = self._encode_tail(B, row_bytes, out, clipped, gain)
        rc = self.lib.lass_remix_encode(self.ctx, *head, *dry_args, rs.ENCODINGS[encoding], _ptr(gain), _ptr(out), out_stride, frames_out,
                                        _ptr(clipped), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_remix_encode")
        return out[:, :row_bytes]

    def remix_peak(self, planes: torch.Tensor, rate_in: int, rate_out: int, dry: torch.Tensor, dry_encoding: str, amount: torch.Tensor,
                   frames_out: Optional[int] = None) -> torch.Tensor:
        """(B,) float32: max |v| over the channels and the first frames_out frames of each recording, v the very float32 values
        `remix_encode` of the same arguments (without a gain) quantises (lass_remix_peak); a NaN is skipped."""
        head, B, _, frames_out, dry_args = self._remix_args(planes, rate_in, rate_out, dry, dry_encoding, amount, frames_out)
        peak = _alloc.empty(B, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_remix_peak(self.ctx, *head, *dry_args, frames_out, _ptr(peak), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_remix_peak")
        return peak

    def resample_true_peak(self, planes: torch.Tensor, rate_in: int, rate_out: int, frames_out: Optional[int] = None) -> torch.Tensor:
        """(B,) float32: the true peak of what `resample_encode` of the same arguments quantises - the larger of `resample_peak`
        and the peak of those samples interpolated os = loudness.oversampling(rate_out) times, phase 0 left out
        (lass_resample_true_peak; lass_amd.loudness.true_peak is its float64 definition).  Bit-identical to `resample` of
        `resample`'s own output at (os, 1); a NaN is skipped.  With os == 1 it is `resample_peak`.  A ratio
        `resample.true_peak_fits` refuses raises LassError."""
        from . import loudness as ld
        from . import resample as rs
        os_ = ld.oversampling(rate_out)
        if os_ == 1:
            return self.resample_peak(planes, rate_in, rate_out, frames_out)
        head, B, _, frames_out = self._export_plan(planes, rate_in, rate_out, frames_out)
        os_taps = rs.device_taps(os_, 1, self.device)
        peak = _alloc.empty(B, dtype=torch.float32, device=self.device)
        rc = self.lib.lass_resample_true_peak(self.ctx, *head, frames_out, os_, _ptr(os_taps), os_taps.numel(), _ptr(peak),
                                              _stream(self.device))
        _lib.check(self.ctx, rc, "lass_resample_true_peak")
        return peak

    STATS_COLUMNS = ("loudness", "blocks", "blocks_kept", "max_momentary", "max_short_term", "loudness_range", "short_term_blocks",
                     "short_term_kept", "p10", "p95")

    def loudness_stats(self, planes: torch.Tensor, rate: int, lengths=None, weights=None, return_short_term: bool = False):
        """`loudness` with the other EBU R 128 figures, on the device (lass_loudness_stats; lass_amd.loudness is the float64
        definition): a dict of (B,) float64 tensors - "loudness" (as `loudness`, bit for bit), "blocks", "blocks_kept",
        "max_momentary" and "max_short_term" (LUFS, ungated), "loudness_range" (LU, EBU Tech 3342), "short_term_blocks",
        "short_term_kept", "p10", "p95" (the two percentile powers) - views of one (B, 10) tensor, which is "all".
        return_short_term: also "short_term", the (B, ns) short-term powers (zeros past a recording's own count)."""
        from . import loudness as ld
        planes, row_stride, plane_stride = self._planes(planes)
        B, C, L = planes.shape
        coef = ld.coefficients(rate)
        hop = int(rate) // 10
        lengths, weights = self._meter_args(lengths, weights, B, C)
        out = _alloc.empty(B, 10, dtype=torch.float64, device=self.device)
        ns = ld.n_short_term(L, rate)
        short = _alloc.empty(B, ns, dtype=torch.float64, device=self.device) if return_short_term else None
        scratch = _alloc.empty(max((5 * C + 1) * B * (L // hop), 1), dtype=torch.float64, device=self.device)
        rc = self.lib.lass_loudness_stats(self.ctx, _ptr(planes), row_stride, plane_stride, B, C, L, _ptr(lengths), hop,
                                          (c_double * 10)(*coef.tolist()), _ptr(weights), _ptr(out), None, 0, _ptr(short), ns,
                                          _ptr(scratch), scratch.numel() * 8, _stream(self.device))
        _lib.check(self.ctx, rc, "lass_loudness_stats")
        res = {name: out[:, k] for k, name in enumerate(self.STATS_COLUMNS)}
        res["all"] = out
        if return_short_term:
            res["short_term"] = short
        return res

    def _meter_args(self, lengths, weights, B: int, C: int):
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(lengths.shape) != (B,):
                raise _lib.LassError(f"lengths must have shape ({B},)")
        if weights is not None:
            weights = torch.as_tensor(weights).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(weights.shape) != (C,):
                raise _lib.LassError(f"weights must have shape ({C},)")
        return lengths, weights

    def loudness(self, planes: torch.Tensor, rate: int, lengths=None, weights=None, return_blocks: bool = False,
                 return_counts: bool = False):
        """ITU-R BS.1770-4 gated integrated loudness on the device (lass_loudness; lass_amd.loudness is its float64 definition):
        planes (B, C, L) or (C, L) float32 at `rate` (any strides with contiguous samples; C 1 ... 8), lengths (B,) int32 (each
        <= L; default L), weights (C,) float32 channel weights (default ones) -> (B,) float64 LUFS, -inf where no block survives.
        return_blocks: also the (B, nb) float64 block powers (zeros past a recording's own count); return_counts: also a (B, 2)
        float64 tensor of (blocks, blocks past both gates).  Order of the extras: blocks, counts."""
        from . import loudness as ld
        planes, row_stride, plane_stride = self._planes(planes)
        B, C, L = planes.shape
        coef = ld.coefficients(rate)
        hop = int(rate) // 10
        lengths, weights = self._meter_args(lengths, weights, B, C)
        nb = max(ld.n_blocks(L, rate), 0)
        out = _alloc.empty(B, 3, dtype=torch.float64, device=self.device)
        blocks = _alloc.empty(B, nb, dtype=torch.float64, device=self.device) if return_blocks else None
        scratch = _alloc.empty(max(5 * B * C * (L // hop), 1), dtype=torch.float64, device=self.device)
        rc = self.lib.lass_loudness(self.ctx, _ptr(planes), row_stride, plane_stride, B, C, L, _ptr(lengths), hop,
                                    (c_double * 10)(*coef.tolist()), _ptr(weights), _ptr(out), _ptr(blocks), nb, _ptr(scratch),
                                    scratch.numel() * 8, _stream(self.device))
        _lib.check(self.ctx, rc, "lass_loudness")
        res = (out[:, 0],) + ((blocks,) if return_blocks else ()) + ((out[:, 1:],) if return_counts else ())
        return res[0] if len(res) == 1 else res

    def loudness_gain(self, loudness: torch.Tensor, peak: Optional[torch.Tensor] = None, target: Optional[float] = None,
                      ceiling: Optional[float] = None):
        """((B,) float32 gain, (B,) int32 flags of the rows the ceiling bit) from (B,) float64 loudness and (B,) float32 peak, on
        the device: lass_amd.loudness.gain_for's rule (lass_loudness_gain).  target in LUFS or None, ceiling linear or None."""
        loudness = loudness.to(device=self.device, dtype=torch.float64).contiguous()
        B = loudness.shape[0]
        if peak is not None:
            peak = peak.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(peak.shape) != (B,):
                raise _lib.LassError(f"peak must have shape ({B},)")
        gain = _alloc.empty(B, dtype=torch.float32, device=self.device)
        limited = _alloc.empty(B, dtype=torch.int32, device=self.device)
        rc = self.lib.lass_loudness_gain(self.ctx, _ptr(loudness), _ptr(peak), B, float("nan") if target is None else float(target),
                                         0.0 if ceiling is None else float(ceiling), _ptr(gain), _ptr(limited), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_loudness_gain")
        return gain, limited

    def limit(self, planes: torch.Tensor, rate: int, gain: torch.Tensor, ceiling: float, lookahead: int, peak: str = "true",
              return_curve: bool = False):
        """The look-ahead limiter on the device (lass_limit; lass_amd.loudness.limit is its float64 definition): planes (B, C, L) or
        (C, L) float32 at `rate` (any strides with contiguous samples; C 1 ... 8), gain (B,) float32 on the device, ceiling linear
        (> 0), lookahead the reach H in frames (`loudness.reach`; 1 ... 512) -> (limited, info): limited (B, C, L) float32 with
        limited[b, c, n] = (gain[b] * G_b[n]) * planes[b, c, n], G_b the one gain curve of recording b, which holds gain x envelope
        under the ceiling and is 1 wherever no frame within 2H needs a reduction.  peak "true": the envelope holds the signal
        between the samples too, loudness.oversampling(rate) times oversampled; "sample": |x| alone.  info: "min_gain" (B,) float32,
        the smallest G of each recording, and "frames" (B,) int32, the frames whose look-ahead minimum is below 1; with
        return_curve also "curve" and "envelope", (B, L) float32.  Everything stays on the device; nothing is read back."""
        from . import loudness as ld
        from . import resample as rs
        if peak not in ("sample", "true"):
            raise _lib.LassError('peak must be "sample" or "true"')
        planes, row_stride, plane_stride = self._planes(planes)
        B, C, L = planes.shape
        H = int(lookahead)
        if not 1 <= H <= ld.LIMITER_MAX_REACH:
            raise _lib.LassError(f"lookahead must lie in 1 ... {ld.LIMITER_MAX_REACH} frames")
        self._per_row("gain", gain, B, torch.float32)
        os_ = ld.oversampling(rate) if peak == "true" else 1
        os_taps = rs.device_taps(os_, 1, self.device) if os_ > 1 else None
        key = (H, str(self.device))
        window = _LIMITER_WINDOWS.get(key)
        if window is None:
            window = _LIMITER_WINDOWS[key] = torch.from_numpy(ld.limiter_window(H)).to(self.device)
        out = _alloc.empty(B, C, L, dtype=torch.float32, device=self.device)
        min_gain = _alloc.empty(B, dtype=torch.float32, device=self.device)
        frames = _alloc.empty(B, dtype=torch.int32, device=self.device)
        curve = _alloc.empty(B, L, dtype=torch.float32, device=self.device) if return_curve else None
        envelope = _alloc.empty(B, L, dtype=torch.float32, device=self.device) if return_curve else None
        rc = self.lib.lass_limit(self.ctx, _ptr(planes), row_stride, plane_stride, B, C, L, os_, _ptr(os_taps),
                                 os_taps.numel() if os_ > 1 else 0, _ptr(gain), float(ceiling), H, _ptr(window), _ptr(out), C * L, L,
                                 _ptr(curve), _ptr(envelope), L, _ptr(min_gain), _ptr(frames), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_limit")
        info = {"min_gain": min_gain, "frames": frames}
        if return_curve:
            info["curve"], info["envelope"] = curve, envelope
        return out, info

    def segment_mix(self, waveforms: torch.Tensor, mix_num: torch.Tensor, comp_db: torch.Tensor, noise_db: torch.Tensor):
        """data/waveform_mixers.py:19-62 on the device with the random draws given: waveforms (B,L), mix_num (B) int32,
        comp_db (B, max_mix_num - 1) f32, noise_db (B) f32 -> (mixture (B,L), segment (B,L))."""
        waveforms = self._dev(waveforms)
        B, L = waveforms.shape
        mix_num = mix_num.to(device=self.device, dtype=torch.int32).contiguous()
        comp_db = comp_db.to(device=self.device, dtype=torch.float32).contiguous()
        noise_db = noise_db.to(device=self.device, dtype=torch.float32).contiguous()
        if mix_num.shape != (B,) or noise_db.shape != (B,) or comp_db.dim() != 2 or comp_db.shape[0] != B:
            raise ValueError("segment_mix: mix_num (B), comp_db (B, max_mix_num - 1), noise_db (B) expected")
        mixture, segment = _alloc.empty_like(waveforms), _alloc.empty_like(waveforms)
        scratch = _alloc.empty(B, 4, dtype=torch.float64, device=self.device)
        rc = self.lib.lass_segment_mix(self.ctx, _ptr(waveforms), B, L, _ptr(mix_num), _ptr(comp_db), int(comp_db.shape[1]),
                                       _ptr(noise_db), _ptr(mixture), _ptr(segment), _ptr(scratch), _stream(self.device))
        _lib.check(self.ctx, rc, "lass_segment_mix")
        return mixture, segment

    def graph_stats(self):
        """(enabled, captures, replays) of the hipGraph replay of lass_separate."""
        from ctypes import c_long
        cap, rep = c_long(), c_long()
        on = self.lib.lass_graph_stats(self.ctx, byref(cap), byref(rep))
        return bool(on), cap.value, rep.value

    def set_graph_replay(self, on: bool):
        """hipGraph replay of lass_separate on / off (off: every call launches eagerly; a measurement switch)."""
        _lib.check(self.ctx, self.lib.lass_set_graph_replay(self.ctx, 1 if on else 0), "lass_set_graph_replay")

    # ---- instrumentation -------------------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self.lib.lass_set_profiling(self.ctx, 1 if on else 0)

    def profile(self, reset: bool = True) -> Dict[str, tuple]:
        """{kernel class: (ms, launches)} accumulated since the last reset.  Caller must have synchronised."""
        out = {}
        for i in range(self.lib.lass_profile_count(self.ctx)):
            name, ms, n = c_char_p(), c_double(), c_int()
            self.lib.lass_profile_get(self.ctx, i, byref(name), byref(ms), byref(n))
            out[name.value.decode()] = (ms.value, n.value)
        if reset:
            self.lib.lass_profile_reset(self.ctx)
        return out


def arch_cond() -> int:
    return 512


_ENGINES: Dict[int, Engine] = {}
_LIMITER_WINDOWS: Dict[tuple, torch.Tensor] = {}   # (H, device) -> loudness.limiter_window(H) on the device, uploaded once


def get_engine(device) -> Engine:
    """Process-wide engine for a device (weights are per ResUNet30 instance -> each model owns its own Engine;
    this shared one serves weight-free ops: STFT, iSTFT, SDR statistics)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _ENGINES:
        _ENGINES[idx] = Engine(torch.device("cuda", idx))
    return _ENGINES[idx]
