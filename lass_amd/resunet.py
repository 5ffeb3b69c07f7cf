"""Host-side mirror of the reference separator interface (drop-in for /root/reference/models/resunet.py:621-714).

`ResUNet30(input_channels, output_channels, condition_size)` is an nn.Module whose state_dict keys, shapes and init
are the reference's, so reference checkpoints load unchanged; `forward(input_dict) -> {'waveform': (B,1,L)}` and
`chunk_inference(input_dict) -> ndarray (1,L) float64` keep the reference signatures.  The module holds parameters
only - all arithmetic happens in liblass_hip (HIP kernels, include/lass_hip.h).  Inference (eval mode) only:
BatchNorm uses running statistics (dcase_evaluator.py:57).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _alloc, arch, longform, ragged
from ._lib import LassError
from .engine import Engine

_IGNORED_PREFIXES = ("base.stft.", "base.istft.")  # torchlibrosa's frozen DFT buffers in reference checkpoints


class _Holder(nn.Module):
    """Parameter container; the tree of these reproduces the reference's module names."""


def _init_tensor(kind: str, shape) -> torch.Tensor:
    """Reference initialisation: models/base.py:9-21 (xavier_uniform weights, zero bias; BN gamma=1, beta=0)."""
    if kind in ("conv_w", "tconv_w", "linear_w"):
        t = torch.empty(*shape)
        nn.init.xavier_uniform_(t)
        return t
    if kind in ("bias", "linear_b", "bn_bias", "bn_mean"):
        return torch.zeros(*shape)
    if kind in ("bn_weight", "bn_var"):
        return torch.ones(*shape)
    if kind == "bn_nbt":
        return torch.tensor(0, dtype=torch.long)
    raise ValueError(kind)


class ResUNet30(nn.Module):
    def __init__(self, input_channels: int = 1, output_channels: int = 1, condition_size: int = 512, *, n_fft: int = arch.N_FFT,
                 hop: int = arch.HOP):
        """n_fft, hop: the model's STFT geometry - (1024, 160), the reference's 16 kHz layout, or (2048, 320), the same network
        at 32 kHz with a 1025-bin bn0 (arch.STFT_GEOMETRIES; upstream AudioSep's released model).  Every method below takes
        its frame counts, bucket width and length limits from it, through the engine."""
        super().__init__()
        self.n_fft, self.hop = arch.check_stft(n_fft, hop)
        if (input_channels, output_channels, condition_size) != (1, 1, 512):
            # config/audiosep_base.yaml:23-30 is the only configuration the reference ships or evaluates
            raise NotImplementedError("lass_amd.ResUNet30 supports input_channels=1, output_channels=1, "
                                      "condition_size=512 (config/audiosep_base.yaml)")
        self.input_channels, self.output_channels, self.condition_size = input_channels, output_channels, condition_size
        self.film_meta = self._film_meta()
        for name, shape, kind in self._param_specs():
            parts = name.split(".")
            mod: nn.Module = self
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, _Holder())
                mod = mod._modules[p]
            t = _init_tensor(kind, shape)
            if kind in ("bn_mean", "bn_var", "bn_nbt"):
                mod.register_buffer(parts[-1], t)
            else:
                mod.register_parameter(parts[-1], nn.Parameter(t, requires_grad=False))
        self._engine: Optional[Engine] = None
        self._uploaded_sig = None
        self.compute_dtype = "f32"  # "bf16" = BASELINE configs[2] (bf16-MFMA convolutions, reduced precision)
        self.eval()

    # ---- what a variant of the model overrides (lass_amd/resunet_with_multistft.py) ---------------------------------
    def _param_specs(self):
        return arch.param_specs(self.input_channels, self.output_channels, self.condition_size, n_fft=self.n_fft)

    def _film_sites(self):
        return arch.film_sites()

    def _make_engine(self, dev) -> Engine:
        return Engine(dev, stft=(self.n_fft, self.hop))

    def _film_meta(self) -> Dict:
        """Nested {module: {'beta1': C, 'beta2': C}} as get_film_meta returns (resunet.py:598-618)."""
        meta: Dict = {}
        for site, c, _used in self._film_sites():
            d = meta
            parts = site.split("->")
            for p in parts[:-1]:
                d = d.setdefault(p, {})
            d[parts[-1]] = c
        return meta

    # ---- state handling ------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = {k: v for k, v in state_dict.items() if not k.startswith(_IGNORED_PREFIXES)}
        self._check_geometry(sd)
        r = super().load_state_dict(sd, strict=strict, **kw)
        self._uploaded_sig = None
        return r

    def _check_geometry(self, sd) -> None:
        """A checkpoint of the other STFT geometry differs in `base.bn0.*` alone (n_fft/2 + 1 entries): say which model it
        needs instead of leaving a bare shape mismatch."""
        own = getattr(getattr(self, "base", None), "bn0", None)
        w = sd.get("base.bn0.weight")
        if own is None or w is None or getattr(w, "ndim", 0) != 1:
            return
        have, got = int(own.weight.shape[0]), int(w.shape[0])
        if got == have:
            return
        match = [g for g in arch.STFT_GEOMETRIES if g[0] // 2 + 1 == got]
        hint = (f"it belongs to ResUNet30(..., n_fft={match[0][0]}, hop={match[0][1]})" if match else
                "no supported (n_fft, hop) has that many bins")
        raise ValueError(f"base.bn0 of this state dict has {got} entries, this model was built with n_fft={self.n_fft}, "
                         f"hop={self.hop} ({have} bins): {hint}")

    def set_compute_dtype(self, compute_dtype: str) -> "ResUNet30":
        if compute_dtype not in Engine.COMPUTE_MODES:
            raise ValueError(f"compute_dtype must be one of {sorted(Engine.COMPUTE_MODES)}")
        self.compute_dtype = compute_dtype
        self._uploaded_sig = None
        return self

    def _signature(self):
        return (self.compute_dtype,) + tuple((t.data_ptr(), t._version) for t in self.state_dict(keep_vars=True).values())

    def _device(self) -> torch.device:
        return self.base.after_conv.weight.device

    def _ensure_engine(self) -> Engine:
        dev = self._device()
        if dev.type != "cuda":
            raise LassError("lass_amd.ResUNet30 computes on an MI355X only: move the module with .to('cuda'). "
                            "There is no CPU fallback.")
        if self._engine is None or self._engine.device != dev:
            self._engine = self._make_engine(dev)
            self._uploaded_sig = None
        sig = self._signature()
        if sig != self._uploaded_sig:
            self._engine.load_state_dict({k: v for k, v in self.state_dict().items()}, self.compute_dtype)
            self._uploaded_sig = sig
        return self._engine

    @property
    def engine(self) -> Engine:
        return self._ensure_engine()

    # ---- reference interface -------------------------------------------------------------------------------------
    def _separate(self, mixtures: torch.Tensor, conditions: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        if mixtures.dim() != 3 or mixtures.shape[1] != 1:
            raise ValueError("mixture must be (batch_size, 1, segment_samples)")
        eng = self._ensure_engine()
        dev = eng.device
        mix = mixtures.to(device=dev, dtype=torch.float32)[:, 0, :].contiguous()
        cond = conditions.to(device=dev, dtype=torch.float32).contiguous()
        return eng.separate(mix, cond)[:, None, :]

    @torch.no_grad()
    def separate_into(self, mixture: torch.Tensor, condition: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """The same call with caller-kept buffers: mixture (B,L), condition (B,512) -> `out` (B,L), all float32 on the model's
        device.  A caller that presents the SAME buffers again (the evaluator's resident batches) reaches lass_separate's
        replayed hipGraph and its two overlapping half-batches; `forward` allocates its output and therefore launches eagerly."""
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        return self._ensure_engine().separate(mixture, condition, out)

    @torch.no_grad()
    def separate_ragged(self, mixture: torch.Tensor, lengths, condition: torch.Tensor, out: Optional[torch.Tensor] = None,
                        checked: bool = False) -> torch.Tensor:
        """Clips of different lengths of ONE 32-frame bucket in one call (Engine.separate_ragged): mixture (B,L) zero-padded
        rows, lengths (B), condition (B,512) -> (B,L), row b the clip's own separation followed by zeros."""
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        return self._ensure_engine().separate_ragged(mixture, lengths, condition, out, checked=checked)

    @torch.no_grad()
    def separate_list(self, waveforms: Sequence[torch.Tensor], conditions, max_batch: int = 16) -> List[torch.Tensor]:
        """Separate clips of ANY lengths: waveforms = 1-D float32 tensors, conditions (N,512) (or N tensors of 512) ->
        N 1-D tensors on the model's device, in input order, each of its clip's length and equal to separating that clip
        alone.  The clips are sorted into 32-frame buckets (lass_amd.ragged.plan_batches); each batch of up to `max_batch`
        clips of one bucket is staged as zero-padded rows and runs as one launch set."""
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        eng = self._ensure_engine()
        dev = eng.device
        n = len(waveforms)
        if any(w.dim() != 1 for w in waveforms):
            raise ValueError("separate_list takes 1-D waveforms")
        cond = conditions if torch.is_tensor(conditions) else torch.stack(list(conditions))
        cond = cond.to(device=dev, dtype=torch.float32)
        if cond.shape != (n, self.condition_size):
            raise ValueError(f"conditions must be ({n}, {self.condition_size})")
        lengths = [int(w.shape[0]) for w in waveforms]
        results: List[Optional[torch.Tensor]] = [None] * n
        for idx, row_length in ragged.plan_batches(lengths, max_batch, eng.n_fft, eng.hop):
            mix = torch.zeros(len(idx), row_length, dtype=torch.float32, device=dev)
            for r, i in enumerate(idx):
                mix[r, :lengths[i]].copy_(waveforms[i], non_blocking=True)
            sep = eng.separate_ragged(mix, [lengths[i] for i in idx], cond[idx].contiguous())
            for r, i in enumerate(idx):
                results[i] = sep[r, :lengths[i]]
        return results

    @torch.no_grad()
    def separate_long(self, waveform: torch.Tensor, condition: torch.Tensor, window: int = 160000, context: int = 16000,
                      max_batch: int = 16, out: Optional[torch.Tensor] = None, fade: int = 0,
                      fade_shape: str = "linear") -> torch.Tensor:
        """Separate a recording of ANY length (> n_fft/2): 1-D waveform, condition (512,) or (1,512) -> 1-D float32 tensor of
        the same length on the model's device.  The recording is cut into overlapping windows of `window` samples of which
        only the inner part is kept (`context` samples discarded towards each neighbour: lass_amd.longform.plan_windows) and
        stays on the device throughout: groups of `max_batch` windows run as one Engine.separate_windows each, all on the same
        recording, output, index buffers and workspace, so from the third group on a group is one replayed hipGraph.  The index
        buffers are rewritten by stream-ordered device copies between groups: no host synchronisation, no copy to the host.
        total <= window: one plain `separate`.
        fade > 0 (even, <= 2 * context and <= window - 2 * context: lass_amd.longform.plan_windows_faded): neighbouring windows are
        cross-faded over the `fade` samples around each seam, with complementary "linear" or "hann" weights
        (lass_amd.longform.fade_ramp), instead of switched between.  Both windows' samples of a zone are ADDED into the output,
        which is therefore zero-filled first - a caller-passed `out` too, whatever it held.  fade = 0: hard seams."""
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        if waveform.dim() != 1:
            raise ValueError("separate_long takes a 1-D waveform")
        eng = self._ensure_engine()
        dev = eng.device
        total = int(waveform.shape[0])
        fade = int(fade)
        if fade < 0:
            raise ValueError("fade must not be negative")
        if fade:
            plan = longform.plan_windows_faded(total, window, context, fade, eng.n_fft)
            ramp = longform.fade_ramp(fade, fade_shape)
        else:
            plan = longform.plan_windows(total, window, context, eng.n_fft)
            ramp = None
        rec = waveform.to(device=dev, dtype=torch.float32).contiguous()
        cond = condition.to(device=dev, dtype=torch.float32).reshape(1, -1).contiguous()
        if cond.shape != (1, self.condition_size):
            raise ValueError(f"condition must be ({self.condition_size},) or (1, {self.condition_size})")
        if out is not None and (out.shape != rec.shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()):
            raise LassError(f"out must be a contiguous float32 {tuple(rec.shape)} tensor on {dev}")
        if total <= window:
            sep = eng.separate(rec[None], cond)[0]
            return sep if out is None else out.copy_(sep)
        if fade:
            out = torch.zeros_like(rec) if out is None else out.zero_()
            groups = longform.group_windows_faded(plan, max_batch)
        else:
            if out is None:
                out = _alloc.empty_like(rec)  # the kept ranges tile it exactly once
            groups = longform.group_windows(plan, max_batch)
        self._run_windows(eng, rec, out, window, groups, cond, None, ramp)
        return out

    @staticmethod
    def _run_windows(eng: Engine, rec: torch.Tensor, out: torch.Tensor, window: int, groups, cond: torch.Tensor, cond_rows, ramp,
                     planes: Optional[torch.Tensor] = None) -> None:
        """Groups of equally many windows of ONE row - (start, lo, hi) or, with a `ramp`, (start, lo, hi, fade_in, fade_out) - as
        one Engine.separate_windows each, on the engine's persistent index buffers.  cond_rows None: row 0 of `cond` for every
        window; else the row of `cond` per window, grouped as `groups`.  The whole plan goes up in a few copies; each group's rows
        reach the index buffers by stream-ordered device copies: no host synchronisation.  planes (C, total): the linked form -
        `rec` is the guide, `out` (C, total), every group one Engine.separate_windows_linked."""
        dev, B = eng.device, len(groups[0])
        all_starts = torch.tensor([[w[0] for w in g] for g in groups], dtype=torch.int64).to(dev)
        all_keeps = torch.tensor([[w[1:3] for w in g] for g in groups], dtype=torch.int32).to(dev)
        idx_s, idx_k, cond_b = eng.window_buffers(B)
        idx_f = ramp_d = None
        if ramp is not None:
            all_fades = torch.tensor([[w[3:5] for w in g] for g in groups], dtype=torch.int32).to(dev)
            idx_f, ramp_d = eng.fade_buffer(B), torch.from_numpy(ramp).to(dev)  # (the ramp is uploaded once)
        if cond_rows is None:
            cond_b.copy_(cond.expand(B, -1))
        else:
            all_rows = torch.tensor(cond_rows, dtype=torch.int64).to(dev)
        for gi in range(len(groups)):
            idx_s.copy_(all_starts[gi])
            idx_k.copy_(all_keeps[gi])
            if idx_f is not None:
                idx_f.copy_(all_fades[gi])
            if cond_rows is not None:
                torch.index_select(cond, 0, all_rows[gi], out=cond_b)
            if planes is not None:
                eng.separate_windows_linked(rec, planes, idx_s, idx_k, cond_b, window, out=out, checked=True, fade=idx_f, ramp=ramp_d)
                continue
            eng.separate_windows(rec, idx_s, idx_k, cond_b, window, out=out, checked=True, fade=idx_f, ramp=ramp_d)

    @torch.no_grad()
    def separate_long_list(self, waveforms: Sequence[torch.Tensor], conditions, window: int = 160000, context: int = 16000,
                           max_batch: int = 16, fade: int = 0, fade_shape: str = "linear") -> List[torch.Tensor]:
        """`separate_long` for several recordings in one pass: waveforms = 1-D float32 tensors of ANY lengths, conditions (N,512)
        (or N tensors of 512) -> N 1-D tensors on the model's device, in input order, each what `separate_long` gives for that
        recording alone (f32: bit for bit).  The recordings longer than `window` are laid end to end in one device row and each
        is planned on its own (lass_amd.longform.plan_windows / plan_windows_faded, the starts offset by its position): no
        window straddles two recordings and no fade crosses a boundary.  The windows of all of them are then grouped together,
        each with its own recording's condition, and run as Engine.separate_windows calls on that one row, one output and one
        set of index buffers - so a folder of short files fills every group and reaches graph replay, which one `separate_long`
        per file does not.  The results are views of the one output row.  Recordings not longer than `window` go through
        `separate_list`."""
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        eng = self._ensure_engine()
        dev = eng.device
        n = len(waveforms)
        if any(w.dim() != 1 for w in waveforms):
            raise ValueError("separate_long_list takes 1-D waveforms")
        cond = conditions if torch.is_tensor(conditions) else torch.stack(list(conditions))
        cond = cond.to(device=dev, dtype=torch.float32).contiguous()
        if cond.shape != (n, self.condition_size):
            raise ValueError(f"conditions must be ({n}, {self.condition_size})")
        window, fade = int(window), int(fade)
        if fade < 0:
            raise ValueError("fade must not be negative")
        lengths = [int(w.shape[0]) for w in waveforms]
        long_ids = [i for i in range(n) if lengths[i] > window]
        short_ids = [i for i in range(n) if lengths[i] <= window]
        results: List[Optional[torch.Tensor]] = [None] * n
        if short_ids:
            for i, sep in zip(short_ids, self.separate_list([waveforms[i] for i in short_ids], cond[short_ids], max_batch)):
                results[i] = sep
        if not long_ids:
            return results
        rows, cond_rows, offsets, at = [], [], {}, 0
        for i in long_ids:
            if fade:
                plan = longform.plan_windows_faded(lengths[i], window, context, fade, eng.n_fft)
            else:
                plan = longform.plan_windows(lengths[i], window, context, eng.n_fft)
            rows += [(w[0] + at,) + tuple(w[1:]) for w in plan]
            cond_rows += [i] * len(plan)
            offsets[i] = at
            at += lengths[i]
        rec = torch.empty(at, dtype=torch.float32, device=dev)
        for i in long_ids:
            rec[offsets[i]:offsets[i] + lengths[i]].copy_(waveforms[i], non_blocking=True)
        if fade:
            out, ramp = torch.zeros_like(rec), longform.fade_ramp(fade, fade_shape)
            groups = longform.group_windows_faded(rows, max_batch)
        else:
            out, ramp = _alloc.empty_like(rec), None  # the kept ranges tile it exactly once
            groups = longform.group_windows(rows, max_batch)
        B = len(groups[0])
        cond_rows += [cond_rows[-1]] * (len(groups) * B - len(cond_rows))  # (the padding rows store nothing)
        self._run_windows(eng, rec, out, window, groups, cond, [cond_rows[g * B:(g + 1) * B] for g in range(len(groups))], ramp)
        for i in long_ids:
            results[i] = out[offsets[i]:offsets[i] + lengths[i]]
        return results

    # ---- linked channels: one mask from a guide, applied to every channel ---------------------------
    @staticmethod
    def downmix(planes: torch.Tensor) -> torch.Tensor:
        """The default guide of a (C, L) recording: the float32 mean of its planes, summed in ascending channel order and divided
        by C once (a single plane comes back as it is, bit for bit)."""
        acc = planes[0]
        for c in range(1, planes.shape[0]):
            acc = acc + planes[c]
        return acc / planes.shape[0] if planes.shape[0] > 1 else acc

    @torch.no_grad()
    def separate_long_linked(self, planes: torch.Tensor, condition: torch.Tensor, guide: Optional[torch.Tensor] = None,
                             window: int = 160000, context: int = 16000, max_batch: int = 16, fade: int = 0,
                             fade_shape: str = "linear") -> torch.Tensor:
        """`separate_long` for a multi-channel recording with LINKED channels: planes (C, L), 1 <= C <= 8 -> (C, L).  One mask
        per window is estimated from `guide` (L,) - None: `downmix(planes)` - and applied to that window of every channel
        (Engine.separate_windows_linked), so the network runs once per window whatever C and every channel is attenuated alike,
        bin by bin.  window, context, max_batch, fade, fade_shape: `separate_long`'s.  L <= window: one
        Engine.separate_ragged_linked."""
        return self.separate_long_list_linked([planes], condition.reshape(1, -1), None if guide is None else [guide], window=window,
                                              context=context, max_batch=max_batch, fade=fade, fade_shape=fade_shape)[0]

    @torch.no_grad()
    def separate_long_list_linked(self, recordings: Sequence[torch.Tensor], conditions, guides=None, window: int = 160000,
                                  context: int = 16000, max_batch: int = 16, fade: int = 0,
                                  fade_shape: str = "linear") -> List[torch.Tensor]:
        """`separate_long_list` with linked channels: recordings = (C, L_i) float32 tensors with the SAME C, conditions (N,512),
        guides = None or N 1-D tensors (L_i,) (an entry None: that recording's `downmix`) -> N (C, L_i) tensors on the model's
        device, each what `separate_long_linked` gives for that recording alone (f32: bit for bit).  Recordings longer than
        `window` are laid end to end - the guides in one device row, the planes in C rows - planned each on its own and run as
        Engine.separate_windows_linked calls, exactly as `separate_long_list` lays out its one row; the others go through
        Engine.separate_ragged_linked in batches of one 32-frame bucket (lass_amd.ragged.plan_batches)."""
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        eng = self._ensure_engine()
        dev = eng.device
        n = len(recordings)
        if n == 0:
            return []
        C = int(recordings[0].shape[0]) if recordings[0].dim() == 2 else 0
        if any(r.dim() != 2 or int(r.shape[0]) != C for r in recordings) or not 1 <= C <= eng.MAX_LINKED_CHANNELS:
            raise ValueError(f"separate_long_list_linked takes (C, L) recordings of one channel count, 1 <= C <= {eng.MAX_LINKED_CHANNELS}")
        cond = conditions if torch.is_tensor(conditions) else torch.stack(list(conditions))
        cond = cond.to(device=dev, dtype=torch.float32).contiguous()
        if cond.shape != (n, self.condition_size):
            raise ValueError(f"conditions must be ({n}, {self.condition_size})")
        window, fade = int(window), int(fade)
        if fade < 0:
            raise ValueError("fade must not be negative")
        lengths = [int(r.shape[1]) for r in recordings]
        if guides is not None and (len(guides) != n or any(g is not None and tuple(g.shape) != (lengths[i],) for i, g in enumerate(guides))):
            raise ValueError("guides must be one 1-D tensor (or None) per recording, of its recording's length")
        recs = [r.to(device=dev, dtype=torch.float32) for r in recordings]
        gds = [self.downmix(recs[i]) if guides is None or guides[i] is None else guides[i].to(device=dev, dtype=torch.float32)
               for i in range(n)]
        long_ids = [i for i in range(n) if lengths[i] > window]
        short_ids = [i for i in range(n) if lengths[i] <= window]
        results: List[Optional[torch.Tensor]] = [None] * n
        if short_ids:
            for idx, row_length in ragged.plan_batches([lengths[i] for i in short_ids], max_batch, eng.n_fft, eng.hop):
                idx = [short_ids[j] for j in idx]
                guide = torch.zeros(len(idx), row_length, dtype=torch.float32, device=dev)
                planes = torch.zeros(C, len(idx), row_length, dtype=torch.float32, device=dev)
                for r, i in enumerate(idx):
                    guide[r, :lengths[i]].copy_(gds[i], non_blocking=True)
                    planes[:, r, :lengths[i]].copy_(recs[i], non_blocking=True)
                sep = eng.separate_ragged_linked(guide, [lengths[i] for i in idx], planes, cond[idx].contiguous())
                for r, i in enumerate(idx):
                    results[i] = sep[:, r, :lengths[i]]
        if not long_ids:
            return results
        rows, cond_rows, offsets, at = [], [], {}, 0
        for i in long_ids:
            if fade:
                plan = longform.plan_windows_faded(lengths[i], window, context, fade, eng.n_fft)
            else:
                plan = longform.plan_windows(lengths[i], window, context, eng.n_fft)
            rows += [(w[0] + at,) + tuple(w[1:]) for w in plan]
            cond_rows += [i] * len(plan)
            offsets[i] = at
            at += lengths[i]
        guide = torch.empty(at, dtype=torch.float32, device=dev)
        planes = torch.empty(C, at, dtype=torch.float32, device=dev)
        for i in long_ids:
            guide[offsets[i]:offsets[i] + lengths[i]].copy_(gds[i], non_blocking=True)
            planes[:, offsets[i]:offsets[i] + lengths[i]].copy_(recs[i], non_blocking=True)
        if fade:
            out, ramp = torch.zeros_like(planes), longform.fade_ramp(fade, fade_shape)
            groups = longform.group_windows_faded(rows, max_batch)
        else:
            out, ramp = _alloc.empty_like(planes), None  # the kept ranges tile every row exactly once
            groups = longform.group_windows(rows, max_batch)
        B = len(groups[0])
        cond_rows += [cond_rows[-1]] * (len(groups) * B - len(cond_rows))  # (the padding rows store nothing)
        self._run_windows(eng, guide, out, window, groups, cond, [cond_rows[g * B:(g + 1) * B] for g in range(len(groups))], ramp, planes)
        for i in long_ids:
            results[i] = out[:, offsets[i]:offsets[i] + lengths[i]]
        return results

    @torch.no_grad()
    def forward(self, input_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """resunet.py:640-653."""
        return {"waveform": self._separate(input_dict["mixture"], input_dict["condition"])}

    @torch.no_grad()
    def chunk_inference(self, input_dict: Dict[str, torch.Tensor], max_batch: int = 16, resident: bool = False) -> np.ndarray:
        """resunet.py:655-714, including its quirks: RATE hard-coded to 32000, batch 1, float64 result, zeros when
        the input is not longer than one window.  The reference runs a second, overlapping forward inside each loop
        iteration whose write is overwritten by the next iteration except at the tail; the same writes are made here in
        the same order, so outputs are identical sample for sample.  Execution differs: the windows are independent
        (eval-mode BatchNorm), so every DISTINCT window is separated once, `max_batch` windows per launch, instead of
        two batch-1 forwards per iteration (the second forward of iteration i is the first of iteration i+1).
        resident=True: the same result, sample for sample, with the recording and the output kept on the device
        (`_chunk_inference_resident`)."""
        if resident:
            return self._chunk_inference_resident(input_dict, max_batch)
        mixtures, conditions = input_dict["mixture"], input_dict["condition"]
        rate = 32000
        nl, nc, nr = int(1.0 * rate), int(3.0 * rate), int(1.0 * rate)
        length = mixtures.shape[2]
        out_np = np.zeros([1, length])
        window = nl + nc + nr
        # pass 1: the reference's control flow, recording (segment, destination slice, source slice) per write
        writes = []
        idx = 0
        while idx + window < length:
            seg = (idx, idx + window)
            if idx == 0:
                writes.append((seg, slice(idx, idx + window - nr), slice(None, -nr)))
            else:
                writes.append((seg, slice(idx + nl, idx + window - nr), slice(nl, -nr)))
            idx += nc
            if idx < length:
                seg = (idx, min(idx + window, length))
                writes.append((seg, slice(idx + nl, seg[1]), slice(nl, None)))
        # pass 2: separate every distinct segment once, batching segments of equal length
        results: Dict[tuple, np.ndarray] = {}
        by_len: Dict[int, list] = {}
        for seg, _, _ in writes:
            if seg not in results:
                results[seg] = None
                by_len.setdefault(seg[1] - seg[0], []).append(seg)
        for segs in by_len.values():
            for i in range(0, len(segs), max_batch):
                group = segs[i:i + max_batch]
                batch = torch.cat([mixtures[:1, :, a:b] for a, b in group], dim=0)
                sep = self._separate(batch, conditions[:1].expand(len(group), -1)).squeeze(1).cpu().numpy()
                for seg, row in zip(group, sep):
                    results[seg] = row[None, :]
        # pass 3: replay the writes in the reference's order
        for seg, dst, src in writes:
            out_np[:, dst] = results[seg][:, src]
        return out_np

    def _chunk_inference_resident(self, input_dict: Dict[str, torch.Tensor], max_batch: int) -> np.ndarray:
        """chunk_inference's result through Engine.separate_windows: what survives of the reference's writes is one range per
        distinct window (lass_amd.longform.reference_plan), so every window stores its range straight into one output row on
        the device - one call per `max_batch` windows of equal length (the shorter tail window is a call of its own length), the
        same batches in the same order as the default path - and ONE copy to the host at the end fills the reference's (1, L)
        float64 array, zero where the reference never writes."""
        if self.training:
            raise LassError("lass_amd.ResUNet30 is inference-only (call .eval()); training is out of scope")
        mixtures, conditions = input_dict["mixture"], input_dict["condition"]
        if mixtures.dim() != 3 or mixtures.shape[1] != 1:
            raise ValueError("mixture must be (batch_size, 1, segment_samples)")
        rate = 32000
        nl, nc, nr = int(1.0 * rate), int(3.0 * rate), int(1.0 * rate)
        length = mixtures.shape[2]
        _, ranges = longform.reference_plan(length, nl, nc, nr)
        if not ranges:
            return np.zeros([1, length])
        eng = self._ensure_engine()
        dev = eng.device
        rec = mixtures[0, 0].to(device=dev, dtype=torch.float32).contiguous()
        cond = conditions[:1].to(device=dev, dtype=torch.float32).contiguous()
        out = torch.zeros_like(rec)
        by_len: Dict[int, list] = {}
        for a, b, lo, hi in ranges:
            by_len.setdefault(b - a, []).append((a, lo, hi))
        for w, wins in by_len.items():
            for i in range(0, len(wins), max_batch):
                group = wins[i:i + max_batch]
                eng.separate_windows(rec, [g[0] for g in group], [g[1:] for g in group], cond, w, out=out)
        return out.cpu().numpy().astype(np.float64)[None, :]
