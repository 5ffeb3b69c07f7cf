"""CLAP audio encoder on the device: clips -> (B,512) unit-norm query embeddings (the `audio` modality of the reference's
`CLAP_Encoder.get_query_embed`, models/clap_encoder.py:50-76, 93-106), and `ClapQueryEncoder`, which serves `text`,
`audio` and `hybird` from one object.

`ClapAudioEncoder` mirrors the parameter tree of the CLAP model's audio tower - `model.audio_branch.*` (HTSAT, a Swin
transformer over a 256 x 256 fold of the log-mel spectrogram, CLAP/open_clip/htsat.py) and `model.audio_projection.{0,2}.*`
- so the `query_encoder.*` sub-dict of an AudioSep Lightning checkpoint loads into it key for key.  torch only holds the
weights; every number is computed by the HIP kernels of lass_amd/csrc/audio_clap.hip behind `lass_audioq_*`
(include/lass_hip.h): 32 -> 48 kHz resampler, repeat-pad + log-mel front end, patch embedding, window attention, GEMMs,
projection head.  There is no CPU fallback.

Two deliberate differences from the reference: a batch (B, L) gives (B, 512) - row n is what the
reference returns for audio[n:n+1] (its loop returns after the first clip) - and clips longer than 10 s raise ValueError
(the reference takes a random crop).
"""
from __future__ import annotations

import ctypes
import math
import random
from ctypes import POINTER, byref, c_int, c_size_t, c_void_p
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _alloc, _lib
from .clap_text import ClapTextEncoder, _module

EMBED_DIM, DEPTHS, HEADS0, WINDOW, PROJ = 128, (2, 2, 12, 2), 4, 8, 512
MEL_BINS, SPEC_SIZE, CLASS_NUM = 64, 256, 527
SR_IN, SR_CLAP, CLIP_SAMPLES = 32000, 48000, 480000
MAX_SAMPLES_32K = 320000                       # 10 s: longer clips take a random crop in the reference (not mirrored)
N_FFT, HOP, FRAMES, FMIN, FMAX = 1024, 480, 1001, 50.0, 14000.0
GRID = SPEC_SIZE // 4                          # 64 x 64 tokens after the 4x4 / stride-4 patch embedding

_PRE = "model.audio_branch."
# CLAP model keys that are not the audio tower, and the buffers a checkpoint carries that are derived, not learned
_IGNORED = ("model.text_branch.", "model.text_projection.", "model.logit_scale_")
_IGNORED_BUFFERS = (".relative_position_index", ".attn_mask", "spectrogram_extractor.", "logmel_extractor.")
_UNUSED = ("tscam_conv.", "head.")             # classification heads: loadable, never uploaded


def _tscam_rows(stages: int) -> int:
    return SPEC_SIZE // (1 << (stages - 1)) // 4 // (SPEC_SIZE // MEL_BINS)


def param_specs(depths: Sequence[int] = DEPTHS, embed_dim: int = EMBED_DIM) -> List[Tuple[str, tuple, str]]:
    """(key, shape, kind) of every state_dict entry of the audio tower in the module's order.  kind: 'w' matrix, 'g'
    norm weight, 'b' bias, 'm' running mean, 'v' running variance (positive), 'buf' derived buffer (not a weight)."""
    s = [(_PRE + "bn0.weight", (MEL_BINS,), "g"), (_PRE + "bn0.bias", (MEL_BINS,), "b"),
         (_PRE + "bn0.running_mean", (MEL_BINS,), "m"), (_PRE + "bn0.running_var", (MEL_BINS,), "v"),
         (_PRE + "bn0.num_batches_tracked", (), "buf"),
         (_PRE + "patch_embed.proj.weight", (embed_dim, 1, 4, 4), "w"), (_PRE + "patch_embed.proj.bias", (embed_dim,), "b"),
         (_PRE + "patch_embed.norm.weight", (embed_dim,), "g"), (_PRE + "patch_embed.norm.bias", (embed_dim,), "b")]
    for i, depth in enumerate(depths):
        C, heads, res = embed_dim << i, HEADS0 << i, GRID >> i
        for j in range(depth):
            p = f"{_PRE}layers.{i}.blocks.{j}."
            if j % 2 == 1 and res > WINDOW:
                s.append((p + "attn_mask", ((res // WINDOW) ** 2, WINDOW * WINDOW, WINDOW * WINDOW), "buf"))
            s += [(p + "norm1.weight", (C,), "g"), (p + "norm1.bias", (C,), "b"),
                  (p + "attn.relative_position_bias_table", ((2 * WINDOW - 1) ** 2, heads), "w"),
                  (p + "attn.relative_position_index", (WINDOW * WINDOW, WINDOW * WINDOW), "buf"),
                  (p + "attn.qkv.weight", (3 * C, C), "w"), (p + "attn.qkv.bias", (3 * C,), "b"),
                  (p + "attn.proj.weight", (C, C), "w"), (p + "attn.proj.bias", (C,), "b"),
                  (p + "norm2.weight", (C,), "g"), (p + "norm2.bias", (C,), "b"),
                  (p + "mlp.fc1.weight", (4 * C, C), "w"), (p + "mlp.fc1.bias", (4 * C,), "b"),
                  (p + "mlp.fc2.weight", (C, 4 * C), "w"), (p + "mlp.fc2.bias", (C,), "b")]
        if i < len(depths) - 1:
            p = f"{_PRE}layers.{i}.downsample."
            s += [(p + "reduction.weight", (2 * C, 4 * C), "w"), (p + "norm.weight", (4 * C,), "g"), (p + "norm.bias", (4 * C,), "b")]
    F = embed_dim << (len(depths) - 1)
    sf = _tscam_rows(len(depths))
    s += [(_PRE + "norm.weight", (F,), "g"), (_PRE + "norm.bias", (F,), "b"),
          (_PRE + "tscam_conv.weight", (CLASS_NUM, F, sf, 3), "w"), (_PRE + "tscam_conv.bias", (CLASS_NUM,), "b"),
          (_PRE + "head.weight", (CLASS_NUM, CLASS_NUM), "w"), (_PRE + "head.bias", (CLASS_NUM,), "b"),
          ("model.audio_projection.0.weight", (PROJ, F), "w"), ("model.audio_projection.0.bias", (PROJ,), "b"),
          ("model.audio_projection.2.weight", (PROJ, PROJ), "w"), ("model.audio_projection.2.bias", (PROJ,), "b")]
    return s


# ---- derived tables (own derivation; the kernels compute the same two things from token coordinates) ----------------
def relative_position_index(window: int = WINDOW) -> torch.Tensor:
    """index[i, j] into the (2w-1)^2 bias table for query i, key j of a w x w window (row-major tokens)."""
    r, c = torch.arange(window * window) // window, torch.arange(window * window) % window
    return (r[:, None] - r[None, :] + window - 1) * (2 * window - 1) + (c[:, None] - c[None, :] + window - 1)


def shift_mask(res: int, window: int = WINDOW) -> torch.Tensor:
    """(windows, w*w, w*w): -100 where two tokens of a window of the cyclically shifted res x res grid come from
    different sides of the wrap-around, else 0."""
    x = torch.arange(res)
    reg = (x >= res - window).long() + (x >= res - window // 2).long()
    img = reg[:, None] * 3 + reg[None, :]
    n = res // window
    win = img.view(n, window, n, window).permute(0, 2, 1, 3).reshape(n * n, window * window)
    return torch.where(win[:, None, :] != win[:, :, None], -100.0, 0.0).float()


# ---- front-end constants, built on the host in float64 -------------------------------------------------------------
def resample_taps() -> np.ndarray:
    """(3, 16) float64 polyphase taps of torchaudio.functional.resample(x, 32000, 48000) with its published defaults
    (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): y[3i + p] = sum_k taps[p, k] * x[2i + k - 7]."""
    orig, new, lowpass, rolloff = 2, 3, 6, 0.99
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx[None, :]) * base
    t = np.clip(t, -lowpass, lowpass)
    window = np.cos(t * math.pi / lowpass / 2) ** 2
    t = t * math.pi
    sinc = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
    return sinc * window * (base / orig)


def resample_host(x: np.ndarray) -> np.ndarray:
    """float64 host evaluation of the same taps (the yardstick of the resampler tests): (L,) -> (ceil(1.5 L),)."""
    h, L = resample_taps(), len(x)
    n = (L + 1) // 2 + 1
    xp = np.zeros(2 * n + 16, dtype=np.float64)
    xp[7:7 + L] = x
    fr = np.lib.stride_tricks.sliding_window_view(xp, 16)[0:2 * n:2]
    return (fr @ h.T).reshape(-1)[:(3 * L + 1) // 2]


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), 200.0 * m / 3.0)


def mel_filter() -> np.ndarray:
    """(513, 64) float64 slaney mel filter bank (slaney scale, slaney area normalisation) for sr 48000, n_fft 1024,
    50 .. 14000 Hz: triangles between 66 mel-spaced edge frequencies, each scaled by 2 / (its width in Hz)."""
    fft_freqs = np.linspace(0.0, SR_CLAP / 2, N_FFT // 2 + 1)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(FMIN), _hz_to_mel(FMAX), MEL_BINS + 2))
    diff = np.diff(edges)
    slopes = edges[None, :] - fft_freqs[:, None]
    down, up = -slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    return fb * (2.0 / (edges[2:] - edges[:-2]))[None, :]


class lass_audioq_taps(ctypes.Structure):
    """include/lass_hip.h: optional device outputs of lass_audioq_encode_*; a NULL member is not written."""
    _fields_ = [("wave48k", c_void_p), ("logmel", c_void_p), ("tokens", c_void_p), ("stage", c_void_p * 4),
                ("embedding", c_void_p)]


def _block(C: int, heads: int, res: int, shifted: bool) -> nn.Module:
    attn = _module(qkv=nn.Linear(C, 3 * C), proj=nn.Linear(C, C))
    attn.relative_position_bias_table = nn.Parameter(torch.zeros((2 * WINDOW - 1) ** 2, heads))
    attn.register_buffer("relative_position_index", relative_position_index())
    blk = nn.Module()
    if shifted:
        blk.register_buffer("attn_mask", shift_mask(res))
    blk.add_module("norm1", nn.LayerNorm(C))
    blk.add_module("attn", attn)
    blk.add_module("norm2", nn.LayerNorm(C))
    blk.add_module("mlp", _module(fc1=nn.Linear(C, 4 * C), fc2=nn.Linear(4 * C, C)))
    return blk


class ClapAudioEncoder(nn.Module):
    """The audio modality of `get_query_embed` (models/clap_encoder.py:93-106) on the device."""

    encoder_type = "CLAP"

    def __init__(self, depths: Sequence[int] = DEPTHS, embed_dim: int = EMBED_DIM):
        super().__init__()
        depths = tuple(int(d) for d in depths)
        if not 1 <= len(depths) <= 4 or min(depths) < 1:
            raise ValueError("ClapAudioEncoder: 1-4 stages of >= 1 block each")
        if embed_dim != EMBED_DIM:
            raise ValueError(f"ClapAudioEncoder: the kernels are built for HTSAT-base's embedding width {EMBED_DIM} "
                             f"(got {embed_dim}: HTSAT-tiny / -large are not supported)")
        layers = []
        for i, depth in enumerate(depths):
            C, heads, res = embed_dim << i, HEADS0 << i, GRID >> i
            st = _module(blocks=nn.ModuleList([_block(C, heads, res, j % 2 == 1 and res > WINDOW) for j in range(depth)]))
            if i < len(depths) - 1:
                st.add_module("downsample", _module(reduction=nn.Linear(4 * C, 2 * C, bias=False), norm=nn.LayerNorm(4 * C)))
            layers.append(st)
        F = embed_dim << (len(depths) - 1)
        sf = _tscam_rows(len(depths))
        branch = _module(bn0=nn.BatchNorm2d(MEL_BINS),
                         patch_embed=_module(proj=nn.Conv2d(1, embed_dim, 4, 4), norm=nn.LayerNorm(embed_dim)),
                         layers=nn.ModuleList(layers), norm=nn.LayerNorm(F),
                         tscam_conv=nn.Conv2d(F, CLASS_NUM, (sf, 3), padding=(0, 1)), head=nn.Linear(CLASS_NUM, CLASS_NUM))
        proj = nn.Sequential(nn.Linear(F, PROJ), nn.ReLU(), nn.Linear(PROJ, PROJ))
        self.model = _module(audio_branch=branch, audio_projection=proj)
        with torch.no_grad():  # weights come from a checkpoint; zeros (unit variance) until then
            for n, p in self.model.named_parameters():
                p.zero_()
        self.eval()
        self.depths, self.embed_dim, self.features = depths, embed_dim, F
        self._ctx: Optional[_lib.TowerContext] = None
        self._ws: Optional[torch.Tensor] = None

    # ---- weights ---------------------------------------------------------------------------------------------
    @staticmethod
    def audio_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The audio-tower entries of a checkpoint state_dict (Lightning `query_encoder.model.*` or a bare `model.*`
        dict), keyed as this module's state_dict; text / transform / logit-scale keys and the derived buffers
        (relative_position_index, attn_mask, the torchlibrosa DFT and mel matrices) are dropped."""
        if any(k.startswith("query_encoder.") for k in sd):
            sd = {k[len("query_encoder."):]: v for k, v in sd.items() if k.startswith("query_encoder.")}
        out = {}
        for k, v in sd.items():
            if not k.startswith("model.") or k.startswith(_IGNORED) or any(b in k for b in _IGNORED_BUFFERS):
                continue
            if k.split(".")[1].endswith("_transform"):
                continue
            out[k] = v
        return out

    def load_audio_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Load a checkpoint's audio tower (see audio_state_dict); a missing audio key is an error that names it."""
        sd = self.audio_state_dict(sd)
        own = self.state_dict()
        # derived buffers are this module's own; bn0's batch counter is loaded when present and means nothing in eval
        derived = {k: v for k, v in own.items()
                   if any(b in k for b in _IGNORED_BUFFERS) or (k.endswith("num_batches_tracked") and k not in sd)}
        for k in own:
            if k not in sd and k not in derived:
                raise KeyError(f"checkpoint has no audio-tower parameter 'query_encoder.{k}'")
        unexpected = sorted(set(sd) - set(own))
        if unexpected:
            raise KeyError(f"unexpected audio-tower parameter(s) 'query_encoder.{unexpected[0]}'"
                           + (f" and {len(unexpected) - 1} more" if len(unexpected) > 1 else ""))
        self.load_state_dict({**sd, **derived}, strict=True)
        return self

    @classmethod
    def from_checkpoint(cls, path: str):
        """Audio tower of an AudioSep Lightning checkpoint (read with weights_only=True: nothing in the file runs).
        Depths and the embedding width are the checkpoint's."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        sd = cls.audio_state_dict(ck.get("state_dict", ck) if isinstance(ck, dict) else ck)
        depth: Dict[int, int] = {}
        for k in sd:
            if k.startswith(_PRE + "layers."):
                part = k[len(_PRE + "layers."):].split(".")
                if part[1] == "blocks":
                    depth[int(part[0])] = max(depth.get(int(part[0]), 0), int(part[2]) + 1)
        if not depth or sorted(depth) != list(range(len(depth))):
            raise KeyError(f"checkpoint has no audio-tower parameter 'query_encoder.{_PRE}layers.0.blocks.0.*'")
        w = sd.get(_PRE + "patch_embed.proj.weight")
        enc = cls(depths=[depth[i] for i in range(len(depth))], embed_dim=int(w.shape[0]) if w is not None else EMBED_DIM)
        return enc.load_audio_state_dict(sd)

    # ---- device ----------------------------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self.model.audio_projection[0].weight.device

    def _uploaded(self):
        """(name relative to the CLAP model, tensor) of everything the kernels read."""
        for name, t in list(self.model.named_parameters()) + [(n, b) for n, b in self.model.named_buffers() if "running_" in n]:
            if not any(u in name for u in _UNUSED):
                yield name, t

    def _context(self) -> _lib.TowerContext:
        dev = self.device
        if dev.type != "cuda":
            raise _lib.LassError("ClapAudioEncoder computes on an MI355X only: move it to a cuda/HIP device first "
                                 "(lass_amd has no CPU fallback)")
        params = list(self._uploaded())
        if self._ctx is None or self._ctx.key != _lib.TowerContext.key_of(dev, params):
            self._ctx = None  # the previous upload is freed before the new one is made
            self._ctx = _lib.TowerContext("lass_audioq", dev, params)
        return self._ctx

    # ---- compute ---------------------------------------------------------------------------------------------
    @staticmethod
    def _validate(wave, lengths, max_len: int, rate: str) -> Tuple[torch.Tensor, np.ndarray]:
        if not torch.is_tensor(wave):
            wave = torch.as_tensor(np.asarray(wave))
        if wave.dim() != 2 or not wave.dtype.is_floating_point:
            raise ValueError(f"audio must be a float (B, L) tensor, got {tuple(wave.shape)} {wave.dtype}")
        B, L = wave.shape
        if B < 1 or L < 1:
            raise ValueError("empty batch")
        if L > max_len:
            raise ValueError(f"clip of {L} samples exceeds the limit of {max_len} samples at {rate} (10 s); longer clips "
                             "take a random crop in the reference, which is not mirrored")
        if lengths is None:
            lens = np.full(B, L, dtype=np.int32)
        else:
            lens = np.asarray(torch.as_tensor(lengths).cpu() if torch.is_tensor(lengths) else lengths)
            if lens.shape != (B,) or lens.dtype.kind not in "iu":
                raise ValueError(f"lengths must be {B} integers")
            if lens.min() < 1 or lens.max() > L:
                raise ValueError(f"lengths must lie in [1, {L}]")
            lens = lens.astype(np.int32)
        return wave, np.ascontiguousarray(lens)

    def _encode(self, wave, lengths, taps, rate32k: bool):
        wave, lens = self._validate(wave, lengths, MAX_SAMPLES_32K if rate32k else CLIP_SAMPLES, "32 kHz" if rate32k else "48 kHz")
        ctx = self._context()
        dev = self.device
        if wave.device != dev:
            raise _lib.LassError(f"audio is on {wave.device}, the encoder on {dev}")
        wave = wave.detach().to(torch.float32).contiguous()
        B, L = wave.shape
        n = c_size_t()
        ctx.check(ctx.lib.lass_audioq_workspace_bytes(ctx.ctx, B, byref(n)), "lass_audioq_workspace_bytes")
        ws = _lib.grow_workspace(self, n.value, dev)
        out = _alloc.empty(B, PROJ, dtype=torch.float32, device=dev)
        t = lass_audioq_taps()
        res = {}
        if taps:
            new = lambda *s: _alloc.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
            if rate32k:
                res["wave48k"] = new(B, (3 * L + 1) // 2)
                t.wave48k = res["wave48k"].data_ptr()
            res["logmel"], res["tokens"], res["embedding"] = new(B, FRAMES, MEL_BINS), new(B, GRID * GRID, self.embed_dim), new(B, self.features)
            t.logmel, t.tokens, t.embedding = res["logmel"].data_ptr(), res["tokens"].data_ptr(), res["embedding"].data_ptr()
            res["stages"] = []
            for i in range(len(self.depths)):
                last = i == len(self.depths) - 1
                r, C = GRID >> (i if last else i + 1), self.embed_dim << (i if last else i + 1)
                res["stages"].append(new(B, r * r, C))
                t.stage[i] = res["stages"][-1].data_ptr()
        fn = ctx.lib.lass_audioq_encode_wave32k if rate32k else ctx.lib.lass_audioq_encode_wave48k
        rc = fn(ctx.ctx, c_void_p(wave.data_ptr()), lens.ctypes.data_as(POINTER(c_int)), B, L, c_void_p(out.data_ptr()),
                byref(t) if taps else None, c_void_p(ws.data_ptr()), ws.numel(),
                c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        ctx.check(rc, fn.__name__)
        return (out, res) if taps else out

    @torch.no_grad()
    def encode_wave48k(self, wave, lengths=None, return_taps: bool = False):
        """wave (B, L) float at 48 kHz on this module's device, 1 <= L <= 480 000 (clip n uses its first lengths[n]
        samples, default L) -> (B, 512) float32 unit-norm embeddings; with return_taps also a dict of the log-mel after
        bn0 (B,1001,64), the patch-embedding tokens, every stage's output and the (B, features) pooled embedding."""
        return self._encode(wave, lengths, return_taps, False)

    @torch.no_grad()
    def encode_wave32k(self, wave, lengths=None, return_taps: bool = False):
        """Same from 32 kHz input, 1 <= L <= 320 000: the 3/2 polyphase resampler runs in front (taps: + 'wave48k')."""
        return self._encode(wave, lengths, return_taps, True)

    def get_query_embed(self, modality, audio=None, text=None, use_text_ratio=0.5, device=None) -> torch.Tensor:
        if modality != "audio":
            raise NotImplementedError(f"ClapAudioEncoder serves modality='audio' only (got {modality!r}); "
                                      "ClapQueryEncoder serves 'text', 'audio' and 'hybird'")
        if audio is None:
            raise ValueError("modality='audio' needs audio=(B, L) at 32 kHz")
        emb = self.encode_wave32k(audio).float()
        return emb.to(device) if device is not None else emb


class ClapQueryEncoder(nn.Module):
    """Both towers behind the reference's `get_query_embed(modality, audio, text, use_text_ratio, device)`."""

    encoder_type = "CLAP"

    def __init__(self, text_encoder: ClapTextEncoder, audio_encoder: ClapAudioEncoder):
        super().__init__()
        self.text_encoder, self.audio_encoder = text_encoder, audio_encoder

    @classmethod
    def from_checkpoint(cls, path: str, tokenizer=None, tokenizer_dir: Optional[str] = None):
        return cls(ClapTextEncoder.from_checkpoint(path, tokenizer=tokenizer, tokenizer_dir=tokenizer_dir),
                   ClapAudioEncoder.from_checkpoint(path))

    def get_query_embed(self, modality, audio=None, text=None, use_text_ratio=0.5, device=None) -> torch.Tensor:
        if modality == "hybird":  # the reference's spelling; one draw per call (models/clap_encoder.py:99-103)
            modality = "audio" if random.random() > use_text_ratio else "text"
        if modality == "audio":
            return self.audio_encoder.get_query_embed("audio", audio=audio, device=device)
        if modality == "text":
            return self.text_encoder.get_query_embed("text", text=text, device=device)
        raise NotImplementedError("Please check flag 'training_modality'.")
