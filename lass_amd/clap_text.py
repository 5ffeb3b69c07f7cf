"""CLAP text encoder on the device: captions -> (N,512) unit-norm query embeddings (the `text` modality of the reference's
`CLAP_Encoder.get_query_embed`, models/clap_encoder.py:78-116).

The module mirrors the parameter tree of the CLAP model's text tower - `model.text_branch.*` (a RoBERTa-base,
CLAP/open_clip/model.py:516-531) and `model.text_projection.{0,2}.*` (Linear -> ReLU -> Linear, :432,454) - so the
`query_encoder.*` sub-dict of an AudioSep Lightning checkpoint loads into it key for key.  torch only holds the weights;
every number is computed by the HIP kernels of lass_amd/csrc/text.hip behind `lass_text_*` (include/lass_hip.h).
There is no CPU fallback and no tokenizer implementation: captions are tokenized by a caller-supplied callable or by
`transformers.RobertaTokenizer` built from a local roberta-base `vocab.json` + `merges.txt`.
"""
from __future__ import annotations

import os
from ctypes import byref, c_size_t, c_void_p
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _alloc, _lib

HIDDEN, HEADS, FFN, PROJ = 768, 12, 3072, 512
VOCAB, MAX_POSITIONS, TYPE_VOCAB = 50265, 514, 1  # roberta-base config.json
LAYER_NORM_EPS = 1e-5                              # roberta-base config.json (not RobertaConfig()'s 1e-12)
MAX_LENGTH, PAD_ID = 512, 1
# the reference's tokenizer call (models/clap_encoder.py:108-116)
TOKENIZER_KWARGS = dict(padding="max_length", truncation=True, max_length=MAX_LENGTH, return_tensors="pt")

_LAYER_PREFIX = "model.text_branch.encoder.layer."
# CLAP model keys that are not the text tower (audio tower, fusion transforms, temperature) and buffers transformers 4.x saved
_IGNORED = ("model.audio_branch.", "model.audio_projection.", "model.logit_scale_")
_IGNORED_EXACT = ("model.text_branch.embeddings.position_ids", "model.text_branch.embeddings.token_type_ids")


def param_specs(layers: int = 12, vocab: int = VOCAB, max_positions: int = MAX_POSITIONS) -> List[Tuple[str, tuple, str]]:
    """(key, shape, kind) of every text-tower parameter in the module's state_dict order; kind is 'w' (matrix), 'g'
    (LayerNorm weight) or 'b' (bias / LayerNorm bias)."""
    e = "model.text_branch.embeddings."
    specs = [(e + "word_embeddings.weight", (vocab, HIDDEN), "w"), (e + "position_embeddings.weight", (max_positions, HIDDEN), "w"),
             (e + "token_type_embeddings.weight", (TYPE_VOCAB, HIDDEN), "w"),
             (e + "LayerNorm.weight", (HIDDEN,), "g"), (e + "LayerNorm.bias", (HIDDEN,), "b")]
    for i in range(layers):
        p = f"{_LAYER_PREFIX}{i}."
        for lin, o, k in (("attention.self.query", HIDDEN, HIDDEN), ("attention.self.key", HIDDEN, HIDDEN),
                          ("attention.self.value", HIDDEN, HIDDEN), ("attention.output.dense", HIDDEN, HIDDEN)):
            specs += [(p + lin + ".weight", (o, k), "w"), (p + lin + ".bias", (o,), "b")]
        specs += [(p + "attention.output.LayerNorm.weight", (HIDDEN,), "g"), (p + "attention.output.LayerNorm.bias", (HIDDEN,), "b"),
                  (p + "intermediate.dense.weight", (FFN, HIDDEN), "w"), (p + "intermediate.dense.bias", (FFN,), "b"),
                  (p + "output.dense.weight", (HIDDEN, FFN), "w"), (p + "output.dense.bias", (HIDDEN,), "b"),
                  (p + "output.LayerNorm.weight", (HIDDEN,), "g"), (p + "output.LayerNorm.bias", (HIDDEN,), "b")]
    specs += [("model.text_branch.pooler.dense.weight", (HIDDEN, HIDDEN), "w"), ("model.text_branch.pooler.dense.bias", (HIDDEN,), "b"),
              ("model.text_projection.0.weight", (PROJ, HIDDEN), "w"), ("model.text_projection.0.bias", (PROJ,), "b"),
              ("model.text_projection.2.weight", (PROJ, PROJ), "w"), ("model.text_projection.2.bias", (PROJ,), "b")]
    return specs


def _module(**children) -> nn.Module:
    m = nn.Module()
    for k, v in children.items():
        m.add_module(k, v)
    return m


def _layer() -> nn.Module:
    ln = lambda: nn.LayerNorm(HIDDEN, eps=LAYER_NORM_EPS)  # noqa: E731
    return _module(attention=_module(self=_module(query=nn.Linear(HIDDEN, HIDDEN), key=nn.Linear(HIDDEN, HIDDEN),
                                                  value=nn.Linear(HIDDEN, HIDDEN)),
                                     output=_module(dense=nn.Linear(HIDDEN, HIDDEN), LayerNorm=ln())),
                   intermediate=_module(dense=nn.Linear(HIDDEN, FFN)),
                   output=_module(dense=nn.Linear(FFN, HIDDEN), LayerNorm=ln()))


class ClapTextEncoder(nn.Module):
    """Drop-in query encoder (`get_query_embed` signature of models/clap_encoder.py:93-106) for the text modality."""

    encoder_type = "CLAP"

    def __init__(self, layers: int = 12, vocab_size: int = VOCAB, max_positions: int = MAX_POSITIONS,
                 tokenizer: Optional[Callable] = None, tokenizer_dir: Optional[str] = None):
        super().__init__()
        with torch.device("meta"):
            emb = _module(word_embeddings=nn.Embedding(vocab_size, HIDDEN),
                          position_embeddings=nn.Embedding(max_positions, HIDDEN),
                          token_type_embeddings=nn.Embedding(TYPE_VOCAB, HIDDEN),
                          LayerNorm=nn.LayerNorm(HIDDEN, eps=LAYER_NORM_EPS))
            branch = _module(embeddings=emb, encoder=_module(layer=nn.ModuleList([_layer() for _ in range(layers)])),
                             pooler=_module(dense=nn.Linear(HIDDEN, HIDDEN)))
            proj = nn.Sequential(nn.Linear(HIDDEN, PROJ), nn.ReLU(), nn.Linear(PROJ, PROJ))
            self.model = _module(text_branch=branch, text_projection=proj)
        self.model.to_empty(device="cpu")  # weights come from a checkpoint; zeros until then
        with torch.no_grad():
            for p in self.model.parameters():
                p.zero_()
        self.layers, self.vocab_size, self.max_positions = layers, vocab_size, max_positions
        self.tokenizer = tokenizer
        self.tokenizer_dir = tokenizer_dir
        self._ctx: Optional[_lib.TowerContext] = None
        self._ws: Optional[torch.Tensor] = None

    # ---- weights ---------------------------------------------------------------------------------------------
    @staticmethod
    def text_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The text-tower entries of a checkpoint state_dict (Lightning `query_encoder.model.*`, a bare
        `query_encoder` dict `model.*`), keyed as this module's state_dict; audio / transform / logit-scale keys and
        the position_ids / token_type_ids buffers are dropped."""
        if any(k.startswith("query_encoder.") for k in sd):
            sd = {k[len("query_encoder."):]: v for k, v in sd.items() if k.startswith("query_encoder.")}
        out = {}
        for k, v in sd.items():
            if not k.startswith("model.") or k.startswith(_IGNORED) or k in _IGNORED_EXACT:
                continue
            if k.split(".")[1].endswith("_transform"):
                continue
            out[k] = v
        return out

    def load_text_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Load a checkpoint's text tower (see text_state_dict); a missing text key is an error that names it."""
        sd = self.text_state_dict(sd)
        own = self.state_dict()
        for k in own:
            if k not in sd:
                raise KeyError(f"checkpoint has no text-tower parameter 'query_encoder.{k}'")
        unexpected = sorted(set(sd) - set(own))
        if unexpected:
            raise KeyError(f"unexpected text-tower parameter(s) 'query_encoder.{unexpected[0]}'"
                           + (f" and {len(unexpected) - 1} more" if len(unexpected) > 1 else ""))
        self.load_state_dict(sd, strict=True)
        return self

    @classmethod
    def from_checkpoint(cls, path: str, tokenizer: Optional[Callable] = None, tokenizer_dir: Optional[str] = None):
        """Text tower of an AudioSep Lightning checkpoint (read with weights_only=True: nothing in the file runs).  The
        layer count, vocabulary and position-table sizes are the checkpoint's."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        sd = cls.text_state_dict(ck.get("state_dict", ck) if isinstance(ck, dict) else ck)
        idx = {int(k[len(_LAYER_PREFIX):].split(".")[0]) for k in sd if k.startswith(_LAYER_PREFIX)}
        layers = max(idx) + 1 if idx else 0
        if layers == 0:
            raise KeyError(f"checkpoint has no text-tower parameter 'query_encoder.{_LAYER_PREFIX}0.*'")
        shape = lambda k, d: sd[k].shape[0] if k in sd else d  # noqa: E731  (a missing key is reported by load_text_state_dict)
        enc = cls(layers=layers, vocab_size=shape("model.text_branch.embeddings.word_embeddings.weight", VOCAB),
                  max_positions=shape("model.text_branch.embeddings.position_embeddings.weight", MAX_POSITIONS),
                  tokenizer=tokenizer, tokenizer_dir=tokenizer_dir)
        return enc.load_text_state_dict(sd)

    # ---- device ----------------------------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self.model.text_projection[0].weight.device

    def _context(self) -> _lib.TowerContext:
        dev = self.device
        if dev.type != "cuda":
            raise _lib.LassError("ClapTextEncoder computes on an MI355X only: move it to a cuda/HIP device first "
                                 "(lass_amd has no CPU fallback)")
        params = list(self.model.named_parameters())  # keys relative to the CLAP model: text_branch.*, text_projection.*
        if self._ctx is None or self._ctx.key != _lib.TowerContext.key_of(dev, params):
            self._ctx = None  # the previous upload is freed before the new one is made
            self._ctx = _lib.TowerContext("lass_text", dev, params)
        return self._ctx

    # ---- compute ---------------------------------------------------------------------------------------------
    def _validate(self, input_ids, attention_mask) -> Tuple[torch.Tensor, torch.Tensor]:
        ids = torch.as_tensor(input_ids).detach().to("cpu")
        mask = torch.as_tensor(attention_mask).detach().to("cpu")
        if ids.dim() != 2 or mask.shape != ids.shape:
            raise ValueError(f"input_ids and attention_mask must be (N, S) of the same shape, got {tuple(ids.shape)} "
                             f"and {tuple(mask.shape)}")
        N, S = ids.shape
        if N < 1 or S < 1:
            raise ValueError("empty batch")
        if S > MAX_LENGTH or S + 2 > self.max_positions:
            raise ValueError(f"sequence length {S} exceeds {min(MAX_LENGTH, self.max_positions - 2)} tokens")
        if ids.dtype.is_floating_point or mask.dtype.is_floating_point:
            raise ValueError("input_ids and attention_mask must be integer tensors")
        ids, mask = ids.to(torch.int64).contiguous(), mask.to(torch.int64).contiguous()
        if bool(((ids < 0) | (ids >= self.vocab_size)).any()):
            raise ValueError(f"token id out of range [0, {self.vocab_size})")
        if bool(((mask != 0) & (mask != 1)).any()):
            raise ValueError("attention_mask must hold 0 / 1")
        if not bool((mask[:, 0] == 1).all()):
            raise ValueError("attention_mask[:, 0] must be 1 for every caption (the <s> token)")
        return ids, mask

    @torch.no_grad()
    def encode_ids(self, input_ids, attention_mask, return_pooler: bool = False):
        """input_ids, attention_mask (N, S) integer (S <= 512) -> (N, 512) float32 unit-norm embeddings on this module's
        device; with return_pooler also the (N, 768) RoBERTa pooler_output.  All checks run on the host first."""
        ids, mask = self._validate(input_ids, attention_mask)
        ctx = self._context()
        dev = self.device
        N, S = ids.shape
        n = c_size_t()
        ctx.check(ctx.lib.lass_text_workspace_bytes(ctx.ctx, N, S, byref(n)), "lass_text_workspace_bytes")
        ws = _lib.grow_workspace(self, n.value, dev)
        ids_dev = ids.to(dev)
        out = _alloc.empty(N, PROJ, dtype=torch.float32, device=dev)
        pool = _alloc.empty(N, HIDDEN, dtype=torch.float32, device=dev) if return_pooler else None
        rc = ctx.lib.lass_text_encode(ctx.ctx, c_void_p(ids_dev.data_ptr()), c_void_p(mask.data_ptr()), N, S,
                                      c_void_p(out.data_ptr()), c_void_p(pool.data_ptr() if pool is not None else 0),
                                      c_void_p(ws.data_ptr()), ws.numel(),
                                      c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        ctx.check(rc, "lass_text_encode")
        return (out, pool) if return_pooler else out

    def _tokenizer(self) -> Callable:
        if self.tokenizer is not None:
            return self.tokenizer
        if self.tokenizer_dir is None:
            raise RuntimeError("ClapTextEncoder has no tokenizer: pass tokenizer=<callable> or tokenizer_dir=<directory "
                               "holding roberta-base's vocab.json and merges.txt> (no tokenizer is bundled and nothing is "
                               "downloaded)")
        from transformers import RobertaTokenizer

        self.tokenizer = RobertaTokenizer(vocab_file=os.path.join(self.tokenizer_dir, "vocab.json"),
                                          merges_file=os.path.join(self.tokenizer_dir, "merges.txt"))
        return self.tokenizer

    def tokenize(self, text: List[str]):
        """models/clap_encoder.py:108-116 (the batch is never squeezed here: encode_ids takes (N, S))."""
        return self._tokenizer()(text, **TOKENIZER_KWARGS)

    def get_query_embed(self, modality, audio=None, text=None, use_text_ratio=0.5, device=None) -> torch.Tensor:
        if modality != "text":
            raise NotImplementedError(f"ClapTextEncoder serves modality='text' only (got {modality!r}); the audio tower "
                                      "(HTSAT) is not implemented")
        if text is None:
            raise ValueError("modality='text' needs text=[captions]")
        tok = self.tokenize(list(text))
        emb = self.encode_ids(tok["input_ids"], tok["attention_mask"]).float()
        return emb.to(device) if device is not None else emb
