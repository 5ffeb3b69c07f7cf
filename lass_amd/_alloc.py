"""The one place the package allocates what the library is to write: workspaces, scratch buffers and outputs.

By default `empty` / `empty_like` are `torch.empty` / `torch.empty_like`: no fill, no launch.  Inside `poisoned(byte)` - or process-wide
with LASS_POISON=<hex byte> in the environment, read once at import - every such buffer is filled with that byte, and the persistent
ones (the engine's workspace, the towers' cached workspaces) are refilled through `refill` before each call that uses them, on the
call's stream.  No result may change under any fill (include/lass_hip.h, conventions; tests/test_gpu_poison.py): 0xFF is a NaN as
f32 and as bf16, 0x7F is 3.39e38, which survives what a NaN does not (fmaxf, comparisons, integer maxima on the bits).

Buffers whose contract is "zero-filled by the caller" (`clipped`, the `out` of a faded window call) are torch.zeros at their call
sites and never come through here."""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch


def _parse(text: Optional[str]) -> Optional[int]:
    if text is None or text.strip() == "":
        return None
    byte = int(text, 16)
    if not 0 <= byte <= 0xFF:
        raise ValueError(f"LASS_POISON must be one byte in hex (00 ... ff), got {text!r}")
    return byte


_byte: Optional[int] = _parse(os.environ.get("LASS_POISON"))


def poison_byte() -> Optional[int]:
    """The fill in force, None for none."""
    return _byte


@contextlib.contextmanager
def poisoned(byte: int):
    """Every buffer made by `empty` / `empty_like` inside holds `byte` in every byte; `refill` fills.  Nests: the outer setting
    returns on exit."""
    global _byte
    byte = int(byte)
    if not 0 <= byte <= 0xFF:
        raise ValueError(f"a poison fill is one byte (0 ... 255), got {byte}")
    outer, _byte = _byte, byte
    try:
        yield
    finally:
        _byte = outer


def fill_bytes(t: torch.Tensor, byte: int) -> torch.Tensor:
    """Every byte of the contiguous tensor `t` := byte (on the current stream for a device tensor)."""
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(byte)
    return t


def refill(t: torch.Tensor) -> torch.Tensor:
    """A persistent buffer before a call that uses it: filled again under poison, untouched otherwise."""
    return t if _byte is None else fill_bytes(t, _byte)


def empty(*shape, dtype=None, device=None) -> torch.Tensor:
    """torch.empty(*shape, dtype=dtype, device=device), poisoned when a fill is in force."""
    t = torch.empty(*shape, dtype=dtype, device=device)
    return t if _byte is None else fill_bytes(t, _byte)


def empty_like(t: torch.Tensor) -> torch.Tensor:
    """torch.empty_like(t) for a contiguous result, poisoned when a fill is in force."""
    r = torch.empty_like(t)
    if _byte is None:
        return r
    if not r.is_contiguous():
        r = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    return fill_bytes(r, _byte)
