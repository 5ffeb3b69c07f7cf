"""The float64 statement of the linked-channel semantics, shared by tests/test_linked_cpu.py and
tests/test_linked_gpu.py.  The network, the transforms and the mask's three maps are the oracle's own functions, run in float64;
what is new - the mask as a complex number and its product with each plane's spectrum - is numpy."""
import numpy as np
import torch

from oracle import resunet as orr
from oracle import stft as ostft


def complex_mask(logits: torch.Tensor):
    """(B,3,T,F) logits -> (M_re, M_im) (B,T,F) float64 numpy: M = sigmoid(l0) * (mc + i ms), (mc, ms) the unit phasor of
    (tanh(l1), tanh(l2)) by the oracle's magphase (resunet.py:436-519 with a unit input spectrum)."""
    mask_mag = torch.sigmoid(logits[:, 0:1])
    _, mc, ms = ostft.magphase(torch.tanh(logits[:, 1:2]), torch.tanh(logits[:, 2:3]))
    return (mask_mag * mc)[:, 0].numpy(), (mask_mag * ms)[:, 0].numpy()


def linked_forward(sd64, guide: np.ndarray, planes: np.ndarray, cond: np.ndarray, n_fft: int = 1024, hop: int = 160) -> np.ndarray:
    """guide (B,L), planes (C,B,L), cond (B,512) -> (C,B,L) float64.  sd64: orr.to_torch(state dict, torch.float64).  (The oracle's
    network is the (1024, 160) geometry's.)"""
    assert (n_fft, hop) == (1024, 160)
    g = torch.from_numpy(np.asarray(guide, dtype=np.float64))
    taps = {}
    orr.forward(sd64, {"mixture": g[:, None, :], "condition": torch.from_numpy(np.asarray(cond, dtype=np.float64))}, taps)
    m_re, m_im = complex_mask(taps["logits"])
    out = []
    for plane in np.asarray(planes, dtype=np.float64):
        re, im = ostft.stft_fft(torch.from_numpy(plane))
        x_re, x_im = re[:, 0].numpy(), im[:, 0].numpy()
        y_re = x_re * m_re - x_im * m_im
        y_im = x_re * m_im + x_im * m_re
        wav = ostft.istft_fft(torch.from_numpy(y_re)[:, None], torch.from_numpy(y_im)[:, None], plane.shape[-1])
        out.append(wav.reshape(plane.shape).numpy())
    return np.stack(out)


def stitch(total: int, plan, per_window) -> np.ndarray:
    """The kept ranges of `plan` ((start, lo, hi) rows, hard seams) of the windows' outputs, in one row."""
    out = np.zeros(total, dtype=np.float64)
    for (s, lo, hi), w in zip(plan, per_window):
        out[s + lo:s + hi] = w[lo:hi]
    return out
