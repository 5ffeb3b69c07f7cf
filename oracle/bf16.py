"""A model of the bf16 MFMA modes, launch by launch (TEST INFRASTRUCTURE - see oracle/__init__.py).

The bf16 kernels (lass_amd/csrc/conv_bf16.hip, conv_bf16_fused.hip) round their conv operands to bf16 at the points
DESIGN.md "bf16 MFMA modes" names and accumulate in f32.  This module restates one ConvBlockRes and one kernel = stride
transposed conv with exactly those rounding points, in torch on the CPU with the arithmetic type a parameter:

* every conv operand is rounded after its BN + FiLM + leaky prologue, weights are rounded as stored.  The prologue is f32
  arithmetic in every kernel - leaky(fma(x, s, h)) with s = g / sqrt(var + eps) and the per-clip shift h = beta - mean s + FiLM
  (lass_film's output) as f32 values - so r(.) of an activated operand is "to f32 by that formula, then RNE to bf16" in the
  float64 model too, and the shifts are INPUTS of the model: a GPU test hands it the vector the launches read;
* the block intermediate is r(act2(conv1));
* the 1x1 shortcut reads the raw input rounded, with weights r(Wsc);
* bias, identity residual, pooling, after_conv and the mask stay unrounded.

`pieces=1` is LASS_COMPUTE_BF16; `pieces=2` is LASS_COMPUTE_BF16X3 (operands hi + lo, the lo x lo product left out).
`dtype=torch.float64` is the reference; `dtype=torch.float32` is the same model with the contractions (and pooling, after_conv,
the mask) in f32 - one algorithm at every shape: ATen's own convolution, not oneDNN's choice among direct, GEMM and Winograd
forms - and measures what f32 accumulation alone costs: the yardstick D the GPU tests scale their bars by.  Every function also returns the
elementwise scale S (the same contractions over |operands| and |weights|): errors are read as |got - ref| / S.

A launch inside lass_separate reads and writes blocked bf16 copies; the functions take such copies as given
(`act_copy`, `raw_copy`: already rounded, used as they are) and `copies` / `pool` form what a launch writes.  `unblock`
decodes the hand-over layout [C/8][H][W][8 x bf16] of api.hip's separate_impl.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

LEAK = 0.01
BN_EPS = 1e-5

# the ways the model can be made wrong on purpose (tests/test_bf16_oracle_cpu.py: the bars can tell right from wrong)
MUTATIONS = ("w_trunc", "mid_unrounded", "drop_tap", "replicate_pad", "row_shift", "film_swap", "cout_swap", "raw_for_act")


# ---- rounding -----------------------------------------------------------------------------------------------------------
def _round_bits(t: torch.Tensor, nearest: bool) -> torch.Tensor:
    """Keep sign, exponent and 7 mantissa bits of t (f32: drop 16 bits; f64: drop 45 - same grid inside bf16's range)."""
    if t.dtype == torch.float32:
        bits, drop = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF, 16
    elif t.dtype == torch.float64:
        bits, drop = t.contiguous().view(torch.int64), 45
    else:
        raise TypeError(t.dtype)
    if nearest:  # round to nearest, ties to even: add half an ulp minus one, plus the bit that will be the last kept
        bits = bits + ((bits >> drop) & 1) + ((1 << (drop - 1)) - 1)
    bits = (bits >> drop) << drop
    if t.dtype == torch.float32:
        bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
        return bits.view(torch.float32)
    return bits.view(torch.float64)


def rne_bf16(t: torch.Tensor) -> torch.Tensor:
    """t rounded to the nearest bf16 value (ties to even), returned in t's own dtype.  Finite input."""
    return _round_bits(t, True)


def trunc_bf16(t: torch.Tensor) -> torch.Tensor:
    """t with the mantissa cut to bf16's (round toward zero): what a conversion by shifting would do."""
    return _round_bits(t, False)


def split2(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hi, lo) of weights_bf16_kernel and the staging of the split mode: hi = r(t), lo = r(t - hi)."""
    hi = rne_bf16(t)
    return hi, rne_bf16(t - hi)


def _q(t, pieces, rnd=rne_bf16):
    hi = rnd(t)
    return (hi,) if pieces == 1 else (hi, rnd(t - hi))


def _contract(fn, a, w):
    """fn(a, w) over split operands: (hi + lo)(hi + lo) - lo lo = hi hi + hi lo + lo hi."""
    y = fn(sum(a), sum(w))
    if len(a) == 2 and len(w) == 2:
        y = y - fn(a[1], w[1])
    return y


def _scale(fn, a, w):
    return fn(sum(a).abs(), sum(w).abs())


# ---- the blocked hand-over layout ---------------------------------------------------------------------------------------
def unblock(buf, B: int, C: int, H: int, W: int) -> torch.Tensor:
    """buf: the bytes of ONE blocked copy, [B][C/8][H][W][8 x bf16] (clip stride (C/8) H W 16 bytes; in a concat or pooled
    slot the activated copy comes first and the raw copy B C H W 2 bytes behind it) -> (B, C, H, W) float32."""
    if not torch.is_tensor(buf):
        buf = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    n = B * C * H * W
    u = buf.contiguous().view(torch.uint8)[:2 * n].view(torch.int16).to(torch.int32)
    f = (u << 16).view(torch.float32).reshape(B, C // 8, H, W, 8)
    return f.permute(0, 1, 4, 2, 3).reshape(B, C, H, W).contiguous()


# ---- prologues ----------------------------------------------------------------------------------------------------------
def site_bn(site: str) -> str:
    """'encoder_block2->conv_block1->beta1' -> 'base.encoder_block2.conv_block1.bn1' (the BatchNorm a FiLM site shifts)"""
    return "base." + site.replace("->", ".").replace("beta", "bn")


def bn_scale(sd, bn: str) -> torch.Tensor:
    """s = g * (1 / sqrt(var + eps)) as bnfold_kernel (misc.hip) forms it: four correctly rounded f32 operations, (C,).
    (numpy, step by step: torch's `sqrt(v + 1e-5)` on a float32 tensor is one ulp off that on some channels, and one ulp of s
    moves an operand across a bf16 rounding boundary about once in 1e5 elements - seen as isolated errors of 30-500 x D.)"""
    g, v = (sd[f"{bn}.{k}"].float().numpy().astype(np.float32) for k in ("weight", "running_var"))
    inv = np.float32(1.0) / np.sqrt(v + np.float32(BN_EPS), dtype=np.float32)
    return torch.from_numpy((g * inv).astype(np.float32))


def shift(sd, cond: torch.Tensor, site: str) -> torch.Tensor:
    """The per-clip shift of a FiLM site as lass_film writes it, computed here in f32: beta - mean s + FiLM(cond), (B, C).
    (A GPU test passes the engine's own vector instead: the launches are then modelled on the shifts they really read.)"""
    bn = site_bn(site)
    base = sd[bn + ".bias"].float() - sd[bn + ".running_mean"].float() * bn_scale(sd, bn)
    return base[None, :] + F.linear(cond.float(), sd[f"film.{site}.weight"].float(), sd[f"film.{site}.bias"].float())


_LEAK32 = float(torch.tensor(LEAK, dtype=torch.float32))


def _f32(t64: torch.Tensor) -> torch.Tensor:
    return t64.float()


def act(x: torch.Tensor, s: torch.Tensor, h: torch.Tensor, dtype) -> torch.Tensor:
    """leaky(fma(x, s, h)) in f32 - the prologue of every kernel (pixel_ops.h: fmaxf(v, 0.01f v)) - returned in `dtype`.
    x (B, C, H, W) in any float type (a float64 x is rounded once, as the fma does); s (C,), h (B, C) f32."""
    t = _f32(x.double() * s.double()[None, :, None, None] + h.double()[:, :, None, None])
    return torch.maximum(t, _f32(t.double() * _LEAK32)).to(dtype)


def pool(y, down):
    return F.avg_pool2d(y, kernel_size=tuple(down))


class _plain_f32:
    """ATen's own f32 convolution (im2col + GEMM) at every shape while the float32 model runs."""

    def __init__(self, dtype):
        self.ctx = torch.backends.mkldnn.flags(enabled=False) if dtype == torch.float32 else None

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _tile_row0(H: int, W: int) -> int:
    """First row of the last row tile: 8-row tiles at W >= 16, 32-row tiles at W = 8."""
    t = 8 if W >= 16 else 32
    return ((H - 1) // t) * t


def _conv3(a, w, replicate_left=False):
    a = F.pad(a, (1, 1, 1, 1))
    if replicate_left:
        a = a.clone()
        a[..., :, 0] = a[..., :, 1]
    return F.conv2d(a, w)


def _swap_pair(C):
    return (31, 32) if C > 32 else (15, 16)  # a 32-cout block has no cout 32: the same swap across its octet border


# ---- one ConvBlockRes ---------------------------------------------------------------------------------------------------
def _block(sd, prefix: str, x: Optional[torch.Tensor], h1, h2, pieces: int = 1, dtype=torch.float64,
          act_copy: Optional[torch.Tensor] = None, raw_copy: Optional[torch.Tensor] = None, mutate: Optional[str] = None,
          shortcut=None, rows: Optional[int] = None, mid_copy=None):
    """resunet.py:147-165 with the bf16 modes' rounding points.  x: the raw input (B, Cin, H, W); h1, h2: the shifts (B, C)
    of bn1 and bn2 (`shift`); act_copy / raw_copy: the
    blocked copies a launch inside lass_separate reads instead (conv1's operand, prologue applied; the shortcut's operand).
    shortcut: (value, scale) of the 1x1 shortcut without its bias, where the launch forms it another way (dec6u).
    rows: the rows of the output that anything reads (the output head masks the padded frames), for the row_shift mutation.
    mid_copy: the intermediate conv1's launch really wrote ((hi,) or (hi, lo)), where the caller can read it (the stage calls'
    scratch): conv2 is then modelled on it, and the returned `mid` is (t, St) - the model's own unrounded act2(conv1) and its
    scale - for the caller to hold the written intermediate to.
    Returns (y, S, mid): output, elementwise scale, and the intermediate r(act2(conv1)) (its hi + lo sum for pieces = 2)."""
    assert mutate is None or mutate in MUTATIONS
    wr = trunc_bf16 if mutate == "w_trunc" else rne_bf16
    w1 = sd[prefix + ".conv1.weight"].to(dtype)
    w2 = sd[prefix + ".conv2.weight"].to(dtype)
    s1, s2 = bn_scale(sd, prefix + ".bn1"), bn_scale(sd, prefix + ".bn2")
    if mutate == "film_swap":
        h1, h2 = h1.clone(), h2.clone()
        h1[1], h2[1] = h1[0], h2[0]
    if x is not None:
        x = x.to(dtype)
    if mutate == "raw_for_act":
        a1 = _q(x if raw_copy is None else raw_copy.to(dtype), pieces)
    elif act_copy is not None:
        a1 = (act_copy.to(dtype),)
    else:
        a1 = _q(act(x, s1, h1, dtype), pieces)
    W1 = _q(w1, pieces, wr)
    if mutate == "drop_tap":  # one tap of the last 16-channel chunk
        W1 = tuple(w.clone() for w in W1)
        for w in W1:
            w[:, -16:, 0, 2] = 0
    rep = mutate == "replicate_pad"
    c1 = _contract(lambda a, w: _conv3(a, w, rep), a1, W1)
    t = act(c1, s2, h2, dtype)
    a2 = (t,) if mutate == "mid_unrounded" else _q(t, pieces)
    if mid_copy is not None:
        a2 = tuple(m.to(dtype) for m in mid_copy)
        St = _scale(lambda a, w: _conv3(a, w, rep), a1, W1) * s2.abs().to(dtype)[None, :, None, None]
    W2 = _q(w2, pieces, wr)
    y = _contract(_conv3, a2, W2)
    S = _scale(_conv3, a2, W2)
    if (prefix + ".shortcut.weight") in sd:
        wsc = sd[prefix + ".shortcut.weight"].to(dtype)
        bias = sd[prefix + ".shortcut.bias"].to(dtype)[None, :, None, None]
        if shortcut is not None:
            y = y + shortcut[0] + bias
            S = S + shortcut[1] + bias.abs()
        else:
            xr = (raw_copy.to(dtype),) if raw_copy is not None else _q(x, pieces)
            Wsc = _q(wsc, pieces, wr)
            y = y + _contract(F.conv2d, xr, Wsc) + bias
            S = S + _scale(F.conv2d, xr, Wsc) + bias.abs()
    else:
        y = y + x
        S = S + x.abs()
    H, W = y.shape[-2:]
    H = rows or H
    if mutate == "row_shift":
        r0 = _tile_row0(H, W)
        y = y.clone()
        y[:, :, r0:H - 1] = y[:, :, r0 + 1:H].clone()
    if mutate == "cout_swap":
        i, j = _swap_pair(y.shape[1])
        y = y.clone()
        y[:, [i, j]] = y[:, [j, i]]
    return y, S, ((t, St) if mid_copy is not None else sum(a2))


# ---- one transposed conv (kernel = stride) ------------------------------------------------------------------------------
def _upconv(sd, name: str, x: Optional[torch.Tensor], h, up, pieces: int = 1, dtype=torch.float64,
           act_copy: Optional[torch.Tensor] = None, mutate: Optional[str] = None):
    """resunet.py:240-247 (bn1 + FiLM + leaky, ConvTranspose2d) of decoder `name` ('base.decoder_block3').  x: the raw input;
    act_copy: the producer's activated blocked copy instead.  Returns (y, S)."""
    assert mutate is None or mutate in MUTATIONS
    wr = trunc_bf16 if mutate == "w_trunc" else rne_bf16
    w = sd[name + ".conv1.weight"].to(dtype)  # (cin, cout, uh, uw)
    s = bn_scale(sd, name + ".bn1")
    if mutate == "film_swap":
        h = h.clone()
        h[1] = h[0]
    if x is not None:
        x = x.to(dtype)
    if mutate == "raw_for_act":
        a = _q(x, pieces)
    elif act_copy is not None:
        a = (act_copy.to(dtype),)
    else:
        a = _q(act(x, s, h, dtype), pieces)
    Wt = _q(w, pieces, wr)
    if mutate == "drop_tap":
        Wt = tuple(v.clone() for v in Wt)
        for v in Wt:
            v[-16:, :, 0, 1] = 0
    fn = lambda a_, w_: F.conv_transpose2d(a_, w_, stride=tuple(up))
    y = _contract(fn, a, Wt)
    S = _scale(fn, a, Wt)
    if mutate == "row_shift":
        r0 = _tile_row0(a[0].shape[-2], a[0].shape[-1]) * up[0]
        y = y.clone()
        y[:, :, r0:y.shape[2] - 1] = y[:, :, r0 + 1:].clone()
    if mutate == "cout_swap":
        i, j = _swap_pair(y.shape[1])
        y = y.clone()
        y[:, [i, j]] = y[:, [j, i]]
    return y, S


def block(*args, **kw):
    with _plain_f32(kw.get("dtype", args[6] if len(args) > 6 else torch.float64)):
        return _block(*args, **kw)


def upconv(*args, **kw):
    with _plain_f32(kw.get("dtype", args[6] if len(args) > 6 else torch.float64)):
        return _upconv(*args, **kw)


block.__doc__, upconv.__doc__ = _block.__doc__, _upconv.__doc__


# ---- decoder_block6 with the output head --------------------------------------------------------------------------------
def composed_up_shortcut(sd, dtype=torch.float64) -> torch.Tensor:
    """dec6u_fused: the 1x1 shortcut over the up-sampled half of decoder_block6's concat composed with its transposed conv,
    W'[n][ci][a][b] = sum_co Wsc[n][co] Wt[ci][co][a][b], formed in double and rounded once."""
    wsc = sd["base.decoder_block6.conv_block2.shortcut.weight"].double()[:, :, 0, 0]
    wt = sd["base.decoder_block6.conv1.weight"].double()
    co = wt.shape[1]
    return rne_bf16(torch.einsum("no,ioab->niab", wsc[:, :co], wt)).to(dtype)


def head(sd, y, mag, cos_in, sin_in, T: int, dtype=torch.float64):
    """after_conv + the complex ratio mask (resunet.py:570-574, 436-519) on decoder_block6's output y (B, 32, Tp, 512), all in
    `dtype`: -> (out_real, out_imag) (B, 1, T, 513), and the logits (B, 3, T, 513)."""
    x = F.conv2d(y.to(dtype), sd["base.after_conv.weight"].to(dtype), sd["base.after_conv.bias"].to(dtype))
    x = F.pad(x, (0, 1))[:, :, 0:T, :]
    mag, cos_in, sin_in = (t.to(dtype).reshape(t.shape[0], 1, T, -1) for t in (mag, cos_in, sin_in))
    mask_mag = torch.sigmoid(x[:, 0:1])
    mr, mi = torch.tanh(x[:, 1:2]), torch.tanh(x[:, 2:3])
    mm = torch.clamp((mr * mr + mi * mi).sqrt(), min=1e-10)  # torchlibrosa magphase: the clamp is on |M|
    mc, ms = mr / mm, mi / mm
    out_mag = F.relu(mag * mask_mag)
    return out_mag * (cos_in * mc - sin_in * ms), out_mag * (sin_in * mc + cos_in * ms), x


def err(got: torch.Tensor, ref: torch.Tensor, S: torch.Tensor) -> Tuple[float, float]:
    """(max, RMS) of |got - ref| / S."""
    e = (got.double() - ref.double()).abs() / S.double().clamp_min(1e-30)
    return float(e.max()), float(e.pow(2).mean().sqrt())


# ---- the whole network, free-running (f32 hand-overs: LASS_COMPUTE_BF16X3, or bf16 with LASS_FUSE_CATB=0) ---------------
_ENC = (("encoder_block1", 32, 32, (2, 2)), ("encoder_block2", 32, 64, (2, 2)), ("encoder_block3", 64, 128, (2, 2)),
        ("encoder_block4", 128, 256, (2, 2)), ("encoder_block5", 256, 384, (2, 2)), ("encoder_block6", 384, 384, (1, 2)),
        ("conv_block7a", 384, 384, (1, 1)))
_DEC = (("decoder_block1", 384, 384, (1, 2)), ("decoder_block2", 384, 384, (2, 2)), ("decoder_block3", 384, 256, (2, 2)),
        ("decoder_block4", 256, 128, (2, 2)), ("decoder_block5", 128, 64, (2, 2)), ("decoder_block6", 64, 32, (2, 2)))


def pre_conv(sd, x0, dtype):
    """resunet.py:555 on the one-channel x0 (B, 1, Tp, 512), as encoder_block1's kernels form it while staging: one f32 fma."""
    w = sd["base.pre_conv.weight"].double().reshape(1, -1, 1, 1)
    return _f32(x0.double() * w + sd["base.pre_conv.bias"].double().reshape(1, -1, 1, 1)).to(dtype)


def forward_taps(sd, taps_in: dict, shifts, pieces: int, dtype=torch.float64) -> dict:
    """The U-Net between x0 and the separated spectrum with every conv through `block` / `upconv` and f32 tensors between
    launches (what bf16x3 runs).  taps_in: the plain oracle's taps (x0, mag, cos, sin of the same clip); shifts(site) -> (B, C).
    Returns the tensors of oracle.resunet.base_forward's taps, under the same names."""
    out = {}
    x = pre_conv(sd, taps_in["x0"], dtype)
    T = taps_in["mag"].shape[2]
    skips = []
    for name, _cin, _cout, down in _ENC:
        stem = f"{name}->conv_block1"
        y, _, _ = block(sd, f"base.{name}.conv_block1", x, shifts(stem + "->beta1"), shifts(stem + "->beta2"), pieces, dtype)
        y = y.float().to(dtype)  # the launch stores f32
        x = pool(y, down).float().to(dtype)
        skips.append(y)
        out[name] = y
        out[name + ".pool"] = x
    skips.pop()
    for name, _cin, _cout, up in _DEC:
        u, _ = upconv(sd, f"base.{name}", x, shifts(f"{name}->beta1"), up, pieces, dtype)
        u = u.float().to(dtype)
        out[name + ".up"] = u
        stem = f"{name}->conv_block2"
        x, _, _ = block(sd, f"base.{name}.conv_block2", torch.cat((u, skips.pop()), 1), shifts(stem + "->beta1"), shifts(stem + "->beta2"),
                        pieces, dtype)
        x = x.float().to(dtype)
        out[name] = x
    with _plain_f32(dtype):
        out["out_real"], out["out_imag"], _ = head(sd, x, taps_in["mag"], taps_in["cos"], taps_in["sin"], T, dtype)
    return out


# ---- one lass_separate in mode bf16, launch by launch (teacher forcing) ---------------------------------------------------
def levels(t_pad: int):
    """(H, W) of encoder level i (conv_route.h: model_levels)."""
    lv, h, w = [], t_pad, 512
    for _n, _ci, _co, down in _ENC:
        lv.append((h, w))
        h, w = h // down[0], w // down[1]
    return lv


class Out:
    """One tensor a launch writes.  key: its name in the store (a workspace tensor's name for f32, 'cat<d>.act' / '.raw',
    'pool<i>.act' / '.raw', 'decout<d>.act' for the blocked copies); ch0: first channel inside that tensor; value: the
    model's unrounded value; S: its elementwise scale; bf16: written rounded, as a blocked copy."""

    def __init__(self, key, ch0, value, S, bf16):
        self.key, self.ch0, self.value, self.S, self.bf16 = key, ch0, value, S, bf16


class Launch:
    """name: the block or transposed conv with the form it runs in; reads: {store key: tensor} it was built from; form: its
    hand-overs as the plan states them; model(dtype, mutate=None) -> [Out].
    replay: None, or (kind, block, cout, pool) of a block that runs as two launches on an f32 input reads["x"].  Its conv1 launch
    is the one the stage call of that block makes on the same tensor, so a caller can repeat it and read the intermediate, which
    inside lass_separate lies in a slot that later blocks overwrite; model(dtype, mid=(hi,)) then models conv2 on that
    intermediate and returns, first, Out("mid", ...): the model's own unrounded act2(conv1) and its scale."""

    def __init__(self, name, reads, model, form="", replay=None):
        self.name, self.reads, self.model, self.form, self.replay = name, reads, model, form, replay


def _act_out(key, ch0, y, S, s, h, dtype, mutate=None):
    """An activated blocked copy of y: the consumer's prologue (s (C,), h (B, C)) applied in the producer's epilogue."""
    if mutate == "film_swap":
        h = h.clone()
        h[1] = h[0]
    return Out(key, ch0, act(y, s, h, dtype), S * s.abs().to(dtype)[None, :, None, None], True)


def _dec6u_block(sd, a_low, skip_act, skip_raw, h1, h2, dtype, mutate, rows):
    """decoder_block6 with its transposed conv inside (dec6u_fused): the up-sampled half of the concat is formed from the
    activated low-resolution copy, its share of the 1x1 shortcut by the composed weights."""
    name, co = "base.decoder_block6", 32
    a_low, skip_act, skip_raw = a_low.to(dtype), skip_act.to(dtype), skip_raw.to(dtype)
    wt = rne_bf16(sd[name + ".conv1.weight"].to(dtype))
    up = F.conv_transpose2d(a_low, wt, stride=(2, 2))
    s1 = bn_scale(sd, name + ".conv_block2.bn1")
    act_up = rne_bf16(act(up, s1[:co], h1[:, :co], dtype))
    wc = composed_up_shortcut(sd, dtype).permute(1, 0, 2, 3).contiguous()  # (ci, n, a, b)
    wsk = rne_bf16(sd[name + ".conv_block2.shortcut.weight"].to(dtype))[:, co:]
    sc = F.conv_transpose2d(a_low, wc, stride=(2, 2)) + F.conv2d(skip_raw, wsk)
    sS = F.conv_transpose2d(a_low.abs(), wc.abs(), stride=(2, 2)) + F.conv2d(skip_raw.abs(), wsk.abs())
    return _block(sd, name + ".conv_block2", None, h1, h2, 1, dtype, act_copy=torch.cat((act_up, skip_act), 1),
                  raw_copy=torch.cat((rne_bf16(up), skip_raw), 1), mutate=mutate, shortcut=(sc, sS), rows=rows)


def _head_outs(sd, y, S, mag, cos_in, sin_in, T, dtype):
    """out_real / out_imag with a first-order scale: |d out| <= mag (S_l0 + (S_l1 + S_l2) / |m|), m the complex mask before
    its normalisation (sigmoid' <= 1, tanh' <= 1, |d (m / |m|)| <= |dm| / |m|)."""
    re, im, x = head(sd, y, mag, cos_in, sin_in, T, dtype)
    wl = sd["base.after_conv.weight"].to(dtype).abs()
    Sl = F.pad(F.conv2d(S.to(dtype), wl, sd["base.after_conv.bias"].to(dtype).abs()), (0, 1))[:, :, 0:T, :]
    m = (torch.tanh(x[:, 1:2]) ** 2 + torch.tanh(x[:, 2:3]) ** 2).sqrt().clamp_min(1e-3)
    So = mag.to(dtype).reshape(re.shape) * (Sl[:, 0:1] + (Sl[:, 1:2] + Sl[:, 2:3]) / m)
    return [Out("out_real", 0, re, So, False), Out("out_imag", 0, im, So, False)]


def separate_launches(sd, shifts, plan: dict, store, t_pad: int, T: int):
    """Generator over the conv launches of one ResUNet30 lass_separate in mode bf16, in stream order.  shifts(site) -> the
    (B, C) f32 shift of a FiLM site (`shift`, or the engine's own vector); plan: the hand-over table {"bf16": {block: {form,
    cat_in, skip_out, pool_copies, act_out}}, "up": {decoder: (family, in_act, out_copies)}} as tools/route_table.cpp prints
    it; store.get(key) returns the tensor a launch reads (what the producer really wrote).  A launch is built - its inputs are
    read - when the generator reaches it, so a caller that fills the store from the model's own outputs gets the free-running
    chain."""
    for i, (name, cin, cout, down) in enumerate(_ENC):
        p = plan["bf16"][name]
        if i == 0:
            reads = {"x0": store.get("x0")}
        elif p["cat_in"]:
            reads = {k: store.get(f"pool{i - 1}.{k}") for k in ("act", "raw")}
        else:
            reads = {"x": store.get(_ENC[i - 1][0] + ".pool")}

        def model(dtype, mutate=None, mid=None, i=i, name=name, cout=cout, down=down, p=p, reads=reads):
            prefix, stem, d = f"base.{name}.conv_block1", f"{name}->conv_block1", 5 - i
            h1, h2 = shifts(stem + "->beta1"), shifts(stem + "->beta2")
            assert mid is None or "x" in reads
            with _plain_f32(dtype):
                if i == 0:
                    y, S, _ = _block(sd, prefix, pre_conv(sd, reads["x0"], dtype), h1, h2, 1, dtype, mutate=mutate)
                elif p["cat_in"]:
                    y, S, _ = _block(sd, prefix, None, h1, h2, 1, dtype, act_copy=reads["act"], raw_copy=reads["raw"], mutate=mutate)
                else:
                    y, S, m = _block(sd, prefix, reads["x"], h1, h2, 1, dtype, mutate=mutate, mid_copy=mid)
                outs = [] if mid is None else [Out("mid", 0, m[0], m[1], True)]
                if p["skip_out"]:  # into the concat of decoder d, behind its transposed conv's channels, with that block's prologue
                    dn, dco = _DEC[d][0], _DEC[d][2]
                    s, h = bn_scale(sd, f"base.{dn}.conv_block2.bn1")[dco:], shifts(f"{dn}->conv_block2->beta1")[:, dco:]
                    outs += [Out(f"cat{d}.raw", dco, y, S, True), _act_out(f"cat{d}.act", dco, y, S, s, h, dtype, mutate)]
                else:
                    outs.append(Out(name, 0, y, S, False))
                if i < 6:
                    py, pS = pool(y, down), pool(S, down)
                    if p["pool_copies"]:
                        nn_ = _ENC[i + 1][0]
                        s, h = bn_scale(sd, f"base.{nn_}.conv_block1.bn1"), shifts(f"{nn_}->conv_block1->beta1")
                        outs += [Out(f"pool{i}.raw", 0, py, pS, True), _act_out(f"pool{i}.act", 0, py, pS, s, h, dtype, mutate)]
                    else:
                        outs.append(Out(name + ".pool", 0, py, pS, False))
            return outs

        yield Launch(f"{name} ({p['form']})", reads, model, repr(sorted(p.items())),
                     ("enc", name, cout, down) if "x" in reads and p["form"] == "two" else None)
    for d, (name, cin, cout, up) in enumerate(_DEC):
        p, u = plan["bf16"][name], plan["up"][name]
        prev = "conv_block7a" if d == 0 else _DEC[d - 1][0]
        if u[0] != "inside":
            reads = {"act": store.get(f"decout{d - 1}.act")} if u[1] else {"x": store.get(prev)}

            def upmodel(dtype, mutate=None, name=name, cout=cout, up=up, u=u, d=d, reads=reads):
                y, S = upconv(sd, f"base.{name}", reads.get("x"), shifts(f"{name}->beta1"), up, 1, dtype, act_copy=reads.get("act"),
                              mutate=mutate)
                if not u[2]:
                    return [Out(name + ".up", 0, y, S, False)]
                s, h = bn_scale(sd, f"base.{name}.conv_block2.bn1")[:cout], shifts(f"{name}->conv_block2->beta1")[:, :cout]
                return [Out(f"cat{d}.raw", 0, y, S, True), _act_out(f"cat{d}.act", 0, y, S, s, h, dtype, mutate)]

            yield Launch(f"{name}.up", reads, upmodel, repr(u))
        if p["form"] == "dec6u":
            reads = {"low": store.get(f"decout{d - 1}.act"), "act": store.get(f"cat{d}.act")[:, cout:],
                     "raw": store.get(f"cat{d}.raw")[:, cout:]}
        elif p["cat_in"]:
            reads = {k: store.get(f"cat{d}.{k}") for k in ("act", "raw")}
        else:
            reads = {"x": store.get(f"cat{d}.f32")}
        if d == 5:
            reads.update({k: store.get(k) for k in ("mag", "cos", "sin")})

        def bmodel(dtype, mutate=None, mid=None, name=name, d=d, p=p, reads=reads):
            prefix, stem = f"base.{name}.conv_block2", f"{name}->conv_block2"
            h1, h2 = shifts(stem + "->beta1"), shifts(stem + "->beta2")
            rows = T if d == 5 else None
            assert mid is None or "x" in reads
            pre = []
            with _plain_f32(dtype):
                if p["form"] == "dec6u":
                    y, S, _ = _dec6u_block(sd, reads["low"], reads["act"], reads["raw"], h1, h2, dtype, mutate, rows)
                elif p["cat_in"]:
                    y, S, _ = _block(sd, prefix, None, h1, h2, 1, dtype, act_copy=reads["act"], raw_copy=reads["raw"], mutate=mutate,
                                     rows=rows)
                else:
                    y, S, m = _block(sd, prefix, reads["x"], h1, h2, 1, dtype, mutate=mutate, rows=rows, mid_copy=mid)
                    pre = [] if mid is None else [Out("mid", 0, m[0], m[1], True)]
                if d == 5:
                    return pre + _head_outs(sd, y, S, reads["mag"], reads["cos"], reads["sin"], T, dtype)
            if not p["act_out"]:
                return pre + [Out(name, 0, y, S, False)]
            nn_ = _DEC[d + 1][0]
            return pre + [_act_out(f"decout{d}.act", 0, y, S, bn_scale(sd, f"base.{nn_}.bn1"), shifts(f"{nn_}->beta1"), dtype, mutate)]

        yield Launch(f"{name} ({p['form']})", reads, bmodel, repr(sorted(p.items())),
                     ("dec", name, cout, (1, 1)) if "x" in reads and p["form"] == "two" else None)


def bf16_key(t: torch.Tensor) -> torch.Tensor:
    """bf16-exact values as integers in which neighbouring bf16 values differ by one (sign-magnitude -> ordered)."""
    b = t.float().contiguous().view(torch.int32) >> 16
    return torch.where(b < 0, -(b & 0x7FFF), b)


def distinct(value: torch.Tensor):
    """(group index per element, number of groups): elements of one tensor with the SAME float64 model value are one computed
    value, counted once.  The zero-padded frames of a short clip make whole planes of a hand-over tensor one repeated value; a
    single rounding that falls the other way there would otherwise count thousands of times."""
    _, inv = torch.unique(value.double().flatten(), return_inverse=True)
    return inv, int(inv.max()) + 1


def share_differing(a_key: torch.Tensor, b_key: torch.Tensor, groups) -> float:
    """share of the distinct computed values (`distinct`) at which two bf16 tensors (as `bf16_key`) differ anywhere"""
    inv, n = groups
    hit = torch.zeros(n, dtype=torch.int32).index_reduce_(0, inv, (a_key != b_key).flatten().to(torch.int32), "amax", include_self=True)
    return float(hit.sum()) / n
