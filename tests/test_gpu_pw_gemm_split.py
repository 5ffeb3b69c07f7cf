"""pw_gemm.hip's split-bf16 kernel (three exact bf16 pieces per f32 operand, six v_mfma_f32_32x32x16_bf16 products summed in f32)
against its f32-MFMA kernel, both from one engine through lass_set_pw_split, both measured against a float64 product of the
same f32 inputs on the CPU.  The bar of every accuracy case is err_split <= 2 err_f32 (relative RMS, and max |deviation|): the
two kernels are limited by the same f32 accumulation (a CPU emulation of the split gives 0.73-0.74 of a plain f32 GEMM's error),
and err_f32 comes from the kernel that is NOT under test.  Every case prints both values.

The transposed convs are called alone (engine.upconv); their float64 reference starts from the activated input as the kernels
stage it (f32 BN scale, f32 fma with the FiLM shift the engine returns, f32 leaky).  The 1x1 shortcuts are reached through
engine.convblock on a second engine whose conv2 weights of the tested blocks are zero: the Winograd conv of zero weights is
exactly 0, so the block's output is bias + Wsc x as pw_gemm.hip wrote it.  A block's shortcut runs in pw_gemm.hip only where its
conv2 tiles into F(4x4,3x3) blocks (conv_route.h: plan_block), i.e. on images of a multiple of 512 pixels - a shortcut launch has
no partial pixel tile, the transposed convs hold the tail.  So decoder_block4 and decoder_block2 are held at 8 x 64 and 16 x 32,
the smallest images that reach the kernel; at 4 x 8 decoder_block2's shortcut runs fused in wino.hip, which the switch must
leave alone bit for bit (and 4 x 36 is an image no conv kernel of the library takes: lass_convblock refuses it).  Non-finite
inputs are outside the split's contract and are not tested."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lass_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 2.0

DEC = {  # decoder: (cin, cout, (uh, uw)) of its transposed conv
    "decoder_block1": (384, 384, (1, 2)), "decoder_block3": (384, 256, (2, 2)), "decoder_block5": (128, 64, (2, 2)),
}
ZEROED = ["base.decoder_block4.conv_block2", "base.decoder_block2.conv_block2", "base.decoder_block3.conv_block2",
          "base.encoder_block5.conv_block1"]
NO_BIAS = "base.decoder_block3.conv_block2"      # ... and no shortcut bias: the exponent-range case scales X alone
BF16_W = "base.encoder_block5.conv_block1"       # ... and a shortcut matrix that is exact in bf16


def _split(e, on):
    _lib.check(e.ctx, e.lib.lass_set_pw_split(e.ctx, 1 if on else 0), "lass_set_pw_split")


def _both(e, fn):
    """(split route, f32 route) of one call, on the CPU; the default (on) is restored"""
    try:
        _split(e, 1)
        on = fn().cpu().clone()
        _split(e, 0)
        off = fn().cpu().clone()
    finally:
        _split(e, 1)
    return on, off


def _errs(got, ref):
    d = got.double() - ref
    return float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max())


def _hold(what, on, off, ref):
    (r_on, m_on), (r_off, m_off) = _errs(on, ref), _errs(off, ref)
    print(f"{what}: relative RMS error split {r_on:.3e} / f32 {r_off:.3e} (ratio {r_on / r_off:.3f}); "
          f"max |deviation| split {m_on:.3e} / f32 {m_off:.3e} (ratio {m_on / m_off:.3f}); max |ref| {float(ref.abs().max()):.3e}")
    assert bool(torch.isfinite(on).all()) and on.shape == ref.shape
    assert 0 < r_off < 1e-6, r_off   # the yardstick itself is an f32 GEMM of K <= 768
    assert r_on <= MARGIN * r_off, (r_on, r_off)
    assert m_on <= MARGIN * m_off, (m_on, m_off)
    return r_on, r_off


@pytest.fixture(scope="module")
def engine(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    return e


@pytest.fixture(scope="module")
def sd2(synthetic_sd):
    sd = {k: np.array(v, copy=True) for k, v in synthetic_sd.items() if any(k.startswith(p) for p in ZEROED)}
    for p in ZEROED:
        sd[p + ".conv2.weight"][...] = 0
    sd[NO_BIAS + ".shortcut.bias"][...] = 0
    w = torch.from_numpy(sd[BF16_W + ".shortcut.weight"])
    sd[BF16_W + ".shortcut.weight"] = w.bfloat16().float().numpy()
    return {**synthetic_sd, **sd}


@pytest.fixture(scope="module")
def engine2(sd2):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(sd2)
    return e


# ---- the transposed convs ----------------------------------------------------------------------------------------------------------
def _act(sd, e, name, x, cond):
    """the staged input of the transposed conv, as pw_gemm.hip forms it in f32: leaky(fma(x, scale, shift))"""
    cin = x.shape[1]
    bn = f"base.{name}.bn1."
    g, var = (torch.from_numpy(np.asarray(sd[bn + k])) for k in ("weight", "running_var"))
    scale = g * (1.0 / torch.sqrt(var + torch.tensor(1e-5)))                     # misc.hip: bnfold_kernel, in f32
    off = e.film_offset(f"{name}->beta1")
    shift = e.film(cond.to(DEV)).cpu()[:, off:off + cin]                          # FiLM beta + the folded BN shift, the kernel's bits
    v = (x.double() * scale.double()[None, :, None, None] + shift.double()[:, :, None, None]).float()   # one rounding: an fma
    small = (v.double() * float(np.float32(0.01))).float()
    return torch.maximum(v, small), scale, shift


def _tconv_ref(sd, name, act):
    w = torch.from_numpy(np.asarray(sd[f"base.{name}.conv1.weight"])).double()
    return F.conv_transpose2d(act.double(), w, stride=DEC[name][2])


@pytest.mark.parametrize("name,h,w", [
    ("decoder_block5", 3, 12),    # P = 36: less than one 128-pixel tile
    ("decoder_block1", 4, 8),     # P = 32, the (1, 2) stride
    ("decoder_block3", 5, 36),    # P = 180: one full tile and a partial one
])
def test_transposed_conv_split_against_f32_and_float64(engine, synthetic_sd, name, h, w):
    cin, cout, up = DEC[name]
    B = 2
    x = torch.randn(B, cin, h, w, generator=torch.Generator().manual_seed(h * 100 + w + 15))
    cond = torch.from_numpy(synthetic.make_condition(B))
    shift = engine.film(cond.to(DEV))
    xd = x.to(DEV)
    on, off = _both(engine, lambda: engine.upconv("base." + name, xd, shift, cout, up))
    act, _, _ = _act(synthetic_sd, engine, name, x, cond)
    _hold(f"{name} {cin}->{cout} {up} at {h}x{w}", on, off, _tconv_ref(synthetic_sd, name, act))
    assert not torch.equal(on, off)   # the switch changed the launch: the split kernel really ran


def test_transposed_conv_leaky_branch(engine, synthetic_sd):
    """every staged element is negative: the prologue's 0.01 v branch in front of the split"""
    name, h, w = "decoder_block5", 3, 12
    cin, cout, up = DEC[name]
    B = 2
    cond = torch.from_numpy(synthetic.make_condition(B))
    r = torch.randn(B, cin, h, w, generator=torch.Generator().manual_seed(77))
    _, scale, shift = _act(synthetic_sd, engine, name, r, cond)
    assert float(scale.abs().min()) > 1e-3
    target = -(shift.abs()[:, :, None, None] + 1.0 + r.abs())                      # x scale + shift, wanted
    x = ((target - shift[:, :, None, None]) / scale[None, :, None, None]).float()
    act, _, _ = _act(synthetic_sd, engine, name, x, cond)
    assert bool((act < 0).all())
    dshift = engine.film(cond.to(DEV))
    xd = x.to(DEV)
    on, off = _both(engine, lambda: engine.upconv("base." + name, xd, dshift, cout, up))
    _hold(f"{name} leaky branch", on, off, _tconv_ref(synthetic_sd, name, act))


# ---- the 1x1 shortcuts -------------------------------------------------------------------------------------------------------------
def _shortcut(e, sd, prefix, x):
    cout = sd[prefix + ".shortcut.weight"].shape[0]
    cond = torch.from_numpy(synthetic.make_condition(x.shape[0]))
    shift = e.film(cond.to(DEV))
    xd = x.to(DEV)
    return _both(e, lambda: e.convblock(prefix, xd, shift, cout))


def _shortcut_ref(sd, prefix, x):
    w = torch.from_numpy(np.asarray(sd[prefix + ".shortcut.weight"])).double()
    b = torch.from_numpy(np.asarray(sd[prefix + ".shortcut.bias"])).double()
    return torch.einsum("nk,bkhw->bnhw", w.reshape(w.shape[0], w.shape[1]), x.double()) + b[None, :, None, None]


@pytest.mark.parametrize("prefix,cin,H,W", [
    ("base.decoder_block4.conv_block2", 256, 8, 64),    # the smallest images whose shortcut is a pw_gemm.hip launch:
    ("base.decoder_block2.conv_block2", 768, 16, 32),   # 8 x 64 and 16 x 32 Winograd blocks, P = 512 (four pixel tiles)
])
def test_shortcut_split_against_f32_and_float64(engine2, sd2, prefix, cin, H, W):
    B = 2
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(H * 1000 + W + cin))
    on, off = _shortcut(engine2, sd2, prefix, x)
    _hold(f"{prefix} shortcut K={cin} at {H}x{W}", on, off, _shortcut_ref(sd2, prefix, x))
    assert not torch.equal(on, off)   # the switch changed the launch: the split kernel really ran


def test_shortcut_off_the_route_is_left_alone(engine2, sd2):
    """decoder_block2 at 4 x 8: no F(4x4,3x3) block fits, the shortcut stays fused in wino.hip - the switch changes no bit"""
    prefix = "base.decoder_block2.conv_block2"
    x = torch.randn(2, 768, 4, 8, generator=torch.Generator().manual_seed(4 * 1000 + 8 + 768))
    on, off = _shortcut(engine2, sd2, prefix, x)
    ref = _shortcut_ref(sd2, prefix, x)
    print(f"{prefix} shortcut at 4x8 (wino.hip): relative RMS error {_errs(on, ref)[0]:.3e}")
    assert bool(torch.isfinite(on).all()) and torch.equal(on, off)
    assert _errs(on, ref)[0] < 2e-5   # the block bar of test_gpu_pw_gemm.py: it is bias + Wsc x, from another kernel


def test_bf16_exact_operands_agree(engine2, sd2):
    """X and W exact in bf16: the m and l pieces are zero and the split is the hh product alone, every product exact in f32"""
    prefix = BF16_W
    x = torch.randn(1, 256, 8, 64, generator=torch.Generator().manual_seed(5)).bfloat16().float()
    on, off = _shortcut(engine2, sd2, prefix, x)
    ref = _shortcut_ref(sd2, prefix, x)
    d = float((on.double() - off.double()).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"bf16-exact operands: split vs f32 relative RMS difference {d:.3e}; vs float64: split {_errs(on, ref)[0]:.3e}, f32 {_errs(off, ref)[0]:.3e}")
    assert d < 1e-6, d
    assert _errs(on, ref)[0] < 1e-6


def test_exponent_range_is_f32s(engine2, sd2):
    """X scaled by 2^60 and by 2^-60 (no bias in this block): the split's relative error does not move - the pieces carry f32's
    exponent, not a narrower one"""
    prefix = NO_BIAS
    x = torch.randn(1, 512, 8, 64, generator=torch.Generator().manual_seed(6))
    base = None
    for e2 in (0, 60, -60):
        xs = x * float(2.0 ** e2)
        on, off = _shortcut(engine2, sd2, prefix, xs)
        r_on, r_off = _hold(f"X * 2^{e2}", on, off, _shortcut_ref(sd2, prefix, xs))
        base = r_on if base is None else base
        assert abs(r_on - base) <= 0.1 * base, (e2, r_on, base)


# ---- determinism -------------------------------------------------------------------------------------------------------------------
def test_same_call_twice_and_a_clip_alone_are_bit_equal(engine, engine2, sd2):
    _split(engine, 1)
    _split(engine2, 1)
    name, h, w = "decoder_block3", 5, 36
    cin, cout, up = DEC[name]
    B = 3
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    shift = engine.film(cond)
    x = torch.randn(B, cin, h, w, generator=torch.Generator().manual_seed(8)).to(DEV)
    a = engine.upconv("base." + name, x, shift, cout, up).cpu().clone()
    b = engine.upconv("base." + name, x, shift, cout, up).cpu().clone()
    one = engine.upconv("base." + name, x[:1].contiguous(), shift[:1].contiguous(), cout, up).cpu()
    assert torch.equal(a, b) and torch.equal(a[:1], one)
    prefix = "base.decoder_block4.conv_block2"
    shift2 = engine2.film(cond)
    x = torch.randn(B, 256, 8, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    a = engine2.convblock(prefix, x, shift2, 128).cpu().clone()
    b = engine2.convblock(prefix, x, shift2, 128).cpu().clone()
    one = engine2.convblock(prefix, x[:1].contiguous(), shift2[:1].contiguous(), 128).cpu()
    assert torch.equal(a, b) and torch.equal(a[:1], one)
