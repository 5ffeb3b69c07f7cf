"""The chunk loop of pw_gemm_split_body.h - fragment reads in the order the products take them, the staging of the other LDS buffer
between the MFMAs - in all four kernels it is included in, at the smallest shapes the routes admit where a schedule error (a
fragment taken before it landed, a stage register reloaded before it was written to LDS, a buffer written while it is read)
would show: the shortest loop any route runs (K = 128, 8 chunks), a partial and clamped last column tile, a 128-column tile that
spans clips, and the second accumulator set of the 32 x 16 level.

  pw_gemm_split_kernel<true>    decoder_block5's transposed conv (128 -> 64, stride (2, 2)) at 5 x 36: P = 180, one full 128-pixel
                                tile and a partial one; every staged element negative, so the prologue takes its 0.01 v branch
  pw_gemm_split_kernel<false>   decoder_block4's 1x1 shortcut (256 -> 128) at 8 x 64, the smallest image whose shortcut is a
                                pw_gemm.hip launch (test_gpu_pw_gemm_split.py), B = 2
  wino4_gemm_kernel<false>      encoder_block5 (256 -> 384) at 16 x 64 and 32 x 32, B = 3: P = 192 columns
  wino4_gemm_kernel<true>       encoder_block6 (384 -> 384) at 32 x 16, B = 1 and B = 2: P = 32, 64 columns

The bars are those of test_gpu_pw_gemm_split.py and test_gpu_wino4_gemm.py, with no new tolerance: against a float64 reference of the
same f32 inputs the route's relative RMS error and its largest deviation are at most twice those of the f32 kernels behind the
route's switch, and both routes stay under 2e-5 relative RMS; the switched-off route differs (the kernel really ran); the same
call twice is bit-equal; a clip alone is bit-equal to the same clip inside a batch (the middle one of B = 3).  Every case prints
its figures.  `stage_outputs` is what a comparison of two builds dumps: the route's outputs of every case here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lass_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 2.0
BAR = 2e-5  # relative RMS of either route against float64 (the F(4x4,3x3) block bar)

TCONV = ("decoder_block5", 128, 64, (2, 2), 5, 36, 3)          # name, cin, cout, stride, h, w, B
SHORTCUT = ("base.decoder_block4.conv_block2", 256, 128, 8, 64, 2)   # prefix, cin, cout, H, W, B
WINO = {  # name -> (block number, cin, H, W, pool, largest B)
    "enc5_16x64": (5, 256, 16, 64, (2, 2), 3),
    "enc5_32x32": (5, 256, 32, 32, (2, 2), 3),
    "enc6_32x16": (6, 384, 32, 16, (1, 2), 2),
}
WINO_RUNS = [("enc5_16x64", 3), ("enc5_32x32", 3), ("enc6_32x16", 1), ("enc6_32x16", 2)]


def _switch(e, which, on):
    fn = e.lib.lass_set_pw_split if which == "pw" else e.lib.lass_set_wino4_gemm
    _lib.check(e.ctx, fn(e.ctx, 1 if on else 0), "lass_set_" + which)


def _errs(got, ref):
    d = got.double() - ref
    return float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max())


def _hold(what, on, off, ref):
    (r_on, m_on), (r_off, m_off) = _errs(on, ref), _errs(off, ref)
    print(f"{what}: relative RMS error route {r_on:.3e} / f32 {r_off:.3e} (ratio {r_on / r_off:.3f}); "
          f"max |deviation| route {m_on:.3e} / f32 {m_off:.3e} (ratio {m_on / m_off:.3f})")
    assert on.shape == ref.shape and bool(torch.isfinite(on).all())
    assert not torch.equal(on, off), "the switch changed nothing: the kernel did not run"
    assert 0 < r_off < BAR and r_on < BAR, (r_on, r_off)
    assert r_on <= MARGIN * r_off, (r_on, r_off)
    assert m_on <= MARGIN * m_off, (m_on, m_off)


@pytest.fixture(scope="module")
def engine(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    return e


def zeroed_conv2(sd):
    """the state dict of test_gpu_pw_gemm_split.py's second engine: decoder_block4's conv2 weights are zero, the Winograd conv of
    zero weights is exactly 0, so the block's output is bias + Wsc x as pw_gemm.hip wrote it"""
    k = SHORTCUT[0] + ".conv2.weight"
    return {**sd, k: np.zeros_like(np.asarray(sd[k]))}


@pytest.fixture(scope="module")
def engine2(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(zeroed_conv2(synthetic_sd))
    return e


# ---- the inputs of every case, the same whoever asks ------------------------------------------------------------------------------
def tconv_inputs(e, sd):
    """-> (x, cond, act): x is chosen so that every staged element leaky(fma(x, scale, shift)) is negative; act is that element as
    the kernel forms it in f32"""
    name, cin, _cout, _up, h, w, B = TCONV
    cond = torch.from_numpy(synthetic.make_condition(B))
    bn = f"base.{name}.bn1."
    g, var = (torch.from_numpy(np.asarray(sd[bn + k])) for k in ("weight", "running_var"))
    scale = g * (1.0 / torch.sqrt(var + torch.tensor(1e-5)))                     # misc.hip: bnfold_kernel, in f32
    off = e.film_offset(f"{name}->beta1")
    shift = e.film(cond.to(DEV)).cpu()[:, off:off + cin]                          # FiLM beta + the folded BN shift, the kernel's bits
    assert float(scale.abs().min()) > 1e-3
    r = torch.randn(B, cin, h, w, generator=torch.Generator().manual_seed(2100 + h * w))
    target = -(shift.abs()[:, :, None, None] + 1.0 + r.abs())                      # x scale + shift, wanted
    x = ((target - shift[:, :, None, None]) / scale[None, :, None, None]).float()
    v = (x.double() * scale.double()[None, :, None, None] + shift.double()[:, :, None, None]).float()   # one rounding: an fma
    act = torch.maximum(v, (v.double() * float(np.float32(0.01))).float())
    assert bool((act < 0).all())
    return x, cond, act


def run_tconv(e, x, cond):
    name, _cin, cout, up, _h, _w, _B = TCONV
    return e.upconv("base." + name, x.to(DEV), e.film(cond.to(DEV)), cout, up).cpu()


def shortcut_inputs():
    _prefix, cin, _cout, H, W, B = SHORTCUT
    return torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(2100 + cin)), torch.from_numpy(synthetic.make_condition(B))


def run_shortcut(e2, x, cond):
    return e2.convblock(SHORTCUT[0], x.to(DEV), e2.film(cond.to(DEV)), SHORTCUT[2]).cpu()


def wino_inputs(name):
    _n, cin, H, W, _pool, B = WINO[name]
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(2100 + sum(map(ord, name))))
    return x, torch.from_numpy(synthetic.make_condition(B))


def run_wino(e, name, x, cond):
    """-> (y, pool) on the CPU"""
    n, _cin, _H, _W, pool, _B = WINO[name]
    y, p = e.encoder_block(f"base.encoder_block{n}", x.to(DEV), e.film(cond.to(DEV)), 384, pool)
    return y.cpu(), p.cpu()


def stage_outputs(e, e2, sd):
    """name -> array: the routes' outputs of every case of this file (both switches at their default, on)"""
    out = {}
    x, cond, _ = tconv_inputs(e, sd)
    out["tconv_dec5_5x36_B3"] = run_tconv(e, x, cond).numpy()
    x, cond = shortcut_inputs()
    out["shortcut_dec4_8x64_B2"] = run_shortcut(e2, x, cond).numpy()
    for name, B in WINO_RUNS:
        x, cond = wino_inputs(name)
        y, p = run_wino(e, name, x[:B].contiguous(), cond[:B].contiguous())
        out[f"{name}_B{B}_y"], out[f"{name}_B{B}_pool"] = y.numpy(), p.numpy()
    return out


# ---- pw_gemm_split_kernel<true>: K = 128, a partial tile, the leaky branch ----------------------------------------------------------
def test_transposed_conv_k128_partial_tile_leaky_branch(engine, synthetic_sd):
    name, cin, cout, up, h, w, B = TCONV
    x, cond, act = tconv_inputs(engine, synthetic_sd)
    wt = torch.from_numpy(np.asarray(synthetic_sd[f"base.{name}.conv1.weight"])).double()
    ref = F.conv_transpose2d(act.double(), wt, stride=up)
    try:
        _switch(engine, "pw", True)
        on = run_tconv(engine, x, cond)
        again = run_tconv(engine, x, cond)
        mid = run_tconv(engine, x[1:2].contiguous(), cond[1:2].contiguous())
        _switch(engine, "pw", False)
        off = run_tconv(engine, x, cond)
    finally:
        _switch(engine, "pw", True)
    _hold(f"{name} {cin}->{cout} {up} at {h}x{w}, B={B}, all staged elements negative", on, off, ref)
    assert torch.equal(on, again)
    assert torch.equal(on[1:2], mid)   # the middle clip of B = 3


# ---- pw_gemm_split_kernel<false>: K = 256 ---------------------------------------------------------------------------------------------
def test_shortcut_k256(engine2, synthetic_sd):
    prefix, cin, cout, H, W, B = SHORTCUT
    x, cond = shortcut_inputs()
    wsc = torch.from_numpy(np.asarray(synthetic_sd[prefix + ".shortcut.weight"])).double().reshape(cout, cin)
    bias = torch.from_numpy(np.asarray(synthetic_sd[prefix + ".shortcut.bias"])).double()
    ref = torch.einsum("nk,bkhw->bnhw", wsc, x.double()) + bias[None, :, None, None]
    try:
        _switch(engine2, "pw", True)
        on = run_shortcut(engine2, x, cond)
        again = run_shortcut(engine2, x, cond)
        last = run_shortcut(engine2, x[1:2].contiguous(), cond[1:2].contiguous())
        _switch(engine2, "pw", False)
        off = run_shortcut(engine2, x, cond)
    finally:
        _switch(engine2, "pw", True)
    _hold(f"{prefix} shortcut K={cin} at {H}x{W}, B={B}", on, off, ref)
    assert torch.equal(on, again)
    assert torch.equal(on[1:2], last)


# ---- wino4_gemm_kernel<false / true> --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wino_refs(synthetic_sd):
    """name -> (x, cond, ref, ref_pool) at the case's largest B, computed once: a clip's reference does not depend on its batch"""
    from oracle import resunet as orr
    sd64 = orr.to_torch(synthetic_sd, torch.float64)
    cache = {}

    def get(name):
        if name not in cache:
            n, _cin, _H, _W, pool, _B = WINO[name]
            x, cond = wino_inputs(name)
            block, prefix = f"encoder_block{n}->conv_block1", f"base.encoder_block{n}.conv_block1"
            c64 = cond.double()
            ref = orr.conv_block_res(sd64, prefix, x.double(), orr.film(sd64, c64, block + "->beta1"), orr.film(sd64, c64, block + "->beta2"))
            cache[name] = (x, cond, ref, F.avg_pool2d(ref, pool))
        return cache[name]

    return get


@pytest.mark.parametrize("name,B", WINO_RUNS)
def test_wino4_gemm_contractions(engine, wino_refs, name, B):
    x, cond, ref, rpool = wino_refs(name)
    full = x.shape[0]
    xb, cb = x[:B].contiguous(), cond[:B].contiguous()
    m = 1 if B == 3 else B - 1   # the middle clip of B = 3; the last of B = 2; B = 1: the clip against itself inside the largest batch
    try:
        _switch(engine, "wino4_gemm", True)
        on = run_wino(engine, name, xb, cb)
        again = run_wino(engine, name, xb, cb)
        one = run_wino(engine, name, x[m:m + 1].contiguous(), cond[m:m + 1].contiguous())
        inside = run_wino(engine, name, x, cond) if B == 1 else on
        _switch(engine, "wino4_gemm", False)
        off = run_wino(engine, name, xb, cb)
    finally:
        _switch(engine, "wino4_gemm", True)
    for what, a, b, r in (("y", on[0], off[0], ref[:B]), ("pool", on[1], off[1], rpool[:B])):
        _hold(f"{name} B={B} {what}", a, b, r)
    assert torch.equal(on[0], again[0]) and torch.equal(on[1], again[1])
    assert B == 1 or B == full
    assert torch.equal(inside[0][m:m + 1], one[0]) and torch.equal(inside[1][m:m + 1], one[1])
