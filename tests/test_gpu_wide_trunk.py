"""The deep trunk on a 1024-bin context (ResUNet30 at the 32 kHz geometry, n_fft 2048 / hop 320, and the multi-STFT model) at the
frame counts its 5 s and 10 s clips run at - the routes that tests/test_wide_trunk_routing_cpu.py pins and that no 16 kHz shape
reaches: conv_block7a on the narrow 32 x 16 F(4x4,3x3) blocks (gemm route, split-K with its combine launch, an identity conv2 with
no pool), encoder_block6 as a mixed block (a gemm-route conv1 in front of an F(2x2,3x3) conv2 with the fused 1 x 2 pool at 32 bins),
decoder_block1 with its 1 x 2 transposed conv on 16 x 32 blocks, and a narrow level with two stacked blocks per plane (64 x 16).

1. Stage calls, each switch position against a torch-CPU float64 ConvBlockRes of the same f32 inputs and weights.
2. The same launches inside lass_separate, teacher-forced: every trunk block's float64 model is fed the tensors the kernels read
   (workspace taps) and compared with the tap they wrote; then the whole model against the oracle, batch invariance and the switch.

Every bar is one the suite already holds these kinds of block to (named where it is defined below).  What is new is where they are
applied: not only over a tensor but band by band - one clip x one cout tile x one F(4x4,3x3) block of the image's geometry - each
band against its own reference RMS, so that an error confined to one block, one seam or one cout tile does not dilute in the mean.

Out of scope here: the bf16 modes (their routes depend on the width alone; tests/test_gpu_bf16_exact.py holds them), the half-batch
split and graph replay at these shapes (covered at other shapes), and anything that reads kernel assembly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lass_amd import arch, synthetic
from test_gpu_geometry import oracle_at_geometry

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_FFT, HOP = 2048, 320
W4_BAR = 2e-5      # relative RMS of a block with an F(4x4,3x3) conv against the oracle (test_gpu_wino4_splitk.py)
W2_BAR = 5e-6      # ... of a pure F(2x2,3x3) block (test_gpu_wino4_splitk.py, test_gpu_stages.py)
SPLIT_BAR = 1e-5   # S = 2, 4 against S = 1: two draws of the route's rounding through two convs (test_gpu_wino4_splitk.py)
WAVE_BAR = 3e-6    # RMS of the f32 10 s waveform between the gemm and the f32 route (test_gpu_wino4_gemm.py)
MODEL_BAR = 1e-5   # RMS error of the whole model against the oracle (test_gpu_geometry.py)


# ---- measuring -----------------------------------------------------------------------------------------------------------------
def _errs(got, ref):
    d = got.double() - ref
    return float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max())


def _geom(H, W):
    """the F(4x4,3x3) block of an H x W image (conv_route.h: lass_wino4_block_tc); an image that tiles into none is one band"""
    if W % 64 == 0 and H % 8 == 0:
        return 8, 64
    if W % 32 == 0 and H % 16 == 0:
        return 16, 32
    if W % 32 == 16 and H % 32 == 0:
        return 32, 16
    return H, W


def _worst_band(got, ref, bh, bw, cg):
    """relative RMS error of every (clip, cg-channel group, bh x bw block) band against that band's reference RMS -> (worst, index)"""
    B, C, H, W = ref.shape
    assert C % cg == 0 and H % bh == 0 and W % bw == 0, (ref.shape, bh, bw, cg)
    cut = (B, C // cg, cg, H // bh, bh, W // bw, bw)
    d2 = (got.double() - ref).pow(2).reshape(cut).mean(dim=(2, 4, 6))
    r2 = ref.pow(2).reshape(cut).mean(dim=(2, 4, 6))
    rel = (d2 / r2).sqrt()
    i = int(rel.argmax())
    return float(rel.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(rel.shape)))


class Figures:
    """prints every figure as it is measured and collects the bars it misses, so that one run shows them all"""

    def __init__(self):
        self.missed = []

    def hold(self, ok, what):
        if not ok:
            print("   MISSED:", what)
            self.missed.append(what)

    def block(self, what, got, ref, bar, cg, pool=(1, 1)):
        """tensor and band bars of one output.  pool: the avg-pool between the conv's image and this tensor (its bands are the
        pooled blocks).  A 64 x 16 image additionally has rows 30-33, the seam between its two stacked blocks, as a band."""
        rel, dev = _errs(got, ref)
        H, W = ref.shape[2] * pool[0], ref.shape[3] * pool[1]
        bh, bw = _geom(H, W)
        worst, at = _worst_band(got, ref, bh // pool[0], bw // pool[1], cg)
        line = f"{what}: rel RMS {rel:.3e} max dev {dev:.3e} (|ref| max {float(ref.abs().max()):.2f}) | worst band {worst:.3e} at (clip, group, by, bx) {at}"
        seam = None
        if (H, W) == (64, 16):
            lo, hi = 30 // pool[0], 34 // pool[0]
            seam, sat = _worst_band(got[:, :, lo:hi], ref[:, :, lo:hi], hi - lo, W // pool[1], cg)
            line += f" | seam rows {seam:.3e} at {sat[:2]}"
        print(line)
        self.hold(got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: shape / finite")
        self.hold(rel < bar, f"{what}: rel RMS {rel:.3e} >= {bar}")
        self.hold(dev < 3e-4 * max(1.0, float(ref.abs().max())), f"{what}: max dev {dev:.3e}")
        self.hold(worst < bar, f"{what}: band {at} rel RMS {worst:.3e} >= {bar}")
        if seam is not None:
            self.hold(seam < bar, f"{what}: seam rows rel RMS {seam:.3e} >= {bar}")
        return rel, dev

    def done(self):
        assert not self.missed, self.missed


# ---- engines and weights -------------------------------------------------------------------------------------------------------
def _make_engine(sd, stft, wino4=None):
    from lass_amd.engine import Engine
    with pytest.MonkeyPatch.context() as mp:
        if wino4 is not None:
            mp.setenv("LASS_WINO4", wino4)
        e = Engine(DEV, stft=stft)
    e.load_state_dict(sd)
    return e


@pytest.fixture(scope="module")
def wide_sd():
    return synthetic.make_state_dict(n_fft=N_FFT)


@pytest.fixture(scope="module")
def engines(wide_sd, synthetic_sd):
    """ctx -> (engine, the same weights with LASS_WINO4=0: F(2x2,3x3) everywhere); "wide": 1024 bins, "base": the 16 kHz context"""
    return {"wide": (_make_engine(wide_sd, (N_FFT, HOP)), _make_engine(wide_sd, (N_FFT, HOP), "0")),
            "base": (_make_engine(synthetic_sd, None), _make_engine(synthetic_sd, None, "0"))}


@pytest.fixture(scope="module")
def sd64(wide_sd, synthetic_sd):
    from oracle import resunet as orr
    return {"wide": orr.to_torch(wide_sd, torch.float64), "base": orr.to_torch(synthetic_sd, torch.float64)}


def _set(e, fn, v):
    from lass_amd import _lib
    _lib.check(e.ctx, getattr(e.lib, fn)(e.ctx, v), fn)


# ---- float64 models --------------------------------------------------------------------------------------------------------------
def _enc_ref(sd, name, x, cond):
    from oracle import resunet as orr
    return orr.conv_block_res(sd, f"base.{name}.conv_block1", x, orr.film(sd, cond, f"{name}->conv_block1->beta1"),
                              orr.film(sd, cond, f"{name}->conv_block1->beta2"))


def _up_ref(sd, name, x, cond, up):
    from oracle import resunet as orr
    h = F.leaky_relu(orr._bn(sd, f"base.{name}.bn1", x) + orr.film(sd, cond, f"{name}->beta1"), 0.01)
    return F.conv_transpose2d(h, sd[f"base.{name}.conv1.weight"], stride=up)


def _dec_ref(sd, name, cat, cond):
    from oracle import resunet as orr
    return orr.conv_block_res(sd, f"base.{name}.conv_block2", cat, orr.film(sd, cond, f"{name}->conv_block2->beta1"),
                              orr.film(sd, cond, f"{name}->conv_block2->beta2"))


# ---- 1. stage calls --------------------------------------------------------------------------------------------------------------
# name -> (context, block, H, W, largest B, narrow (the blocks take a split factor), channel group of a band: the 128-cout tile of
# the F(4x4,3x3) routes, the 32-cout group of wino.hip where the block's conv2 is F(2x2,3x3))
CASES = {
    "c7a_32x16": ("wide", "conv_block7a", 32, 16, 3, True, 128),     # GEMM columns 32, 64, 96: a partial tile, a tile across clips
    "c7a_64x16": ("wide", "conv_block7a", 64, 16, 2, True, 128),     # two blocks per plane, 128 columns
    "enc6_32x32": ("wide", "encoder_block6", 32, 32, 3, False, 32),  # the mixed block
    "enc6_16x32": ("wide", "encoder_block6", 16, 32, 2, False, 32),  # ... at 512 padded frames
    "dec1_32x32": ("wide", "decoder_block1", 32, 32, 2, False, 128),
    "dec1_16x32": ("wide", "decoder_block1", 16, 32, 2, False, 128),
    "enc6_64x16": ("base", "encoder_block6", 64, 16, 2, True, 128),  # 16 kHz, a 20 s clip: the seam between two 32 x 16 blocks
    "dec1_64x16": ("base", "decoder_block1", 64, 16, 2, True, 128),
}
RUNS = [("c7a_32x16", 1), ("c7a_32x16", 2), ("c7a_32x16", 3), ("c7a_64x16", 2), ("enc6_32x32", 1), ("enc6_32x32", 2), ("enc6_32x32", 3),
        ("enc6_16x32", 2), ("dec1_32x32", 2), ("dec1_16x32", 2), ("enc6_64x16", 1), ("enc6_64x16", 2), ("dec1_64x16", 1), ("dec1_64x16", 2)]
POOL = {"conv_block7a": None, "encoder_block6": (1, 2), "decoder_block1": None}


@pytest.fixture(scope="module")
def case_data(sd64):
    """name -> (inputs, cond, ref, pooled ref or None) at the case's largest B, computed once and never modified: a clip's reference
    does not depend on its batch, so a smaller B takes the leading clips"""
    cache = {}

    def get(name):
        if name not in cache:
            ctx, block, H, W, B, _narrow, _cg = CASES[name]
            g = torch.Generator().manual_seed(2900 + sum(map(ord, name)))
            cond = torch.from_numpy(synthetic.make_condition(B))   # a different condition per clip
            sd, c64 = sd64[ctx], cond.double()
            if block == "decoder_block1":
                xlow, skip = torch.randn(B, 384, H, W // 2, generator=g), torch.randn(B, 384, H, W, generator=g)
                ref = _dec_ref(sd, block, torch.cat((_up_ref(sd, block, xlow.double(), c64, (1, 2)), skip.double()), 1), c64)
                cache[name] = ((xlow, skip), cond, ref, None)
            else:
                x = torch.randn(B, 384, H, W, generator=g)
                ref = _enc_ref(sd, block, x.double(), c64)
                cache[name] = ((x,), cond, ref, F.avg_pool2d(ref, POOL[block]) if POOL[block] else None)
        return cache[name]

    return get


def _run(e, block, xs, cond):
    """-> (y, pool or None) on the CPU.  conv_block7a goes through lass_encoder_block with pool == NULL; decoder_block1 as
    lass_separate runs it: the (1, 2) transposed conv, the concat with the skip, the ConvBlockRes 768 -> 384"""
    shift = e.film(cond.to(DEV))
    if block == "decoder_block1":
        up = e.upconv("base.decoder_block1", xs[0].to(DEV), shift, 384, (1, 2))
        cat = torch.cat((up, xs[1].to(DEV)), 1).contiguous()
        return e.convblock("base.decoder_block1.conv_block2", cat, shift, 384).cpu(), None
    y, p = e.encoder_block("base." + block, xs[0].to(DEV), shift, 384, POOL[block] or (1, 1))
    return y.cpu(), (p.cpu() if p is not None else None)


@pytest.mark.parametrize("name,B", RUNS)
def test_every_route_of_a_block_vs_float64(engines, case_data, name, B):
    ctx, block, H, W, _bmax, narrow, cg = CASES[name]
    e, e0 = engines[ctx]
    xs, cond, ref, rpool = case_data(name)
    xs, cond = tuple(x[:B].contiguous() for x in xs), cond[:B].contiguous()
    refs = [("y", ref[:B], (1, 1))] + ([("pool", rpool[:B], POOL[block])] if rpool is not None else [])
    got = {}
    try:
        got["gemm"] = _run(e, block, xs, cond)
        for s in ((1, 2, 4) if narrow else (4,)):
            _set(e, "lass_set_wino4_splits", s)
            got[f"S={s}"] = _run(e, block, xs, cond)
        _set(e, "lass_set_wino4_splits", 0)
        _set(e, "lass_set_wino4_gemm", 0)
        got["f32"] = _run(e, block, xs, cond)
        _set(e, "lass_set_wino4_gemm", 1)
        if block == "decoder_block1":
            _set(e, "lass_set_pw_split", 0)
            got["pw_split=0"] = _run(e, block, xs, cond)
    finally:
        _set(e, "lass_set_wino4_splits", 0)
        _set(e, "lass_set_wino4_gemm", 1)
        _set(e, "lass_set_pw_split", 1)
    got["f2x2"] = _run(e0, block, xs, cond)
    fig = Figures()
    for k, (what, r, pool) in enumerate(refs):
        err = {}
        for route, out in got.items():
            err[route] = fig.block(f"{name} B={B} {what} [{route}]", out[k], r, W2_BAR if route == "f2x2" else W4_BAR, cg, pool)
        (ra, ma), (rb, mb) = err["gemm"], err["f32"]
        print(f"{name} B={B} {what}: gemm / f32 route ratios: rel RMS {ra / rb:.3f}, max dev {ma / mb:.3f}")
        # the bar of test_gpu_wino4_gemm.py: the route may be at most twice as far from float64 as the f32 route on the same case
        fig.hold(ra <= 2 * rb, f"{what}: gemm route rel RMS {ra:.3e} > 2 x {rb:.3e}")
        fig.hold(ma <= 2 * mb, f"{what}: gemm route max dev {ma:.3e} > 2 x {mb:.3e}")
        # each route really ran
        fig.hold(not torch.equal(got["gemm"][k], got["f32"][k]), f"{what}: the gemm switch changed nothing")
        fig.hold(torch.equal(got["S=4"][k], got["f32"][k]), f"{what}: a forced split factor must keep the launches of the switch-off route")
        for route in ("gemm", "f32"):
            fig.hold(not torch.equal(got[route][k], got["f2x2"][k]), f"{what}: LASS_WINO4=0 gives the bits of {route}")
        if narrow:
            for s in (2, 4):
                d = _errs(got[f"S={s}"][k], got["S=1"][k].double())[0]
                print(f"{name} B={B} {what}: S={s} vs S=1 rel RMS {d:.3e}")
                fig.hold(d < SPLIT_BAR, f"{what}: S={s} vs S=1 {d:.3e}")
            fig.hold(not torch.equal(got["S=4"][k], got["S=1"][k]) and not torch.equal(got["S=2"][k], got["S=1"][k]),
                     f"{what}: the split factors gave the same bits")
        if block == "decoder_block1":
            fig.hold(not torch.equal(got["pw_split=0"][k], got["gemm"][k]), f"{what}: lass_set_pw_split changed nothing")
    fig.done()


@pytest.mark.parametrize("name", ["c7a_32x16", "c7a_64x16", "enc6_32x32", "enc6_16x32", "enc6_64x16"])
def test_a_clip_does_not_depend_on_its_batch(engines, case_data, name):
    ctx, block = CASES[name][:2]
    e = engines[ctx][0]
    xs, cond, _, _ = case_data(name)
    B = cond.shape[0]
    m = 1 if B == 3 else B - 1   # the middle clip of B = 3; the last of B = 2 (the second half of a GEMM tile that spans both clips)
    yb, pb = _run(e, block, xs, cond)
    y1, p1 = _run(e, block, tuple(x[m:m + 1].contiguous() for x in xs), cond[m:m + 1].contiguous())
    assert torch.equal(yb[m:m + 1], y1)
    assert pb is None or torch.equal(pb[m:m + 1], p1)


# ---- 2. the same launches inside lass_separate, teacher-forced -------------------------------------------------------------------
def _noise(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * 0.5


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def model(wide_sd):
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512, n_fft=N_FFT, hop=HOP)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in wide_sd.items()})
    return m.to(DEV).eval()


def _separate(m, mix, cond):
    return m({"mixture": mix.to(DEV), "condition": cond.to(DEV)})["waveform"].cpu()


# block -> (padded frames -> its route's bar, channel group of a band), as tests/test_wide_trunk_routing_cpu.py pins the routes: at 512
# padded frames conv_block7a (16 x 16) is a pure F(2x2,3x3) block; encoder_block6's conv2 is F(2x2,3x3) at either frame count
TRUNK_BARS = {"encoder_block5": ({512: W4_BAR, 1024: W4_BAR}, 128), "encoder_block6": ({512: W4_BAR, 1024: W4_BAR}, 32),
              "conv_block7a": ({512: W2_BAR, 1024: W4_BAR}, 128), "decoder_block1": ({512: W4_BAR, 1024: W4_BAR}, 128),
              "decoder_block2": ({512: W4_BAR, 1024: W4_BAR}, 128)}


def _teacher_forced(eng, sd, cond, B, L, t_pad, who):
    """every trunk block's float64 model on the tensors the kernels read, against the tensors they wrote"""
    names = ("encoder_block4.pool", "encoder_block5", "encoder_block5.pool", "encoder_block6", "encoder_block6.pool", "conv_block7a",
             "decoder_block1.up", "decoder_block1", "decoder_block2.up", "decoder_block2")
    tap = {n: eng.workspace_tensor(n, B, L).clone().cpu() for n in names}
    assert tap["conv_block7a"].shape == (B, 384, t_pad // 32, 16) and tap["encoder_block5"].shape == (B, 384, t_pad // 16, 64)
    c64 = cond.double()
    fig = Figures()
    x = tap["encoder_block4.pool"]
    for block, pool in (("encoder_block5", (2, 2)), ("encoder_block6", (1, 2)), ("conv_block7a", None)):
        bars, cg = TRUNK_BARS[block]
        if block == "conv_block7a" and t_pad == 512:
            cg = 32   # wino.hip's cout group
        ref = _enc_ref(sd, block, x.double(), c64)
        fig.block(f"{who} {block} {tuple(ref.shape[2:])}", tap[block], ref, bars[t_pad], cg)
        if pool:
            fig.block(f"{who} {block}.pool", tap[block + ".pool"], F.avg_pool2d(ref, pool), bars[t_pad], cg, pool)
            x = tap[block + ".pool"]
    x = tap["conv_block7a"]
    for block, up, skip in (("decoder_block1", (1, 2), "encoder_block6"), ("decoder_block2", (2, 2), "encoder_block5")):
        bars, cg = TRUNK_BARS[block]
        # a transposed conv with stride = kernel is a pointwise GEMM of K = 384 (pw_gemm.hip): held to the tighter of the block bars
        fig.block(f"{who} {block}.up", tap[block + ".up"], _up_ref(sd, block, x.double(), c64, up), W2_BAR, cg)
        ref = _dec_ref(sd, block, torch.cat((tap[block + ".up"], tap[skip]), 1).double(), c64)
        fig.block(f"{who} {block} {tuple(ref.shape[2:])}", tap[block], ref, bars[t_pad], cg)
        x = tap[block]
    fig.done()


@pytest.fixture(scope="module")
def clips():
    """L -> (mixture (2,1,L), condition (2,512))"""
    return {L: (_noise((2, 1, L), 700 + L), torch.from_numpy(synthetic.make_condition(2))) for L in (160000, 317440)}


@pytest.mark.parametrize("L,t_pad", [(160000, 512), (317440, 1024)])   # T = 501 and T = 993, the shortest clip of 1024 padded frames
def test_trunk_launches_of_a_separate_teacher_forced(model, sd64, clips, L, t_pad):
    assert arch.padded_frames(arch.frames_for(L, HOP)) == t_pad
    mix, cond = clips[L]
    out = _separate(model, mix[:1], cond[:1])   # eager and unsplit: fresh buffers, B = 1
    assert out.shape == (1, 1, L) and bool(torch.isfinite(out).all()) and _rms(out) > 1e-3
    _teacher_forced(model.engine, sd64["wide"], cond[:1], 1, L, t_pad, f"32 kHz L={L}")


@pytest.mark.parametrize("L", [160000, 317440])
def test_whole_model_vs_oracle_and_batch_invariance(model, wide_sd, clips, L):
    mix, cond = clips[L]
    with oracle_at_geometry() as orr:
        ref = orr.forward(orr.to_torch(wide_sd), {"mixture": mix[:1], "condition": cond[:1]})["waveform"]
    one = _separate(model, mix[:1], cond[:1])
    err = _rms(one - ref)
    print(f"32 kHz L={L} B=1: waveform RMS error vs oracle {err:.3e} (signal {_rms(ref):.3e})")
    assert _rms(ref) > 1e-3 and err <= MODEL_BAR, err
    if L == 160000:   # row 0 of a batch of two is the clip run alone, bit for bit
        both = _separate(model, mix, cond)
        assert torch.equal(both[0], one[0])


def test_the_gemm_switch_at_1024_frames(model, clips):
    L = 317440
    mix, cond = clips[L]
    eng = model.engine
    on = _separate(model, mix[:1], cond[:1])
    need_on = eng.workspace_bytes(1, L)
    try:
        _set(eng, "lass_set_wino4_gemm", 0)
        need_off = eng.workspace_bytes(1, L)   # (Engine.separate asks again on every call: the size follows the switch)
        off = _separate(model, mix[:1], cond[:1])
    finally:
        _set(eng, "lass_set_wino4_gemm", 1)
    assert eng.workspace_bytes(1, L) == need_on and need_off < need_on   # the product image is the route's alone
    err = _rms(on - off)
    rel = err / _rms(off)
    print(f"32 kHz L={L}: gemm route vs f32 route: waveform RMS difference {err:.3e}, relative {rel:.3e}")
    assert bool(torch.isfinite(on).all()) and _rms(off) > 1e-3
    assert not torch.equal(on, off)
    assert rel < WAVE_BAR and err < WAVE_BAR, (rel, err)


def test_multistft_trunk_launches_teacher_forced():
    """the multi-STFT context (windows 256 / 512 / 2048 at n_fft 2048, hop 160): 10 s at 16 kHz is 1024 padded frames"""
    from lass_amd.resunet_with_multistft import ResUNet30
    from oracle import resunet as orr
    L = 160000
    sd = synthetic.make_state_dict_ms()
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(DEV).eval()
    mix, cond = _noise((1, 1, L), 911), torch.from_numpy(synthetic.make_condition(1))
    out = _separate(m, mix, cond)
    assert out.shape == (1, 1, L) and bool(torch.isfinite(out).all()) and _rms(out) > 1e-3
    _teacher_forced(m.engine, orr.to_torch(sd, torch.float64), cond, 1, L, 1024, f"multi-STFT L={L}")
