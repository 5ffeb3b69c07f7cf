"""The folded head's shortcut logits formed where their inputs are produced (conv_route.h: head_sc_fold): encoder_block1.conv2's
epilogue writes Wsc'_skip x1, decoder_block6's transposed conv writes Wt' act(x11) from one more cout block, and the head
(wino4_headfold_planes_kernel) adds the two sets of planes instead of running a shortcut phase over the concat.  Held against the
route off (lass_set_head_sc_fold(ctx, 0): round 11's launches) and the oracle at the bars of test_gpu_head_fold.py; the route
re-associates the shortcut's sum, so on and off are not bitwise equal.

Every case but the last runs clips of L = 16 000: 101 frames padded to 128, at 512 bins - the last valid frame falls inside a 4-row
tile, whole 8-row blocks lie beyond mask_T, and the Nyquist column is written."""
import numpy as np
import pytest
import torch

from lass_amd import _lib, arch, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WAVE_BAR = 3e-6   # RMS of an f32 waveform, relative and absolute (test_gpu_head_fold.py)
SPEC_BAR = 3e-5   # max |deviation| of the separated spectrum / its largest magnitude
PLANE_BAR = 1e-5  # an f32 sum of 32 or 64 products against float64, of the planes' largest magnitude
L = 16000


def _sc(e, on):
    _lib.check(e.ctx, e.lib.lass_set_head_sc_fold(e.ctx, 1 if on else 0), "lass_set_head_sc_fold")


def _fold(e, on):
    _lib.check(e.ctx, e.lib.lass_set_head_fold(e.ctx, 1 if on else 0), "lass_set_head_fold")


def _relerr(got, ref):
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30))


@pytest.fixture(scope="module")
def engine(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    return e


def _run(e, mix, cond, B, length):
    """(waveform, out_real, out_imag) of one lass_separate, on the CPU"""
    T = arch.frames_for(length)
    wav = e.separate(mix, cond).cpu()
    torch.cuda.synchronize()
    re = e.workspace_tensor("out_real", B, length).clone().cpu()[:, :, :T]
    im = e.workspace_tensor("out_imag", B, length).clone().cpu()[:, :, :T]
    return wav, re, im


def _on_against_off(e, sd_torch, mix_np, cond_np, what):
    from oracle import resunet as orr
    B, length = mix_np.shape
    mix, cond = torch.from_numpy(mix_np).to(DEV), torch.from_numpy(cond_np).to(DEV)
    try:
        _sc(e, 1)
        on = _run(e, mix, cond, B, length)
        _sc(e, 0)
        off = _run(e, mix, cond, B, length)
    finally:
        _sc(e, 1)
    err, rel = float((on[0] - off[0]).pow(2).mean().sqrt()), _relerr(on[0], off[0])
    print(f"{what}: route on vs off, waveform RMS difference {err:.3e}, relative {rel:.3e}, bitwise equal {torch.equal(on[0], off[0])}")
    assert bool(torch.isfinite(on[0]).all()) and float(off[0].pow(2).mean().sqrt()) > 1e-3   # a real waveform to be relative to
    assert rel < WAVE_BAR, rel
    assert err < WAVE_BAR, err
    if sd_torch is None:
        return on, off
    for i, name in ((1, "out_real"), (2, "out_imag")):
        d = float((on[i] - off[i]).abs().max()) / float(off[i].abs().max())
        print(f"{what}: {name} route on vs off, max |difference| / max |value| {d:.3e}")
        assert d < SPEC_BAR, (name, d)
    assert bool((on[1][..., -1] == 0).all()) and bool((on[2][..., -1] == 0).all())   # the dropped Nyquist bin: an exact zero
    taps = {}
    orr.forward(sd_torch, {"mixture": torch.from_numpy(mix_np)[:, None, :], "condition": torch.from_numpy(cond_np)}, taps=taps)
    for i, name in ((1, "out_real"), (2, "out_imag")):
        ref = taps[name].reshape(on[i].shape)
        scale = float(ref.abs().max())
        d_on, d_off = float((on[i] - ref).abs().max()) / scale, float((off[i] - ref).abs().max()) / scale
        print(f"{what}: {name} max |dev| / max |ref| vs the oracle: route on {d_on:.3e}, route off {d_off:.3e}")
        assert d_on < SPEC_BAR, (name, "route on", d_on)
        assert d_off < SPEC_BAR, (name, "route off", d_off)
    return on, off


def test_route_on_against_route_off_and_the_oracle(engine, synthetic_sd):
    from oracle import resunet as orr
    B = 2
    _, mix = synthetic.make_mixtures(B, L)
    on, off = _on_against_off(engine, orr.to_torch(synthetic_sd), mix, synthetic.make_condition(B), "B=2 L=16000")
    # the switch changes lass_separate's bits: the route really ran
    assert not torch.equal(on[1], off[1]) and not torch.equal(on[2], off[2])


def test_a_clip_does_not_depend_on_its_batch(engine):
    _sc(engine, 1)
    _, mix = synthetic.make_mixtures(8, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(8)).to(DEV)
    singles = [engine.separate(mix[i:i + 1].contiguous(), cond[i:i + 1].contiguous()).cpu().clone() for i in range(8)]
    three = engine.separate(mix[:3].contiguous(), cond[:3].contiguous()).cpu()
    for i in range(3):
        assert torch.equal(three[i:i + 1], singles[i]), i
    # B = 8: two half-batch branches; the third call with the same pointers captures the graph, the fourth replays it
    out = torch.empty_like(mix)
    _, _, rep0 = engine.graph_stats()
    runs = []
    for _ in range(4):
        engine.separate(mix, cond, out=out)
        torch.cuda.synchronize()
        runs.append(out.cpu().clone())
    on, _, rep = engine.graph_stats()
    assert on and rep - rep0 >= 1, (on, rep0, rep)
    assert bool(torch.isfinite(runs[0]).all())
    for r in runs:
        for i in range(8):
            assert torch.equal(r[i:i + 1], singles[i]), i


def test_the_switch_leaves_every_other_route_alone(engine, synthetic_sd):
    """under lass_set_head_fold(0), in the stage calls and in the bf16 mode the switch changes no bit"""
    B = 2
    _, mix_np = synthetic.make_mixtures(B, L)
    mix, cond = torch.from_numpy(mix_np).to(DEV), torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    g = torch.Generator().manual_seed(67)
    x_enc = torch.randn(B, 32, 16, 64, generator=g).to(DEV)
    x_low = torch.randn(B, 64, 8, 256, generator=g).to(DEV)
    cat = torch.randn(B, 64, 16, 512, generator=g).to(DEV)
    shift = engine.film(cond)

    def stages():
        y, pool = engine.encoder_block("base.encoder_block1", x_enc, shift, 32, (2, 2))
        up = engine.upconv("base.decoder_block6", x_low, shift, 32, (2, 2))
        blk = engine.convblock("base.decoder_block6.conv_block2", cat, shift, 32)
        return [t.cpu().clone() for t in (y, pool, up, blk)]
    try:
        _sc(engine, 1)
        st_on = stages()
        _fold(engine, 0)
        unfolded_on = _run(engine, mix, cond, B, L)
        _sc(engine, 0)
        unfolded_off = _run(engine, mix, cond, B, L)
        _fold(engine, 1)
        st_off = stages()
    finally:
        _fold(engine, 1)
        _sc(engine, 1)
    for a, b in zip(unfolded_on, unfolded_off):
        assert torch.equal(a, b)
    for a, b in zip(st_on, st_off):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    from lass_amd.engine import Engine
    e16 = Engine(DEV)
    e16.load_state_dict(synthetic_sd, compute_dtype="bf16")
    on = e16.separate(mix, cond).cpu().clone()
    _sc(e16, 0)
    off = e16.separate(mix, cond).cpu().clone()
    assert bool(torch.isfinite(on).all()) and torch.equal(on, off)


def test_the_switch_leaves_the_multistft_model_alone():
    """1 024 bins, 3 clips of 5 000 samples (32 frames): the smallest clip test_multistft_model.py runs through the model"""
    from lass_amd.resunet_with_multistft import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict_ms().items()})
    m = m.to(DEV).eval()
    B, length = 3, 5000
    _, mix = synthetic.make_mixtures(B, length)
    inp = {"mixture": torch.from_numpy(mix)[:, None].to(DEV), "condition": torch.from_numpy(synthetic.make_condition(B)).to(DEV)}
    on = m(inp)["waveform"].cpu().clone()   # (the first call creates the engine: the switch is on by default)
    e = m.engine
    try:
        _sc(e, 0)
        off = m(inp)["waveform"].cpu().clone()
    finally:
        _sc(e, 1)
    assert bool(torch.isfinite(on).all()) and float(on.pow(2).mean().sqrt()) > 1e-3
    assert torch.equal(on, off)


def test_the_logit_planes_hold_the_composed_shortcut_of_their_inputs(engine, synthetic_sd):
    """after one call with the route on: head_sc.skip = Wsc'_skip x1 and head_sc.up = Wt' act(x11), against float64 references
    formed on the host from the skip and x11 as the workspace holds them"""
    B = 2
    _, mix = synthetic.make_mixtures(B, L)
    mix, cond = torch.from_numpy(mix).to(DEV), torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    _sc(engine, 1)
    engine.separate(mix, cond)
    torch.cuda.synchronize()
    skip = engine.workspace_tensor("encoder_block1", B, L).clone().cpu().double()    # x1 (B, 32, 128, 512)
    x11 = engine.workspace_tensor("decoder_block5", B, L).clone().cpu().double()     # (B, 64, 64, 256)
    p_skip = engine.workspace_tensor("head_sc.skip", B, L).clone().cpu().double()
    p_up = engine.workspace_tensor("head_sc.up", B, L).clone().cpu().double()
    assert p_skip.shape == p_up.shape == (B, 3, skip.shape[2], skip.shape[3])
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synthetic_sd.items()
          if k.startswith(("base.after_conv", "base.decoder_block6.bn1", "base.decoder_block6.conv1", "base.decoder_block6.conv_block2.shortcut"))}
    wsc = sd["base.after_conv.weight"].reshape(3, 32) @ sd["base.decoder_block6.conv_block2.shortcut.weight"].reshape(32, 64)   # Wsc' (3, 64)
    ref_skip = torch.einsum("qc,bchw->bqhw", wsc[:, 32:], skip)
    bn = "base.decoder_block6.bn1."
    scale = sd[bn + "weight"] / torch.sqrt(sd[bn + "running_var"] + 1e-5)
    off = engine.film_offset("decoder_block6->beta1")
    shift = engine.film(cond).cpu().double()[:, off:off + 64]   # FiLM beta + the folded BN shift, as the kernels read it
    act = torch.nn.functional.leaky_relu(x11 * scale[None, :, None, None] + shift[:, :, None, None], 0.01)
    up = torch.nn.functional.conv_transpose2d(act, sd["base.decoder_block6.conv1.weight"], stride=(2, 2))
    ref_up = torch.einsum("qc,bchw->bqhw", wsc[:, :32], up)
    for name, got, ref in (("head_sc.skip", p_skip, ref_skip), ("head_sc.up", p_up, ref_up)):
        d = float((got - ref).abs().max()) / float(ref.abs().max())
        print(f"{name}: max |dev| / max |ref| {d:.3e} (max |ref| {float(ref.abs().max()):.3e})")
        assert float(ref.abs().max()) > 1e-3
        assert d < PLANE_BAR, (name, d)
    # with the route off the plan has no such tensors
    try:
        _sc(engine, 0)
        with pytest.raises(_lib.LassError):
            engine.workspace_tensor("head_sc.skip", B, L)
    finally:
        _sc(engine, 1)


def test_second_weight_set_route_on_against_route_off():
    """the on-against-off comparison on the weights, conditions and clips of fixture G4 (320 x 512: 40 rows of blocks), at the
    waveform bars only: what holds this weight set to the reference is the G4 test itself, with the route as the default."""
    from lass_amd.engine import Engine
    from test_oracle_golden import G4_SEED
    sd = synthetic.make_state_dict(seed=G4_SEED)
    e = Engine(DEV)
    e.load_state_dict(sd)
    B, length = 2, 48000
    _, mix = synthetic.make_mixtures(B, length, first=20)
    _on_against_off(e, None, mix, synthetic.make_condition(B, seed=G4_SEED), "second weight set B=2 L=48000")
