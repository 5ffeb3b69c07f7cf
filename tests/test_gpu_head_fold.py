"""The folded output head: lass_separate's last launch (decoder_block6's conv2 + 1x1 shortcut + after_conv + mask) on weights
composed with after_conv (head_fold.h, wino4_headfold_kernel), against the unfolded launch (lass_set_head_fold(ctx, 0)) and the
oracle.  The fold re-associates the last linear layer, so the two are not bitwise equal; they are held to the suite's f32 bars.

Cases 1 to 3 run B = 2 or 3 clips of L = 16 000: 101 frames padded to 128, at 512 bins - the last valid frame falls inside a
4-row tile, whole 8-row blocks lie beyond mask_T, and the Nyquist column is written: the smallest shape that exercises the row
guards, the block edges and the Nyquist zero."""
import numpy as np
import pytest
import torch

from lass_amd import _lib, arch, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WAVE_BAR = 3e-6   # RMS of an f32 waveform, relative and absolute (test_gpu_wino4_vprep.py)
SPEC_BAR = 3e-5   # max |deviation| of the separated spectrum / its largest magnitude (test_hip_taps_vs_oracle_every_element)
L = 16000


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
    """the waveform of fold on against fold off at the f32 bar and the two separated spectra against each other, every element
    (two f32 evaluations of one tensor must agree at least as well as either must agree with the oracle: SPEC_BAR); with
    sd_torch each run's spectrum against the oracle's as well"""
    from oracle import resunet as orr
    B, length = mix_np.shape
    mix, cond = torch.from_numpy(mix_np).to(DEV), torch.from_numpy(cond_np).to(DEV)
    try:
        _fold(e, 1)
        on = _run(e, mix, cond, B, length)
        _fold(e, 0)
        off = _run(e, mix, cond, B, length)
    finally:
        _fold(e, 1)
    err, rel = float((on[0] - off[0]).pow(2).mean().sqrt()), _relerr(on[0], off[0])
    print(f"{what}: fold on vs off, waveform RMS difference {err:.3e}, relative {rel:.3e}, bitwise equal {torch.equal(on[0], off[0])}")
    assert bool(torch.isfinite(on[0]).all()) and float(off[0].pow(2).mean().sqrt()) > 1e-3   # a real waveform to be relative to
    assert rel < WAVE_BAR, rel
    assert err < WAVE_BAR, err
    for i, name in ((1, "out_real"), (2, "out_imag")):
        d = float((on[i] - off[i]).abs().max()) / float(off[i].abs().max())
        print(f"{what}: {name} fold on vs off, max |difference| / max |value| {d:.3e}")
        assert d < SPEC_BAR, (name, d)
    # the dropped Nyquist bin is an exact zero either way
    assert bool((on[1][..., -1] == 0).all()) and bool((on[2][..., -1] == 0).all())
    if sd_torch is None:
        return on, off
    taps = {}
    orr.forward(sd_torch, {"mixture": torch.from_numpy(mix_np)[:, None, :], "condition": torch.from_numpy(cond_np)}, taps=taps)
    devs = {}
    for i, name in ((1, "out_real"), (2, "out_imag")):
        ref = taps[name].reshape(on[i].shape)
        scale = float(ref.abs().max())
        devs[name] = (float((on[i] - ref).abs().max()) / scale, float((off[i] - ref).abs().max()) / scale)
        print(f"{what}: {name} max |dev| / max |ref| vs the oracle: fold on {devs[name][0]:.3e}, fold off {devs[name][1]:.3e}")
    for name, (d_on, d_off) in devs.items():
        assert d_on < SPEC_BAR, (name, "fold on", d_on)
        assert d_off < SPEC_BAR, (name, "fold off", d_off)
    return on, off


def test_fold_on_against_fold_off_and_the_oracle(engine, synthetic_sd):
    from oracle import resunet as orr
    B = 2
    _, mix = synthetic.make_mixtures(B, L)
    _on_against_off(engine, orr.to_torch(synthetic_sd), mix, synthetic.make_condition(B), "B=2 L=16000")


def test_the_folded_route_really_runs(engine, tmp_path):
    """the plan sends decoder_block6's conv2 to the folded kernel where it has a head (lass_separate) and nowhere else; the
    switch changes lass_separate's bits (the last layer is re-associated) and leaves the stage call's alone"""
    from test_head_fold_cpu import build_route_table
    rt = build_route_table(tmp_path)
    t_pad = (arch.frames_for(L) + 31) // 32 * 32
    assert {n for n, r in rt(t_pad).items() if r[2]} == {"decoder_block6.conv2"}
    assert not any(r[2] for r in rt(t_pad, head=0).values())        # the stage call: no head
    assert not any(r[2] for r in rt(t_pad, head_fold=0).values())   # the switch
    B = 2
    _, mix = synthetic.make_mixtures(B, L)
    mix, cond = torch.from_numpy(mix).to(DEV), torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    g = torch.Generator().manual_seed(66)
    cat = torch.randn(B, 64, 16, 512, generator=g).to(DEV)
    shift = engine.film(cond)
    try:
        _fold(engine, 1)
        on = _run(engine, mix, cond, B, L)
        st_on = engine.convblock("base.decoder_block6.conv_block2", cat, shift, 32).cpu()
        _fold(engine, 0)
        off = _run(engine, mix, cond, B, L)
        st_off = engine.convblock("base.decoder_block6.conv_block2", cat, shift, 32).cpu()
    finally:
        _fold(engine, 1)
    assert not torch.equal(on[1], off[1]) and not torch.equal(on[2], off[2])
    assert bool(torch.isfinite(st_on).all()) and torch.equal(st_on, st_off)


def test_a_clip_does_not_depend_on_its_batch_and_runs_repeat(engine):
    _, mix = synthetic.make_mixtures(3, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(3)).to(DEV)
    three = _run(engine, mix, cond, 3, L)
    one = _run(engine, mix[1:2].contiguous(), cond[1:2].contiguous(), 1, L)
    for a, b in zip(three, one):
        assert torch.equal(a[1:2], b)
    # five runs at B = 2: the third call with the same pointers captures the graph, later ones replay it
    mix2, cond2 = mix[:2].contiguous(), cond[:2].contiguous()
    out = torch.empty_like(mix2)
    runs = []
    for _ in range(5):
        engine.separate(mix2, cond2, out=out)
        torch.cuda.synchronize()
        runs.append(out.cpu().clone())
    assert bool(torch.isfinite(runs[0]).all())
    for r in runs[1:]:
        assert torch.equal(r, runs[0])


def test_b16_through_the_replayed_two_branch_graph_repeats(engine):
    B = 16
    _, mix = synthetic.make_mixtures(B, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    out = torch.empty_like(mix)
    _, _, rep0 = engine.graph_stats()
    runs = []
    for _ in range(6):   # the third call captures, the last three are replays
        engine.separate(mix, cond, out=out)
        torch.cuda.synchronize()
        runs.append(out.cpu().clone())
    on, _, rep = engine.graph_stats()
    assert on and rep - rep0 >= 3, (on, rep0, rep)
    assert bool(torch.isfinite(runs[0]).all())
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    # ... and clip 9 (second half-batch branch) is the clip alone
    alone = engine.separate(mix[9:10].contiguous(), cond[9:10].contiguous()).cpu()
    assert torch.equal(alone, runs[-1][9:10])


def test_multistft_model_fold_on_against_fold_off():
    """1 024 bins, 3 clips of 5 000 samples (32 frames): the smallest clip test_multistft_model.py runs through the model"""
    from lass_amd.resunet_with_multistft import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict_ms().items()})
    m = m.to(DEV).eval()
    B, length = 3, 5000
    _, mix = synthetic.make_mixtures(B, length)
    inp = {"mixture": torch.from_numpy(mix)[:, None].to(DEV), "condition": torch.from_numpy(synthetic.make_condition(B)).to(DEV)}
    on = m(inp)["waveform"].cpu().clone()   # (the first call creates the engine: fold on is the default)
    e = m.engine
    try:
        _fold(e, 0)
        off = m(inp)["waveform"].cpu().clone()
        _fold(e, 1)
        again = m(inp)["waveform"].cpu().clone()
    finally:
        _fold(e, 1)
    err, rel = float((on - off).pow(2).mean().sqrt()), _relerr(on, off)
    print(f"multi-STFT B=3 L=5000: fold on vs off, waveform RMS difference {err:.3e}, relative {rel:.3e}, bitwise equal {torch.equal(on, off)}")
    assert bool(torch.isfinite(on).all()) and float(off.pow(2).mean().sqrt()) > 1e-3
    assert rel < WAVE_BAR, rel
    assert err < WAVE_BAR, err
    assert torch.equal(on, again) and not torch.equal(on, off)


def test_second_weight_set_fold_on_against_fold_off():
    """the on-against-off comparison of the first test on the weights, conditions and clips of fixture G4 (320 x 512: 40 rows of
    blocks).  What holds this weight set to the reference is the G4 test itself (test_hip_path_vs_reference_fixture_g4, with
    the folded route as the default); the every-element oracle bar of the first test belongs to that test's inputs - here the
    spectra sit at 5.2e-5 / 3.1e-5 of their maximum from the oracle's with the UNFOLDED launch (6.0e-5 / 4.2e-5 folded), the
    f32 error of the 30 layers in front of the head."""
    from lass_amd.engine import Engine
    from test_oracle_golden import G4_SEED
    sd = synthetic.make_state_dict(seed=G4_SEED)
    e = Engine(DEV)
    e.load_state_dict(sd)
    B, length = 2, 48000
    _, mix = synthetic.make_mixtures(B, length, first=20)
    _on_against_off(e, None, mix, synthetic.make_condition(B, seed=G4_SEED), "second weight set B=2 L=48000")
