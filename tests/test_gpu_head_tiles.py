"""The folded head on 4-row MFMA blocks (wino4_head_body.h: both wino4_headfold_planes_kernel, the default, and wino4_headfold_kernel,
lass_set_head_sc_fold(ctx, 0)), its early exit for blocks of rows beyond mask_T, and the transposed conv's three logit planes, at the
two shortest geometries: L = 4 000 (26 frames padded to 32: four 8-row blocks, the last valid frame inside a 4-row tile) and
L = 16 000 (101 frames padded to 128: rows 104 .. 127 are whole blocks beyond mask_T, frame 100 sits inside a tile).  Bars and
helper style of test_gpu_head_sc_fold.py / test_gpu_head_fold.py; seeded synthetic weights; every run is made once and shared."""
import numpy as np
import pytest
import torch

from lass_amd import _lib, arch, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WAVE_BAR = 3e-6   # RMS of an f32 waveform, relative and absolute (test_gpu_head_fold.py)
SPEC_BAR = 3e-5   # max |deviation| of the separated spectrum / its largest magnitude
PLANE_BAR = 1e-5  # an f32 sum of 32 or 64 products against float64, of the planes' largest magnitude
SENTINEL = -12345.678  # no output of mask_pixel: |out| <= mag, and the synthetic mixtures stay far below

# (head_fold, head_sc_fold): the planes kernel, the round-11 kernel with its shortcut phase, the unfolded head
PLANES, SHORTCUT, UNFOLDED = (1, 1), (1, 0), (0, 1)


def _switch(e, fold, sc):
    _lib.check(e.ctx, e.lib.lass_set_head_fold(e.ctx, fold), "lass_set_head_fold")
    _lib.check(e.ctx, e.lib.lass_set_head_sc_fold(e.ctx, sc), "lass_set_head_sc_fold")


def _relerr(got, ref):
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30))


@pytest.fixture(scope="module")
def engine(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    return e


def _inputs(B, length):
    _, mix = synthetic.make_mixtures(B, length)
    return mix, synthetic.make_condition(B)


def _run(e, mix_np, cond_np, route, first=0, n=None):
    """(waveform, out_real, out_imag) of one lass_separate over clips [first, first + n), on the CPU"""
    n = mix_np.shape[0] - first if n is None else n
    length = mix_np.shape[1]
    mix = torch.from_numpy(mix_np[first:first + n]).contiguous().to(DEV)
    cond = torch.from_numpy(cond_np[first:first + n]).contiguous().to(DEV)
    try:
        _switch(e, *route)
        wav = e.separate(mix, cond).cpu().clone()
        torch.cuda.synchronize()
        re = e.workspace_tensor("out_real", n, length).clone().cpu()
        im = e.workspace_tensor("out_imag", n, length).clone().cpu()
    finally:
        _switch(e, 1, 1)
    assert re.shape[2] == arch.frames_for(length)
    return wav, re, im


@pytest.fixture(scope="module")
def runs(engine):
    """runs(length, B, route) -> (waveform, out_real, out_imag), each computed once and never changed"""
    cache = {}

    def get(length, B, route=PLANES):
        key = (length, B, route)
        if key not in cache:
            cache[key] = _run(engine, *_inputs(B, length), route)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def oracle_spec(synthetic_sd):
    """oracle(length, B) -> (out_real, out_imag) of the CPU oracle"""
    from oracle import resunet as orr
    sd_torch = orr.to_torch(synthetic_sd)
    cache = {}

    def get(length, B):
        if (length, B) not in cache:
            mix, cond = _inputs(B, length)
            taps = {}
            orr.forward(sd_torch, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": torch.from_numpy(cond)}, taps=taps)
            cache[(length, B)] = (taps["out_real"], taps["out_imag"])
        return cache[(length, B)]
    return get


def _three_comparisons(runs, oracle_spec, length, B):
    what = f"B={B} L={length}"
    got = {name: runs(length, B, route) for name, route in (("planes", PLANES), ("shortcut", SHORTCUT), ("unfolded", UNFOLDED))}
    for a, b in (("planes", "shortcut"), ("planes", "unfolded"), ("shortcut", "unfolded")):
        on, off = got[a], got[b]
        err, rel = float((on[0] - off[0]).pow(2).mean().sqrt()), _relerr(on[0], off[0])
        print(f"{what}: {a} vs {b}, waveform RMS difference {err:.3e}, relative {rel:.3e}, bitwise equal {torch.equal(on[0], off[0])}")
        assert bool(torch.isfinite(on[0]).all()) and bool(torch.isfinite(off[0]).all())
        assert rel < WAVE_BAR, (a, b, rel)
        assert err < WAVE_BAR, (a, b, err)
        for i, name in ((1, "out_real"), (2, "out_imag")):
            d = float((on[i] - off[i]).abs().max()) / float(off[i].abs().max())
            print(f"{what}: {name} {a} vs {b}, max |difference| / max |value| {d:.3e}")
            assert d < SPEC_BAR, (a, b, name, d)
    ref = oracle_spec(length, B)
    for route, r in got.items():
        assert bool((r[1][..., -1] == 0).all()) and bool((r[2][..., -1] == 0).all())   # the dropped Nyquist bin: an exact zero
        for i, name in ((1, "out_real"), (2, "out_imag")):
            rf = ref[i - 1].reshape(r[i].shape)
            d = float((r[i] - rf).abs().max()) / float(rf.abs().max())
            print(f"{what}: {name} max |dev| / max |ref| vs the oracle, {route}: {d:.3e}")
            assert d < SPEC_BAR, (route, name, d)
    # the switches change lass_separate's bits (the shortcut's sum is re-associated): each route really ran
    assert not torch.equal(got["planes"][1], got["shortcut"][1]) and not torch.equal(got["shortcut"][1], got["unfolded"][1])


@pytest.mark.parametrize("B", [1, 2, 3])
def test_shortest_plan_against_both_switches_and_the_oracle(runs, oracle_spec, B):
    _three_comparisons(runs, oracle_spec, 4000, B)


def test_whole_blocks_beyond_mask_t_against_both_switches_and_the_oracle(runs, oracle_spec):
    _three_comparisons(runs, oracle_spec, 16000, 3)


@pytest.mark.parametrize("route", [PLANES, SHORTCUT], ids=["planes", "shortcut"])
def test_every_valid_row_is_written_and_nothing_else(engine, runs, route):
    """out_real / out_imag filled with a sentinel in front of the call: every element of the T valid rows is written, the Nyquist
    bin with an exact 0, and the result is the shared run's, bit for bit.  The two tensors hold T rows per clip, not the padded
    count: a row >= T of clip i written by mistake would land in clip i + 1's rows (or behind the tensor) and race with their
    owners, which the bitwise comparisons here and below would see; the floats of the alignment gap between the two tensors must
    still hold the sentinel."""
    B, length = 3, 16000
    ref = runs(length, B, route)   # (leaves a workspace of this shape behind)
    T = arch.frames_for(length)
    mix_np, cond_np = _inputs(B, length)
    mix, cond = torch.from_numpy(mix_np).to(DEV), torch.from_numpy(cond_np).to(DEV)
    try:
        _switch(engine, *route)
        engine.separate(mix, cond)
        torch.cuda.synchronize()
        re, im = engine.workspace_tensor("out_real", B, length), engine.workspace_tensor("out_imag", B, length)
        assert re.shape == im.shape == (B, 1, T, 513) and re.is_contiguous() and im.is_contiguous()
        lo, hi = re.data_ptr(), im.data_ptr() + im.numel() * 4
        assert lo < im.data_ptr() and (hi - lo) % 4 == 0
        span = re.as_strided(((hi - lo) // 4,), (1,))   # out_real, the gap, out_imag
        gap = span[re.numel():(im.data_ptr() - lo) // 4]
        span.fill_(SENTINEL)
        wav = engine.separate(mix, cond).cpu().clone()
        torch.cuda.synchronize()
        re_c, im_c, gap_c = re.clone().cpu(), im.clone().cpu(), gap.clone().cpu()
    finally:
        _switch(engine, 1, 1)
    sent = torch.tensor(SENTINEL, dtype=torch.float32)
    assert not bool((re_c == sent).any()) and not bool((im_c == sent).any())
    assert bool((gap_c == sent).all()), "a write between out_real and out_imag"
    assert bool((re_c[..., -1] == 0).all()) and bool((im_c[..., -1] == 0).all())
    assert torch.equal(wav, ref[0]) and torch.equal(re_c, ref[1]) and torch.equal(im_c, ref[2])


@pytest.mark.parametrize("length", [4000, 16000])
def test_a_clip_does_not_depend_on_its_batch(engine, runs, length):
    three = runs(length, 3)
    mix, cond = _inputs(3, length)
    for i in range(3):
        single = _run(engine, mix, cond, PLANES, first=i, n=1)
        for a, b in zip(three, single):
            assert torch.equal(a[i:i + 1], b), (length, i)


def _planes_and_up(engine, B, length, sc):
    mix_np, cond_np = _inputs(B, length)
    mix, cond = torch.from_numpy(mix_np).to(DEV), torch.from_numpy(cond_np).to(DEV)
    try:
        _switch(engine, 1, sc)
        engine.separate(mix, cond)
        torch.cuda.synchronize()
        up = engine.workspace_tensor("decoder_block6.up", B, length).clone().cpu()
        x11 = engine.workspace_tensor("decoder_block5", B, length).clone().cpu()
        p_up = engine.workspace_tensor("head_sc.up", B, length).clone().cpu() if sc else None
    finally:
        _switch(engine, 1, 1)
    return up, x11, p_up, cond


@pytest.mark.parametrize("length", [4000, 16000])
def test_the_up_planes_per_logit_and_sub_pixel_and_the_ordinary_output(engine, synthetic_sd, length):
    """head_sc.up = Wt' act(x11) against a float64 composition of its inputs (as test_gpu_head_sc_fold.py builds it), held per
    logit q and sub-pixel (a, bb) - column (q * 2 + a) * 2 + bb of the slab, so column 11 = (2, 1, 1) and the last row pair of the
    image have a figure of their own - and the transposed conv's 32 ordinary channels byte-equal with the route on and off."""
    B = 2
    up_on, x11_on, p_up, cond = _planes_and_up(engine, B, length, 1)
    up_off, x11_off, _, _ = _planes_and_up(engine, B, length, 0)
    assert torch.equal(x11_on, x11_off)
    assert bool(torch.isfinite(up_on).all()) and torch.equal(up_on, up_off)
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synthetic_sd.items()
          if k.startswith(("base.after_conv", "base.decoder_block6.bn1", "base.decoder_block6.conv1", "base.decoder_block6.conv_block2.shortcut"))}
    wsc = sd["base.after_conv.weight"].reshape(3, 32) @ sd["base.decoder_block6.conv_block2.shortcut.weight"].reshape(32, 64)   # Wsc' (3, 64)
    bn = "base.decoder_block6.bn1."
    scale = sd[bn + "weight"] / torch.sqrt(sd[bn + "running_var"] + 1e-5)
    off = engine.film_offset("decoder_block6->beta1")
    shift = engine.film(cond).cpu().double()[:, off:off + 64]   # FiLM beta + the folded BN shift, as the kernels read it
    act = torch.nn.functional.leaky_relu(x11_on.double() * scale[None, :, None, None] + shift[:, :, None, None], 0.01)
    up = torch.nn.functional.conv_transpose2d(act, sd["base.decoder_block6.conv1.weight"], stride=(2, 2))
    ref = torch.einsum("qc,bchw->bqhw", wsc[:, :32], up)
    got = p_up.double()
    assert got.shape == ref.shape == (B, 3, 2 * x11_on.shape[2], 2 * x11_on.shape[3])
    top = float(ref.abs().max())
    assert top > 1e-3
    for q in range(3):
        for a in range(2):
            for bb in range(2):
                g, r = got[:, q, a::2, bb::2], ref[:, q, a::2, bb::2]
                d = float((g - r).abs().max()) / top
                d_last = float((g[:, -1] - r[:, -1]).abs().max()) / top   # the last input row: the y >= H edge of the block above it
                print(f"L={length} head_sc.up column {(q * 2 + a) * 2 + bb} (q={q}, a={a}, bb={bb}): max |dev| / max |ref| {d:.3e}, last row {d_last:.3e}")
                assert float(r.abs().max()) > 1e-4
                assert d < PLANE_BAR, (q, a, bb, d)


def test_second_weight_set_route_on_against_route_off():
    """the weights, conditions and clips of fixture G4 at L = 16 000, B = 2: the planes kernel against the kernel with the shortcut
    phase, at the waveform bars (what holds this weight set to the reference is the G4 test itself, with the route as the default)"""
    from lass_amd.engine import Engine
    from test_oracle_golden import G4_SEED
    e = Engine(DEV)
    e.load_state_dict(synthetic.make_state_dict(seed=G4_SEED))
    B, length = 2, 16000
    _, mix = synthetic.make_mixtures(B, length, first=20)
    cond = synthetic.make_condition(B, seed=G4_SEED)
    on, off = _run(e, mix, cond, PLANES), _run(e, mix, cond, SHORTCUT)
    err, rel = float((on[0] - off[0]).pow(2).mean().sqrt()), _relerr(on[0], off[0])
    print(f"second weight set B=2 L=16000: route on vs off, waveform RMS difference {err:.3e}, relative {rel:.3e}")
    assert bool(torch.isfinite(on[0]).all()) and float(off[0].pow(2).mean().sqrt()) > 1e-3   # a real waveform to be relative to
    assert rel < WAVE_BAR, rel
    assert err < WAVE_BAR, err
    assert not torch.equal(on[1], off[1])   # the route really ran
