"""wino4.hip at the 32-frame x 16-bin level: encoder_block6 and decoder_block1 as split-K Winograd F(4x4,3x3) launches (the
input-channel loop dealt to S workgroups, partial sums combined in split order by wino4_combine_kernel), held to the oracle
(oracle/resunet.py) at the block bar of test_gpu_stages.py::test_wino4_convblock_vs_oracle_and_wino (2e-5 relative) and to
the F(2x2,3x3) kernels (LASS_WINO4=0) on the same blocks."""
import pytest
import torch
import torch.nn.functional as F

from lass_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W4_BAR = 2e-5   # test_wino4_convblock_vs_oracle_and_wino: relative RMS of a F(4x4,3x3) block
W2_BAR = 5e-6   # ... and of a F(2x2,3x3) block (test_convblock_vs_oracle)
H, W = 32, 16   # one 32 x 16 block per clip plane


def _relerr(got, ref):
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30))


def _check_block(got, ref, what):
    err = _relerr(got, ref)
    print(what, "relative RMS error vs oracle", err, "max abs", float((got - ref).abs().max()))
    assert got.shape == ref.shape
    assert err < W4_BAR, (what, err)
    assert float((got - ref).abs().max()) < 3e-4 * max(1.0, float(ref.abs().max())), what


@pytest.fixture(scope="module")
def oracle_sd(synthetic_sd):
    from oracle import resunet as orr
    return orr.to_torch(synthetic_sd)


def _engine(synthetic_sd, monkeypatch=None, wino4=None):
    from lass_amd.engine import Engine
    if wino4 is not None:
        monkeypatch.setenv("LASS_WINO4", wino4)
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    if wino4 is not None:
        monkeypatch.delenv("LASS_WINO4")
    return e


def _splits(e, n):
    from lass_amd import _lib
    _lib.check(e.ctx, e.lib.lass_set_wino4_splits(e.ctx, n), "lass_set_wino4_splits")


def _enc6(e, x, cond):
    y, pool = e.encoder_block("base.encoder_block6", x.to(DEV), e.film(cond.to(DEV)), 384, (1, 2))
    return y.cpu(), pool.cpu()


def _enc6_ref(oracle_sd, x, cond):
    from oracle import resunet as orr
    ref = orr.conv_block_res(oracle_sd, "base.encoder_block6.conv_block1", x, orr.film(oracle_sd, cond, "encoder_block6->conv_block1->beta1"),
                             orr.film(oracle_sd, cond, "encoder_block6->conv_block1->beta2"))
    return ref, F.avg_pool2d(ref, (1, 2))


def _dec1(e, xlow, skip, cond):
    """decoder_block1 as lass_separate runs it: the (1, 2) transposed conv, the concat with the skip, the ConvBlockRes (768 -> 384)
    whose 1x1 shortcut runs in pw_gemm.hip"""
    shift = e.film(cond.to(DEV))
    up = e.upconv("base.decoder_block1", xlow.to(DEV), shift, 384, (1, 2))
    cat = torch.cat((up, skip.to(DEV)), 1).contiguous()
    return e.convblock("base.decoder_block1.conv_block2", cat, shift, 384).cpu()


def _dec1_ref(oracle_sd, xlow, skip, cond):
    from oracle import resunet as orr
    hh = F.leaky_relu(orr._bn(oracle_sd, "base.decoder_block1.bn1", xlow) + orr.film(oracle_sd, cond, "decoder_block1->beta1"), 0.01)
    up = F.conv_transpose2d(hh, oracle_sd["base.decoder_block1.conv1.weight"], stride=(1, 2))
    return orr.conv_block_res(oracle_sd, "base.decoder_block1.conv_block2", torch.cat((up, skip), 1),
                              orr.film(oracle_sd, cond, "decoder_block1->conv_block2->beta1"),
                              orr.film(oracle_sd, cond, "decoder_block1->conv_block2->beta2"))


@pytest.fixture(scope="module")
def engine(synthetic_sd):
    return _engine(synthetic_sd)


@pytest.mark.parametrize("B", [1, 2, 16])
def test_encoder_block6_with_1x2_pool_vs_oracle(engine, oracle_sd, B):
    g = torch.Generator().manual_seed(600 + B)
    x = torch.randn(B, 384, H, W, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    y, pool = _enc6(engine, x, cond)
    ref, rpool = _enc6_ref(oracle_sd, x, cond)
    _check_block(y, ref, f"encoder_block6 B={B}")
    _check_block(pool, rpool, f"encoder_block6 pool B={B}")


@pytest.mark.parametrize("B", [1, 2, 16])
def test_decoder_block1_with_upconv_and_shortcut_vs_oracle(engine, oracle_sd, B):
    g = torch.Generator().manual_seed(100 + B)
    xlow = torch.randn(B, 384, H, W // 2, generator=g)
    skip = torch.randn(B, 384, H, W, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    _check_block(_dec1(engine, xlow, skip, cond), _dec1_ref(oracle_sd, xlow, skip, cond), f"decoder_block1 B={B}")


def test_forced_splits_agree_and_match_the_f2x2_route(synthetic_sd, oracle_sd, monkeypatch):
    """S = 1 (the unsplit 32 x 16 kernels, fused 1 x 2 pool), 2 and 4 compute the same sums in another order: they agree to f32
    summation noise (far inside the block bar), each meets the oracle at the F(4x4,3x3) bar, and the F(2x2,3x3) route
    (LASS_WINO4=0) on the same input meets its own bar and is within the F(4x4,3x3) bar of them."""
    B = 2
    g = torch.Generator().manual_seed(4242)
    x = torch.randn(B, 384, H, W, generator=g)
    xlow = torch.randn(B, 384, H, W // 2, generator=g)
    skip = torch.randn(B, 384, H, W, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    e = _engine(synthetic_sd)
    enc, dec = {}, {}
    for s in (1, 2, 4):
        _splits(e, s)
        enc[s] = _enc6(e, x, cond)
        dec[s] = _dec1(e, xlow, skip, cond)
    e2 = _engine(synthetic_sd, monkeypatch, "0")
    enc[0] = _enc6(e2, x, cond)
    dec[0] = _dec1(e2, xlow, skip, cond)
    ref, rpool = _enc6_ref(oracle_sd, x, cond)
    dref = _dec1_ref(oracle_sd, xlow, skip, cond)
    for s in (1, 2, 4):
        _check_block(enc[s][0], ref, f"encoder_block6 S={s}")
        _check_block(enc[s][1], rpool, f"encoder_block6 pool S={s}")
        _check_block(dec[s], dref, f"decoder_block1 S={s}")
    for s in (2, 4):
        for got, one, what in ((enc[s][0], enc[1][0], "enc6"), (enc[s][1], enc[1][1], "enc6 pool"), (dec[s], dec[1], "dec1")):
            d = _relerr(got, one)
            print(what, f"S={s} vs S=1 relative RMS", d)
            # Another summation order re-draws the route's rounding: DESIGN.md section 4 puts that at 2-5e-6 relative per
            # F(4x4,3x3) layer, so two independent draws differ by up to sqrt(2) * 5e-6 per layer, through the two convs of a
            # block sqrt(2) times that again: 1e-5, half the block bar
            assert d < 1e-5, (what, s, d)
    assert not torch.equal(enc[4][0], enc[1][0]) and not torch.equal(dec[2], dec[1])   # really other launches
    for got, r, what in ((enc[0][0], ref, "enc6"), (enc[0][1], rpool, "enc6 pool"), (dec[0], dref, "dec1")):
        assert _relerr(got, r) < W2_BAR, (what, _relerr(got, r))                          # F(2x2,3x3) at its own bar
    for s in (1, 2, 4):
        for got, two, what in ((enc[s][0], enc[0][0], "enc6"), (enc[s][1], enc[0][1], "enc6 pool"), (dec[s], dec[0], "dec1")):
            assert _relerr(got, two) < W4_BAR, (what, s, _relerr(got, two))
            assert not torch.equal(got, two)                                                  # really another kernel


@pytest.mark.parametrize("B", [16, 2])   # 16: two half-batch branches of the replayed graph; 2: one stream
def test_separate_is_bit_identical_from_run_to_run(synthetic_sd, B):
    e = _engine(synthetic_sd)
    L = 160000   # 1001 frames -> 1024 padded: the 16-bin level is 32 x 16
    _, mix = synthetic.make_mixtures(B, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    out = torch.empty_like(mix)
    runs = []
    for _ in range(5):   # the third call with the same pointers captures the graph; later ones replay it
        e.separate(mix, cond, out=out)
        torch.cuda.synchronize()
        runs.append(out.cpu().clone())
    assert bool(torch.isfinite(runs[0]).all())
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    e3 = _engine(synthetic_sd)
    assert torch.equal(e3.separate(mix, cond).cpu(), runs[0])   # another context, another workspace


def test_other_frame_counts_stay_on_f2x2_at_the_bottom(synthetic_sd, oracle_sd):
    """T = 151 -> 160 padded frames: the 16-bin level is 5 x 16, no 32 x 16 block - encoder_block6 and decoder_block1 keep the
    F(2x2,3x3) kernels (forcing a split factor changes nothing, bit for bit) and the waveform meets the parity bar."""
    from oracle import resunet as orr
    B, L = 2, 24000
    _, mix = synthetic.make_mixtures(B, L)
    cond = synthetic.make_condition(B)
    e = _engine(synthetic_sd)
    a = e.separate(torch.from_numpy(mix).to(DEV), torch.from_numpy(cond).to(DEV)).cpu()
    _splits(e, 4)
    b = e.separate(torch.from_numpy(mix).to(DEV), torch.from_numpy(cond).to(DEV)).cpu()
    assert torch.equal(a, b)
    ref = orr.forward(oracle_sd, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": torch.from_numpy(cond)})["waveform"]
    err = float((a - ref.reshape(a.shape)).pow(2).mean().sqrt())
    print("T=151 waveform RMS error vs oracle", err)
    assert err <= 1e-4, err
    # the same at the stage level: a 6 x 16 plane through encoder_block6
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 384, 6, 16, generator=g)
    c = torch.from_numpy(cond)
    y4, p4 = _enc6(e, x, c)
    _splits(e, 0)
    y0, p0 = _enc6(e, x, c)
    assert torch.equal(y4, y0) and torch.equal(p4, p0)
    r = orr.conv_block_res(oracle_sd, "base.encoder_block6.conv_block1", x, orr.film(oracle_sd, c, "encoder_block6->conv_block1->beta1"),
                           orr.film(oracle_sd, c, "encoder_block6->conv_block1->beta2"))
    assert _relerr(y0, r) < W2_BAR, _relerr(y0, r)


def test_whole_model_with_the_new_routes_vs_f2x2_everywhere(synthetic_sd, monkeypatch):
    """10 s clips (the bench shape): the default routes against LASS_WINO4=0 at test_wino4_routes_agree's bar (2e-5 RMS)."""
    B, L = 2, 160000
    _, mix = synthetic.make_mixtures(B, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    a = _engine(synthetic_sd).separate(mix, cond).cpu()
    b = _engine(synthetic_sd, monkeypatch, "0").separate(mix, cond).cpu()
    err = float((a - b).pow(2).mean().sqrt())
    print("default routes vs LASS_WINO4=0: waveform RMS difference", err, "signal RMS", float(b.pow(2).mean().sqrt()))
    assert err <= 2e-5, err
