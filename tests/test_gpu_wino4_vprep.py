"""wino4.hip, V from memory: the layers with many output-channel groups read their transformed input image from one prep launch
(wino4_vprep_kernel) instead of forming it in every group's workgroups.  The route (lass_set_wino4_vprep, mode 2 = every layer
whose kind admits it) is held to the oracle at the F(4x4,3x3) block bar of test_gpu_wino4_splitk.py, to the kernels that transform
their own input (mode 0) on the same data at the same bar, and to batch invariance, run-to-run identity and the workspace rules.

encoder_block5 / decoder_block2 run at 32 x 32: two 16 x 32 blocks per plane - all four borders and an interior block edge.  No
other height is tested: at W = 32 lass_wino4_supported admits H % 16 == 0 only (the 8-row blocks need W % 64 == 0, the 32 x 16
ones W % 32 == 16), so no admitted H is not a multiple of 16."""
import pytest
import torch
import torch.nn.functional as F

from lass_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W4_BAR = 2e-5   # relative RMS of a F(4x4,3x3) block against the oracle (test_gpu_wino4_splitk.py)
WAVE_BAR = 3e-6  # RMS of the f32 10 s waveform against the oracle's (test_gpu_parity.py: test_separate_10s_vs_golden)


def _relerr(got, ref):
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30))


def _check_block(got, ref, what):
    err = _relerr(got, ref)
    print(what, "relative RMS error", err, "max abs", float((got - ref).abs().max()))
    assert got.shape == ref.shape
    assert err < W4_BAR, (what, err)
    assert float((got - ref).abs().max()) < 3e-4 * max(1.0, float(ref.abs().max())), what


@pytest.fixture(scope="module")
def oracle_sd(synthetic_sd):
    from oracle import resunet as orr
    return orr.to_torch(synthetic_sd)


@pytest.fixture(scope="module")
def engine(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    return e


def _vprep(e, mode):
    from lass_amd import _lib
    _lib.check(e.ctx, e.lib.lass_set_wino4_vprep(e.ctx, mode), "lass_set_wino4_vprep")


def _splits(e, n):
    from lass_amd import _lib
    _lib.check(e.ctx, e.lib.lass_set_wino4_splits(e.ctx, n), "lass_set_wino4_splits")


def _enc(e, n, x, cond, down):
    y, pool = e.encoder_block(f"base.encoder_block{n}", x.to(DEV), e.film(cond.to(DEV)), 384, down)
    return y.cpu(), pool.cpu()


def _enc_ref(oracle_sd, n, x, cond, down):
    from oracle import resunet as orr
    ref = orr.conv_block_res(oracle_sd, f"base.encoder_block{n}.conv_block1", x,
                             orr.film(oracle_sd, cond, f"encoder_block{n}->conv_block1->beta1"),
                             orr.film(oracle_sd, cond, f"encoder_block{n}->conv_block1->beta2"))
    return ref, F.avg_pool2d(ref, down)


def _dec(e, n, xlow, skip, cond, up):
    """decoder_block n as lass_separate runs it: transposed conv, concat with the skip, ConvBlockRes 768 -> 384 (shortcut in pw_gemm.hip)"""
    shift = e.film(cond.to(DEV))
    u = e.upconv(f"base.decoder_block{n}", xlow.to(DEV), shift, 384, up)
    cat = torch.cat((u, skip.to(DEV)), 1).contiguous()
    return e.convblock(f"base.decoder_block{n}.conv_block2", cat, shift, 384).cpu()


def _dec_ref(oracle_sd, n, xlow, skip, cond, up):
    from oracle import resunet as orr
    hh = F.leaky_relu(orr._bn(oracle_sd, f"base.decoder_block{n}.bn1", xlow) + orr.film(oracle_sd, cond, f"decoder_block{n}->beta1"), 0.01)
    u = F.conv_transpose2d(hh, oracle_sd[f"base.decoder_block{n}.conv1.weight"], stride=up)
    return orr.conv_block_res(oracle_sd, f"base.decoder_block{n}.conv_block2", torch.cat((u, skip), 1),
                              orr.film(oracle_sd, cond, f"decoder_block{n}->conv_block2->beta1"),
                              orr.film(oracle_sd, cond, f"decoder_block{n}->conv_block2->beta2"))


def _both_modes(e, fn):
    """fn() under mode 2 and mode 0; restores the shipped routing"""
    try:
        _vprep(e, 2)
        a = fn()
        _vprep(e, 0)
        b = fn()
    finally:
        _vprep(e, 1)
    return a, b


@pytest.mark.parametrize("B", [1, 2, 3])
def test_encoder_block5_vs_oracle_and_mode0(engine, oracle_sd, B):
    g = torch.Generator().manual_seed(500 + B)
    x = torch.randn(B, 256, 32, 32, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    (y2, p2), (y0, p0) = _both_modes(engine, lambda: _enc(engine, 5, x, cond, (2, 2)))
    ref, rpool = _enc_ref(oracle_sd, 5, x, cond, (2, 2))
    _check_block(y2, ref, f"encoder_block5 B={B} mode 2 vs oracle")
    _check_block(p2, rpool, f"encoder_block5 pool B={B} mode 2 vs oracle")
    _check_block(y0, ref, f"encoder_block5 B={B} mode 0 vs oracle")
    _check_block(y2, y0, f"encoder_block5 B={B} mode 2 vs mode 0")
    _check_block(p2, p0, f"encoder_block5 pool B={B} mode 2 vs mode 0")
    print(f"encoder_block5 B={B}: mode 2 bitwise equal to mode 0:", torch.equal(y2, y0) and torch.equal(p2, p0))


@pytest.mark.parametrize("B", [1, 2, 3])
def test_decoder_block2_vs_oracle_and_mode0(engine, oracle_sd, B):
    g = torch.Generator().manual_seed(200 + B)
    xlow = torch.randn(B, 384, 16, 16, generator=g)
    skip = torch.randn(B, 384, 32, 32, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    y2, y0 = _both_modes(engine, lambda: _dec(engine, 2, xlow, skip, cond, (2, 2)))
    ref = _dec_ref(oracle_sd, 2, xlow, skip, cond, (2, 2))
    _check_block(y2, ref, f"decoder_block2 B={B} mode 2 vs oracle")
    _check_block(y0, ref, f"decoder_block2 B={B} mode 0 vs oracle")
    _check_block(y2, y0, f"decoder_block2 B={B} mode 2 vs mode 0")
    print(f"decoder_block2 B={B}: mode 2 bitwise equal to mode 0:", torch.equal(y2, y0))


@pytest.mark.parametrize("splits", [4, 1])
@pytest.mark.parametrize("B", [1, 2])
def test_16_bin_level_split_and_unsplit_vs_oracle_and_mode0(engine, oracle_sd, B, splits):
    g = torch.Generator().manual_seed(60 + B)
    x = torch.randn(B, 384, 32, 16, generator=g)
    xlow = torch.randn(B, 384, 32, 8, generator=g)
    skip = torch.randn(B, 384, 32, 16, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    try:
        _splits(engine, splits)
        (y2, p2), (y0, p0) = _both_modes(engine, lambda: _enc(engine, 6, x, cond, (1, 2)))
        d2, d0 = _both_modes(engine, lambda: _dec(engine, 1, xlow, skip, cond, (1, 2)))
    finally:
        _splits(engine, 0)
    ref, rpool = _enc_ref(oracle_sd, 6, x, cond, (1, 2))
    dref = _dec_ref(oracle_sd, 1, xlow, skip, cond, (1, 2))
    what = f"B={B} S={splits}"
    _check_block(y2, ref, f"encoder_block6 {what} mode 2 vs oracle")
    _check_block(p2, rpool, f"encoder_block6 pool {what} mode 2 vs oracle")
    _check_block(d2, dref, f"decoder_block1 {what} mode 2 vs oracle")
    _check_block(y2, y0, f"encoder_block6 {what} mode 2 vs mode 0")
    _check_block(p2, p0, f"encoder_block6 pool {what} mode 2 vs mode 0")
    _check_block(d2, d0, f"decoder_block1 {what} mode 2 vs mode 0")
    print(f"16-bin level {what}: mode 2 bitwise equal to mode 0:", torch.equal(y2, y0) and torch.equal(p2, p0) and torch.equal(d2, d0))


def test_64_column_blocks_vs_oracle_and_mode0(engine, oracle_sd):
    """the 8-row x 64-column block kernels (TC = 16), which no level of the 10 s workload routes here: encoder_block5 and
    decoder_block2 at 16 x 64 - two blocks per plane, one above the other"""
    B = 2
    g = torch.Generator().manual_seed(1664)
    x = torch.randn(B, 256, 16, 64, generator=g)
    xlow = torch.randn(B, 384, 8, 32, generator=g)
    skip = torch.randn(B, 384, 16, 64, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    (y2, p2), (y0, p0) = _both_modes(engine, lambda: _enc(engine, 5, x, cond, (2, 2)))
    d2, d0 = _both_modes(engine, lambda: _dec(engine, 2, xlow, skip, cond, (2, 2)))
    ref, rpool = _enc_ref(oracle_sd, 5, x, cond, (2, 2))
    dref = _dec_ref(oracle_sd, 2, xlow, skip, cond, (2, 2))
    _check_block(y2, ref, "encoder_block5 16x64 mode 2 vs oracle")
    _check_block(p2, rpool, "encoder_block5 16x64 pool mode 2 vs oracle")
    _check_block(d2, dref, "decoder_block2 16x64 mode 2 vs oracle")
    _check_block(y2, y0, "encoder_block5 16x64 mode 2 vs mode 0")
    _check_block(p2, p0, "encoder_block5 16x64 pool mode 2 vs mode 0")
    _check_block(d2, d0, "decoder_block2 16x64 mode 2 vs mode 0")
    print("64-column blocks: mode 2 bitwise equal to mode 0:", torch.equal(y2, y0) and torch.equal(p2, p0) and torch.equal(d2, d0))


@pytest.mark.parametrize("case", ["enc5_32x32", "dec2_32x32", "enc5_16x64", "enc6_32x16_split1", "enc6_32x16_split4", "dec1_32x16_split1"])
def test_mode_2_takes_the_route(engine, case):
    """mode 2 must really run the prep launch for these layers, or its comparisons with mode 0 above would compare a route with
    itself: the stage call is given a zeroed V buffer of the caller's, which a routed layer leaves written and mode 0 untouched"""
    name, hw, split = (case.split("_") + ["split0"])[:3]
    H, W = (int(v) for v in hw.split("x"))
    B = 1
    g = torch.Generator().manual_seed(9)
    cond = torch.from_numpy(synthetic.make_condition(B))
    if name.startswith("enc"):
        n, down = int(name[3]), (2, 2) if name == "enc5" else (1, 2)
        x = torch.randn(B, 256 if n == 5 else 384, H, W, generator=g)
        run = lambda: _enc(engine, n, x, cond, down)[0]
        cmax = 384
    else:
        n, up = int(name[3]), (2, 2) if name == "dec2" else (1, 2)
        xlow = torch.randn(B, 384, H // up[0], W // up[1], generator=g)
        skip = torch.randn(B, 384, H, W, generator=g)
        run = lambda: _dec(engine, n, xlow, skip, cond, up)
        cmax = 768
    v = torch.zeros(B * cmax * H * W * 9 // 4, dtype=torch.float32, device=DEV)
    try:
        _splits(engine, int(split[5:]))
        assert engine.lib.lass_set_wino4_vprep_buffer(engine.ctx, v.data_ptr(), v.numel()) == 0
        _vprep(engine, 0)
        y0 = run()
        torch.cuda.synchronize()
        assert not bool((v != 0).any()), "mode 0 wrote the V image"
        _vprep(engine, 2)
        y2 = run()
        torch.cuda.synchronize()
        written = int((v != 0).sum())
    finally:
        engine.lib.lass_set_wino4_vprep_buffer(engine.ctx, None, 0)
        _splits(engine, 0)
        _vprep(engine, 1)
    print(case, "V floats written", written, "of", v.numel())
    # the last image in the buffer is conv2's (384 channels, 36 values per 16 pixels); random data leaves hardly an exact zero
    assert written > 0.9 * B * 384 * H * W * 9 // 4, (case, written)
    assert bool(torch.isfinite(y2).all()) and _relerr(y2, y0) < W4_BAR


def test_a_clip_does_not_depend_on_its_batch(engine):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 256, 32, 32, generator=g)
    x6 = torch.randn(3, 384, 32, 16, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(3))
    try:
        _vprep(engine, 2)
        y3, p3 = _enc(engine, 5, x, cond, (2, 2))
        y1, p1 = _enc(engine, 5, x[1:2].contiguous(), cond[1:2].contiguous(), (2, 2))
        z3, q3 = _enc(engine, 6, x6, cond, (1, 2))
        z1, q1 = _enc(engine, 6, x6[1:2].contiguous(), cond[1:2].contiguous(), (1, 2))
    finally:
        _vprep(engine, 1)
    assert torch.equal(y3[1:2], y1) and torch.equal(p3[1:2], p1)
    assert torch.equal(z3[1:2], z1) and torch.equal(q3[1:2], q1)


@pytest.mark.parametrize("B", [16, 2])   # 16: two half-batch branches of the replayed graph; 2: one stream
def test_separate_is_bit_identical_from_run_to_run(engine, B):
    L = 160000
    _, mix = synthetic.make_mixtures(B, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    out = torch.empty_like(mix)
    runs = []
    for _ in range(5):   # the third call with the same pointers captures the graph; later ones replay it
        engine.separate(mix, cond, out=out)
        torch.cuda.synchronize()
        runs.append(out.cpu().clone())
    assert bool(torch.isfinite(runs[0]).all())
    for r in runs[1:]:
        assert torch.equal(r, runs[0])


def test_separate_shipped_routing_vs_off(engine):
    """the suite's bar of the f32 10 s waveform against the oracle's, 3e-6 RMS, held here as a RELATIVE RMS (the waveform's own
    RMS is below 1, so that is the tighter reading) and as an absolute one"""
    B, L = 2, 160000
    _, mix = synthetic.make_mixtures(B, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    try:
        a = engine.separate(mix, cond).cpu()
        _vprep(engine, 0)
        b = engine.separate(mix, cond).cpu()
    finally:
        _vprep(engine, 1)
    err, rel = float((a - b).pow(2).mean().sqrt()), _relerr(a, b)
    print("shipped routing vs mode 0: waveform RMS difference", err, "relative", rel, "bitwise equal", torch.equal(a, b))
    assert bool(torch.isfinite(a).all()) and float(b.pow(2).mean().sqrt()) > 1e-3   # a real waveform to be relative to
    assert rel < WAVE_BAR, rel
    assert err < WAVE_BAR, err


def test_workspace_grows_with_the_route_and_overlap_is_refused(engine):
    B, L = 2, 160000
    try:
        _vprep(engine, 0)
        off = engine.workspace_bytes(B, L)
        _vprep(engine, 1)
        on = engine.workspace_bytes(B, L)
        _vprep(engine, 2)
        every = engine.workspace_bytes(B, L)
        print("workspace bytes B=2: mode 0", off, "mode 1", on, "mode 2", every)
        assert on >= off and every >= on
        # a stage call whose V image overlaps the block's input: the state error, and nothing launched
        cin, cout, H, W = 384, 384, 32, 16
        n_x, n_v = B * cin * H * W, B * cin * H * W * 9 // 4
        buf = torch.zeros(n_v, dtype=torch.float32, device=DEV)
        x = buf[:n_x].view(B, cin, H, W)
        shift = engine.film(torch.from_numpy(synthetic.make_condition(B)).to(DEV))
        y = torch.full((B, cout, H, W), 7.0, dtype=torch.float32, device=DEV)
        pool = torch.full((B, cout, H, W // 2), 7.0, dtype=torch.float32, device=DEV)
        scratch = torch.full_like(y, 7.0)
        args = (engine.ctx, b"base.encoder_block6", x.data_ptr(), B, H, W, shift.data_ptr(), y.data_ptr(), pool.data_ptr(),
                scratch.data_ptr(), None)
        assert engine.lib.lass_set_wino4_vprep_buffer(engine.ctx, buf.data_ptr(), n_v) == 0
        rc = engine.lib.lass_encoder_block(*args)
        torch.cuda.synchronize()
        assert rc == -3, rc   # LASS_ERR_STATE
        assert b"overlap" in engine.lib.lass_last_error(engine.ctx)
        assert bool((y == 7.0).all()) and bool((scratch == 7.0).all()) and bool((pool == 7.0).all()) and bool((buf == 0).all())
        # ... a buffer that is too small likewise; a separate one of the right size runs
        small = torch.zeros(1024, dtype=torch.float32, device=DEV)
        assert engine.lib.lass_set_wino4_vprep_buffer(engine.ctx, small.data_ptr(), small.numel()) == 0
        assert engine.lib.lass_encoder_block(*args) == -3
        own = torch.zeros(n_v, dtype=torch.float32, device=DEV)
        assert engine.lib.lass_set_wino4_vprep_buffer(engine.ctx, own.data_ptr(), n_v) == 0
        assert engine.lib.lass_encoder_block(*args) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()) and not bool((y == 7.0).all()) and bool((own != 0).any())
    finally:
        engine.lib.lass_set_wino4_vprep_buffer(engine.ctx, None, 0)
        _vprep(engine, 1)
