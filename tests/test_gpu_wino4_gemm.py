"""wino4_gemm.hip - the f32 F(4x4,3x3) convs with 384 output channels as scatter, 36 batched split-bf16 GEMMs and gather
(lass_set_wino4_gemm, on by default) against the prep + conv (+ combine) launches of wino4.hip (switch off), both from one engine
through the stage calls, both measured against a torch-CPU float64 ConvBlockRes of the same f32 inputs and weights.

The bar is test_gpu_pw_gemm_split.py's: the route's relative RMS error and its largest deviation may be at most twice those of the
f32 route on the same case, and both routes stay under the F(4x4,3x3) block bar of 2e-5.  Shapes: encoder_block5 at 32 x 32 is two
16 x 32 blocks per plane, so B = 1, 2, 3 give the GEMMs P = 64, 128, 192 columns - a partial 128-column tile, a tile that spans two
clips, and both; decoder_block2 has K = 768 with the shortcut GEMM in front and the residual in place; the 32 x 16 level has the
narrow blocks and encoder_block6's 1 x 2 pool (P = 32, 64); 16 x 64 is the 8 x 64 block geometry."""
import pytest
import torch
import torch.nn.functional as F

from lass_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W4_BAR = 2e-5    # relative RMS of a F(4x4,3x3) block against the oracle (test_gpu_wino4_splitk.py)
WAVE_BAR = 3e-6  # RMS of the f32 10 s waveform (test_gpu_wino4_vprep.py)

# name -> (kind, block number, cin, H, W, pool or None, largest B)
CASES = {
    "enc5_32x32": ("enc", 5, 256, 32, 32, (2, 2), 3),
    "dec2_32x32": ("dec", 2, 768, 32, 32, None, 2),
    "enc6_32x16": ("enc", 6, 384, 32, 16, (1, 2), 2),
    "dec1_32x16": ("dec", 1, 768, 32, 16, None, 2),
    "enc5_16x64": ("enc", 5, 256, 16, 64, (2, 2), 2),
    "dec2_16x64": ("dec", 2, 768, 16, 64, None, 2),
}
RUNS = [("enc5_32x32", 1), ("enc5_32x32", 2), ("enc5_32x32", 3), ("dec2_32x32", 2), ("enc6_32x16", 1), ("enc6_32x16", 2),
        ("dec1_32x16", 2), ("enc5_16x64", 2), ("dec2_16x64", 2)]


@pytest.fixture(scope="module")
def engine(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    return e


@pytest.fixture(scope="module")
def sd64(synthetic_sd):
    from oracle import resunet as orr
    return orr.to_torch(synthetic_sd, torch.float64)


@pytest.fixture(scope="module")
def case_data(sd64):
    """name -> (x, cond, ref, ref_pool) at the case's largest B, computed once: a clip's reference does not depend on its batch, so
    a smaller B takes the leading clips"""
    from oracle import resunet as orr
    cache = {}

    def get(name):
        if name not in cache:
            kind, n, cin, H, W, pool, B = CASES[name]
            g = torch.Generator().manual_seed(1800 + sum(map(ord, name)))
            x = torch.randn(B, cin, H, W, generator=g)
            cond = torch.from_numpy(synthetic.make_condition(B))
            block = f"encoder_block{n}->conv_block1" if kind == "enc" else f"decoder_block{n}->conv_block2"
            prefix = f"base.encoder_block{n}.conv_block1" if kind == "enc" else f"base.decoder_block{n}.conv_block2"
            c64 = cond.double()
            ref = orr.conv_block_res(sd64, prefix, x.double(), orr.film(sd64, c64, block + "->beta1"), orr.film(sd64, c64, block + "->beta2"))
            cache[name] = (x, cond, ref, F.avg_pool2d(ref, pool) if pool else None)
        return cache[name]

    return get


def _gemm(e, on):
    from lass_amd import _lib
    _lib.check(e.ctx, e.lib.lass_set_wino4_gemm(e.ctx, 1 if on else 0), "lass_set_wino4_gemm")


def _splits(e, n):
    from lass_amd import _lib
    _lib.check(e.ctx, e.lib.lass_set_wino4_splits(e.ctx, n), "lass_set_wino4_splits")


def _run(e, name, x, cond):
    """-> (y, pool or None) on the CPU"""
    kind, n, _cin, _H, _W, pool, _B = CASES[name]
    shift = e.film(cond.to(DEV))
    if kind == "enc":
        y, p = e.encoder_block(f"base.encoder_block{n}", x.to(DEV), shift, 384, pool)
        return y.cpu(), p.cpu()
    return e.convblock(f"base.decoder_block{n}.conv_block2", x.to(DEV), shift, 384).cpu(), None


def _errs(got, ref):
    d = got.double() - ref
    return float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max())


@pytest.mark.parametrize("name,B", RUNS)
def test_route_vs_float64_and_the_f32_route(engine, case_data, name, B):
    x, cond, ref, rpool = case_data(name)
    x, cond, ref = x[:B].contiguous(), cond[:B].contiguous(), ref[:B]
    try:
        _gemm(engine, True)
        on = _run(engine, name, x, cond)
        _splits(engine, 4)   # a forced split factor keeps the f32 kernels (4 is the narrow level's own factor: the launches of `off`)
        forced = _run(engine, name, x, cond)
        _splits(engine, 0)
        _gemm(engine, False)
        off = _run(engine, name, x, cond)
    finally:
        _splits(engine, 0)
        _gemm(engine, True)
    pairs = [("y", on[0], off[0], forced[0], ref)]
    if rpool is not None:
        pairs.append(("pool", on[1], off[1], forced[1], rpool[:B]))
    for what, a, b, f, r in pairs:
        (ra, ma), (rb, mb) = _errs(a, r), _errs(b, r)
        print(f"{name} B={B} {what}: gemm route rel RMS {ra:.3e} max dev {ma:.3e} | f32 route rel RMS {rb:.3e} max dev {mb:.3e} | "
              f"ratio {ra / rb:.3f} {ma / mb:.3f}")
        assert a.shape == r.shape and bool(torch.isfinite(a).all())
        assert not torch.equal(a, b), "the switch changed nothing: the route did not run"
        assert torch.equal(f, b), "a forced split factor must keep the f32 kernels"
        assert ra < W4_BAR and rb < W4_BAR, (ra, rb)
        assert ra <= 2 * rb, (ra, rb)
        assert ma <= 2 * mb, (ma, mb)


def test_a_clip_does_not_depend_on_its_batch(engine, case_data):
    for name in ("enc5_32x32", "enc6_32x16"):
        x, cond, _, _ = case_data(name)
        B = x.shape[0]
        m = 1 if B == 3 else B - 1   # the middle clip of B = 3; the last of B = 2 (second half of a tile that spans both clips)
        yb, pb = _run(engine, name, x, cond)
        y1, p1 = _run(engine, name, x[m:m + 1].contiguous(), cond[m:m + 1].contiguous())
        assert torch.equal(yb[m:m + 1], y1) and torch.equal(pb[m:m + 1], p1), name


def test_separate_replays_bit_identically_and_stays_at_the_f32_route(engine):
    B, L = 2, 160000
    _, mix = synthetic.make_mixtures(B, L)
    mix = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    out = torch.empty_like(mix)
    runs = []
    for _ in range(5):   # the third call with the same pointers captures the graph; later ones replay it
        engine.separate(mix, cond, out=out)
        torch.cuda.synchronize()
        runs.append(out.cpu().clone())
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    try:
        _gemm(engine, False)
        off = engine.separate(mix, cond).cpu()
    finally:
        _gemm(engine, True)
    a = runs[0]
    err = float((a - off).pow(2).mean().sqrt())
    rel = err / float(off.pow(2).mean().sqrt())
    print("gemm route vs f32 route: waveform RMS difference", err, "relative", rel)
    assert bool(torch.isfinite(a).all()) and float(off.pow(2).mean().sqrt()) > 1e-3
    assert not torch.equal(a, off)
    assert rel < WAVE_BAR and err < WAVE_BAR, (rel, err)
