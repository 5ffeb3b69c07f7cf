"""pw_gemm.hip - the f32 pointwise GEMMs: the 1x1 shortcut of the >= 128-cout ConvBlockRes layers (written into the block's
output slot, then read back and overwritten in place by conv2 = wino4.hip CONV2_IDENT) and the transposed convs, held to the
oracle (oracle/resunet.py) at the bars of test_gpu_stages.py::test_wino4_convblock_vs_oracle_and_wino / the upconv tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lass_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _relerr(got, ref):
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30))


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


def _check_block(got, ref):
    err = _relerr(got, ref)
    assert got.shape == ref.shape
    assert err < 2e-5, err
    assert float((got - ref).abs().max()) < 3e-4 * max(1.0, float(ref.abs().max()))


ROUTED_DEC = [  # (decoder, concat channels, cout, H, W): every routed decoder ConvBlockRes; 8 x 64 and 16 x 32 Winograd blocks
    ("decoder_block2", 768, 384, 16, 32),
    ("decoder_block3", 512, 256, 8, 128),
    ("decoder_block4", 256, 128, 16, 64),
    ("decoder_block3", 512, 256, 16, 256),   # the multi-STFT model's width (1024 bins, two levels down)
]


@pytest.mark.parametrize("name,cin,cout,H,W", ROUTED_DEC)
def test_routed_decoder_convblock_vs_oracle(engine, oracle_sd, name, cin, cout, H, W):
    from oracle import resunet as orr
    B = 2
    g = torch.Generator().manual_seed(H * 1000 + W + cin)
    x = torch.randn(B, cin, H, W, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    prefix, stem = f"base.{name}.conv_block2", f"{name}->conv_block2"
    y = engine.convblock(prefix, x.to(DEV), engine.film(cond.to(DEV)), cout).cpu()
    ref = orr.conv_block_res(oracle_sd, prefix, x, orr.film(oracle_sd, cond, stem + "->beta1"), orr.film(oracle_sd, cond, stem + "->beta2"))
    _check_block(y, ref)


@pytest.mark.parametrize("name,cin,cout,H,W", [("encoder_block3", 64, 128, 32, 128), ("encoder_block4", 128, 256, 16, 64),
                                               ("encoder_block5", 256, 384, 16, 32)])
def test_routed_encoder_block_with_fused_pool_vs_oracle(engine, oracle_sd, name, cin, cout, H, W):
    """The fused 2x2 avg-pool sums conv2's output WITH the residual it read from the output slot."""
    from oracle import resunet as orr
    B = 2
    g = torch.Generator().manual_seed(H * 1000 + W + cin + 7)
    x = torch.randn(B, cin, H, W, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    y, pool = engine.encoder_block("base." + name, x.to(DEV), engine.film(cond.to(DEV)), cout, (2, 2))
    ref = orr.conv_block_res(oracle_sd, f"base.{name}.conv_block1", x, orr.film(oracle_sd, cond, f"{name}->conv_block1->beta1"),
                             orr.film(oracle_sd, cond, f"{name}->conv_block1->beta2"))
    _check_block(y.cpu(), ref)
    _check_block(pool.cpu(), F.avg_pool2d(ref, (2, 2)))


UPS = [  # (decoder, cin, cout, (uh, uw), h, w): every decoder's transposed conv; h * w not a multiple of the 128-pixel tile
    ("decoder_block1", 384, 384, (1, 2), 4, 8), ("decoder_block2", 384, 384, (2, 2), 5, 16),
    ("decoder_block3", 384, 256, (2, 2), 8, 32), ("decoder_block4", 256, 128, (2, 2), 12, 64),
    ("decoder_block5", 128, 64, (2, 2), 16, 128), ("decoder_block6", 64, 32, (2, 2), 9, 256),
]


@pytest.mark.parametrize("name,cin,cout,up,h,w", UPS)
def test_every_transposed_conv_vs_oracle(engine, oracle_sd, name, cin, cout, up, h, w):
    from oracle import resunet as orr
    B = 3
    g = torch.Generator().manual_seed(h * 100 + w + 1)
    x = torch.randn(B, cin, h, w, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    y = engine.upconv("base." + name, x.to(DEV), engine.film(cond.to(DEV)), cout, up).cpu()
    hh = F.leaky_relu(orr._bn(oracle_sd, f"base.{name}.bn1", x) + orr.film(oracle_sd, cond, f"{name}->beta1"), 0.01)
    ref = F.conv_transpose2d(hh, oracle_sd[f"base.{name}.conv1.weight"], stride=up)
    assert y.shape == ref.shape
    assert _relerr(y, ref) < 2e-6, _relerr(y, ref)
