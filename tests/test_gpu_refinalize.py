"""One context finalized again and again in another compute mode: lass_finalize frees the derived buffers of the previous mode and
starts from value-initialised image slots (weight_plan.h), so nothing of the earlier mode may be read afterwards - not a stale
image, not a graph captured on the earlier buffers.  Each round is held bit for bit to a fresh context finalized once in that mode:
same kernels, same weights, and the suite pins run-to-run and batch invariance bit for bit."""
import gc

import pytest
import torch

from lass_amd import synthetic
from lass_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ORDER = ("f32", "bf16", "bf16x3", "f32")
L = 1024   # the shortest single clip of test_gpu_parity.py (test_silence_and_edge_lengths)


def _engine(sd):
    e = Engine(DEV)
    for k, v in sd.items():
        e.set_param(k, v)
    return e


def _stage_calls(e, cond, x6, x2):
    """(b) encoder_block6's block on a 32 x 16 image: split-K F(4x4,3x3) and gemm images; (c) decoder_block2's on 16 x 32: the
    shortcut GEMM with its split weights"""
    shift = e.film(cond)
    return (e.convblock("base.encoder_block6.conv_block1", x6, shift, 384).cpu(),
            e.convblock("base.decoder_block2.conv_block2", x2, shift, 384).cpu())


def test_refinalize_in_another_mode_matches_a_fresh_context(synthetic_sd):
    g = torch.Generator().manual_seed(7)
    mix = torch.from_numpy(synthetic.make_mixtures(1, L)[1]).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(1)).to(DEV)
    x6 = (torch.randn(1, 384, 32, 16, generator=g) * 0.5).to(DEV)
    x2 = (torch.randn(1, 768, 16, 32, generator=g) * 0.5).to(DEV)
    e = _engine(synthetic_sd)
    out = torch.empty_like(mix)
    seen = []
    for mode in ORDER:
        e.finalize(mode)
        on, captures, replays = e.graph_stats()
        # the same buffers three times: the third call captures, on the buffers of THIS finalize (gen moved: no replay of an earlier graph)
        got = [e.separate(mix, cond, out=out).cpu().clone() for _ in range(3)]
        if on:
            assert e.graph_stats() == (True, captures + 1, replays), mode
        assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), mode
        got_b, got_c = _stage_calls(e, cond, x6, x2)
        fresh = _engine(synthetic_sd)      # (the second context alive; gone before the next round)
        fresh.finalize(mode)
        want = fresh.separate(mix, cond).cpu()
        want_b, want_c = _stage_calls(fresh, cond, x6, x2)
        del fresh
        gc.collect()
        assert torch.isfinite(want).all() and float(want.abs().max()) > 0
        assert torch.equal(got[0], want), (mode, float((got[0] - want).abs().max()))
        assert torch.equal(got_b, want_b), (mode, float((got_b - want_b).abs().max()))
        assert torch.equal(got_c, want_c), (mode, float((got_c - want_c).abs().max()))
        seen.append((mode, want, want_b, want_c))
    # the modes do differ (a stale image of another mode would show), and the second f32 round is the first one again
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][2], seen[2][2])
    assert all(torch.equal(a, b) for a, b in zip(seen[0][1:], seen[3][1:]))
