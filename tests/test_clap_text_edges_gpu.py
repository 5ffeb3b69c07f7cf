"""CLAP text tower on the MI355X (lass_text_*, text.hip) where tests/test_clap_text_gpu.py cannot see a mistake: peaked
attention, every tile edge, small embedding tables, and the C-ABI's refusals.

Fixture: tests/golden/clap_text_g7.npz (tools/gen_clap_text_edges_golden.py) - transformers' RobertaModel and the CLAP head in
FLOAT64 on synthetic.make_clap_text_state_dict(regime="peaked") weights (mean largest attention probability over 512 keys about
0.9, tanh saturated, GELU in its curved range), captions whose real-token counts are 1, 2, 3 and every count on and beside 16
(k_attn's online-softmax step), 64 (its LDS key block and query block, k_gemm's row tile), 128 and 512, masks with a hole across
the 16-key step and across the 64-key block, the pad id inside a mask, the vocabulary's last row; and one weight set with a
300 x 768 vocabulary and 40 positions.

Bars.  Per set and tensor, 4 x the largest per-caption deviation of the reference's own float32 run from its float64 run, as
recorded in the fixture (4 x: the device sums its rows in k order on the f32 MFMA, not in ATen's order - the factor
tests/test_clap_audio_gpu.py uses for the same k_gemm); the cosine likewise.  tests/test_clap_text_cpu.py holds the fixture to
the condition that makes these bars mean something: each is at most a quarter of what a 1 % error in the softmax scale moves
the float64 result of any caption of two or more tokens.  Every figure is printed before it is asserted.

Measured on an MI355X (largest error over the captions of the set / bar):

    set                         embedding            pooler               1 - cosine
    2 layers                    2.85e-7 / 1.54e-6    1.18e-5 / 4.78e-5    1.94e-12 / 1.56e-11
    12 layers                   4.69e-6 / 1.80e-5    1.62e-4 / 9.38e-4    5.02e-10 / 1.93e-9
    1 layer, 300 x 40 tables    1.20e-7 / 5.76e-7    4.27e-6 / 2.47e-5    3.24e-13 / 2.33e-12

These are the figures of k_gemm summing k in chunks of 64 (tower_parts.h).  With one accumulator chain over all of K, as the
kernel was when this module was written, they were 6.95e-7, 3.15e-5, 1.29e-11 (2 layers) and 1.25e-5, 6.81e-4, 3.96e-9
(12 layers): the 12-layer cosine missed its bar, by order of summation alone - the one-token caption, which has no softmax
to get wrong, lay 3.5 x as far from float64 as ATen's float32.  With `dot * 0.125f` in k_attn changed to `0.12375f` every
caption of two or more tokens misses its embedding bar: by 54 x or more at 2 layers, 9 x or more at 12 layers, 130 x or more
on the small tables.
"""
import ctypes
import os
from ctypes import byref, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from lass_amd import _lib, synthetic
from lass_amd.clap_text import ClapTextEncoder

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR_FACTOR = 4


@pytest.fixture(scope="module")
def g7(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "clap_text_g7.npz")))


def _encoder(g7, si):
    layers, vocab, npos = int(g7["layers"][si]), int(g7["vocab"][si]), int(g7["max_positions"][si])
    sd = synthetic.make_clap_text_state_dict(int(g7["seeds"][si]), layers, regime="peaked", vocab=vocab, max_positions=npos)
    enc = ClapTextEncoder(layers=layers, vocab_size=vocab, max_positions=npos)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return enc.to(DEV)


@pytest.fixture(scope="module")
def enc2(g7):
    assert int(g7["layers"][0]) == 2
    return _encoder(g7, 0)


def _captions(g7, si):
    s = "_small" if g7["small_tables"][si] else ""
    return g7["input_ids" + s], g7["attention_mask" + s], g7["counts" + s]


def _hold(name, got, ref, bar, counts):
    """got, ref (captions, ...) float64: every caption's max abs error within the set's bar."""
    err = np.abs(got - ref).reshape(len(ref), -1).max(1)
    print(f"{name}: bar {bar:.3e}, largest error {err.max():.3e}; per caption (real tokens: error) "
          + ", ".join(f"{c}: {e:.2e}" for c, e in zip(counts, err)))
    assert (err <= bar).all(), (name, bar, [(int(c), float(e)) for c, e in zip(counts, err) if e > bar])


def _parity(g7, si, enc):
    ids, mask, counts = _captions(g7, si)
    emb, pool = enc.encode_ids(ids, mask, return_pooler=True)
    emb, pool = emb.cpu().double().numpy(), pool.cpu().double().numpy()
    ref_e, ref_p = g7[f"embed_s{si}"], g7[f"pooler_s{si}"]
    assert ref_e.dtype == ref_p.dtype == np.float64
    _hold(f"set {si} embedding", emb, ref_e, BAR_FACTOR * g7[f"embed_dev_s{si}"].max(), counts)
    _hold(f"set {si} pooler", pool, ref_p, BAR_FACTOR * g7[f"pooler_dev_s{si}"].max(), counts)
    cos = (emb * ref_e).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref_e, axis=1)
    cos_bar = BAR_FACTOR * g7[f"embed_cosdev_s{si}"].max()
    print(f"set {si} 1 - cosine: bar {cos_bar:.3e}, largest {(1 - cos).max():.3e}; per caption {1 - cos}")
    assert (1 - cos <= cos_bar).all()
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-5


@pytest.mark.parametrize("si", [0, 1], ids=["2-layers", "12-layers"])
def test_parity_at_peaked_attention(g7, si, enc2):
    _parity(g7, si, enc2 if si == 0 else _encoder(g7, si))


def _both(enc, ids, mask):
    """(N, 512 + 768): embedding and pooler of every caption, on the host."""
    emb, pool = enc.encode_ids(ids, mask, return_pooler=True)
    return torch.cat([emb, pool], dim=1).cpu()


def _filled_to(counts, plain, i, target):
    """Rows of a batch whose real tokens number exactly `target`: caption i last, in front of it the largest plain captions
    that still fit (a one-token caption exists, so the count is always met)."""
    rows, left = [], target - int(counts[i])
    for j in sorted(plain, key=lambda j: -counts[j]):
        while counts[j] <= left:
            rows.append(j)
            left -= int(counts[j])
    assert left == 0
    return rows + [i]


def test_bitwise_invariance_at_the_edges(g7, enc2):
    """Every caption alone, trimmed to its own length, against itself in the full batch at S = 512, in the reversed batch (the
    longest caption last: k_attn's grid is sized by it), and in batches of exactly 64 and 65 packed rows (one k_gemm row tile,
    and one row into the second)."""
    ids, mask, counts = _captions(g7, 0)
    N, S = ids.shape
    spans = [S - int(np.argmax(mask[i, ::-1])) for i in range(N)]
    alone = [_both(enc2, ids[i:i + 1, :spans[i]], mask[i:i + 1, :spans[i]])[0] for i in range(N)]
    full = _both(enc2, ids, mask)
    rev = _both(enc2, ids[::-1].copy(), mask[::-1].copy())
    for i in range(N):
        assert torch.equal(alone[i], full[i]), ("full batch", i, int(counts[i]))
        assert torch.equal(alone[i], rev[N - 1 - i]), ("reversed batch", i, int(counts[i]))
    one = int(np.nonzero(counts == 1)[0][0])
    assert spans[one] == 1 and torch.equal(alone[one], full[one])  # N = 1, M = 1: a launch of one row
    plain = [i for i in range(N) if counts[i] == spans[i] and (ids[i, :spans[i]] != 1).all()]
    for target in (64, 65):
        seen = 0
        for i in range(N):
            if counts[i] > target:
                continue
            rows = _filled_to(counts, plain, i, target)
            width = max(spans[r] for r in rows)
            assert int(mask[rows, :width].sum()) == target
            batch = _both(enc2, ids[rows, :width], mask[rows, :width])
            for j, r in enumerate(rows):
                assert torch.equal(batch[j], alone[r]), (target, rows, j)
            seen += 1
        assert seen >= 12


def _raw(enc, N, S):
    """(lib, handle, workspace bytes, workspace, out, stream) for raw lass_text_encode calls of shape (N, S)."""
    ctx = enc._context()
    n = c_size_t()
    assert ctx.lib.lass_text_workspace_bytes(ctx.ctx, N, S, byref(n)) == 0 and n.value > 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    out = torch.empty(N, 512, device=DEV)
    return ctx.lib, ctx.ctx, n.value, ws, out, c_void_p(torch.cuda.current_stream().cuda_stream)


def test_small_tables(g7):
    """vocab and npos are run-time arguments of k_embed_ln: a 300-row vocabulary and 40 positions, S = 38 the longest they admit."""
    si = int(np.nonzero(g7["small_tables"])[0][0])
    enc = _encoder(g7, si)
    assert (enc.vocab_size, enc.max_positions) == (300, 40)
    _parity(g7, si, enc)
    ids, mask, _ = _captions(g7, si)
    assert ids.shape[1] == 38
    ids39 = np.concatenate([ids[:1], np.full((1, 1), 1, dtype=np.int64)], axis=1)
    mask39 = np.concatenate([mask[:1], np.zeros((1, 1), dtype=np.int64)], axis=1)
    with pytest.raises(ValueError, match="exceeds 38"):
        enc.encode_ids(ids39, mask39)
    lib, h, nbytes, ws, out, st = _raw(enc, 1, 39)
    ids_dev, mask_host = torch.from_numpy(ids39).to(DEV), torch.from_numpy(mask39)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    assert lib.lass_text_encode(h, P(ids_dev), P(mask_host), 1, 39, P(out), None, P(ws), nbytes, st) == -1
    assert "position table" in lib.lass_text_last_error(h).decode()
    with pytest.raises(ValueError, match="out of range"):
        enc.encode_ids(ids[:1] * 0 + 300, mask[:1])


def test_text_c_abi_error_paths(g7, enc2):
    """Every refusal carries its code and message, nothing is launched, and the context computes the same bits afterwards."""
    ids, mask, _ = _captions(g7, 0)
    rows, S = [3, 5, 0], 17                                   # 15, 17 and 1 real tokens
    ids, mask = ids[rows, :S].copy(), mask[rows, :S].copy()
    N = len(rows)
    before = _both(enc2, ids, mask)
    lib, h, nbytes, ws, out, st = _raw(enc2, N, S)
    ids_dev, mask_host = torch.from_numpy(ids).to(DEV), torch.from_numpy(mask)
    headless = mask_host.clone()
    headless[1, 0] = 0
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    err = lambda: lib.lass_text_last_error(h).decode()  # noqa: E731
    bad = [
        ("workspace too small", (h, P(ids_dev), P(mask_host), N, S, P(out), None, P(ws), nbytes - 1, st)),
        ("non-NULL", (h, None, P(mask_host), N, S, P(out), None, P(ws), nbytes, st)),
        ("non-NULL", (h, P(ids_dev), None, N, S, P(out), None, P(ws), nbytes, st)),
        ("non-NULL", (h, P(ids_dev), P(mask_host), N, S, None, None, P(ws), nbytes, st)),
        ("non-NULL", (h, P(ids_dev), P(mask_host), N, S, P(out), None, None, nbytes, st)),
        ("N >= 1", (h, P(ids_dev), P(mask_host), 0, S, P(out), None, P(ws), nbytes, st)),
        ("S <= 512", (h, P(ids_dev), P(mask_host), N, 0, P(out), None, P(ws), nbytes, st)),
        ("S <= 512", (h, P(ids_dev), P(mask_host), N, 513, P(out), None, P(ws), nbytes, st)),
        ("attention_mask[:, 0]", (h, P(ids_dev), P(headless), N, S, P(out), None, P(ws), nbytes, st)),
    ]
    for msg, args in bad:
        assert lib.lass_text_encode(*args) == -1, msg
        assert msg in err(), (msg, err())
    n = c_size_t()
    assert lib.lass_text_workspace_bytes(h, N, 513, byref(n)) == -1
    assert "lass_text_workspace_bytes" in err() and "S <= 512" in err(), err()
    bias = enc2.model.text_branch.pooler.dense.bias
    shape = lambda *d: (ctypes.c_int64 * len(d))(*d)  # noqa: E731
    assert lib.lass_text_set_param(h, b"text_branch.head.weight", P(bias), shape(768), 1) == -1
    assert "unknown" in err(), err()
    assert lib.lass_text_set_param(h, b"text_branch.pooler.dense.bias", P(bias), shape(767), 1) == -1
    assert "expected shape (768,)" in err(), err()
    good = (h, P(ids_dev), P(mask_host), N, S, P(out), None, P(ws), nbytes, st)
    assert lib.lass_text_encode(*good) == 0                   # none of the refusals above unset the finalized state
    # a valid upload after finalize: the fused QKV images may be stale, so encode refuses until finalize is called again
    torch.cuda.synchronize()
    assert lib.lass_text_set_param(h, b"text_branch.pooler.dense.bias", P(bias), shape(768), 1) == 0
    assert lib.lass_text_layers(h) == 0
    assert lib.lass_text_encode(*good) == -3
    assert "lass_text_finalize" in err(), err()
    assert lib.lass_text_finalize(h) == 0 and lib.lass_text_layers(h) == 2
    assert lib.lass_text_encode(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), before[:, :512])
    with pytest.raises(_lib.LassError):
        ClapTextEncoder(layers=2).encode_ids(ids, mask)      # a module on the CPU
    assert torch.equal(_both(enc2, ids, mask), before)
