"""CLAP text encoder on the MI355X (lass_text_*, text.hip): parity with transformers' RobertaModel + the CLAP head
(tests/golden/clap_text_g5.npz, tools/gen_clap_golden.py), exactness of packing (padding and batch invariance, bitwise),
checkpoint loading, and the evaluator end to end with the encoder as query encoder."""
import os

import numpy as np
import pytest
import torch

from lass_amd import _lib, synthetic
from lass_amd.clap_text import ClapTextEncoder

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def g5(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "clap_text_g5.npz")))


def _text_sd(g5, layers):
    seed = int(g5["seeds"][list(g5["layers"]).index(layers)])
    return synthetic.make_clap_text_state_dict(seed, layers)


def _encoder(sd, layers, **kw):
    enc = ClapTextEncoder(layers=layers, **kw)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return enc.to(DEV)


@pytest.fixture(scope="module")
def enc2(g5):
    return _encoder(_text_sd(g5, 2), 2)


@pytest.mark.parametrize("layers", [12, 2])
def test_parity_with_transformers(g5, layers, enc2):
    enc = enc2 if layers == 2 else _encoder(_text_sd(g5, 12), 12)
    emb, pool = enc.encode_ids(g5["input_ids"], g5["attention_mask"], return_pooler=True)
    emb, pool = emb.cpu().double().numpy(), pool.cpu().double().numpy()
    ref_e, ref_p = g5[f"embed_l{layers}"].astype(np.float64), g5[f"pooler_l{layers}"].astype(np.float64)
    assert np.abs(emb - ref_e).max() <= 2e-5
    cos = (emb * ref_e).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref_e, axis=1)
    assert cos.min() >= 1 - 1e-6
    assert np.abs(pool - ref_p).max() <= 5e-5
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-5


def test_padding_invariance_bitwise(g5, enc2):
    ids, mask, lengths = g5["input_ids"], g5["attention_mask"], g5["lengths"]
    rows = [i for i, L in enumerate(lengths) if L <= 77]
    full = enc2.encode_ids(ids[rows], mask[rows]).cpu()
    p77 = enc2.encode_ids(ids[rows, :77], mask[rows, :77]).cpu()
    assert torch.equal(full, p77)
    for j, i in enumerate(rows):
        own = enc2.encode_ids(ids[i:i + 1, :lengths[i]], mask[i:i + 1, :lengths[i]]).cpu()
        assert torch.equal(own[0], full[j]), i


def test_batch_invariance_bitwise(g5, enc2):
    ids, mask = g5["input_ids"], g5["attention_mask"]
    order = np.random.Generator(np.random.PCG64(5)).permutation(np.arange(16) % len(ids))
    batch = enc2.encode_ids(ids[order], mask[order]).cpu()
    for i in range(len(ids)):
        alone = enc2.encode_ids(ids[i:i + 1], mask[i:i + 1]).cpu()
        for j in np.nonzero(order == i)[0]:
            assert torch.equal(alone[0], batch[j]), (i, j)


def _checkpoint(path, ss_sd, text_sd):
    sd = {"ss_model." + k: torch.from_numpy(np.asarray(v)) for k, v in ss_sd.items()}
    sd.update({"query_encoder." + k: torch.from_numpy(v) for k, v in text_sd.items()})
    sd["query_encoder.model.audio_projection.0.weight"] = torch.zeros(512, 768)
    sd["query_encoder.model.logit_scale_a"] = torch.zeros(())
    sd["query_encoder.model.text_branch.embeddings.position_ids"] = torch.arange(514)[None]
    torch.save({"state_dict": sd, "epoch": 1}, path)
    return path


def test_from_checkpoint_reproduces_fixture(tmp_path, g5):
    path = _checkpoint(str(tmp_path / "a.ckpt"), {}, _text_sd(g5, 2))
    enc = ClapTextEncoder.from_checkpoint(path).to(DEV)
    emb = enc.encode_ids(g5["input_ids"], g5["attention_mask"]).cpu().numpy()
    assert np.abs(emb - g5["embed_l2"]).max() <= 2e-5


def test_eval_end_to_end_with_clap_query_encoder(tmp_path, g5, synthetic_sd):
    """eval(evaluator, ckpt, query_encoder=load_query_encoder(ckpt, tokenizer=...)) equals the oracle evaluator fed the
    fixture embeddings; the default eval(evaluator, ckpt) on the same file is the PrecomputedQueryEncoder result."""
    from lass_amd import evaluator as lev
    from lass_amd.audiosep import PrecomputedQueryEncoder
    from lass_amd.utils import load_query_encoder
    from oracle import evaluator as oev
    from oracle import resunet as orr
    n, L = 8, 32000
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=n, length=L)
    ckpt = _checkpoint(str(tmp_path / "audiosep.ckpt"), synthetic_sd, _text_sd(g5, 2))
    row_of = {f"synthetic tone cluster {i}": i for i in range(4)}   # caption -> fixture id row

    def tokenizer(text, **kw):
        assert kw == {"padding": "max_length", "truncation": True, "max_length": 512, "return_tensors": "pt"}
        r = [row_of[t] for t in text]
        return {"input_ids": torch.from_numpy(g5["input_ids"][r]), "attention_mask": torch.from_numpy(g5["attention_mask"][r])}

    audio_dir = os.path.join(str(tmp_path), "lass_validation")
    clips = [synthetic.make_clip(i, L) for i in range(n)]
    oracle_sd = orr.to_torch(synthetic_sd)
    ev = lev.DCASEEvaluator(sampling_rate=16000, eval_indexes=csv_path, audio_dir=audio_dir, batch_size=5)
    sdr, sdri, sisdr = lev.eval(ev, ckpt, device="cuda", query_encoder=load_query_encoder(ckpt, tokenizer=tokenizer))
    conds = g5["embed_l2"][[i % 4 for i in range(n)]]
    (o_sisdr, o_sdri, o_sdr), rows = oev.evaluate(oracle_sd, clips, conds)
    np.testing.assert_allclose(ev.last_rows, rows, atol=0.01)
    assert abs(sdr - o_sdr) < 0.01 and abs(sdri - o_sdri) < 0.01 and abs(sisdr - o_sisdr) < 0.01
    # the default query encoder is unchanged by a checkpoint that carries the text tower
    ev2 = lev.DCASEEvaluator(sampling_rate=16000, eval_indexes=csv_path, audio_dir=audio_dir, batch_size=5)
    d_sdr, d_sdri, d_sisdr = lev.eval(ev2, ckpt, device="cuda")
    conds = PrecomputedQueryEncoder().get_query_embed("text", [f"synthetic tone cluster {i % 4}" for i in range(n)]).numpy()
    (p_sisdr, p_sdri, p_sdr), prow = oev.evaluate(oracle_sd, clips, conds)
    np.testing.assert_allclose(ev2.last_rows, prow, atol=0.01)
    assert abs(d_sdr - p_sdr) < 0.01 and abs(d_sdri - p_sdri) < 0.01 and abs(d_sisdr - p_sisdr) < 0.01


def test_errors(g5, enc2):
    with pytest.raises(NotImplementedError):
        enc2.get_query_embed("audio", audio=torch.zeros(1, 16000, device=DEV))
    cpu = ClapTextEncoder(layers=2)
    with pytest.raises(_lib.LassError):
        cpu.encode_ids(g5["input_ids"][:2], g5["attention_mask"][:2])
    with pytest.raises(ValueError):
        enc2.encode_ids(g5["input_ids"][:2] * 0 + 50265, g5["attention_mask"][:2])


def test_weights_reloaded_after_change(g5, enc2):
    """The device copy follows the module: loading other weights changes the result, loading the fixture's back restores
    it bit for bit."""
    ids, mask = g5["input_ids"][:3], g5["attention_mask"][:3]
    a = enc2.encode_ids(ids, mask).cpu()
    sd = {k: v.clone() for k, v in enc2.state_dict().items()}
    other = synthetic.make_clap_text_state_dict(1, 2)
    enc2.load_state_dict({k: torch.from_numpy(v) for k, v in other.items()})
    b = enc2.encode_ids(ids, mask).cpu()
    enc2.load_state_dict(sd)
    c = enc2.encode_ids(ids, mask).cpu()
    assert not torch.equal(a, b) and torch.equal(a, c)
