"""CLAP text encoder, host side: parameter tree vs the checkpoint layout, checkpoint filtering, host-side validation,
the tokenizer call, and the no-CPU-fallback rule.  Needs no GPU."""
import json
import os

import numpy as np
import pytest
import torch

from lass_amd import _lib, clap_text, synthetic
from lass_amd.clap_text import ClapTextEncoder


def _roberta_base_keys():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.RobertaConfig(vocab_size=50265, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                                     intermediate_size=3072, max_position_embeddings=514, type_vocab_size=1,
                                     layer_norm_eps=1e-5, pad_token_id=1)
    with torch.device("meta"):
        m = transformers.RobertaModel(cfg)
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_state_dict_matches_spec(golden_dir):
    spec = json.load(open(os.path.join(golden_dir, "clap_text_state_dict_spec.json")))
    sd = ClapTextEncoder().state_dict()
    assert list(sd) == list(spec)
    assert {k: list(v.shape) for k, v in sd.items()} == spec
    assert all(v.dtype == torch.float32 for v in sd.values())


def test_state_dict_matches_transformers_roberta_base():
    ref = _roberta_base_keys()
    ours = {k: tuple(v.shape) for k, v in ClapTextEncoder().state_dict().items()}
    proj = {"model.text_projection.0.weight": (512, 768), "model.text_projection.0.bias": (512,),
            "model.text_projection.2.weight": (512, 512), "model.text_projection.2.bias": (512,)}
    assert ours == {"model.text_branch." + k: v for k, v in ref.items()} | proj


def _lightning_checkpoint(path, text_sd, drop=None):
    sd = {"query_encoder." + k: torch.from_numpy(v) for k, v in text_sd.items() if k != drop}
    sd["query_encoder.model.audio_branch.patch_embed.proj.weight"] = torch.zeros(96, 1, 4, 4)
    sd["query_encoder.model.audio_projection.0.weight"] = torch.zeros(512, 768)
    sd["query_encoder.model.audio_transform.sequential.0.weight"] = torch.zeros(512, 512)
    sd["query_encoder.model.text_transform.sequential.0.weight"] = torch.zeros(512, 512)
    sd["query_encoder.model.logit_scale_a"] = torch.zeros(())
    sd["query_encoder.model.logit_scale_t"] = torch.zeros(())
    sd["query_encoder.model.text_branch.embeddings.position_ids"] = torch.arange(514)[None]
    sd["query_encoder.model.text_branch.embeddings.token_type_ids"] = torch.zeros(1, 514, dtype=torch.int64)
    sd["ss_model.base.after_conv.weight"] = torch.zeros(3, 32, 1, 1)
    torch.save({"state_dict": sd, "epoch": 1, "pytorch-lightning_version": "2.1.0"}, path)
    return path


def test_from_lightning_checkpoint(tmp_path):
    text_sd = synthetic.make_clap_text_state_dict(7, layers=2)
    enc = ClapTextEncoder.from_checkpoint(_lightning_checkpoint(str(tmp_path / "a.ckpt"), text_sd))
    assert enc.layers == 2 and enc.encoder_type == "CLAP"
    got = enc.state_dict()
    assert set(got) == set(text_sd)
    for k, v in text_sd.items():
        assert torch.equal(got[k], torch.from_numpy(v)), k


def test_missing_text_key_is_named(tmp_path):
    text_sd = synthetic.make_clap_text_state_dict(7, layers=2)
    key = "model.text_branch.encoder.layer.1.output.LayerNorm.bias"
    path = _lightning_checkpoint(str(tmp_path / "b.ckpt"), text_sd, drop=key)
    with pytest.raises(KeyError, match=r"query_encoder\.model\.text_branch\.encoder\.layer\.1\.output\.LayerNorm\.bias"):
        ClapTextEncoder.from_checkpoint(path)


def test_synthetic_weights_are_seeded():
    a = synthetic.make_clap_text_state_dict(3, layers=1)
    b = synthetic.make_clap_text_state_dict(3, layers=1)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    g = a["model.text_branch.embeddings.LayerNorm.weight"]
    w = a["model.text_branch.encoder.layer.0.intermediate.dense.weight"]
    assert abs(g.mean() - 1) < 0.02 and abs(g.std() - 0.1) < 0.01 and abs(w.std() - 0.02) < 1e-3
    # regime "flat" is the default; "peaked" is the same draws with four kinds of matrix scaled, everything else untouched
    assert all(np.array_equal(a[k], v) for k, v in synthetic.make_clap_text_state_dict(3, layers=1, regime="flat").items())
    p = synthetic.make_clap_text_state_dict(3, layers=1, regime="peaked")
    layer = "model.text_branch.encoder.layer.0."
    scaled = {layer + "attention.self.query.weight": 8, layer + "attention.self.key.weight": 8,
              layer + "intermediate.dense.weight": 6, "model.text_branch.pooler.dense.weight": 6}
    assert list(p) == list(a)
    for k in a:
        assert p[k].dtype == np.float32 and np.array_equal(p[k], a[k] * np.float32(scaled.get(k, 1))), k
    assert p[layer + "attention.self.query.weight"][0, 0] == np.float32(-0.16578889)
    assert p[layer + "attention.self.key.weight"][5, 7] == np.float32(0.10597573)
    assert p[layer + "intermediate.dense.weight"][3071, 767] == np.float32(0.046068795)
    assert p["model.text_branch.pooler.dense.weight"][1, 2] == np.float32(-0.11622642)
    assert p[layer + "attention.self.value.weight"][0, 0] == np.float32(-0.027986238)
    small = synthetic.make_clap_text_state_dict(3, layers=1, regime="peaked", vocab=300, max_positions=40)
    assert small["model.text_branch.embeddings.word_embeddings.weight"].shape == (300, 768)
    assert small["model.text_branch.embeddings.position_embeddings.weight"].shape == (40, 768)
    with pytest.raises(ValueError):
        synthetic.make_clap_text_state_dict(3, layers=1, regime="sharp")


def _edges_tool():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_clap_text_edges_golden.py")
    spec = importlib.util.spec_from_file_location("gen_clap_text_edges_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def g7(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "clap_text_g7.npz")))


def test_g7_fixture_is_sharp(g7):
    """tests/golden/clap_text_g7.npz meets the conditions its generator enforces - restated here, not imported, so that a
    regenerated fixture that has gone soft (or a generator whose conditions were loosened) fails on any machine."""
    assert [int(x) for x in g7["layers"][:2]] == [2, 12] and g7["layers"][2] in (1, 2)
    assert [bool(x) for x in g7["small_tables"]] == [False, False, True]
    assert (int(g7["vocab"][2]), int(g7["max_positions"][2])) == (300, 40)
    assert [(int(v), int(p)) for v, p in zip(g7["vocab"][:2], g7["max_positions"][:2])] == [(50265, 514)] * 2
    for si in range(3):
        counts = g7["counts_small" if g7["small_tables"][si] else "counts"]
        multi = counts >= 2
        assert multi.sum() == len(counts) - 1
        for t in ("embed", "pooler"):
            ref, dev, mut = g7[f"{t}_s{si}"], g7[f"{t}_dev_s{si}"], g7[f"{t}_mut_s{si}"]
            assert ref.dtype == np.float64 and ref.shape[0] == dev.shape[0] == mut.shape[0] == len(counts)
            assert (dev > 0).all() and np.isfinite(ref).all()
            bar = 4 * dev.max()
            print(f"set {si} {t}: bar {bar:.3e}, smallest 1 % mutation effect {mut[multi].min():.3e}")
            assert bar <= 0.25 * mut[multi].min()
        assert (g7[f"embed_cosdev_s{si}"] >= 0).all() and g7[f"embed_cosdev_s{si}"].max() > 0 and g7[f"embed_cosdev_s{si}"].max() < 1e-8
        assert np.abs(np.linalg.norm(g7[f"embed_s{si}"], axis=1) - 1).max() < 1e-14
        assert g7["peak"][si] >= 0.5
        assert np.abs(g7[f"pooler_s{si}"]).max() > 0.999


def test_g7_captions_sit_on_the_edges(g7):
    ids, mask, counts = g7["input_ids"], g7["attention_mask"], g7["counts"]
    assert ids.shape == mask.shape == (len(counts), 512) and 18 <= len(counts) <= 24
    assert np.array_equal(counts, mask.sum(1)) and (mask[:, 0] == 1).all() and set(np.unique(mask)) == {0, 1}
    assert {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 511, 512} <= set(int(c) for c in counts)
    assert 2600 <= counts.sum() <= 2800
    assert ids.min() == 0 and ids.max() == 50264
    one = int(np.nonzero(counts == 1)[0][0])
    assert ids[one, 0] == 0 and (ids[one, 1:] == 1).all()                    # <s> alone
    span = 512 - np.argmax(mask[:, ::-1], axis=1)                             # one past the last real token
    holes = [(i, int(s)) for i in range(len(counts)) for s in np.nonzero(mask[i, :span[i]] == 0)[0]]
    assert len(holes) == 2 and holes[0][0] != holes[1][0]
    assert sorted(s for _, s in holes)[0] in (15, 16) and sorted(s for _, s in holes)[1] in (63, 64)
    assert all(ids[i, s] != 1 for i, s in holes)                              # the id under a hole still counts as a position
    inside = [(i, s) for i in range(len(counts)) for s in range(span[i]) if mask[i, s] == 1 and ids[i, s] == 1]
    assert len(inside) == 1 and 0 < inside[0][1] < span[inside[0][0]] - 1     # the pad id inside a mask
    assert any(ids[i, 1] == 3 and (ids[i, :span[i]] == 50264).any() for i in range(len(counts)))
    ids, mask, counts = g7["input_ids_small"], g7["attention_mask_small"], g7["counts_small"]
    assert ids.shape == mask.shape == (4, 38) and [int(c) for c in counts] == [1, 16, 17, 38]
    assert np.array_equal(counts, mask.sum(1)) and ids.max() == 299 and {0, 2, 299} <= set(int(v) for v in ids[mask == 1])


def test_g7_reference_recomputed_in_float64(g7):
    """Two short captions of the 2-layer set through transformers in float64, as the generator runs them."""
    pytest.importorskip("transformers")
    tool = _edges_tool()
    ids, mask, counts = tool.make_captions()
    assert np.array_equal(ids, g7["input_ids"]) and np.array_equal(mask, g7["attention_mask"])
    s_ids, s_mask, _ = tool.make_small_captions()
    assert np.array_equal(s_ids, g7["input_ids_small"]) and np.array_equal(s_mask, g7["attention_mask_small"])
    seed, layers, vocab, npos = (int(g7[k][0]) for k in ("seeds", "layers", "vocab", "max_positions"))
    assert tool.SETS[0][:4] == (seed, layers, vocab, npos)
    sd = synthetic.make_clap_text_state_dict(seed, layers, regime="peaked", vocab=vocab, max_positions=npos)
    rows = [int(np.nonzero(counts == c)[0][0]) for c in (3, 17)]
    pooler, emb = tool.forward(tool.build(sd, layers, vocab, npos), sd, ids[rows, :32], mask[rows, :32])
    assert pooler.dtype == emb.dtype == np.float64
    assert np.abs(pooler - g7["pooler_s0"][rows]).max() <= 1e-12
    assert np.abs(emb - g7["embed_s0"][rows]).max() <= 1e-12


def _ids(N=2, S=8):
    ids = torch.full((N, S), 1, dtype=torch.int64)
    ids[:, 0], ids[:, 1], ids[:, 2] = 0, 100, 2
    mask = (ids != 1).long()
    return ids, mask


@pytest.mark.parametrize("case", ["id_high", "id_negative", "cls_masked", "too_long", "mask_value", "shape"])
def test_encode_ids_validates_on_host(case):
    enc = ClapTextEncoder(layers=1)   # on the CPU: any launch attempt would be a LassError, not a ValueError
    ids, mask = _ids()
    if case == "id_high":
        ids[0, 1] = 50265
    elif case == "id_negative":
        ids[1, 1] = -1
    elif case == "cls_masked":
        mask[1, 0] = 0
    elif case == "too_long":
        ids, mask = _ids(S=513)
    elif case == "mask_value":
        mask[0, 1] = 2
    elif case == "shape":
        mask = mask[:, :4]
    with pytest.raises(ValueError):
        enc.encode_ids(ids, mask)


def test_encoder_on_cpu_raises_lass_error():
    enc = ClapTextEncoder(layers=1)
    with pytest.raises(_lib.LassError):
        enc.encode_ids(*_ids())


def test_tokenizer_call_matches_reference():
    calls = []

    def stub(text, **kw):
        calls.append((list(text), kw))
        ids, mask = _ids(len(text), 512)
        return {"input_ids": ids, "attention_mask": mask}

    enc = ClapTextEncoder(layers=1, tokenizer=stub)
    with pytest.raises(_lib.LassError):   # tokenizes, validates, then refuses to compute on the CPU
        enc.get_query_embed("text", text=["a dog barks", "rain"])
    assert calls == [(["a dog barks", "rain"],
                      {"padding": "max_length", "truncation": True, "max_length": 512, "return_tensors": "pt"})]
    assert clap_text.TOKENIZER_KWARGS == calls[0][1]


def test_no_tokenizer_is_an_error():
    with pytest.raises(RuntimeError, match="no tokenizer"):
        ClapTextEncoder(layers=1).get_query_embed("text", text=["a dog"])


def test_audio_modality_not_implemented():
    enc = ClapTextEncoder(layers=1)
    for modality in ("audio", "hybird"):
        with pytest.raises(NotImplementedError):
            enc.get_query_embed(modality, audio=torch.zeros(1, 16000), text=["a dog"])


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_text_create_fails_without_gpu():
    import ctypes
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.lass_text_create(ctypes.byref(h), 0) < 0
    assert not h.value
    assert b"no HIP device" in lib.lass_text_last_error(None) or b"hip" in lib.lass_text_last_error(None).lower()


def test_load_query_encoder(tmp_path):
    from lass_amd.utils import load_query_encoder
    text_sd = synthetic.make_clap_text_state_dict(7, layers=2)
    tok = lambda text, **kw: None  # noqa: E731
    enc = load_query_encoder(_lightning_checkpoint(str(tmp_path / "c.ckpt"), text_sd), tokenizer=tok)
    assert isinstance(enc, ClapTextEncoder) and enc.tokenizer is tok and enc.layers == 2
