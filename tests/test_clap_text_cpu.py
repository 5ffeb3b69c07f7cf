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
