"""CLAP audio encoder, the parts that need no GPU: parameter tree against the reference's own state_dict spec, checkpoint
loading, the C-ABI's symbols, host validation, the host-built mel filter and resampler taps, and ClapQueryEncoder's routing."""
import json
import os
import random
import re
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

from lass_amd import _lib, clap_audio as ca, synthetic
from lass_amd.clap_audio import ClapAudioEncoder, ClapQueryEncoder
from lass_amd.clap_text import ClapTextEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHALLOW = (1, 1, 1, 1)


def test_state_dict_matches_reference_spec(golden_dir):
    with open(os.path.join(golden_dir, "clap_audio_state_dict_spec.json")) as f:
        spec = json.load(f)
    sd = ClapAudioEncoder().state_dict()
    assert list(sd) == list(spec)
    assert {k: list(v.shape) for k, v in sd.items()} == spec
    assert [(k, list(s)) for k, s, _ in ca.param_specs()] == [(k, v) for k, v in spec.items()]
    assert len([k for k in spec if k.startswith("model.audio_branch.")]) == 284


def test_derived_buffers_are_swin_tables():
    idx = ca.relative_position_index()
    assert idx.shape == (64, 64) and int(idx.min()) == 0 and int(idx.max()) == 224
    assert int(idx[0, 0]) == 112 and int(idx[0, 63]) == 0 and int(idx[63, 0]) == 224 and int(idx[0, 1]) == 111
    m = ca.shift_mask(16)
    assert m.shape == (4, 64, 64) and set(m.unique().tolist()) == {-100.0, 0.0}
    assert float(m[0].abs().sum()) == 0.0                       # the first window lies inside one region
    assert float(m[3, 0, 63]) == -100.0 and float(m[3, 0, 0]) == 0.0  # the last one straddles both wrap-arounds


def _checkpoint(path, drop=None):
    audio = synthetic.make_clap_audio_state_dict(3, SHALLOW)
    sd = {"query_encoder." + k: torch.from_numpy(v) for k, v in audio.items() if k != drop}
    sd["ss_model.base.after_conv.bias"] = torch.zeros(3)
    sd["query_encoder.model.text_branch.pooler.dense.bias"] = torch.zeros(768)
    sd["query_encoder.model.text_projection.0.bias"] = torch.zeros(512)
    sd["query_encoder.model.text_transform.layers.0.weight"] = torch.zeros(4, 4)
    sd["query_encoder.model.audio_transform.layers.0.weight"] = torch.zeros(4, 4)
    sd["query_encoder.model.logit_scale_a"] = torch.zeros(())
    sd["query_encoder.model.logit_scale_t"] = torch.zeros(())
    sd["query_encoder.model.audio_branch.spectrogram_extractor.stft.conv_real.weight"] = torch.zeros(513, 1, 1024)
    sd["query_encoder.model.audio_branch.logmel_extractor.melW"] = torch.zeros(513, 64)
    sd["query_encoder.model.audio_branch.layers.0.blocks.0.attn.relative_position_index"] = torch.zeros(64, 64, dtype=torch.int64)
    torch.save({"state_dict": sd, "epoch": 1}, path)
    return audio


def test_from_checkpoint_loads_lightning_shaped_file(tmp_path):
    audio = _checkpoint(str(tmp_path / "a.ckpt"))
    enc = ClapAudioEncoder.from_checkpoint(str(tmp_path / "a.ckpt"))
    assert enc.depths == SHALLOW and enc.embed_dim == 128 and enc.features == 1024
    own = enc.state_dict()
    for k, v in audio.items():
        assert torch.equal(own[k], torch.from_numpy(v)), k
    assert torch.equal(own["model.audio_branch.layers.0.blocks.0.attn.relative_position_index"], ca.relative_position_index())
    uploaded = [n for n, _ in enc._uploaded()]
    assert not [n for n in uploaded if "tscam_conv" in n or "head." in n]
    assert "audio_branch.bn0.running_var" in uploaded and "audio_projection.2.bias" in uploaded


def test_missing_audio_key_is_named(tmp_path):
    drop = "model.audio_branch.layers.2.blocks.0.mlp.fc2.bias"
    _checkpoint(str(tmp_path / "b.ckpt"), drop=drop)
    with pytest.raises(KeyError, match=re.escape("query_encoder." + drop)):
        ClapAudioEncoder.from_checkpoint(str(tmp_path / "b.ckpt"))


def test_symbols_exported_and_bound():
    with open(os.path.join(ROOT, "include", "lass_hip.h")) as f:
        declared = set(re.findall(r"\b(lass_audioq_[a-z0-9_]+)\s*\(", f.read()))
    assert {"lass_audioq_create", "lass_audioq_destroy", "lass_audioq_last_error", "lass_audioq_set_param", "lass_audioq_finalize",
            "lass_audioq_workspace_bytes", "lass_audioq_encode_wave48k", "lass_audioq_encode_wave32k"} <= declared
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert declared <= bound
    lib = _lib.load()
    for name in declared:
        assert getattr(lib, name) is not None


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a machine without a GPU")
def test_create_fails_without_a_device():
    lib = _lib.load()
    h = c_void_p()
    assert lib.lass_audioq_create(byref(h), 0) < 0 and not h.value
    assert "no CPU fallback" in lib.lass_audioq_last_error(None).decode()


def test_host_validation_precedes_any_launch():
    enc = ClapAudioEncoder(depths=SHALLOW)
    with pytest.raises(_lib.LassError, match="no CPU fallback"):
        enc.encode_wave48k(torch.zeros(2, 4800))
    with pytest.raises(_lib.LassError):
        enc.get_query_embed("audio", audio=torch.zeros(1, 3200))
    for bad in (torch.zeros(4800), torch.zeros(1, 2, 4800), torch.zeros(1, 4800, dtype=torch.int16), torch.zeros(0, 4800),
                torch.zeros(1, 0)):
        with pytest.raises(ValueError):
            enc.encode_wave32k(bad)
    with pytest.raises(ValueError, match="320000"):
        enc.encode_wave32k(torch.zeros(1, 320001))
    with pytest.raises(ValueError, match="480000"):
        enc.encode_wave48k(torch.zeros(1, 480001))
    for lengths in ([0, 5], [5, 4801], [5], [1.5, 2.0]):
        with pytest.raises(ValueError):
            enc.encode_wave48k(torch.zeros(2, 4800), lengths=lengths)
    with pytest.raises(NotImplementedError):
        enc.get_query_embed("text", text=["a"])


def test_mel_filter_equals_the_feature_extractors(golden_dir):
    ref = np.load(os.path.join(golden_dir, "clap_audio_g6.npz"))["mel_filter"]
    own = ca.mel_filter()
    assert own.shape == ref.shape == (513, 64) and own.dtype == np.float64
    assert np.abs(own - ref).max() <= 4 * np.finfo(np.float64).eps * ref.max()
    width = (own > 0).sum(0)
    assert width.min() >= 1 and width.max() <= 32  # the kernel's run of taps per band
    for m in range(64):  # each band is one contiguous run of bins
        nz = np.nonzero(own[:, m])[0]
        assert nz[-1] - nz[0] + 1 == len(nz)


def test_resampler_taps():
    h = ca.resample_taps()
    assert h.shape == (3, 16)
    # DC gain of each phase: rolloff 0.99 puts the cutoff just below Nyquist, so the windowed sinc sums close to, not
    # exactly, 1.  The float64 taps give |gain - 1| = 3.9e-5 (phase 0) and 6.8e-4 (phases 1, 2); bound = 2 x that.
    gain = np.abs(h.sum(1) - 1)
    assert gain[0] <= 2 * 3.9e-5 and gain[1] <= 2 * 6.8e-4 and gain[2] <= 2 * 6.8e-4
    # symmetry of the published kernel: phase 0 is even about its centre tap (index 7; tap 15 sits on the window's zero),
    # phases 1 and 2 are mirror images of each other
    assert np.abs(h[0, :7] - h[0, 14:7:-1]).max() <= 1e-15 and abs(h[0, 15]) <= 1e-30
    assert np.abs(h[2, 1:] - h[1, 15:0:-1]).max() <= 1e-15
    assert abs(h[0, 7] - 0.99) <= 1e-15  # sinc(0) * window(0) * base_freq / orig_freq
    y = ca.resample_host(np.ones(64))
    assert y.shape == (96,) and np.abs(y[24:-24] - np.tile(h.sum(1), 16)).max() <= 1e-15


class _Stub(torch.nn.Module):
    def __init__(self, tag):
        super().__init__()
        self.tag, self.calls = tag, []

    def get_query_embed(self, modality, audio=None, text=None, device=None):
        self.calls.append((modality, audio, text))
        return torch.full((1, 512), float(self.tag))


def test_query_encoder_routes_as_the_reference():
    text, audio = _Stub(1), _Stub(2)
    qe = ClapQueryEncoder(text, audio)
    assert float(qe.get_query_embed("text", text=["a"])[0, 0]) == 1 and float(qe.get_query_embed("audio", audio="x")[0, 0]) == 2
    with pytest.raises(NotImplementedError):
        qe.get_query_embed("video")
    for ratio in (0.5, 0.2, 1.0):
        random.seed(7)
        want = [2.0 if random.random() > ratio else 1.0 for _ in range(32)]
        state_after = random.getstate()
        random.seed(7)
        got = [float(qe.get_query_embed("hybird", audio="x", text=["a"], use_text_ratio=ratio)[0, 0]) for _ in range(32)]
        assert got == want
        assert random.getstate() == state_after  # exactly one draw per call


def test_load_query_encoder_default_is_the_text_encoder(tmp_path):
    from lass_amd.utils import load_query_encoder
    audio = synthetic.make_clap_audio_state_dict(3, SHALLOW)
    text = synthetic.make_clap_text_state_dict(4, 1)
    sd = {"query_encoder." + k: torch.from_numpy(v) for k, v in {**audio, **text}.items()}
    path = str(tmp_path / "c.ckpt")
    torch.save({"state_dict": sd}, path)
    enc = load_query_encoder(path, tokenizer=lambda *a, **k: None)
    assert type(enc) is ClapTextEncoder
    both = load_query_encoder(path, tokenizer=lambda *a, **k: None, modalities=("text", "audio"))
    assert isinstance(both, ClapQueryEncoder) and both.audio_encoder.depths == SHALLOW and both.text_encoder.layers == 1
    assert type(load_query_encoder(path, modalities=("audio",))) is ClapAudioEncoder
    with pytest.raises(ValueError):
        load_query_encoder(path, modalities=("video",))
    with pytest.raises(ValueError, match="128"):
        ClapAudioEncoder(embed_dim=96)
