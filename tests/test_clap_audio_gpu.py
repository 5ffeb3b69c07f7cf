"""CLAP audio encoder on the MI355X (lass_audioq_*, audio_clap.hip): parity of the front end, tower and head with the
fixture (tests/golden/clap_audio_g6*.npz, tools/gen_clap_audio_golden.py: the reference's own HTSAT in float64 behind
transformers' ClapFeatureExtractor), bitwise batch / position / repeat-pad invariance, the resampler's closed forms,
checkpoint loading, query by example end to end, and the C-ABI's error paths.

Tolerances.  The unit-norm embedding is first held to the text tower's bars (max abs 2e-5, cosine >= 1 - 1e-6,
tests/test_clap_text_gpu.py).  Every other tensor, and the embedding where those bars are the smaller ones, is held to
4 x the deviation of the reference's own float32 run from its float64 run on the same clip and tensor, as recorded in the
fixture (4 x: the device sums 1024-long rows in MFMA order rather than ATen's and stage 3 is 12 blocks deep).  Each figure
is printed before it is asserted."""
import ctypes
import os
from ctypes import byref, c_int, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from lass_amd import _lib, clap_audio as ca, synthetic
from lass_amd.clap_audio import ClapAudioEncoder, ClapQueryEncoder

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NCLIP = len(synthetic.CLAP_AUDIO_CLIPS)


@pytest.fixture(scope="module")
def g6(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "clap_audio_g6.npz")))
    g.update(np.load(os.path.join(golden_dir, "clap_audio_g6_logmel.npz")))
    return g


@pytest.fixture(scope="module")
def clips():
    return [synthetic.make_clap_audio_clip(i) for i in range(NCLIP)]


def _sd(g6, si):
    return synthetic.make_clap_audio_state_dict(int(g6["seeds"][si]), tuple(int(d) for d in g6["depths"][si]))


def _encoder(g6, si):
    enc = ClapAudioEncoder(depths=g6["depths"][si])
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(g6, si).items()}, strict=False)
    return enc.to(DEV)


@pytest.fixture(scope="module")
def enc_shallow(g6):
    return _encoder(g6, 1)


def _batch(clips, order=None):
    order = range(len(clips)) if order is None else order
    L = max(len(clips[i]) for i in order)
    wave = np.zeros((len(order), L), dtype=np.float32)
    for r, i in enumerate(order):
        wave[r, :len(clips[i])] = clips[i]
    return torch.from_numpy(wave).to(DEV), np.asarray([len(clips[i]) for i in order], dtype=np.int32)


def _hold(name, got, ref, bar):
    """got, ref (clips, ...) float64; bar (clips,): per-clip max abs error within its bar."""
    err = np.abs(got - ref).reshape(len(ref), -1).max(1)
    print(f"{name}: max abs error per clip {err}, bar {bar}")
    assert (err <= bar).all(), (name, err, bar)


@pytest.mark.parametrize("si", [0, 1], ids=["depths-2-2-12-2", "depths-2-2-2-2"])
def test_parity_with_reference(g6, clips, si, enc_shallow):
    enc = enc_shallow if si == 1 else _encoder(g6, 0)
    wave, lens = _batch(clips)
    emb, taps = enc.encode_wave48k(wave, lens, return_taps=True)
    emb = emb.cpu().double().numpy()
    D = lambda t: t.cpu().double().numpy()  # noqa: E731
    ref = g6[f"embed_s{si}"]
    _hold("embedding", emb, ref, np.maximum(2e-5, 4 * g6[f"embed_dev_s{si}"]))
    cos = (emb * ref).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref, axis=1)
    print("1 - cosine", 1 - cos, "reference f32", g6[f"embed_cosdev_s{si}"])
    assert (1 - cos <= np.maximum(1e-6, 4 * g6[f"embed_cosdev_s{si}"])).all()
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-5
    _hold("pooled", D(taps["embedding"]), g6[f"pooled_s{si}"], 4 * g6[f"pooled_dev_s{si}"])
    # log-mel after bn0: two clips element by element (dB from the fixture, bn0 applied here in float64), all by margins
    sd = _sd(g6, si)
    p = {k: sd["model.audio_branch.bn0." + k].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var")}
    scale = p["weight"] / np.sqrt(p["running_var"] + 1e-5)
    base = p["bias"] - p["running_mean"] * scale
    lm = D(taps["logmel"])
    full = [int(i) for i in g6["full_logmel_clips"]]
    _hold("log-mel (full)", lm[full], g6["logmel_db"] * scale + base, 4 * g6[f"logmel_dev_s{si}"][full])
    silent = [i for i, (_, level) in enumerate(synthetic.CLAP_AUDIO_CLIPS) if level == 0.0]
    exact = (np.float32(-100.0) * scale.astype(np.float32) + base.astype(np.float32)).astype(np.float32)
    for i in silent:
        assert (taps["logmel"][i].cpu().numpy() == exact[None, :]).all()
    for name, t in [("logmel", lm), ("tokens", D(taps["tokens"]))] + [(f"stage{i}", D(s)) for i, s in enumerate(taps["stages"])]:
        _hold(name + " row sums", t.sum(2), g6[f"{name}_rows_s{si}"], 4 * g6[f"{name}_rows_dev_s{si}"])
        _hold(name + " column sums", t.sum(1), g6[f"{name}_cols_s{si}"], 4 * g6[f"{name}_cols_dev_s{si}"])


def test_batch_and_position_invariance_bitwise(clips, enc_shallow):
    order = np.random.Generator(np.random.PCG64(6)).permutation(np.arange(16) % NCLIP)
    wave, lens = _batch(clips, list(order))
    batch = enc_shallow.encode_wave48k(wave, lens).cpu()
    for i in range(NCLIP):
        alone = enc_shallow.encode_wave48k(torch.from_numpy(clips[i])[None].to(DEV)).cpu()
        for j in np.nonzero(order == i)[0]:
            assert torch.equal(alone[0], batch[j]), (i, j)


def test_repeat_pad_is_index_arithmetic_bitwise(clips, enc_shallow):
    for i in (0, 1):
        x = clips[i]
        padded = np.zeros(ca.CLIP_SAMPLES, dtype=np.float32)
        r = ca.CLIP_SAMPLES // len(x)
        padded[:r * len(x)] = np.tile(x, r)
        a = enc_shallow.encode_wave48k(torch.from_numpy(x)[None].to(DEV)).cpu()
        b = enc_shallow.encode_wave48k(torch.from_numpy(padded)[None].to(DEV)).cpu()
        assert torch.equal(a, b), i


def test_resampler_closed_forms(enc_shallow):
    """Parity unpinned (torchaudio is not available): a constant and two sines against their analytic 48 kHz forms, the
    error bounded by 4 x what the float64 host evaluation of the same taps leaves."""
    L = 32001
    n32, t48 = np.arange(L), np.arange((3 * L + 1) // 2) / 48000.0
    cases = {"constant": (np.full(L, 0.25), np.full(len(t48), 0.25))}
    for f in (1000.0, 10000.0):
        cases[f"{f:.0f} Hz"] = (0.5 * np.sin(2 * np.pi * f * n32 / 32000.0 + 0.3), 0.5 * np.sin(2 * np.pi * f * t48 + 0.3))
    for name, (x, want) in cases.items():
        x = x.astype(np.float32)
        _, taps = enc_shallow.encode_wave32k(torch.from_numpy(x)[None].to(DEV), return_taps=True)
        y = taps["wave48k"][0].cpu().double().numpy()
        assert y.shape == ((3 * L + 1) // 2,) == (int(np.ceil(1.5 * L)),)
        host = ca.resample_host(x.astype(np.float64))
        inner = slice(32, -32)  # away from the edges, where the filter sees the zero padding
        e_dev, e_host = np.abs(y - want)[inner].max(), np.abs(host - want)[inner].max()
        print(f"resampler {name}: device error {e_dev:.3e}, float64 host error {e_host:.3e}, device vs host {np.abs(y - host).max():.3e}")
        assert e_dev <= 4 * e_host


def _checkpoint(path, audio_sd, text_sd=None, ss_sd=None):
    sd = {"query_encoder." + k: torch.from_numpy(v) for k, v in audio_sd.items()}
    sd.update({"query_encoder." + k: torch.from_numpy(v) for k, v in (text_sd or {}).items()})
    sd.update({"ss_model." + k: torch.from_numpy(np.asarray(v)) for k, v in (ss_sd or {}).items()})
    sd["query_encoder.model.logit_scale_a"] = torch.zeros(())
    sd["query_encoder.model.audio_branch.layers.0.blocks.0.attn.relative_position_index"] = torch.zeros(64, 64, dtype=torch.int64)
    sd["query_encoder.model.audio_branch.logmel_extractor.melW"] = torch.zeros(513, 64)
    torch.save({"state_dict": sd, "epoch": 1}, path)
    return path


def test_from_checkpoint_reproduces_fixture(tmp_path, g6, clips):
    enc = ClapAudioEncoder.from_checkpoint(_checkpoint(str(tmp_path / "a.ckpt"), _sd(g6, 1))).to(DEV)
    assert enc.depths == (2, 2, 2, 2)
    wave, lens = _batch(clips)
    emb = enc.encode_wave48k(wave, lens).cpu().double().numpy()
    _hold("embedding", emb, g6["embed_s1"], np.maximum(2e-5, 4 * g6["embed_dev_s1"]))


def test_query_by_example_end_to_end(tmp_path, g6, golden_dir, synthetic_sd):
    """ResUNet30 conditioned on ClapQueryEncoder.get_query_embed('audio', audio=32 kHz clips) against the oracle separator
    conditioned on the fixture's embeddings of the same queries; modality='text' is ClapTextEncoder's result bit for bit."""
    from lass_amd.clap_text import ClapTextEncoder
    from lass_amd.resunet import ResUNet30
    from lass_amd.utils import load_query_encoder
    from oracle import metrics as om
    from oracle import resunet as orr
    g5 = np.load(os.path.join(golden_dir, "clap_text_g5.npz"))
    text_sd = synthetic.make_clap_text_state_dict(int(g5["seeds"][list(g5["layers"]).index(2)]), 2)
    ckpt = _checkpoint(str(tmp_path / "audiosep.ckpt"), _sd(g6, 1), text_sd, synthetic_sd)

    def tokenizer(text, **kw):
        r = [int(t) for t in text]
        return {"input_ids": torch.from_numpy(g5["input_ids"][r]), "attention_mask": torch.from_numpy(g5["attention_mask"][r])}

    qe = load_query_encoder(ckpt, tokenizer=tokenizer, modalities=("text", "audio")).to(DEV)
    assert isinstance(qe, ClapQueryEncoder)
    queries = [synthetic.make_clap_audio_clip(int(i), rate=32000) for i in g6["query32k_clips"]]
    L = max(len(q) for q in queries)
    conds = []
    for q in queries:  # clips of different lengths: one call each (get_query_embed takes a (B, L) tensor)
        conds.append(qe.get_query_embed("audio", audio=torch.from_numpy(q)[None].to(DEV)))
        assert conds[-1].shape == (1, 512) and conds[-1].dtype == torch.float32
    cond = torch.cat(conds)
    ref_cond = g6["query32k_embed_s1"]
    # the resampler is the only unpinned stage in front of these: its float32 output differs from the fixture's float64
    # host evaluation by rounding only, so the embedding bar of the pinned path holds here too
    qi = [int(i) for i in g6["query32k_clips"]]
    _hold("query embedding (32 kHz path)", cond.cpu().double().numpy(), ref_cond, np.maximum(2e-5, 4 * g6["embed_dev_s1"][qi]))
    model = ResUNet30(1, 1, 512)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    model = model.to(DEV).eval()
    src, mix = synthetic.make_mixtures(len(queries), 32000)
    out = model({"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": cond})["waveform"]
    assert out.shape == (len(queries), 1, 32000)
    ref = orr.forward(orr.to_torch(synthetic_sd), {"mixture": torch.from_numpy(mix)[:, None, :],
                                                   "condition": torch.from_numpy(ref_cond.astype(np.float32))})["waveform"]
    out, ref = out.cpu().numpy(), ref.numpy()
    for n in range(len(queries)):
        for fn in (om.calculate_sdr, om.calculate_sisdr):
            a, b = fn(src[n], out[n, 0]), fn(src[n], ref[n, 0])
            print(fn.__name__, n, a, b)
            assert abs(a - b) < 0.01
    text = qe.get_query_embed("text", text=["0", "3"])
    own = ClapTextEncoder.from_checkpoint(ckpt, tokenizer=tokenizer).to(DEV).get_query_embed("text", text=["0", "3"])
    assert torch.equal(text.cpu(), own.cpu())
    assert L <= ca.MAX_SAMPLES_32K


def test_c_abi_error_paths(enc_shallow, clips, g6):
    """Every argument error is LASS_ERR_ARG with a message, nothing is launched, and the context works afterwards."""
    x = torch.from_numpy(clips[0])[None].to(DEV)
    before = enc_shallow.encode_wave48k(x).cpu()
    ctx = enc_shallow._context()
    lib, h = ctx.lib, ctx.ctx
    n = c_size_t()
    assert lib.lass_audioq_workspace_bytes(h, 1, byref(n)) == 0 and n.value > 0
    assert lib.lass_audioq_workspace_bytes(h, 0, byref(n)) == -1
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, 512, device=DEV)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    L = x.shape[1]
    one = (c_int * 1)(L)
    bad = [
        ("workspace too small", lib.lass_audioq_encode_wave48k, (h, P(x), one, 1, L, P(out), None, P(ws), n.value - 1, st)),
        ("non-NULL", lib.lass_audioq_encode_wave48k, (h, None, one, 1, L, P(out), None, P(ws), n.value, st)),
        ("non-NULL", lib.lass_audioq_encode_wave48k, (h, P(x), one, 1, L, None, None, P(ws), n.value, st)),
        ("non-NULL", lib.lass_audioq_encode_wave32k, (h, P(x), one, 1, L, P(out), None, None, n.value, st)),
        ("B must be", lib.lass_audioq_encode_wave48k, (h, P(x), one, 0, L, P(out), None, P(ws), n.value, st)),
        ("480000", lib.lass_audioq_encode_wave48k, (h, P(x), None, 1, 480001, P(out), None, P(ws), n.value, st)),
        ("320000", lib.lass_audioq_encode_wave32k, (h, P(x), None, 1, 320001, P(out), None, P(ws), n.value, st)),
        ("lengths", lib.lass_audioq_encode_wave48k, (h, P(x), (c_int * 1)(L + 1), 1, L, P(out), None, P(ws), n.value, st)),
        ("lengths", lib.lass_audioq_encode_wave48k, (h, P(x), (c_int * 1)(0), 1, L, P(out), None, P(ws), n.value, st)),
    ]
    for msg, fn, args in bad:
        assert fn(*args) == -1, msg
        assert msg in lib.lass_audioq_last_error(h).decode(), (msg, lib.lass_audioq_last_error(h).decode())
    shape = (ctypes.c_int64 * 1)(3)
    assert lib.lass_audioq_set_param(h, b"audio_branch.head.weight", P(x), shape, 1) == -1
    assert "unknown" in lib.lass_audioq_last_error(h).decode()
    with pytest.raises(ValueError, match="320000"):
        enc_shallow.encode_wave32k(torch.zeros(1, 320001, device=DEV))
    with pytest.raises(_lib.LassError):
        enc_shallow.encode_wave48k(torch.zeros(1, 100))  # a CPU tensor
    torch.cuda.synchronize()
    assert torch.equal(enc_shallow.encode_wave48k(x).cpu(), before)
