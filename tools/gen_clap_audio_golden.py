"""Generate tests/golden/clap_audio_g6.npz, tests/golden/clap_audio_g6_logmel.npz and tests/golden/clap_audio_state_dict_spec.json on the CPU.

    python tools/gen_clap_audio_golden.py [--ref /root/reference]

Front end (repeat-pad, STFT power, slaney mel, dB): `transformers.ClapFeatureExtractor(truncation="rand_trunc",
padding="repeatpad", frequency_min=50, frequency_max=14000)` - an implementation independent of this project; it returns
float32, so the stored float64 values are a restatement the tool checks against it to float32 rounding.
Tower: the reference's OWN CLAP/open_clip/htsat.py, imported from --ref at run time with its absent third-party imports
stood in by empty modules (torchlibrosa, torchvision.ops.misc, h5py are only named at import; the spectrogram modules are
never called here: the tool feeds `bn0 -> reshape_wav2img -> forward_features` the log-mel directly), loaded with
lass_amd.synthetic.make_clap_audio_state_dict and run in float64; the head (Linear -> ReLU -> Linear, F.normalize;
CLAP/open_clip/model.py:566-570, 776-779) is restated below.  `transformers.ClapAudioModel` with the same weights remapped
is a second opinion: the tool refuses to write unless both towers agree.  Alongside every float64 result the fixture
records the deviation of the same computation in float32 (front end in torchlibrosa's formulation: conv with a windowed
DFT matrix, dense mel matmul) - the GPU tests' tolerance is a multiple of it.  No reference source is written anywhere:
the outputs are data.
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lass_amd import clap_audio as ca, synthetic  # noqa: E402

SETS = [(synthetic.SEED + 10, (2, 2, 12, 2)), (synthetic.SEED + 11, (2, 2, 2, 2))]  # (seed, depths)
FULL_LOGMEL = (0, 1)  # clips whose log-mel is stored in full
QUERY_32K = (0, 3)    # fixture clips regenerated at 32 kHz for the query-by-example test (shallow set only)


def load_reference_htsat(ref: str):
    d = os.path.join(ref, "models", "CLAP", "open_clip")

    stubs = []

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        stubs.append(name)

    class Absent(nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

    stub("torchlibrosa")
    stub("torchlibrosa.stft", Spectrogram=Absent, LogmelFilterBank=Absent)
    stub("torchlibrosa.augmentation", SpecAugmentation=Absent)
    for n in ("torchvision", "torchvision.ops"):
        if n not in sys.modules:
            stub(n)
    stub("torchvision.ops.misc", FrozenBatchNorm2d=Absent)
    stub("h5py")
    pkg = types.ModuleType("open_clip")  # a bare package: its __init__ (which pulls the whole CLAP stack) does not run
    pkg.__path__ = [d]
    sys.modules["open_clip"] = pkg
    htsat = importlib.import_module("open_clip.htsat")
    for n in stubs:  # the stand-ins are needed while the file is imported only; transformers must not see them
        del sys.modules[n]
    with open(os.path.join(d, "model_configs", "HTSAT-base.json")) as f:
        cfg = types.SimpleNamespace(**json.load(f)["audio_cfg"])
    return htsat, cfg


def front_end_f64(clips):
    from transformers import ClapFeatureExtractor

    fe = ClapFeatureExtractor(truncation="rand_trunc", padding="repeatpad", frequency_min=50, frequency_max=14000)
    n = np.arange(1024)
    assert np.abs(fe.mel_filters_slaney - ca.mel_filter()).max() < 1e-15
    out = []
    for x in clips:
        m = fe(x.astype(np.float64), sampling_rate=48000, return_tensors="np")["input_features"]
        out.append(np.asarray(m, dtype=np.float64).reshape(ca.FRAMES, ca.MEL_BINS))
    # The extractor returns float32.  Restate the front end in float64 (periodic Hann, floor 1e-10, its own filter bank)
    # and require the extractor's float32 values to lie within one float32 ulp of it (7.6e-6 at 64 .. 128 dB):
    # this confirms the window and the floor, and the float64 restatement is what the fixture stores.
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / 1024)
    own = []
    for x, m in zip(clips, out):
        v = repeat_pad(x.astype(np.float64))
        fr = np.lib.stride_tricks.sliding_window_view(np.pad(v, 512, mode="reflect"), 1024)[::480]
        p = np.abs(np.fft.rfft(fr * w, axis=1)) ** 2
        own.append(10.0 * np.log10(np.maximum(p @ fe.mel_filters_slaney, 1e-10)))
        assert np.abs(own[-1] - m).max() <= 7.7e-6, np.abs(own[-1] - m).max()
    return np.stack(own)


def repeat_pad(x):
    r = int(ca.CLIP_SAMPLES / len(x))
    v = np.tile(x, r)
    return np.pad(v, (0, ca.CLIP_SAMPLES - len(v)))


def front_end_f32(clips):
    """torchlibrosa's formulation in float32: conv1d with the windowed DFT matrix, power, dense mel matmul, dB."""
    n = np.arange(1024)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / 1024)
    W = np.exp(-2j * np.pi * np.outer(n, np.arange(513)) / 1024) * w[:, None]
    wr, wi = torch.tensor(W.real.T[:, None, :], dtype=torch.float32), torch.tensor(W.imag.T[:, None, :], dtype=torch.float32)
    mel = torch.tensor(ca.mel_filter(), dtype=torch.float32)
    out = []
    for x in clips:
        v = torch.from_numpy(repeat_pad(x.astype(np.float32)))[None, None, :]
        v = torch.nn.functional.pad(v, (512, 512), mode="reflect")
        re, im = torch.nn.functional.conv1d(v, wr, stride=480), torch.nn.functional.conv1d(v, wi, stride=480)
        p = (re ** 2 + im ** 2)[0].T
        out.append(10.0 * torch.log10(torch.clamp(p @ mel, min=1e-10)))
    return torch.stack(out).numpy()


def run_tower(htsat, cfg, sd, depths, logmel, dtype):
    m = htsat.HTSAT_Swin_Transformer(spec_size=256, patch_size=4, patch_stride=(4, 4), num_classes=cfg.class_num, embed_dim=128,
                                     depths=list(depths), num_heads=[4, 8, 16, 32], window_size=8, config=cfg)
    own = m.state_dict()
    pre = "model.audio_branch."
    load = {k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)}
    missing = [k for k in own if k not in load]
    assert not set(load) - set(own) and all(k.endswith(("relative_position_index", "attn_mask", "num_batches_tracked")) for k in missing)
    m.load_state_dict(load, strict=False)
    m = m.eval().to(dtype)
    taps = {}
    m.patch_embed.register_forward_hook(lambda mod, i, o: taps.__setitem__("tokens", o))
    for i, layer in enumerate(m.layers):
        layer.register_forward_hook(lambda mod, inp, o, i=i: taps.__setitem__(f"stage{i}", o[0]))
    with torch.no_grad():
        x = torch.from_numpy(logmel).to(dtype)[:, None]
        x = m.bn0(x.transpose(1, 3)).transpose(1, 3)
        taps["logmel"] = x[:, 0]
        pooled = m.forward_features(m.reshape_wav2img(x))["embedding"]
        taps[f"stage{len(depths) - 1}"] = taps.pop(f"stage{len(depths) - 1}")  # before the final norm, as stored
        t = lambda k: torch.from_numpy(sd["model.audio_projection." + k]).to(dtype)  # noqa: E731
        emb = torch.nn.functional.normalize(torch.relu(pooled @ t("0.weight").T + t("0.bias")) @ t("2.weight").T + t("2.bias"), dim=-1)
    taps["pooled"], taps["embed"] = pooled, emb
    return {k: v.double().numpy() for k, v in taps.items()}, m


def hf_pooled(sd, depths, logmel):
    """transformers.ClapAudioModel on the same weights and features (float64)."""
    from transformers import ClapAudioConfig, ClapAudioModel

    cfg = ClapAudioConfig(patch_embeds_hidden_size=128, depths=list(depths), hidden_size=1024, enable_fusion=False)
    m = ClapAudioModel(cfg).eval()
    pre = "model.audio_branch."
    ren = [("bn0.", "batch_norm."), (".attn.relative_position_bias_table", ".attention.self.relative_position_bias_table"),
           (".attn.proj.", ".attention.output.dense."), (".norm1.", ".layernorm_before."), (".norm2.", ".layernorm_after."),
           (".mlp.fc1.", ".intermediate.dense."), (".mlp.fc2.", ".output.dense.")]
    load = {}
    for k, v in sd.items():
        if not k.startswith(pre) or "tscam_conv" in k or ".head." in k or k.startswith(pre + "head."):
            continue
        k, v = k[len(pre):], torch.from_numpy(v)
        if ".attn.qkv." in k:
            for j, name in enumerate(("query", "key", "value")):
                load["audio_encoder." + k.replace(".attn.qkv.", f".attention.self.{name}.")] = v.chunk(3, 0)[j]
            continue
        for a, b in ren:
            k = k.replace(a, b)
        load["audio_encoder." + k] = v
    own = m.state_dict()
    missing = [k for k in own if k not in load]
    assert not set(load) - set(own), sorted(set(load) - set(own))[:5]
    assert all(k.endswith(("relative_position_index", "num_batches_tracked")) for k in missing), missing[:5]
    m.load_state_dict(load, strict=False)
    with torch.no_grad():
        return m.double()(input_features=torch.from_numpy(logmel)[:, None]).pooler_output.numpy()


def margins(x):
    """row / column sums of (B, rows, cols): every element counted twice over."""
    return x.sum(2), x.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    htsat, cfg = load_reference_htsat(args.ref)
    nclip = len(synthetic.CLAP_AUDIO_CLIPS)
    clips = [synthetic.make_clap_audio_clip(i) for i in range(nclip)]
    lm64, lm32 = front_end_f64(clips), front_end_f32(clips)
    silent = [i for i, (_, level) in enumerate(synthetic.CLAP_AUDIO_CLIPS) if level == 0.0]
    assert all((lm64[i] == -100.0).all() and (lm32[i] == -100.0).all() for i in silent)
    live = lm64[[i for i in range(nclip) if i not in silent]]
    print(f"log-mel dB: f32 vs f64 max {np.abs(lm32 - lm64).max():.3e}; lowest non-floor value {live[live > -100].min():.1f} dB")
    out = {"clip_seed": np.int64(synthetic.SEED + 12), "clip_lengths": np.asarray([c[0] for c in synthetic.CLAP_AUDIO_CLIPS]),
           "seeds": np.asarray([s for s, _ in SETS]), "depths": np.asarray([d for _, d in SETS]),
           "full_logmel_clips": np.asarray(FULL_LOGMEL),
           "logmel_db_dev": np.abs(lm32 - lm64).reshape(nclip, -1).max(1), "mel_filter": ca.mel_filter()}
    for si, (seed, depths) in enumerate(SETS):
        sd = synthetic.make_clap_audio_state_dict(seed, depths)
        r64, model = run_tower(htsat, cfg, sd, depths, lm64, torch.float64)
        r32, _ = run_tower(htsat, cfg, sd, depths, lm32, torch.float32)
        hf = hf_pooled(sd, depths, lm64)
        agree = np.abs(hf - r64["pooled"]).max()
        print(f"set {si} depths {depths}: reference htsat vs transformers.ClapAudioModel pooled max diff {agree:.3e}")
        assert agree < 1e-9, "the two towers disagree"
        dev = lambda a, b: np.abs(a - b).reshape(nclip, -1).max(1)  # noqa: E731
        out[f"embed_s{si}"], out[f"pooled_s{si}"] = r64["embed"], r64["pooled"]
        out[f"embed_dev_s{si}"], out[f"pooled_dev_s{si}"] = dev(r32["embed"], r64["embed"]), dev(r32["pooled"], r64["pooled"])
        cos = (r32["embed"] * r64["embed"]).sum(1) / np.linalg.norm(r32["embed"], axis=1) / np.linalg.norm(r64["embed"], axis=1)
        out[f"embed_cosdev_s{si}"] = 1.0 - cos
        for k in ["logmel", "tokens"] + [f"stage{i}" for i in range(len(depths))]:
            (a, b), (a32, b32) = margins(r64[k]), margins(r32[k])
            out[f"{k}_rows_s{si}"], out[f"{k}_cols_s{si}"] = a, b
            out[f"{k}_rows_dev_s{si}"], out[f"{k}_cols_dev_s{si}"] = dev(a32, a), dev(b32, b)
        out[f"logmel_dev_s{si}"] = dev(r32["logmel"], r64["logmel"])
        if si == len(SETS) - 1:
            # 32 kHz queries: resampled on the host in float64 with the published taps (this stage is parity unpinned),
            # rounded to float32 as the device's resampler output is, then the pinned path as above
            q48 = [ca.resample_host(synthetic.make_clap_audio_clip(i, rate=32000).astype(np.float64)).astype(np.float32) for i in QUERY_32K]
            out["query32k_clips"] = np.asarray(QUERY_32K)
            out[f"query32k_embed_s{si}"] = run_tower(htsat, cfg, sd, depths, front_end_f64(q48), torch.float64)[0]["embed"]
        print(f"  embed dev {out[f'embed_dev_s{si}'].max():.3e} (1-cos {out[f'embed_cosdev_s{si}'].max():.3e}), pooled dev "
              f"{out[f'pooled_dev_s{si}'].max():.3e}, |pooled| max {np.abs(r64['pooled']).max():.3f}")
    golden = os.path.join(ROOT, "tests", "golden")
    path = os.path.join(golden, "clap_audio_g6.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    # the two full log-mels (dB, before bn0) in float64 are a megabyte by themselves: a file of their own keeps both fixtures
    # under the repository's limit for one committed file
    path = os.path.join(golden, "clap_audio_g6_logmel.npz")
    np.savez_compressed(path, logmel_db=lm64[list(FULL_LOGMEL)])
    print(f"{path}: {os.path.getsize(path)} bytes")
    # the spec is the reference's own base model (its state_dict, buffers included) + the CLAP model's audio_projection
    model_sd = {"model.audio_branch." + k: list(v.shape) for k, v in htsat.create_htsat_model(cfg).state_dict().items()}
    model_sd.update({"model.audio_projection.0.weight": [512, 1024], "model.audio_projection.0.bias": [512],
                     "model.audio_projection.2.weight": [512, 512], "model.audio_projection.2.bias": [512]})
    with open(os.path.join(golden, "clap_audio_state_dict_spec.json"), "w") as f:
        json.dump(model_sd, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
