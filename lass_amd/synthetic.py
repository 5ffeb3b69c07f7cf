"""Seeded synthetic weights, conditions and mixtures.

There is no checkpoint and no audio in the build/test environment, so every parity test, the smoke test and
bench.py regenerate the same tensors from a seed on both sides (HIP path and oracle).  Nothing here is committed
as data.

Weights: conv/linear ~ U(+-xavier bound) (reference init: models/base.py:9-15), but BatchNorm statistics are
randomised (gamma~U(.5,1.5), beta,mean~U(-.1,.1), var~U(.5,1.5)) and biases are non-zero so that BN-folding,
FiLM and bias bugs are visible - the reference's own init (gamma=1, beta=0, mean=0, var=1, bias=0) would hide them.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

from . import arch

SEED = 1234  # config/audiosep_base.yaml:48 (random_seed)


def _xavier_bound(shape: Tuple[int, ...], kind: str) -> float:
    if kind == "linear_w":
        fan_out, fan_in = shape
    else:  # conv_w (O,I,kh,kw) / tconv_w (I,O,kh,kw): torch's fan computation treats dim0 as "out", dim1 as "in"
        rf = int(np.prod(shape[2:]))
        fan_out, fan_in = shape[0] * rf, shape[1] * rf
    return math.sqrt(6.0 / (fan_in + fan_out))


def make_state_dict(seed: int = SEED, input_channels: int = 1, output_channels: int = 1,
                    condition_size: int = 512, specs=None, n_fft: int = arch.N_FFT) -> Dict[str, np.ndarray]:
    """Seeded numpy state_dict with the reference's keys (float32; num_batches_tracked int64).  `specs` defaults to
    arch.param_specs(..., n_fft=n_fft) (ResUNet30; n_fft=2048: the 32 kHz geometry's 1025-entry bn0, which is drawn first, so
    that model's stream differs from the default's from the start); pass arch.ms_param_specs(...) for the multi-STFT model."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd: Dict[str, np.ndarray] = {}
    if specs is None:
        specs = arch.param_specs(input_channels, output_channels, condition_size, n_fft=n_fft)
    for name, shape, kind in specs:
        if kind in ("conv_w", "tconv_w", "linear_w"):
            b = _xavier_bound(shape, kind)
            v = rng.uniform(-b, b, size=shape)
        elif kind in ("bias", "linear_b", "bn_bias", "bn_mean"):
            v = rng.uniform(-0.1, 0.1, size=shape)
        elif kind in ("bn_weight", "bn_var"):
            v = rng.uniform(0.5, 1.5, size=shape)
        elif kind == "bn_nbt":
            sd[name] = np.asarray(0, dtype=np.int64)
            continue
        else:
            raise ValueError(kind)
        sd[name] = v.astype(np.float32)
    # Centre the mask logits so the synthetic net emits a usable mask (|M|~0.5, phase rotation mostly < 45 deg)
    # instead of a random-phase one whose iSTFT cancels to ~0: keeps SDR / SI-SDR parity checks well conditioned.
    sd["base.after_conv.bias"] = (sd["base.after_conv.bias"]
                                  + np.asarray([1.5, 2.0, -0.2] * output_channels, dtype=np.float32))
    return sd


def make_state_dict_ms(seed: int = SEED + 4, win_lengths=arch.MS_WIN_LENGTHS) -> Dict[str, np.ndarray]:
    """Seeded weights of the multi-STFT separator (arch.ms_param_specs)."""
    return make_state_dict(seed, specs=arch.ms_param_specs(win_lengths=win_lengths))


def make_condition(batch: int, seed: int = SEED, condition_size: int = 512, distinct: bool = True) -> np.ndarray:
    """Unit-norm query embeddings (CLAP text embeddings are L2-normalised: CLAP/open_clip/model.py:750)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    n = batch if distinct else 1
    g = rng.standard_normal((n, condition_size))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    if not distinct:
        g = np.repeat(g, batch, axis=0)
    return g.astype(np.float32)


_SNRS = (-15, -10, -5, 0, 5, 10, 15)


def make_clip(index: int, length: int = 160000, sr: int = 16000, seed: int = SEED):
    """(source, noise, snr_db) for synthetic validation clip `index` (float32, mono, already at `sr`)."""
    rng = np.random.Generator(np.random.PCG64([seed, 7919, index]))
    t = np.arange(length) / sr
    src = np.zeros(length)
    for _ in range(3):
        f = rng.uniform(100.0, 4000.0)
        a = rng.uniform(0.05, 0.3)
        ph = rng.uniform(0, 2 * np.pi)
        src += a * np.sin(2 * np.pi * f * t + ph)
    am = 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(0.2, 2.0) * t + rng.uniform(0, 2 * np.pi))
    src = src * am + 0.01 * rng.standard_normal(length)
    noise = np.cumsum(rng.standard_normal(length))
    noise -= np.linspace(noise[0], noise[-1], length)          # remove the random-walk drift
    k = 64
    noise = noise - np.convolve(noise, np.ones(k) / k, mode="same")  # pink-ish: kill the sub-audio part
    noise *= 0.1 / max(np.sqrt(np.mean(noise ** 2)), 1e-12)
    return src.astype(np.float32), noise.astype(np.float32), _SNRS[index % len(_SNRS)]


def mix_at_snr(source: np.ndarray, noise: np.ndarray, snr: int):
    """The evaluator's deterministic mixer (dcase_evaluator.py:76-89). Returns (source', mixture)."""
    source = source.copy()
    source_power = np.mean(source ** 2)
    noise_power = np.mean(noise ** 2)
    desired_noise_power = source_power / (10 ** (snr / 10))
    scaling_factor = np.sqrt(desired_noise_power / noise_power)
    noise = noise * scaling_factor
    mixture = source + noise
    max_value = np.max(np.abs(mixture))
    if max_value > 1:
        source *= 0.9 / max_value
        mixture *= 0.9 / max_value
    return source, mixture


def make_mixtures(batch: int, length: int = 160000, first: int = 0, seed: int = SEED):
    """(sources (B,L), mixtures (B,L)) float32."""
    srcs, mixes = [], []
    for i in range(first, first + batch):
        s, n, snr = make_clip(i, length, seed=seed)
        s2, m = mix_at_snr(s, n, snr)
        srcs.append(s2)
        mixes.append(m.astype(np.float32))
    return np.stack(srcs).astype(np.float32), np.stack(mixes).astype(np.float32)


def write_validation_set(root: str, n_clips: int = 8, length: int = 160000, sr: int = 16000, seed: int = SEED,
                         file_rate: int | None = None, channels: int = 1, encoding: str = "f32") -> str:
    """Write `<root>/lass_validation/*.wav` + `<root>/lass_synthetic_validation.csv` in the DCASE layout
    (header `source,noise,snr,caption`; dcase_evaluator.py:42-47,67-71).  Returns the csv path.
    file_rate / channels / encoding ("f32", "pcm16", "pcm32"): the files' own format when it is not mono float32 at `sr` -
    the clips (still `length / sr` seconds) are then generated at `file_rate`, and channel c carries the clip times
    1 - c / (2 * channels).  The defaults write the files this function always wrote."""
    import os
    from . import wavio

    write = {"f32": wavio.write_wav_f32, "pcm16": wavio.write_wav_pcm16, "pcm32": wavio.write_wav_pcm32}[encoding]
    rate = sr if file_rate is None else int(file_rate)
    frames = length if rate == sr else int(round(length * rate / sr))

    def shaped(x):
        if channels == 1:
            return x
        return np.stack([x * np.float32(1.0 - c / (2.0 * channels)) for c in range(channels)], axis=1)

    adir = os.path.join(root, "lass_validation")
    os.makedirs(adir, exist_ok=True)
    rows = ["source,noise,snr,caption"]
    for i in range(n_clips):
        s, n, snr = make_clip(i, frames, rate, seed)
        write(os.path.join(adir, f"src_{i:04d}.wav"), shaped(s), rate)
        write(os.path.join(adir, f"noise_{i:04d}.wav"), shaped(n), rate)
        rows.append(f"src_{i:04d},noise_{i:04d},{snr},synthetic tone cluster {i % 4}")
    csv_path = os.path.join(root, "lass_synthetic_validation.csv")
    with open(csv_path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return csv_path


# regime "peaked": what the flat draws are multiplied by, by key suffix.  Query and key x 8 take the logits q.k/8 from a
# standard deviation of about 0.3 (attention is an average) to about 19 (one key dominates); intermediate and pooler dense
# x 6 take GELU and the pooler's tanh out of their near-linear range.  Powers of two and 6: the products are exact in float32.
CLAP_TEXT_PEAKED_SCALES = (("attention.self.query.weight", 8.0), ("attention.self.key.weight", 8.0),
                           ("intermediate.dense.weight", 6.0), ("text_branch.pooler.dense.weight", 6.0))


def make_clap_text_state_dict(seed: int = SEED + 8, layers: int = 12, regime: str = "flat", vocab: int | None = None,
                              max_positions: int | None = None) -> Dict[str, np.ndarray]:
    """Seeded weights of the CLAP text tower (RoBERTa-base + projection), keyed as lass_amd.clap_text.ClapTextEncoder's
    state_dict (`model.text_branch.*`, `model.text_projection.{0,2}.*`): float32 from numpy PCG64, matrices and biases
    N(0, 0.02), LayerNorm weights 1 + N(0, 0.1), LayerNorm biases N(0, 0.02).  Drawn tensor by tensor in the module's key
    order, so every machine regenerates the same values.  regime "peaked" makes the same draws and scales them by
    CLAP_TEXT_PEAKED_SCALES: attention with one dominant key, GELU and tanh well inside their curved range.  vocab /
    max_positions: the table sizes (roberta-base's by default; other sizes change the stream from the first draw)."""
    from .clap_text import MAX_POSITIONS, VOCAB, param_specs

    if regime not in ("flat", "peaked"):
        raise ValueError(f"regime must be 'flat' or 'peaked', got {regime!r}")
    rng = np.random.Generator(np.random.PCG64(seed))
    sd: Dict[str, np.ndarray] = {}
    for name, shape, kind in param_specs(layers, VOCAB if vocab is None else vocab,
                                         MAX_POSITIONS if max_positions is None else max_positions):
        v = rng.standard_normal(shape, dtype=np.float32)
        sd[name] = (1.0 + 0.1 * v if kind == "g" else 0.02 * v).astype(np.float32)
        if regime == "peaked":
            for suffix, scale in CLAP_TEXT_PEAKED_SCALES:
                if name.endswith(suffix):
                    sd[name] = sd[name] * np.float32(scale)
    return sd


def make_clap_audio_state_dict(seed: int = SEED + 10, depths=(2, 2, 12, 2)) -> Dict[str, np.ndarray]:
    """Seeded weights of the CLAP audio tower (HTSAT + projection), keyed as lass_amd.clap_audio.ClapAudioEncoder's
    state_dict (`model.audio_branch.*`, `model.audio_projection.{0,2}.*`; the derived buffers are left to the module):
    float32 from numpy PCG64, matrices and biases N(0, 0.02), relative-position tables N(0, 0.5), norm weights
    1 + N(0, 0.1), bn0.running_mean -15 + N(0, 3) (dB), bn0.running_var (10 (1 + N(0, 0.1)))^2 > 0.  Drawn tensor by
    tensor in the module's key order, so every machine regenerates the same values."""
    from .clap_audio import param_specs

    rng = np.random.Generator(np.random.PCG64(seed))
    sd: Dict[str, np.ndarray] = {}
    for name, shape, kind in param_specs(depths):
        if kind == "buf":
            continue
        v = rng.standard_normal(shape, dtype=np.float32)
        if name.endswith("relative_position_bias_table"):
            v = 0.5 * v
        elif kind == "g":
            v = 1.0 + 0.1 * v
        elif kind == "m":
            v = -15.0 + 3.0 * v
        elif kind == "v":
            v = (10.0 * (1.0 + 0.1 * v)) ** 2
        else:
            v = 0.02 * v
        sd[name] = v.astype(np.float32)
    return sd


# (samples at 48 kHz, noise level, tones) of the CLAP audio fixture clips: 0.3 s .. exactly 10 s, one length that does
# not divide 480 000, one all-zero clip, one of low level
CLAP_AUDIO_CLIPS = [(14400, 0.1), (100003, 0.1), (48000, 0.0), (240000, 1e-3), (333333, 0.1), (480000, 0.05)]


def make_clap_audio_clip(index: int, seed: int = SEED + 12, rate: int = 48000) -> np.ndarray:
    """Fixture clip `index` (float32): white noise of the clip's level plus three tones of that amplitude - broadband,
    so no mel band of a non-silent clip sits near the log floor."""
    length, level = CLAP_AUDIO_CLIPS[index]
    rng = np.random.Generator(np.random.PCG64(seed + index))
    t = np.arange(length) / rate
    x = level * rng.standard_normal(length)
    for f in rng.uniform(100.0, 9000.0, 3):
        x += level * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return x.astype(np.float32)
