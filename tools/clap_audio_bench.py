"""CLAP audio encoder timing on one MI355X: ms per `ClapAudioEncoder.encode_wave48k` call for B = 1 and B = 16 ten-second
clips (depths 2-2-12-2, seeded weights), the executed GFLOP of the tower, TFLOP/s and its fraction of the 157.3 TF f32
MFMA peak, with the front end and the tower apart.  The front end (log-mel, patch embedding; with it the three
PatchMergings, the final norm and the head, which do not scale with depth) is the depth-0 intercept of two shallow runs:
t(1,1,1,1) - (t(2,2,2,2) - t(1,1,1,1)); the tower is the full call minus that.  When transformers imports,
transformers.ClapAudioModel of the same shape (random weights: timing only) on PyTorch-ROCm, f32, fed the device's own
log-mel features, is timed as the comparison.

    python tools/clap_audio_bench.py [--iters 20] [--warmup 5]

Each leg runs in a child process under `timeout -k 10`; a failing leg ends the run.  One JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEPTHS, BATCHES, PEAK_TF = (2, 2, 12, 2), (1, 16), 157.3


def tower_gflop(b: int, depths=DEPTHS) -> float:
    """FLOP the tower executes per call: per token and block the QKV / projection / MLP GEMMs and the two window products
    (64 keys), PatchMerging's reduction, the 4x4 patch convolution and the head."""
    f, tokens, C = 2 * 4096 * 16 * 128, 4096, 128
    for i, d in enumerate(depths):
        f += d * tokens * 2 * (3 * C * C + C * C + 8 * C * C + 2 * 64 * C)
        if i < len(depths) - 1:
            tokens //= 4
            f += tokens * 2 * 4 * C * 2 * C
            C *= 2
    return b * (f + 2 * (C * 512 + 512 * 512)) / 1e9


def _time(fn, iters: int, warmup: int) -> float:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _encoder(depths):
    import torch
    from lass_amd import synthetic
    from lass_amd.clap_audio import ClapAudioEncoder
    enc = ClapAudioEncoder(depths=depths)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_clap_audio_state_dict(depths=depths).items()}, strict=False)
    return enc.to("cuda:0")


def _waves(b: int):
    import numpy as np
    import torch
    from lass_amd import synthetic
    x = synthetic.make_clap_audio_clip(5)
    return torch.from_numpy(np.stack([np.roll(x, 1000 * i) for i in range(b)])).to("cuda:0")


def leg_hip(iters: int, warmup: int):
    encs = {d: _encoder(d) for d in (DEPTHS, (1, 1, 1, 1), (2, 2, 2, 2))}
    for b in BATCHES:
        w = _waves(b)
        ms = {d: _time(lambda: e.encode_wave48k(w), iters, warmup) for d, e in encs.items()}
        front = 2 * ms[(1, 1, 1, 1)] - ms[(2, 2, 2, 2)]  # depth-0 intercept: what does not scale with the block count
        tower = ms[DEPTHS] - front
        gf = tower_gflop(b)
        print(json.dumps({"leg": "hip", "B": b, "ms": round(ms[DEPTHS], 4), "ms_depths_1111": round(ms[(1, 1, 1, 1)], 4),
                          "ms_depths_2222": round(ms[(2, 2, 2, 2)], 4), "front_end_ms": round(front, 4),
                          "tower_ms": round(tower, 4), "tower_gflop": round(gf, 2), "tflops_whole_call": round(gf / ms[DEPTHS], 2),
                          "tflops_tower": round(gf / tower, 2), "frac_f32_mfma_peak_whole_call": round(gf / ms[DEPTHS] / PEAK_TF, 4),
                          "frac_f32_mfma_peak_tower": round(gf / tower / PEAK_TF, 4)}), flush=True)


def leg_torch(iters: int, warmup: int):
    import torch
    try:
        from transformers import ClapAudioConfig, ClapAudioModel  # noqa: F401
    except ImportError:
        print(json.dumps({"leg": "torch", "skipped": "transformers does not import"}), flush=True)
        return
    m = ClapAudioModel(ClapAudioConfig(patch_embeds_hidden_size=128, depths=list(DEPTHS), hidden_size=1024,
                                       enable_fusion=False)).eval().to("cuda:0")
    enc = _encoder((1, 1, 1, 1))
    for b in BATCHES:
        feats = enc.encode_wave48k(_waves(b), return_taps=True)[1]["logmel"][:, None].contiguous()
        with torch.no_grad():
            ms = _time(lambda: m(input_features=feats).pooler_output, iters, warmup)
        print(json.dumps({"leg": "torch", "B": b, "ms": round(ms, 4), "note": "tower only, random weights, device log-mel"}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--leg", choices=["hip", "torch"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        (leg_hip if a.leg == "hip" else leg_torch)(a.iters, a.warmup)
        return 0
    for leg in ("hip", "torch"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--iters", str(a.iters), "--warmup", str(a.warmup)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(json.dumps({"leg": leg, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
