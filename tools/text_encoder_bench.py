"""CLAP text encoder timing on one MI355X: ms per `ClapTextEncoder.encode_ids` call for N = 16 captions whose real
length is S_real in {8, 24, 77, 512}, padded to 512 as the reference tokenizes them (12 layers, seeded weights), with
the executed GFLOP, the fraction of the 157.3 TF f32 MFMA peak and the weight bytes against 8 TB/s.  When transformers
imports, the same weights in transformers.RobertaModel on PyTorch-ROCm (f32, eager attention, every call at the full
512 padding, plus the CLAP head) are timed as the comparison.

    python tools/text_encoder_bench.py [--iters 20] [--warmup 5]

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

N, S_PAD, LAYERS = 16, 512, 12
S_REAL = (8, 24, 77, 512)
PEAK_TF, HBM_TBS = 157.3, 8.0
HID, FFN, PROJ = 768, 3072, 512


def executed_gflop(n: int, s_real: int, layers: int = LAYERS) -> float:
    """FLOP the packed path executes: per token and layer the QKV / output / FFN GEMMs, per caption QK^T and PV over
    its real tokens, plus the head (pooler + projection) per caption."""
    tok = 2 * (HID * 3 * HID + HID * HID + 2 * HID * FFN)
    attn = 2 * 2 * s_real * s_real * HID
    head = 2 * (HID * HID + HID * PROJ + PROJ * PROJ)
    return (layers * (n * s_real * tok + n * attn) + n * head) / 1e9


def weight_bytes(layers: int = LAYERS) -> int:
    return 4 * (layers * (HID * 3 * HID + HID * HID + 2 * HID * FFN) + HID * HID + HID * PROJ + PROJ * PROJ)


def _inputs(s_real: int):
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(s_real))
    ids = np.ones((N, S_PAD), dtype=np.int64)
    mask = np.zeros((N, S_PAD), dtype=np.int64)
    ids[:, 0], ids[:, 1:s_real - 1], ids[:, s_real - 1] = 0, rng.integers(3, 50265, (N, s_real - 2)), 2
    mask[:, :s_real] = 1
    return ids, mask


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


def leg_hip(iters: int, warmup: int):
    import torch
    from lass_amd import synthetic
    from lass_amd.clap_text import ClapTextEncoder
    enc = ClapTextEncoder(layers=LAYERS)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_clap_text_state_dict(layers=LAYERS).items()})
    enc = enc.to("cuda:0")
    for s in S_REAL:
        ids, mask = _inputs(s)
        ms = _time(lambda: enc.encode_ids(ids, mask), iters, warmup)
        gf = executed_gflop(N, s)
        print(json.dumps({"leg": "hip", "N": N, "S_pad": S_PAD, "S_real": s, "ms": round(ms, 4), "gflop": round(gf, 2),
                          "tflops": round(gf / ms, 2), "frac_f32_mfma_peak": round(gf / ms / PEAK_TF, 4),
                          "weight_MB": round(weight_bytes() / 1e6, 1),
                          "weight_read_floor_ms": round(weight_bytes() / (HBM_TBS * 1e9), 4)}), flush=True)


def leg_torch(iters: int, warmup: int):
    import torch
    try:
        import transformers  # noqa: F401
    except ImportError:
        print(json.dumps({"leg": "torch", "skipped": "transformers does not import"}), flush=True)
        return
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_clap_golden import roberta
    from lass_amd import synthetic
    sd = synthetic.make_clap_text_state_dict(layers=LAYERS)
    m = roberta(LAYERS)
    pre = "model.text_branch."
    m.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)}, strict=False)
    m = m.to("cuda:0")
    p = {k: torch.from_numpy(sd["model.text_projection." + k]).cuda() for k in ("0.weight", "0.bias", "2.weight", "2.bias")}

    @torch.no_grad()
    def run(ids, mask):
        x = m(input_ids=ids, attention_mask=mask).pooler_output
        x = torch.relu(x @ p["0.weight"].T + p["0.bias"]) @ p["2.weight"].T + p["2.bias"]
        return torch.nn.functional.normalize(x, dim=-1)

    for s in S_REAL:
        ids, mask = (torch.from_numpy(a) for a in _inputs(s))
        ms = _time(lambda: run(ids.cuda(), mask.cuda()), iters, warmup)
        print(json.dumps({"leg": "torch", "N": N, "S_pad": S_PAD, "S_real": s, "ms": round(ms, 4),
                          "gflop_padded": round(executed_gflop(N, S_PAD), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--leg", choices=["hip", "torch"])
    ap.add_argument("--timeout", type=int, default=600, help="seconds per leg")
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
