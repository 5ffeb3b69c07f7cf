"""`lass_decode_resample` timing on one MI355X: ms per launch and GB/s over (raw bytes in + 4 * L_out bytes out) for B = 16
ten-second clips of every pair of the rate table, as PCM16 mono and as float32 stereo.  The kernel is bound by neither: per
output it makes ceil(n_taps / up) LDS-fed fmaf steps (21 ... 61), so the GB/s column says how far from a pure copy it sits.

    python tools/decode_resample_bench.py [--iters 50] [--warmup 10]

Each leg (one encoding) runs in a child process under `timeout -k 10`; a failing leg ends the run.  One JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATE_TABLE = [(32000, 16000), (48000, 16000), (44100, 16000), (22050, 16000), (24000, 16000), (8000, 16000), (11025, 16000),
              (44100, 32000)]
LEGS = {"pcm16_mono": ("pcm16", 1), "f32_stereo": ("f32", 2)}
B = 16


def leg(name: str, iters: int, warmup: int):
    import torch
    from lass_amd import resample as rs
    from lass_amd.engine import get_engine
    enc, nch = LEGS[name]
    eng = get_engine("cuda:0")
    for rate_in, rate_out in RATE_TABLE:
        frames = 10 * rate_in
        up, down = rs.ratio(rate_in, rate_out)
        row = frames * nch * rs.SAMPLE_BYTES[enc]
        g = torch.Generator(device="cuda:0").manual_seed(rate_in)
        if enc == "pcm16":
            raw = torch.randint(-8000, 8000, (B, frames * nch), dtype=torch.int16, device="cuda:0", generator=g).view(torch.uint8)
        else:
            raw = (0.25 * torch.randn(B, frames * nch, device="cuda:0", generator=g)).view(torch.uint8)
        out = torch.empty(B, rs.out_len(frames, up, down), dtype=torch.float32, device="cuda:0")
        fn = lambda: eng.decode_resample(raw, frames, nch, enc, rate_in, rate_out, out=out)  # noqa: E731
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / iters
        nbytes = B * (row + 4 * out.shape[1])
        print(json.dumps({"leg": name, "rate_in": rate_in, "rate_out": rate_out, "up": up, "down": down, "taps": rs.n_taps(up, down),
                          "B": B, "ms_per_launch": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1),
                          "clips_per_s": round(B / ms * 1e3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--timeout", type=int, default=180, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.iters, a.warmup)
        return 0
    for name in LEGS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--iters", str(a.iters), "--warmup", str(a.warmup)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(json.dumps({"leg": name, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
