#!/usr/bin/env python3
"""Throughput of ResUNet30 at one STFT geometry on one MI355X: B clips of L samples (default: 16 clips of 10 s at 32 kHz,
n_fft 2048 / hop 320) through ResUNet30.separate_into on the same buffers, so that from the third call on a call is one replayed
hipGraph (two overlapping half-batches at B >= 8).  Per compute mode: clips/s as the median of `--repeats` windows of `--steps`
calls, each window between two torch.cuda.synchronize(), after `--warmup` calls; then, with `--profile`, the per-class times
of lass_set_profiling over `--steps` eager calls (a profiled context neither replays nor splits: the classes say where the time
goes, their sum is not the replayed call's time).  `--istft` times the two ends of the network alone (front end, iSTFT) with
device events - the measurement behind the iSTFT span constant of stft.hip: run it once per build.
`--n-fft 1024 --hop 160 --length 160000` gives the 16 kHz figures to hold the 32 kHz ones against.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lass_amd import arch, synthetic  # noqa: E402
from lass_amd.resunet import ResUNet30  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-fft", type=int, default=2048)
ap.add_argument("--hop", type=int, default=320)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--length", type=int, default=320000)
ap.add_argument("--compute-dtype", nargs="+", default=["f32", "bf16x3", "bf16"], choices=["f32", "bf16", "bf16x3"])
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--istft", action="store_true", help="time front end and iSTFT alone instead of the model")
ap.add_argument("--label", default="")
args = ap.parse_args()

DEV = "cuda:0"
B, L = args.batch, args.length
T = arch.frames_for(L, args.hop)
gen = torch.Generator().manual_seed(20241019)
mix = ((torch.rand(B, L, generator=gen) * 2 - 1) * 0.5).to(DEV)
cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
out = torch.empty_like(mix)

model = ResUNet30(1, 1, 512, n_fft=args.n_fft, hop=args.hop)
model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict(n_fft=args.n_fft).items()})
model = model.to(DEV).eval()
result = {"label": args.label, "n_fft": args.n_fft, "hop": args.hop, "B": B, "L": L, "frames": T,
          "padded_frames": arch.padded_frames(T)}
print(f"{args.label} n_fft {args.n_fft} hop {args.hop}: B = {B}, L = {L} ({T} frames, {arch.padded_frames(T)} padded)", flush=True)


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(args.repeats):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times), times


if args.istft:
    eng = model.engine
    mag, cos, sin, x0 = eng.front_end(mix)
    bufs = (mag, cos, sin, x0)
    re, im = (mag * cos).contiguous(), (mag * sin).contiguous()
    fe, fe_all = event_ms(lambda: eng.front_end(mix, out=bufs), 20)
    it, it_all = event_ms(lambda: eng.istft_nfft(re, im, L, args.n_fft, args.n_fft), 20)
    back = float((eng.istft_nfft(re, im, L, args.n_fft, args.n_fft) - mix).abs().max())
    print(f"front end {fe:.3f} ms {[round(t, 3) for t in fe_all]}   iSTFT {it:.3f} ms {[round(t, 3) for t in it_all]}   "
          f"STFT -> iSTFT max error {back:.2e}", flush=True)
    result.update(front_end_ms=fe, istft_ms=it, istft_ms_all=it_all, roundtrip_max_error=back)
    print(json.dumps(result))
    sys.exit(0)

result["modes"] = {}
for mode in args.compute_dtype:
    model.set_compute_dtype(mode)
    eng = model.engine
    for _ in range(max(args.warmup, 3)):   # the third call of a key captures its graph
        model.separate_into(mix, cond, out)
    torch.cuda.synchronize()
    _, cap0, rep0 = eng.graph_stats()
    rates = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.separate_into(mix, cond, out)
        torch.cuda.synchronize()
        rates.append(B * args.steps / (time.perf_counter() - t0))
    _, cap1, rep1 = eng.graph_stats()
    entry = {"clips_per_s": statistics.median(rates), "windows": rates, "replays": rep1 - rep0,
             "finite": bool(torch.isfinite(out).all()), "out_rms": float(out.pow(2).mean().sqrt())}
    print(f"{mode:7s} {entry['clips_per_s']:8.1f} clips/s   windows {[round(r, 1) for r in rates]}   "
          f"{rep1 - rep0} graph replays of {args.repeats * args.steps} calls", flush=True)
    if args.profile:
        eng.set_profiling(True)
        model.separate_into(mix, cond, out)
        torch.cuda.synchronize()
        eng.profile(reset=True)
        for _ in range(args.steps):
            model.separate_into(mix, cond, out)
        torch.cuda.synchronize()
        prof = eng.profile(reset=True)
        eng.set_profiling(False)
        entry["profile_ms_per_call"] = {k: ms / args.steps for k, (ms, _n) in prof.items()}
        entry["profile_launches_per_call"] = {k: n / args.steps for k, (_ms, n) in prof.items()}
        total = sum(entry["profile_ms_per_call"].values())
        print("        " + "  ".join(f"{k} {v:.2f}" for k, v in entry["profile_ms_per_call"].items()) + f"  | sum {total:.2f} ms", flush=True)
    result["modes"][mode] = entry
print(json.dumps(result))
