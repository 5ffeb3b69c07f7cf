#!/usr/bin/env python3
"""Ragged-batch throughput on one MI355X: a seeded set of 256 clips whose lengths are drawn uniformly from 5 to 15 s at
16 kHz, separated
  (a) by ResUNet30.separate_list - clips sorted into 32-frame buckets, up to 16 of a bucket per lass_separate_ragged call;
  (b) the way DCASEEvaluator._run_generic batches without ragged=True: consecutive clips of IDENTICAL length share a forward,
      which on such a set means one batch-1 forward per clip.
Both read the same device-resident clips in the same process, after a warm-up pass each, with torch.cuda.synchronize() around
every timed pass; the figure is the median of 5 passes.  Prints the bucket occupancy of the set, clips/s of both and their
ratio, then the same as one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lass_amd import ragged, synthetic  # noqa: E402
from lass_amd.resunet import ResUNet30  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=256)
ap.add_argument("--max-batch", type=int, default=16)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--compute-dtype", default="f32", choices=["f32", "bf16", "bf16x3"])
args = ap.parse_args()

SR, DEV = 16000, "cuda:0"
rng = np.random.default_rng(20240919)
lengths = [int(n) for n in rng.integers(5 * SR, 15 * SR + 1, size=args.clips)]
clips = [torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 0.1).to(DEV) for n in lengths]
cond = torch.from_numpy(synthetic.make_condition(args.clips)).to(DEV)

model = ResUNet30(1, 1, 512)
model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict().items()})
model = model.to(DEV).eval().set_compute_dtype(args.compute_dtype)

plan = ragged.plan_batches(lengths, args.max_batch)
buckets = {}
for n in lengths:
    buckets[ragged.bucket_of(n)] = buckets.get(ragged.bucket_of(n), 0) + 1
sizes = [len(idx) for idx, _ in plan]
pad = sum(len(idx) * row for idx, row in plan) / sum(lengths) - 1.0


def run_list():
    return model.separate_list(clips, cond, max_batch=args.max_batch)


def run_grouped():
    """_run_generic's grouping: a batch is a run of consecutive clips of identical length (at most max_batch)."""
    outs, i = [], 0
    while i < len(clips):
        j = i + 1
        while j < len(clips) and j - i < args.max_batch and lengths[j] == lengths[i]:
            j += 1
        mix = torch.stack(clips[i:j])[:, None, :]
        outs.append(model({"mixture": mix, "condition": cond[i:j]})["waveform"])
        i = j
    return outs


def rate(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return args.clips / statistics.median(times), [args.clips / t for t in times]


groups = 0
i = 0
while i < len(clips):
    j = i + 1
    while j < len(clips) and j - i < args.max_batch and lengths[j] == lengths[i]:
        j += 1
    groups, i = groups + 1, j

print(f"{args.clips} clips, {min(lengths) / SR:.2f} .. {max(lengths) / SR:.2f} s, {sum(lengths) / SR:.0f} s of audio, {args.compute_dtype}")
print(f"buckets (padded frames: clips): {dict(sorted(buckets.items()))}")
print(f"ragged plan: {len(plan)} batches over {len(buckets)} buckets, mean {np.mean(sizes):.2f} clips per batch "
      f"(min {min(sizes)}, max {max(sizes)}), {100 * pad:.1f} % padded samples; grouped plan: {groups} batches")
a, a_all = rate(run_list)
b, b_all = rate(run_grouped)
print(f"(a) separate_list                 : {a:8.1f} clips/s   passes {[round(x, 1) for x in a_all]}")
print(f"(b) consecutive-equal-length groups: {b:8.1f} clips/s   passes {[round(x, 1) for x in b_all]}")
print(f"ratio (a) / (b): {a / b:.2f}")
print(json.dumps({"clips": args.clips, "compute_dtype": args.compute_dtype, "buckets": len(buckets), "ragged_batches": len(plan),
                  "mean_batch": float(np.mean(sizes)), "grouped_batches": groups, "separate_list_clips_per_s": a,
                  "grouped_clips_per_s": b, "ratio": a / b}))
