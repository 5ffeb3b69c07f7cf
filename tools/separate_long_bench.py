#!/usr/bin/env python3
"""Long-form separation on one MI355X: a seeded 10-minute recording at 16 kHz through
  (A) ResUNet30.chunk_inference - the default path: windows gathered with torch.cat, eager launches, every result copied to the
      host and stitched in numpy;
  (B) chunk_inference(resident=True) - the same windows and the same result (asserted equal, sample for sample), stored by
      the window kernels into one output row on the device, one copy to the host at the end;
  (C) separate_long(window=160000, context=16000) - equal windows planned by lass_amd.longform, groups of `--max-batch` on the
      same buffers (graph replay from the third group on), the result left on the device;
  (D) separate_long(160000, 16000, fade=8000) - (C) with cross-faded seams: the same forwards, one zero-fill of the output and
      atomic adds over the fade zones.  Gate: median(D) <= median(C) + (max - min of C's runs) + the time of out.zero_(),
      measured here too (Z); a miss is reported and fails the run;
  (E) separate_long_list on `--files` seeded one-minute recordings, against (E0) one separate_long per recording: both and
      their ratio, no gate.
Runs alternate A B C D Z E E0 A B ... in one process after one warm-up round, with torch.cuda.synchronize() around every timed run;
the figure is the median of each, with the spread of its runs.  Prints seconds of audio per second of wall time and the
ratios to (A), then the same as one JSON line per compute mode."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lass_amd import longform, synthetic  # noqa: E402
from lass_amd.resunet import ResUNet30  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--max-batch", type=int, default=16)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fade", type=int, default=8000)
ap.add_argument("--files", type=int, default=10, help="one-minute recordings of rows (E) and (E0); 0 = skip them")
ap.add_argument("--compute-dtype", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16", "bf16x3"])
args = ap.parse_args()

SR, DEV = 16000, "cuda:0"
total = int(args.minutes * 60 * SR)
rng = np.random.default_rng(20241019)
rec = torch.from_numpy(rng.standard_normal(total).astype(np.float32) * 0.1).to(DEV)
cond = torch.from_numpy(synthetic.make_condition(1)).to(DEV)
inp = {"mixture": rec[None, None, :], "condition": cond}
sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict().items()}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


files = [torch.from_numpy(rng.standard_normal(60 * SR).astype(np.float32) * 0.1).to(DEV) for _ in range(args.files)]
file_conds = torch.from_numpy(synthetic.make_condition(args.files)).to(DEV) if args.files else None
zeroed = torch.empty_like(rec)

mismatches = []
for mode in args.compute_dtype:
    model = ResUNet30(1, 1, 512)
    model.load_state_dict(sd)
    model = model.to(DEV).eval().set_compute_dtype(mode)
    legs = {
        "A chunk_inference (default)": lambda: model.chunk_inference(inp, max_batch=args.max_batch),
        "B chunk_inference(resident=True)": lambda: model.chunk_inference(inp, max_batch=args.max_batch, resident=True),
        "C separate_long(160000, 16000)": lambda: model.separate_long(rec, cond, window=160000, context=16000, max_batch=args.max_batch),
        "D separate_long(..., fade=%d)" % args.fade: lambda: model.separate_long(rec, cond, window=160000, context=16000,
                                                                                 max_batch=args.max_batch, fade=args.fade),
        "Z out.zero_()": lambda: zeroed.zero_(),
    }
    if args.files:
        legs["E separate_long_list, %d x 60 s" % args.files] = lambda: model.separate_long_list(
            files, file_conds, window=160000, context=16000, max_batch=args.max_batch)
        legs["E0 separate_long x %d" % args.files] = lambda: [
            model.separate_long(f, file_conds[i], window=160000, context=16000, max_batch=args.max_batch) for i, f in enumerate(files)]
    warm = {name: fn() for name, fn in legs.items()}
    torch.cuda.synchronize()
    a, b = warm["A chunk_inference (default)"], warm["B chunk_inference(resident=True)"]
    assert a.shape == b.shape == (1, total)
    if not np.array_equal(a, b):  # reported after this mode's figures
        mismatches.append(f"{mode}: resident chunk_inference differs from the default path, max |difference| {np.abs(a - b).max():.3e}")
    assert bool(torch.isfinite(warm["C separate_long(160000, 16000)"]).all())
    name_d = "D separate_long(..., fade=%d)" % args.fade
    assert bool(torch.isfinite(warm[name_d]).all())
    if args.files and mode == "f32":
        for x, y in zip(warm["E separate_long_list, %d x 60 s" % args.files], warm["E0 separate_long x %d" % args.files]):
            if not torch.equal(x, y):
                mismatches.append(f"{mode}: separate_long_list differs from separate_long of the same recording")
                break
    times = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            times[name].append(timed(fn)[0])
    _, ranges = longform.reference_plan(total, 32000, 96000, 32000)
    plan = longform.plan_windows(total, 160000, 16000)
    print(f"{total / SR:.0f} s of audio at {SR} Hz, {mode}, max_batch {args.max_batch}: chunk_inference {len(ranges)} windows "
          f"(96000 kept of 160000), separate_long {len(plan)} windows (128000 kept of 160000), graph stats {model.engine.graph_stats()}")
    med = {name: statistics.median(t) for name, t in times.items()}
    base = med["A chunk_inference (default)"]
    for name, t in times.items():
        print(f"  {name:34s}: {total / SR / med[name]:8.1f} x real time, median {1e3 * med[name]:8.1f} ms, runs "
              f"{[round(1e3 * x, 1) for x in t]} ms, {base / med[name]:.2f} x (A)")
    print(json.dumps({"compute_dtype": mode, "seconds": total / SR, "max_batch": args.max_batch,
                      "default_ms": 1e3 * base, "default_runs_ms": [1e3 * x for x in times["A chunk_inference (default)"]],
                      "resident_ms": 1e3 * med["B chunk_inference(resident=True)"],
                      "separate_long_ms": 1e3 * med["C separate_long(160000, 16000)"],
                      "resident_over_default": base / med["B chunk_inference(resident=True)"],
                      "separate_long_over_default": base / med["C separate_long(160000, 16000)"],
                      "separate_long_runs_ms": [1e3 * x for x in times["C separate_long(160000, 16000)"]],
                      "faded_ms": 1e3 * med[name_d], "faded_runs_ms": [1e3 * x for x in times[name_d]], "fade": args.fade,
                      "zero_fill_ms": 1e3 * med["Z out.zero_()"],
                      **({"list_ms": 1e3 * med["E separate_long_list, %d x 60 s" % args.files],
                          "one_by_one_ms": 1e3 * med["E0 separate_long x %d" % args.files],
                          "one_by_one_over_list": med["E0 separate_long x %d" % args.files] / med["E separate_long_list, %d x 60 s" % args.files],
                          "files": args.files} if args.files else {})}))
    c_runs = times["C separate_long(160000, 16000)"]
    bound = med["C separate_long(160000, 16000)"] + (max(c_runs) - min(c_runs)) + med["Z out.zero_()"]
    verdict = "holds" if med[name_d] <= bound else "MISSED"
    print(f"  gate (D) <= (C) + spread of (C) + zero-fill: {1e3 * med[name_d]:.2f} ms <= {1e3 * bound:.2f} ms {verdict}")
    if med[name_d] > bound:
        mismatches.append(f"{mode}: (D) {1e3 * med[name_d]:.2f} ms exceeds its gate {1e3 * bound:.2f} ms")
    del model, legs, warm
    import gc
    gc.collect()
if mismatches:
    sys.exit("\n".join(mismatches))
