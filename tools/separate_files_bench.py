"""File in, file out on one MI355X: `pipeline.separate_files` against the same jobs done with the pieces the package had before
it, on 32 seeded one-minute 44.1 kHz stereo PCM16 files (synthetic ResUNet30 weights, 16 kHz, f32 unless --compute-dtype).

    python tools/separate_files_bench.py [--files 32] [--seconds 60] [--reps 5] [--compute-dtype f32] [--loudness [--true-peak] [--meter] [--limiter]]
    python tools/separate_files_bench.py --remix DB
    python tools/separate_files_bench.py --channels linked

Leg A: `separate_files(channels="each")` - decode, resample, separate, resample back, encode and interleave on the device.
Leg B: host decode + de-interleave + `wavio._resample` (scipy, float64), `separate_long_list`, `.cpu()`, host `_resample` back
and `wavio.write_wav_pcm16`.  The legs alternate A B A B ..., `--reps` runs each, every run in a child process of its own under
`timeout -k 10` (a failing run ends the whole); a child separates one file as a warm-up before its timed pass.  Prints one JSON
line per run and a summary line: median seconds, files/s and x real time per leg, and leg A's time split from one further run
with `profile=` (which synchronises after every stage, so its parts add up to more than an unprofiled pass).

--loudness: leg A against leg L, the same call with `loudness=-23.0, peak_ceiling_db=-1.0` (meter, peak and gain on the device, per
file), alternating A L A L ...; no leg B, and the profiled run is leg L's, whose split has the `level` stage.  Leg A with this flag
is the number to hold against the same tool's leg A on the parent commit: it launches the same kernels.

--true-peak / --meter (with --loudness): a third leg R, leg L's call with `peak="true"` and / or `meter=True` (EBU R 128: the
ceiling holds the true peak; loudness range and the two maxima beside the loudness), alternating A L R A L R ...; the profiled run
is then leg R's.  Leg L is the number to hold against the parent's leg L; R over L is what the two arguments add.

--limiter (with --loudness): one more leg M, the call of the leg before it (R, or L without the two flags above) with
`limiter=True` - the look-ahead limiter in front of the level stage - alternating ... M ...; the profiled run is then leg M's, and
it also prints, per file, the limiter's reduction beside the static trim the level stage still applied ("gain_db"): the
limiter's own overshoot.  The legs before M launch what they launched without the flag.

--remix DB: leg A against leg X, the same call with `target_gain_db=DB` (the remix: the raw rows stay on the device and the encode
reads them as its dry source), alternating A X A X ...; no leg B, and BOTH legs are profiled once at the end, so that the two
`encode` stages stand side by side.

--channels linked: leg A against leg K, the same call with `channels="linked"` (one mask per file from its mono down-mix, applied
to both channels: one network pass per file instead of two), alternating A K A K ...; no leg B, and BOTH legs are profiled once at
the end, so that the two `separate` stages stand side by side.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, FILE_RATE, CHANNELS = 16000, 44100, 2


def make_files(d: str, n: int, seconds: float):
    import numpy as np
    from lass_amd import wavio
    frames = int(seconds * FILE_RATE)
    t = np.arange(frames)[:, None] / FILE_RATE
    for i in range(n):
        rng = np.random.Generator(np.random.PCG64([24, i]))
        x = 0.1 * rng.standard_normal((frames, CHANNELS)) + 0.3 * np.sin(2 * np.pi * rng.uniform(100, 4000, CHANNELS) * t)
        wavio.write_wav_pcm16(os.path.join(d, f"in_{i:03d}.wav"), x.astype(np.float32), FILE_RATE)


def _model(mode: str):
    import numpy as np
    import torch
    from lass_amd import synthetic
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict().items()})
    return AudioSep(ss_model=m.to("cuda:0").eval().set_compute_dtype(mode), query_encoder=PrecomputedQueryEncoder())


def _jobs(d: str, n: int, tag: str):
    return [(os.path.join(d, f"in_{i:03d}.wav"), f"caption {i % 4}", os.path.join(d, f"out_{tag}_{i:03d}.wav")) for i in range(n)]


def host_pieces(model, jobs):
    """Leg B: what a caller did before `separate_files` existed."""
    import numpy as np
    import torch
    from lass_amd import wavio
    captions = sorted({q for _, q, _ in jobs})
    emb = model.query_encoder.get_query_embed(modality="text", text=captions, device="cuda:0")
    planes, conds, metas = [], [], []
    for path, q, _ in jobs:
        enc, nch, rate, frames, offset = wavio.wav_info(path)
        with open(path, "rb") as f:
            f.seek(offset)
            x = np.frombuffer(f.read(frames * nch * 2), dtype="<i2").astype(np.float32).reshape(frames, nch) / 32768.0
        for c in range(nch):
            planes.append(torch.from_numpy(wavio._resample(x[:, c], rate, SR)).to("cuda:0"))
            conds.append(emb[captions.index(q)])
        metas.append((nch, rate, frames))
    seps = model.ss_model.separate_long_list(planes, torch.stack(conds))
    at = 0
    for (_, _, out), (nch, rate, frames) in zip(jobs, metas):
        y = np.stack([wavio._resample(s.cpu().numpy(), SR, rate)[:frames] for s in seps[at:at + nch]], axis=1)
        at += nch
        wavio.write_wav_pcm16(out, y, rate)


def leg(name: str, d: str, n: int, mode: str, true_peak: bool = False, meter: bool = False, remix_db=None):
    """One run of leg `name` (A, B, L, R, M, X or K, or one of them with "-profile") in this process."""
    import torch
    from lass_amd import pipeline
    model = _model(mode)
    profile = {} if name.endswith("-profile") else None
    level = dict(loudness=-23.0, peak_ceiling_db=-1.0) if name[0] in "LRM" else {}
    if name[0] in "RM":
        level.update(peak="true" if true_peak else "sample", meter=meter)
    if name.startswith("M"):
        level.update(limiter=True)
    if name.startswith("X"):
        level.update(target_gain_db=remix_db)
    records = []

    def run(jobs, profile=None):
        if name == "B":
            host_pieces(model, jobs)
        else:
            records[:] = pipeline.separate_files(model, jobs, SR, channels="linked" if name.startswith("K") else "each", profile=profile,
                                                 **level)

    run(_jobs(d, 1, "warm"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(_jobs(d, n, name), profile)
    torch.cuda.synchronize()
    res = {"leg": name, "seconds": round(time.perf_counter() - t0, 4)}
    if profile is not None:
        res["split_s"] = {k: round(v, 4) for k, v in profile.items()}
        if name.startswith("M"):
            keys = ("loudness_in", "limiter_gain_db", "limiter_reduction_db", "limiter_frames", "loudness_out", "gain_db")
            res["per_file"] = [{k: round(r[k], 4) for k in keys} for r in records]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compute-dtype", default="f32")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per run")
    ap.add_argument("--loudness", action="store_true", help="leg A against leg L (loudness=-23, peak_ceiling_db=-1) instead of leg B")
    ap.add_argument("--true-peak", action="store_true", help="with --loudness: a leg R with peak=\"true\"")
    ap.add_argument("--meter", action="store_true", help="with --loudness: a leg R with meter=True")
    ap.add_argument("--limiter", action="store_true", help="with --loudness: a leg M, the last leg's call with limiter=True")
    ap.add_argument("--remix", type=float, metavar="DB", help="leg A against leg X (target_gain_db=DB) instead of leg B")
    ap.add_argument("--channels", choices=["each", "linked"], default="each", help="linked: leg A against leg K (channels=\"linked\") instead of leg B")
    ap.add_argument("--leg", choices=["A", "B", "L", "R", "M", "X", "K", "A-profile", "L-profile", "R-profile", "M-profile", "X-profile",
                                      "K-profile"])
    ap.add_argument("--dir")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.dir, a.files, a.compute_dtype, a.true_peak, a.meter, a.remix)
        return 0
    r128 = a.true_peak or a.meter
    if (r128 or a.limiter) and not a.loudness:
        ap.error("--true-peak, --meter and --limiter go with --loudness")
    if a.remix is not None and a.loudness:
        ap.error("--remix stands alone: a remix is not levelled")
    both = a.remix is not None or a.channels == "linked"  # both legs are profiled at the end
    if a.channels == "linked" and (a.loudness or a.remix is not None):
        ap.error("--channels linked stands alone")
    with tempfile.TemporaryDirectory() as d:
        make_files(d, a.files, a.seconds)
        other = "L" if a.loudness else "X" if a.remix is not None else "K" if a.channels == "linked" else "B"
        legs = ["A", other] + (["R"] if r128 else []) + (["M"] if a.limiter else [])
        prof = legs[-1] + "-profile" if a.loudness or both else "A-profile"
        times = {name: [] for name in legs}
        split = per_file = a_split = None
        for name in legs * a.reps + (["A-profile"] if both else []) + [prof]:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", name, "--dir", d,
                   "--files", str(a.files), "--compute-dtype", a.compute_dtype] + ["--true-peak"] * a.true_peak + ["--meter"] * a.meter
            if a.remix is not None:
                cmd += [f"--remix={a.remix}"]
            pr = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(pr.stdout)
            sys.stdout.flush()
            if pr.returncode != 0:
                print(json.dumps({"leg": name, "failed": pr.returncode}), flush=True)
                return pr.returncode
            res = json.loads(pr.stdout.strip().split("\n")[-1])
            if name == prof:
                split, per_file = res["split_s"], res.get("per_file")
            elif name == "A-profile":
                a_split = res["split_s"]
            else:
                times[name].append(res["seconds"])
        audio = a.files * a.seconds
        summary = {"files": a.files, "seconds_each": a.seconds, "compute_dtype": a.compute_dtype, prof[0] + "_split_s": split}
        if a.remix is not None:
            summary.update(remix_db=a.remix, A_split_s=a_split)
        if a.channels == "linked":
            summary.update(channels="linked", A_split_s=a_split)
        for name, ts in times.items():
            med = statistics.median(ts)
            summary[name] = {"median_s": round(med, 4), "files_per_s": round(a.files / med, 2), "x_real_time": round(audio / med, 1),
                             "runs_s": ts}
        summary[other + "_over_A"] = round(summary[other]["median_s"] / summary["A"]["median_s"], 2)
        if r128:
            summary["R"]["true_peak"], summary["R"]["meter"] = a.true_peak, a.meter
            summary["R_over_L"] = round(summary["R"]["median_s"] / summary["L"]["median_s"], 2)
        if a.limiter:
            summary["M_over_" + legs[-2]] = round(summary["M"]["median_s"] / summary[legs[-2]]["median_s"], 2)
            summary["M_per_file"] = per_file
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
