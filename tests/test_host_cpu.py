"""CPU-side tests: C-ABI library loads and exports every symbol of include/lass_hip.h (no compute without a GPU),
host logic (sharding, gather over gloo with world_size 2, wav I/O, metrics dB math, module/state_dict mirror)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported():
    import __graft_entry__ as g
    g.build()
    from lass_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    declared = set(re.findall(r"\b(lass_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert declared == bound, (declared ^ bound)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.lass_version() >= 100


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_fails_loudly_without_gpu():
    from lass_amd import _lib
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    with pytest.raises(_lib.LassError):
        m({"mixture": torch.zeros(1, 1, 16000), "condition": torch.zeros(1, 512)})
    import ctypes
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.lass_create(ctypes.byref(h), 0) < 0
    assert b"no HIP device" in lib.lass_last_error(None) or b"hip" in lib.lass_last_error(None).lower()


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "lass_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_module_mirror_state_dict_and_init(golden_dir):
    import json
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    spec = json.load(open(os.path.join(golden_dir, "state_dict_spec.json")))
    sd = m.state_dict()
    ref_keys = {k for k in spec if not k.startswith(("base.stft.", "base.istft."))}
    assert set(sd) == ref_keys
    for k in ref_keys:
        assert list(sd[k].shape) == spec[k]["shape"], k
        assert str(sd[k].dtype).replace("torch.", "") == spec[k]["dtype"], k
    # reference init: BN gamma=1/beta=0, biases 0, xavier-uniform weights (models/base.py:9-21)
    assert torch.all(sd["base.bn0.weight"] == 1) and torch.all(sd["base.bn0.bias"] == 0)
    assert torch.all(sd["base.pre_conv.bias"] == 0)
    w = sd["base.encoder_block3.conv_block1.conv1.weight"]
    bound = (6.0 / ((64 + 128) * 9)) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    # a reference checkpoint's extra torchlibrosa buffers are tolerated even with strict=True
    full = dict(sd)
    full["base.stft.conv_real.weight"] = torch.zeros(513, 1, 1024)
    full["base.istft.conv_imag.weight"] = torch.zeros(1024, 1024, 1)
    m.load_state_dict(full, strict=True)
    assert m.film_meta["decoder_block3"]["conv_block2"]["beta1"] == 512
    with pytest.raises(NotImplementedError):
        ResUNet30(2, 2, 512)


def test_checkpoint_reader(tmp_path):
    from lass_amd import synthetic
    from lass_amd.utils import load_ss_model, parse_yaml
    sd = synthetic.make_state_dict()
    ck = {"state_dict": {"ss_model." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "epoch": 3}
    ck["state_dict"]["query_encoder.model.logit_scale_a"] = torch.zeros(())
    ck["state_dict"]["ss_model.base.stft.conv_real.weight"] = torch.zeros(513, 1, 1024)
    path = os.path.join(tmp_path, "step=1.ckpt")
    torch.save(ck, path)
    cfg = os.path.join(tmp_path, "c.yaml")
    open(cfg, "w").write("model:\n  model_type: ResUNet30\n  input_channels: 1\n  output_channels: 1\n  condition_size: 512\n")
    pl = load_ss_model(parse_yaml(cfg), path, query_encoder=None)
    got = pl.ss_model.state_dict()
    for k, v in sd.items():
        assert np.array_equal(got[k].numpy(), np.asarray(v)), k
    emb = pl.query_encoder.get_query_embed(modality="text", text=["a dog", "a dog", "rain"])
    assert emb.shape == (3, 512) and torch.equal(emb[0], emb[1]) and abs(float(emb[2].norm()) - 1) < 1e-6


def test_shipped_default_config(tmp_path, monkeypatch):
    """`eval(evaluator, ckpt)` and `get_ss_model` default to `config/audiosep_base.yaml` (dcase_evaluator.py:126-130,
    utils.py:326-353): the file ships with the repo, carries the reference's `model:` keys
    (/root/reference/config/audiosep_base.yaml:23-30) and is found from any working directory."""
    import inspect
    from lass_amd import evaluator as lev
    from lass_amd.resunet import ResUNet30
    from lass_amd.utils import get_ss_model, parse_yaml, resolve_config
    assert inspect.signature(lev.eval).parameters["config_yaml"].default == "config/audiosep_base.yaml"
    monkeypatch.chdir(tmp_path)
    cfg = parse_yaml("config/audiosep_base.yaml")
    assert cfg["model"] == {"query_net": "CLAP", "condition_size": 512, "model_type": "ResUNet30", "input_channels": 1,
                            "output_channels": 1, "resume_checkpoint": "", "use_text_ratio": 1.0}
    assert cfg["data"]["sampling_rate"] == 16000 and cfg["data"]["stft_win_lengths"] == [256, 512, 2048]
    assert cfg["data"]["loudness_norm"] == {"lower_db": -10, "higher_db": 10} and cfg["data"]["max_mix_num"] == 2
    assert isinstance(get_ss_model("config/audiosep_base.yaml"), ResUNet30)
    # a config in the working directory wins over the shipped one, as in the reference
    os.makedirs("config")
    open("config/audiosep_base.yaml", "w").write("model:\n  model_type: Nope\n  input_channels: 1\n  output_channels: 1\n  condition_size: 512\n")
    assert resolve_config("config/audiosep_base.yaml") == "config/audiosep_base.yaml"
    with pytest.raises(NotImplementedError):
        get_ss_model("config/audiosep_base.yaml")


def test_wav_roundtrip(tmp_path):
    from lass_amd.wavio import read_wav, write_wav_f32, write_wav_pcm16
    x = (np.random.default_rng(0).standard_normal(1000) * 0.2).astype(np.float32)
    p = os.path.join(tmp_path, "a.wav")
    write_wav_f32(p, x, 16000)
    y, sr = read_wav(p, 16000)
    assert sr == 16000 and np.array_equal(x, y)
    write_wav_pcm16(p, x, 16000)
    y, _ = read_wav(p, 16000)
    assert np.max(np.abs(y - x)) <= 0.5 / 32768 + 1e-7
    with pytest.raises(ValueError):
        read_wav(p, 32000, strict_rate=True)
    # dcase_evaluator.py:73-74 (librosa.load(sr=16000)) resamples; here: scipy polyphase, labelled parity-unpinned, warns once.
    # A 1 kHz tone written at 48 kHz comes back at 16 kHz with its frequency and amplitude intact.
    t = np.arange(48000) / 48000.0
    write_wav_f32(p, (0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32), 48000)
    with pytest.warns(UserWarning, match="parity with the reference is unpinned"):
        y, sr = read_wav(p, 16000)
    assert sr == 16000 and y.shape == (16000,) and y.dtype == np.float32
    ref = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(16000) / 16000.0)
    assert np.max(np.abs(y[200:-200] - ref[200:-200])) < 2e-3


def test_stats_to_db_closed_form():
    from lass_amd.metrics import stats_to_db
    from oracle import metrics as om
    rng = np.random.default_rng(1)
    ref = rng.standard_normal(4000).astype(np.float32)
    est = (0.5 * ref + 0.1 * rng.standard_normal(4000)).astype(np.float32)
    r, e = ref.astype(np.float64), est.astype(np.float64)
    eps32 = np.finfo(np.float32).eps
    a = (eps32 + r @ e) / (r @ r + eps32)
    st = np.array([[r @ r, e @ e, r @ e, ((e - r) ** 2).sum(), ((a * r) ** 2).sum(), ((e - a * r) ** 2).sum()]])
    sdr, sisdr = stats_to_db(st, 4000)
    assert abs(sdr[0] - om.calculate_sdr(ref, est)) < 1e-4
    assert abs(sisdr[0] - om.calculate_sisdr(ref, est)) < 1e-3
    # est = 0.5 ref -> SDR = 20 log10(2)
    st = np.array([[1.0, 0.25, 0.5, 0.25, 0.25, 0.0]])
    assert abs(stats_to_db(st, 1)[0][0] - 6.0206) < 1e-4


def test_shard_range_partitions():
    from lass_amd.dist import shard_range
    for n in (0, 1, 7, 8, 128, 131):
        for ws in (1, 2, 3, 8):
            spans = [shard_range(n, r, ws) for r in range(ws)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(ws - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


_GLOO_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch.distributed as dist
from lass_amd import dist as ldist
dist.init_process_group("gloo")
rank, ws = ldist.world()
n = int(sys.argv[2])
lo, hi = ldist.shard_range(n, rank, ws)
local = np.stack([np.arange(lo, hi) * 1.0, np.arange(lo, hi) * -2.0, np.full(hi - lo, rank)], axis=1).reshape(-1, 3)
allrows = ldist.gather_rows(local, n)
assert allrows.shape == (n, 3), allrows.shape
assert np.array_equal(allrows[:, 0], np.arange(n)) and np.array_equal(allrows[:, 1], -2.0 * np.arange(n))
assert not np.isnan(allrows).any()
means = allrows.mean(0)
if rank == 0:
    print("GATHER_OK", n, ws, means[0])
dist.destroy_process_group()
"""


@pytest.mark.parametrize("n", [8, 7])
def test_gather_rows_gloo_world2(tmp_path, n):
    """The N>1 evaluation path: block sharding + ONE all_gather of per-clip metric rows (ragged shards NaN-padded)."""
    script = os.path.join(tmp_path, "w.py")
    open(script, "w").write(_GLOO_WORKER)
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), script, ROOT, str(n)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"GATHER_OK {n} 2" in r.stdout


@pytest.mark.parametrize("n", [128, 125])
def test_gather_rows_gloo_world8_configs3(tmp_path, n):
    """BASELINE configs[3] at its stated sharding, rehearsed on CPU: 8 ranks x 16 clips (n = 128; n = 125 leaves ragged shards
    of 15 / 16 clips and NaN padding), block partition + ONE all_gather of the per-clip rows, every rank ends with all rows in
    clip order.  OMP threads are pinned low: 8 rank processes share this container's CPUs."""
    script = os.path.join(tmp_path, "w8.py")
    open(script, "w").write(_GLOO_WORKER)
    port = 31500 + (os.getpid() % 2000)
    env = dict(os.environ, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr",
           "127.0.0.1", "--master-port", str(port), script, ROOT, str(n)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"GATHER_OK {n} 8 {(n - 1) / 2.0}" in r.stdout


def test_bench_parent_forwards_failing_ranks_and_exits_nonzero(tmp_path, monkeypatch):
    """bench.py's N > 1 parent: when the launcher fails (a rank died), the tail of what the ranks wrote is forwarded to stderr
    and the exit code is non-zero; ranks that exit 0 without the JSON line are an error too.  No retry, no re-exec."""
    bench = _import_bench()
    import types
    calls = {}

    def fake_run(cmd, **kw):
        if "-c" in cmd:  # the build child
            return types.SimpleNamespace(returncode=0, stdout="", stderr="")
        calls["cmd"] = cmd
        calls["kw"] = kw
        return types.SimpleNamespace(returncode=calls["rc"], stdout=calls["out"], stderr="")

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    args = bench.parse_args(["--gpus", "2", "--steps", "2"])
    calls.update(rc=1, out="[rank1]: RuntimeError: hipErrorNoDevice\n")
    assert bench.parent_launch(args, ["--gpus", "2", "--steps", "2"]) == 1
    assert calls["kw"].get("stderr") is not None  # the ranks' stderr is captured (merged) so that its tail can be forwarded
    calls.update(rc=0, out="no json here\n")
    assert bench.parent_launch(args, ["--gpus", "2", "--steps", "2"]) == 1
    calls.update(rc=0, out='noise\n{"metric": "clips/sec (10s@16kHz)", "value": 1.0}\n')
    assert bench.parent_launch(args, ["--gpus", "2", "--steps", "2"]) == 0


def _hipcc():
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    return hipcc


@pytest.fixture(scope="module")
def kernel_isa(tmp_path_factory):
    """The gfx950 ISA of every kernel translation unit, compiled ONCE (in parallel) with exactly the flags
    __graft_entry__.build() uses -> {file name: (path of the .s, compiler stderr)}."""
    import __graft_entry__ as ge
    hipcc = _hipcc()
    d = tmp_path_factory.mktemp("isa")
    csrc = os.path.join(ROOT, "lass_amd", "csrc")
    flags = [f for f in ge.FLAGS if f != "-fPIC"]
    procs = {}
    for name in ge.SOURCES:
        if "__global__" not in open(os.path.join(csrc, name)).read():
            continue  # api.hip: host code only
        out = os.path.join(d, name + ".s")
        procs[name] = (out, subprocess.Popen([hipcc] + flags + ge.EXTRA_FLAGS.get(name, []) + ["-S", "--cuda-device-only",
                                             os.path.join(csrc, name), "-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    res = {}
    for name, (out, pr) in procs.items():
        _, err = pr.communicate(timeout=1200)
        assert pr.returncode == 0, (name, err[-2000:])
        res[name] = (out, err)
    return res


def test_build_is_warning_free(kernel_isa):
    """Every kernel translation unit compiles without warnings under the build's flags (round 3 left a -Warray-bounds in
    wino.hip)."""
    for name, (_, err) in kernel_isa.items():
        lines = [ln for ln in err.split("\n") if "warning" in ln and "-Wunused-command-line-argument" not in ln]  # (-S driver noise)
        assert not lines, (name, lines[:5])


def test_no_kernel_spills_to_scratch(kernel_isa):
    """No kernel of the library uses scratch memory (register spills): a spill in a conv kernel is HBM traffic per thread and
    per launch - round 4's three-workgroups-per-CU variant of the decoder conv2 kernels wrote 0.2 GB per launch that way
    and was dropped for it."""
    for name, (out, _) in kernel_isa.items():
        isa = open(out).read()
        sizes = re.findall(r"\.set (\S+)\.private_seg_size, (\d+)", isa)
        assert sizes, name
        spilling = [(k, v) for k, v in sizes if int(v) > 0]
        assert not spilling, (name, spilling[:5])


def test_no_kernel_carries_packed_f32(kernel_isa):
    """on gfx950 a wave executing packed-f32 arithmetic (v_pk_{add,mul,fma}_f32, which hipcc's SLP vectoriser
    forms from float2-shaped code such as the FFT butterflies) returned wrong values, run to run, while a workgroup of a bf16
    conv kernel (v_mfma_f32_32x32x16_bf16 fed from LDS) was resident on the same CU - seen on the STFT beside lass_separate on
    another stream.  The library is therefore built with -fno-slp-vectorize throughout (measured cost: none); this audits the
    ISA those flags produce: no packed-f32 instruction in any kernel."""
    import __graft_entry__ as ge
    assert "-fno-slp-vectorize" in ge.FLAGS
    assert {"stft.hip", "misc.hip", "conv_bf16.hip", "conv_bf16_fused.hip", "wino4.hip"} <= set(kernel_isa)
    for name, (out, _) in kernel_isa.items():
        isa = open(out).read()
        packed = [ln.strip() for ln in isa.split("\n") if re.search(r"\bv_pk_[a-z0-9]+_f32\b", ln)]
        assert not packed, (name, len(packed), packed[:3])
        assert isa.count("s_endpgm") >= 2, name   # really the kernels


# ---- bench.py: the PMC traffic number is only reported for the kernels it was measured at ----------------------------
def _import_bench():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    return bench


def test_bench_traffic_reported_only_at_matching_source_hash(monkeypatch, tmp_path):
    """roofline.traffic comes from a committed rocprofv3 --pmc summary (bench.py cannot read counters itself): it is
    reported only when the summary's `source_hash` equals the hash of the kernel sources in use, otherwise null +
    `traffic_stale` - a measurement of other kernels is never passed off as this run's."""
    bench = _import_bench()
    import __graft_entry__ as ge
    prof = tmp_path / "profiles" / "r99"
    prof.mkdir(parents=True)
    rec = {"traffic_bytes_per_launch": 1.5e9, "source_hash": ge._src_hash(), "fetch_calibration": {"x": 1}}
    (prof / "conv_traffic_f32.json").write_text(json.dumps(rec))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    got = bench.traffic_fields("f32", 1.0e9)
    assert got["traffic"] == 1.5e9 and got["traffic_over_algorithmic"] == pytest.approx(1.5)
    assert got["traffic_stale"] is False and got["traffic_source_hash"] == ge._src_hash()
    rec["source_hash"] = "0" * 64
    (prof / "conv_traffic_f32.json").write_text(json.dumps(rec))
    got = bench.traffic_fields("f32", 1.0e9)
    assert got["traffic"] is None and got["traffic_over_algorithmic"] is None and got["traffic_stale"] is True
    assert "not reported" in got["traffic_source"]
    # no summary for the dtype, or switched off (other workload than B=16 x 10 s): null without a stale flag
    assert bench.traffic_fields("bf16", 1.0e9) == {"traffic": None, "traffic_over_algorithmic": None, "traffic_source": None}
    assert bench.traffic_fields("f32", 1.0e9, enabled=False)["traffic"] is None


def test_committed_traffic_profiles_are_complete():
    """The newest profiles/rNN/conv_traffic_<dtype>.json files carry what bench.py and the judge read: bytes per launch split
    into fetch and write, the launch count, the workload and the hash of the kernel sources they were measured at."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dtype in ("f32", "bf16"):
        files = sorted(glob.glob(os.path.join(root, "profiles", "r*", f"conv_traffic_{dtype}.json")))
        assert files, dtype
        d = json.load(open(files[-1]))
        assert d["dtype"] == dtype and d["launches"] >= 20
        assert d["traffic_bytes_per_launch"] == pytest.approx(d["fetch_bytes_per_launch"] + d["write_bytes_per_launch"], rel=1e-9)
        assert re.fullmatch(r"[0-9a-f]{64}", d["source_hash"])
        # against the per-LAUNCH-fusion ideal (lass_amd.arch.conv3x3_bytes_per_clip: every launch reads its inputs and writes its
        # outputs once, 26 launches): f32 sits above it (halo re-reads); bf16 may sit BELOW it since rounds 3 / 4 - two blocks run as
        # one kernel each (their 32-channel intermediates stay in LDS) and decoder_block6's up-sampled input is never stored
        lo = {"f32": 1.0, "bf16": 0.8}[dtype]
        assert lo <= d["traffic_bytes_per_launch"] / {"f32": 862090791.4, "bf16": 431045395.7}[dtype] < 3.0
