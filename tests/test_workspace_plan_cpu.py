"""Host-only: the workspace layout of one lass_separate and the split decision of the call, as lass_amd/csrc/workspace_plan.h plans
them (make_plan, plan_call), printed by tools/workspace_table.cpp (built here with the host compiler).  What
lass_workspace_bytes and lass_workspace_tensor answer comes from the same functions; tests/test_gpu_workspace_plan.py ties the C-ABI
to this table."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lass_amd", "csrc")
# name -> (WINDOWS, N_FFT, HOP)
MODELS = {"resunet30": ("0", 1024, 160), "resunet30_32k": ("0", 2048, 320), "multistft": ("256,512,2048", 2048, 160)}
MODES = {"f32": 0, "bf16": 1, "bf16x3": 2}
BATCHES = (1, 2, 7, 8, 16)
LENGTHS = (8000, 16000, 160000)
NO_LIMIT = -1
ENC = [f"encoder_block{k}" for k in range(1, 7)]
DEC = [f"decoder_block{k}" for k in range(1, 7)]


def build_workspace_table(tmp_dir):
    """run(model, mode, B, L, split_batch=1, capturing=0, workspace_bytes=NO_LIMIT, **switches) -> the parsed table, None if refused"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    exe = os.path.join(str(tmp_dir), "workspace_table")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tools", "workspace_table.cpp"), "-o", exe], check=True)
    cache = {}

    def run(model, mode, B, L, split_batch=1, capturing=0, workspace_bytes=NO_LIMIT, **switches):
        win, n_fft, hop = MODELS[model]
        argv = tuple(str(v) for v in (win, n_fft, hop, MODES[mode], B, L, split_batch, capturing, workspace_bytes)) + \
            tuple(f"{k}={v}" for k, v in sorted(switches.items()))
        if argv not in cache:
            p = subprocess.run([exe, *argv], capture_output=True, text=True)
            assert p.returncode in (0, 1), (argv, p.stderr)
            cache[argv] = parse(p.stdout) if p.returncode == 0 else None
        return cache[argv]
    return run


def parse(out):
    """{"plan": {B, L, T, Tp, total}, "half": {B, total} | None, "call": {split, need, accepted}, "slots": [(offset, bytes)],
    "tensors": {name: (offset, shape, strides)}}"""
    t = {"half": None, "slots": [], "tensors": {}}
    for line in out.splitlines():
        f = line.split()
        if f[0] in ("plan", "half", "call"):
            t[f[0]] = {k: int(v) for k, v in (x.split("=") for x in f[1:])}
        elif f[0] == "slot":
            t["slots"].append((int(f[2]), int(f[3])))
        elif f[0] == "tensor":
            assert f[1] not in t["tensors"]
            t["tensors"][f[1]] = (int(f[2]), tuple(int(x) for x in f[3].split(",")), tuple(int(x) for x in f[4].split(",")))
    return t


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return build_workspace_table(tmp_path_factory.mktemp("workspace_plan"))


def round256(n):
    return (n + 255) // 256 * 256


def extent(tensor):
    """bytes from the tensor's offset to the end of its last element"""
    _, shape, strides = tensor
    return 4 * (1 + sum((n - 1) * s for n, s in zip(shape, strides)))


CASES = list(itertools.product(MODELS, MODES))


@pytest.mark.parametrize("model,mode", CASES, ids=[f"{m}-{d}" for m, d in CASES])
def test_layout(table, model, mode):
    for B, L in itertools.product(BATCHES, LENGTHS):
        t = table(model, mode, B, L)
        assert t is not None, (B, L)
        total, slots, tensors = t["plan"]["total"], t["slots"], t["tensors"]
        # the slots: 256-byte offsets and sizes, pairwise disjoint, below total (they are handed out back to back and fill it)
        assert all(o % 256 == 0 and n % 256 == 0 and n > 0 for o, n in slots)
        for (o, n), (o2, _) in zip(slots, slots[1:]):
            assert o + n <= o2
        assert slots[-1][0] + slots[-1][1] == total
        # every named tensor lies inside ONE slot, at a 256-byte offset
        home = {}
        for name, ten in tensors.items():
            assert ten[0] % 256 == 0 and ten[1][0] == B, name
            inside = [i for i, (o, n) in enumerate(slots) if o <= ten[0] and ten[0] + extent(ten) <= o + n]
            assert len(inside) == 1, name
            home.setdefault(inside[0], []).append(name)
        # ... and the only slots with two tenants are the decoders' concats: <decoder>.up at the start, its skip behind at channel D.cout
        shared = {i: sorted(v) for i, v in home.items() if len(v) > 1}
        assert sorted(shared.values()) == sorted(sorted([ENC[5 - d], DEC[d] + ".up"]) for d in range(6))
        for i, names in home.items():       # a slot's one tenant, or the concat's .up, begins where the slot begins
            assert min(tensors[n][0] for n in names) == slots[i][0], names
        for d in range(6):
            up, skip = tensors[DEC[d] + ".up"], tensors[ENC[5 - d]]
            cout, H, W = up[1][1:]
            assert skip[0] == up[0] + 4 * cout * H * W and skip[1][2:] == (H, W)
            assert skip[2][0] == up[2][0] == (cout + skip[1][1]) * H * W           # both step over the whole concat per clip
        names = set(tensors)
        assert {"mag", "cos", "sin", "out_real", "out_imag", "conv_block7a", *ENC, *DEC} <= names
        assert ("x0" in names) == (model != "multistft") and ({"x0.256", "x0.512", "x0.2048"} <= names) == (model == "multistft")
        assert ("head_sc.skip" in names) == ("head_sc.up" in names) == (mode == "f32" and model != "multistft")


@pytest.mark.parametrize("model,mode", CASES, ids=[f"{m}-{d}" for m, d in CASES])
def test_need_and_split(table, model, mode):
    for B, L in itertools.product(BATCHES, LENGTHS):
        total = table(model, mode, B, L)["plan"]["total"]
        splittable = B >= 8 and B % 2 == 0
        for split_batch, profiling in ((1, 0), (2, 0), (0, 0), (1, 1)):
            t = table(model, mode, B, L, split_batch=split_batch, profiling=profiling)
            assert t["plan"]["total"] == total
            if splittable and split_batch and not profiling:
                half = table(model, mode, B // 2, L)["plan"]["total"]
                both = 2 * round256(half)
                assert t["half"] == {"B": B // 2, "total": half}
                assert t["call"]["need"] == max(total, both)
            else:
                assert t["half"] is None and t["call"]["need"] == total
            # asking (no workspace, no capture) never splits by the default switch; LASS_SPLIT=2 splits eager calls too
            assert t["call"]["split"] == int(splittable and split_batch == 2 and not profiling)
        need = table(model, mode, B, L)["call"]["need"]
        exact = table(model, mode, B, L, capturing=1, workspace_bytes=need)
        assert exact["call"] == {"split": int(splittable), "need": need, "accepted": 1}
        assert table(model, mode, B, L, capturing=0, workspace_bytes=need)["call"]["split"] == 0        # eager: whole, by default
        assert table(model, mode, B, L, split_batch=2, capturing=0, workspace_bytes=need)["call"]["split"] == int(splittable)
        less = table(model, mode, B, L, capturing=1, workspace_bytes=need - 256)
        assert less["call"]["split"] == 0 and less["call"]["need"] == total
        assert less["call"]["accepted"] == int(total <= need - 256)


def test_refused_shapes(table):
    for model, (_, n_fft, hop) in MODELS.items():
        assert table(model, "f32", 1, n_fft // 2) is None and table(model, "f32", 1, n_fft // 2 + 1) is not None
        assert table(model, "f32", 0, 16000) is None and table(model, "f32", -1, 16000) is None
        # decoder_block6's concat of one clip, f32: dec_cat x Tp x fcrop x 4 bytes, must stay at or below 0xFFFF0000
        per_frame = {"resunet30": 64 * 512 * 4, "resunet30_32k": 64 * 1024 * 4, "multistft": 128 * 1024 * 4}[model]
        tp_max = 0xFFFF0000 // per_frame // 32 * 32
        assert (tp_max + 32) * per_frame > 0xFFFF0000
        ok = table(model, "f32", 1, hop * (tp_max - 1))          # T = tp_max frames
        assert ok is not None and ok["plan"]["Tp"] == tp_max
        assert table(model, "f32", 1, hop * tp_max) is None      # T = tp_max + 1: one more row of 32
