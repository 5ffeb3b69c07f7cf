"""Host-only: the bf16 plan of one lass_separate - which blocks run fused, which tensors travel between launches as blocked bf16
copies, which family runs each transposed conv - as lass_amd/csrc/conv_route.h decides it (plan_separate), printed by
tools/route_table.cpp (built here with the host compiler).  Producer and consumer of every hand-over must agree, or a launch reads
f32 storage as bf16 units: that invariant is held here, over the whole grid of frame counts and switches."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lass_amd", "csrc")
T_PADS = (128, 160, 512, 1024, 2048)
SWITCHES = tuple(itertools.product((1, 0), repeat=3))   # (FUSE_CATB, FUSE_BLOCK, FUSE_UP), the default first
FLAGS = ("cat_in", "skip_out", "pool_copies", "act_out")
ENC = [f"encoder_block{k}" for k in range(1, 7)] + ["conv_block7a"]
DEC = [f"decoder_block{k}" for k in range(1, 7)]


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    return cxx


def _argv(t_pad, windows=0, mode=1, catb=1, block=1, up=1):
    # T_PAD MIN_CIN VPREP_MODE FORCED_SPLITS X_ALIGNED STFT_WINDOWS B HEAD_FOLD HEAD HEAD_SC_FOLD MODE FUSE_CATB FUSE_BLOCK FUSE_UP
    return [str(v) for v in (t_pad, 32, 1, 0, 1, windows, 1, 1, 1, 1, mode, catb, block, up)]


def parse(out):
    """{"up": {decoder: (family, in_act, out_copies)}, "bf16": {block: {"form": .., flag: 0|1}}, "scopes": (conv3x3, tconv)}"""
    t = {"up": {}, "bf16": {}, "scopes": None}
    for line in out.splitlines():
        f = line.split()
        kv = {k: v for k, v in (x.split("=") for x in f[1:] if "=" in x)}
        if f[0] == "up":
            t["up"][f[1]] = (f[2], int(kv["in_act"]), int(kv["out_copies"]))
        elif f[0] == "bf16":
            t["bf16"][f[1]] = {"form": kv["form"], **{k: int(kv[k]) for k in FLAGS}}
        elif f[0] == "scopes":
            t["scopes"] = (int(kv["conv3x3"]), int(kv["tconv"]))
    return t


def build_route_table(tmp_dir, extra=()):
    """run(t_pad, windows=0, mode=1, catb=1, block=1, up=1) -> the parsed table"""
    exe = os.path.join(str(tmp_dir), "route_table")
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, os.path.join(ROOT, "tools", "route_table.cpp"), "-o", exe],
                   check=True)
    cache = {}

    def run(t_pad, **kw):
        argv = tuple(_argv(t_pad, **kw))
        if argv not in cache:
            cache[argv] = parse(subprocess.run([exe, *argv], check=True, capture_output=True, text=True).stdout)
        return cache[argv]
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return build_route_table(tmp_path_factory.mktemp("route_bf16"))


def _flags(t, names, flag):
    return {n for n in names if t["bf16"][n][flag]}


@pytest.mark.parametrize("t_pad", T_PADS)
def test_default_plan_of_resunet30(table, t_pad):
    t = table(t_pad)
    b, up = t["bf16"], t["up"]
    assert set(b) == set(ENC + DEC) and set(up) == set(DEC)
    assert b["encoder_block1"]["form"] == "enc1"
    assert b["decoder_block6"]["form"] == "dec6u" and up["decoder_block6"][0] == "inside"
    assert all(v["form"] == "two" for n, v in b.items() if n not in ("encoder_block1", "decoder_block6"))
    assert _flags(t, ENC + DEC, "cat_in") == set(DEC[1:]) | set(ENC[1:5])
    assert _flags(t, ENC + DEC, "skip_out") == set(ENC[:5])
    assert _flags(t, ENC + DEC, "pool_copies") == set(ENC[:4])
    assert _flags(t, ENC + DEC, "act_out") == set(DEC[:5])
    # decoder_block1's transposed conv is 1 x 2: it writes f32 and its block reads f32
    assert up["decoder_block1"] == ("bf16", 0, 0) and b["decoder_block1"]["cat_in"] == 0
    assert all(b["conv_block7a"][k] == 0 for k in FLAGS)
    for d in DEC[1:5]:
        assert up[d] == ("bf16", 1, 1), d


@pytest.mark.parametrize("t_pad", T_PADS)
def test_fuse_up_off_changes_only_decoder_block6(table, t_pad):
    on, off = table(t_pad), table(t_pad, up=0)
    assert off["bf16"]["decoder_block6"]["form"] == "dec6" and off["up"]["decoder_block6"] == ("bf16", 1, 1)
    assert {n: v for n, v in off["up"].items() if n != "decoder_block6"} == {n: v for n, v in on["up"].items() if n != "decoder_block6"}
    same = dict(off["bf16"])
    same["decoder_block6"] = dict(same["decoder_block6"], form="dec6u")
    assert same == on["bf16"]


@pytest.mark.parametrize("t_pad", T_PADS)
def test_fuse_block_off_runs_both_ends_as_two_launches(table, t_pad):
    on, off = table(t_pad), table(t_pad, block=0)
    assert all(v["form"] == "two" for v in off["bf16"].values())
    assert off["up"]["decoder_block6"] == ("bf16", 1, 1)   # fuse_up needs fuse_block
    assert {n: {k: v[k] for k in FLAGS} for n, v in off["bf16"].items()} == {n: {k: v[k] for k in FLAGS} for n, v in on["bf16"].items()}


@pytest.mark.parametrize("t_pad", T_PADS)
def test_fuse_catb_off_hands_everything_over_as_f32(table, t_pad):
    off = table(t_pad, catb=0)
    assert all(v == {"form": "two", "cat_in": 0, "skip_out": 0, "pool_copies": 0, "act_out": 0} for v in off["bf16"].values())
    assert all(u == ("bf16", 0, 0) for u in off["up"].values()) and len(off["up"]) == 6


@pytest.mark.parametrize("t_pad", T_PADS)
def test_bf16x3_is_the_plan_without_blocked_copies(table, t_pad):
    for sw in SWITCHES:
        assert table(t_pad, mode=2, catb=sw[0], block=sw[1], up=sw[2]) == table(t_pad, mode=1, catb=0)


@pytest.mark.parametrize("t_pad", T_PADS)
def test_multistft_with_three_windows(table, t_pad):
    t, ref = table(t_pad, windows=3), table(t_pad)
    b = t["bf16"]
    branches = [f"encoder_block1s.{k}" for k in range(3)]
    assert set(b) == set(branches + ENC[1:] + DEC)
    for n in branches:
        assert b[n] == ref["bf16"]["encoder_block1"] and b[n]["form"] == "enc1"
    assert b["decoder_block6"]["form"] == "two"   # 128 input channels
    assert t["up"]["decoder_block6"] == ("bf16", 1, 1)
    for n in ENC[1:] + DEC:
        assert {k: b[n][k] for k in FLAGS} == {k: ref["bf16"][n][k] for k in FLAGS}, n


def _check_consistency(t, windows):
    b, up = t["bf16"], t["up"]
    enc1 = [f"encoder_block1s.{k}" for k in range(windows)] if windows else ["encoder_block1"]
    enc = [enc1] + [[n] for n in ENC[1:]]
    for n, v in b.items():
        if v["form"] == "f32":
            assert not any(v[k] for k in FLAGS), n
    for d in range(6):
        dec = b[DEC[d]]
        # the concat's two halves: the transposed conv (or the fused kernel that contains it) and the skip's encoder
        wrote_up = up[DEC[d]][2] == 1 or up[DEC[d]][0] == "inside"
        for e in enc[5 - d]:
            assert b[e]["skip_out"] == dec["cat_in"], (DEC[d], e)
        assert wrote_up == bool(dec["cat_in"]), DEC[d]
        if up[DEC[d]][0] == "inside":
            assert dec["form"] == "dec6u"
        assert (dec["form"] == "dec6u") == (up[DEC[d]][0] == "inside")
        # an activated input follows an activated output, and the reverse
        assert up[DEC[d]][1] == (b[DEC[d - 1]]["act_out"] if d else 0), DEC[d]
    assert b[DEC[5]]["act_out"] == 0
    for i in range(7):
        for e in enc[i]:
            producers = enc[i - 1] if i else []
            assert all(b[p]["pool_copies"] == b[e]["cat_in"] for p in producers), e
            if not producers:
                assert b[e]["cat_in"] == 0
    assert all(b[e]["pool_copies"] == 0 for e in enc[6] + enc[5])   # nobody reads them as copies


@pytest.mark.parametrize("windows", [0, 3])
def test_producers_and_consumers_agree(table, windows):
    for t_pad in T_PADS:
        for sw in SWITCHES:
            _check_consistency(table(t_pad, windows=windows, catb=sw[0], block=sw[1], up=sw[2]), windows)


def test_profiler_scopes_of_a_128_row_plan(table):
    assert table(128)["scopes"] == (24, 5)
    assert table(128, up=0)["scopes"] == (24, 6)
    assert table(128, block=0)["scopes"] == (26, 6)
    assert table(128, catb=0)["scopes"] == (26, 6)
    assert table(128, mode=2)["scopes"] == (26, 6)
    assert table(128, windows=3)["scopes"] == (27, 6)


def test_existing_command_lines_keep_their_meaning(table):
    """ten arguments, as the earlier tests pass them, print the conv and block lines alone; MODE = 0 adds the up and scopes lines
    behind the same conv and block lines"""
    ten = subprocess.run([table.exe] + _argv(1024)[:10], check=True, capture_output=True, text=True).stdout
    full = subprocess.run([table.exe] + _argv(1024, mode=0), check=True, capture_output=True, text=True).stdout
    assert [ln.split()[0] for ln in ten.splitlines()] == ["conv", "conv", "block"] * 13
    assert full.startswith(ten)
    assert [ln.split()[0] for ln in full[len(ten):].splitlines()] == ["up"] * 6 + ["scopes"]


def test_the_tool_runs_clean_under_sanitizers(tmp_path):
    run = build_route_table(tmp_path, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for t_pad in T_PADS:
        for mode in (0, 1, 2):
            for sw in SWITCHES:
                for windows in (0, 3):
                    r = subprocess.run([run.exe] + _argv(t_pad, windows=windows, mode=mode, catb=sw[0], block=sw[1], up=sw[2]),
                                       capture_output=True, text=True)
                    assert r.returncode == 0 and r.stderr == "", (t_pad, mode, sw, windows, r.stderr)
