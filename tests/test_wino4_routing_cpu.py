"""Host-only: lass_amd.arch.wino4_routed (the mirror of the C dispatch that bench.py's executed-FLOP accounting uses) against the
layer list written in DESIGN.md section 4 ("Which 3x3 convs run as F(4x4,3x3)"), and against the C rule itself:
lass_amd/csrc/conv_route.h, printed as a table by tools/route_table.cpp (built here with the host compiler)."""
import os
import re
import shutil
import subprocess

import pytest

from lass_amd import arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _design_lists():
    """The two fenced lists of DESIGN.md: `wino4-routed:` (10 s clips, 1024 padded frames) and `wino-routed:` (what stays F(2x2,3x3))."""
    txt = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    out = {}
    for key in ("wino4-routed", "wino-routed"):
        m = re.search(r"^" + key + r":\s*(.+?)\n\s*\n", txt, re.S | re.M)
        assert m, f"DESIGN.md has no '{key}:' list"
        out[key] = set(re.findall(r"[a-z_0-9]+\.conv[12]", m.group(1)))
    return out


def test_default_layer_table_matches_design_md():
    rows = arch.conv_layer_table(arch.padded_frames(arch.frames_for(160000)))
    all3x3 = {r["name"] for r in rows if r["kind"] == "3x3"}
    routed = arch.wino4_routed(rows)
    lists = _design_lists()
    assert routed == lists["wino4-routed"]
    assert all3x3 - routed == lists["wino-routed"] == {"conv_block7a.conv1", "conv_block7a.conv2"}
    assert len(all3x3) == 26 and len(routed) == 24
    for name in ("encoder_block6.conv1", "encoder_block6.conv2", "decoder_block1.conv1", "decoder_block1.conv2"):
        assert name in routed   # the 32-frame x 16-bin level: split-K F(4x4,3x3)


def test_other_frame_counts_keep_the_16_bin_level_on_f2x2():
    """The 16-bin level tiles into 32 x 16 blocks only when its frame count is a multiple of 32 (1024 padded frames per clip)."""
    for t_pad in (160, 512, 992, 2016):
        routed = arch.wino4_routed(arch.conv_layer_table(t_pad))
        for name in ("encoder_block6.conv1", "encoder_block6.conv2", "decoder_block1.conv1", "decoder_block1.conv2"):
            assert name not in routed, (t_pad, name)
    assert "decoder_block1.conv2" in arch.wino4_routed(arch.conv_layer_table(2048))


def test_wino4_off_routes_nothing():
    assert arch.wino4_routed(arch.conv_layer_table(1024), 0) == set()


def test_min_cin_threshold_applies_to_the_block_at_the_16_bin_level():
    routed = arch.wino4_routed(arch.conv_layer_table(1024), 512)   # only decoder_block1.conv1 has 768 input channels, but
    assert "decoder_block1.conv1" not in routed                      # the block routes as a whole (its cout is 384)
    assert "decoder_block2.conv1" in routed


# ---- the C rule (csrc/conv_route.h) through tools/route_table.cpp ------------------------------------------------------------
T_PADS = (160, 512, 992, 1024, 2016, 2048)
MIN_CINS = (0, 32, 64, 512)
SPLIT_BLOCKS = ("encoder_block6", "decoder_block1")                                       # the 32 x 16 level of a 10 s clip
GEMM_BLOCKS = ("encoder_block5", "decoder_block1", "decoder_block2", "decoder_block3", "decoder_block4")
V_BLOCKS = ("encoder_block5", "encoder_block6", "decoder_block1", "decoder_block2")       # 12 cout groups


@pytest.fixture(scope="module")
def route_table(tmp_path_factory):
    """run(t_pad, min_cin, vprep, splits, aligned, windows) -> ({conv name: (family, kind, splits, v)}, {block: (shortcut, kpart, v)})"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler in this environment")
    exe = str(tmp_path_factory.mktemp("route") / "route_table")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lass_amd", "csrc"),
                    os.path.join(ROOT, "tools", "route_table.cpp"), "-o", exe], check=True)
    cache = {}

    def run(t_pad, min_cin=32, vprep=1, splits=0, aligned=1, windows=0):
        key = (t_pad, min_cin, vprep, splits, aligned, windows)
        if key not in cache:
            out = subprocess.run([exe] + [str(v) for v in key], check=True, capture_output=True, text=True).stdout
            convs, blocks = {}, {}
            for line in out.splitlines():
                f = line.split()
                if f[0] == "conv":
                    convs[f[1]] = (f[2], f[3], int(f[4]), bool(int(f[5])))
                else:
                    blocks[f[1]] = (f[2].split("=")[1], int(f[3].split("=")[1]), int(f[4].split("=")[1]))
            cache[key] = (convs, blocks)
        return cache[key]
    return run


def _f4(convs):
    return {n for n, c in convs.items() if c[0] == "f4x4"}


@pytest.mark.parametrize("min_cin", MIN_CINS)
def test_python_mirror_equals_the_c_rule(route_table, min_cin):
    for t_pad in T_PADS:
        rows = arch.conv_layer_table(t_pad)
        convs, _ = route_table(t_pad, min_cin)
        assert set(convs) == {r["name"] for r in rows if r["kind"] == "3x3"}
        assert _f4(convs) == arch.wino4_routed(rows, min_cin), (t_pad, min_cin)


@pytest.mark.parametrize("min_cin", MIN_CINS)
def test_python_mirror_equals_the_c_rule_multistft(route_table, min_cin):
    wins = arch.MS_WIN_LENGTHS
    for t_pad in T_PADS:
        rows = arch.ms_conv_layer_table(t_pad)
        convs, _ = route_table(t_pad, min_cin, windows=len(wins))
        # the program names the analysis branches by index, the layer table by window length
        convs = {re.sub(r"^encoder_block1s\.(\d+)", lambda m: f"encoder_block1s.{wins[int(m.group(1))]}", n): c for n, c in convs.items()}
        assert set(convs) == {r["name"] for r in rows if r["kind"] == "3x3"}
        assert _f4(convs) == arch.wino4_routed(rows, min_cin), (t_pad, min_cin)


def test_default_routes_of_a_10s_clip(route_table):
    convs, blocks = route_table(1024)
    assert {b for b, v in blocks.items() if v[0] == "gemm"} == set(GEMM_BLOCKS)
    assert {n for n, c in convs.items() if c[2] != 1} == {f"{b}.conv{k}" for b in SPLIT_BLOCKS for k in (1, 2)}
    assert all(c[2] == 4 for n, c in convs.items() if n.rsplit(".", 1)[0] in SPLIT_BLOCKS)
    assert {n for n, c in convs.items() if c[3]} == {f"{b}.conv{k}" for b in V_BLOCKS for k in (1, 2)}
    for b, (shortcut, kpart, v) in blocks.items():
        assert (kpart > 0) == (b in SPLIT_BLOCKS) and (v > 0) == (b in V_BLOCKS), b
        # behind a shortcut GEMM conv2 reads the block's output slot as its residual
        assert (convs[b + ".conv2"][1] == "CONV2_IDENT") == (shortcut == "gemm" or b in ("encoder_block6", "conv_block7a")), b
    assert blocks["encoder_block6"][1] == 4 * 384 * 32 * 16 and blocks["decoder_block2"][2] == 768 * 64 * 32 * 9 // 4


def test_unaligned_input_keeps_the_shortcut_fused(route_table):
    convs, blocks = route_table(1024)
    uconvs, ublocks = route_table(1024, aligned=0)
    assert all(v[0] != "gemm" for v in ublocks.values())
    changed = {n for n in convs if convs[n] != uconvs[n]}
    assert changed == {b + ".conv2" for b in GEMM_BLOCKS}
    for b in GEMM_BLOCKS:
        if b in SPLIT_BLOCKS:   # the 32 x 16 blocks have no fused shortcut phase: F(2x2,3x3)
            assert uconvs[b + ".conv2"] == ("f2x2", "CONV2_SHORTCUT", 1, False)
        else:                   # the unsplit kernels fall back to their fused phase, which reads no V image
            assert uconvs[b + ".conv2"] == ("f4x4", "CONV2_SHORTCUT", 1, False)


def test_vprep_modes_change_only_the_v_column(route_table):
    convs, blocks = route_table(1024)
    for mode in (0, 2):
        mconvs, mblocks = route_table(1024, vprep=mode)
        assert {n: c[:3] for n, c in mconvs.items()} == {n: c[:3] for n, c in convs.items()}
        assert {b: v[:2] for b, v in mblocks.items()} == {b: v[:2] for b, v in blocks.items()}
        if mode == 0:
            assert not any(c[3] for c in mconvs.values()) and not any(v[2] for v in mblocks.values())
        else:   # every F(4x4,3x3) launch without a fused shortcut phase, a head or a pre_conv input
            assert {n for n, c in mconvs.items() if c[3]} == {n for n, c in convs.items() if c[0] == "f4x4" and c[1] in ("CONV1_ACT", "CONV2_IDENT")}
            assert mblocks["decoder_block5"][2] == 128 * 512 * 256 * 9 // 4 and mblocks["encoder_block1"][2] == 0


@pytest.mark.parametrize("n", [1, 2, 4])
def test_forced_splits_change_only_the_split_factor(route_table, n):
    convs, blocks = route_table(1024)
    sconvs, sblocks = route_table(1024, splits=n)
    assert {k: (c[0], c[1], c[3]) for k, c in sconvs.items()} == {k: (c[0], c[1], c[3]) for k, c in convs.items()}
    assert {k for k, c in sconvs.items() if c[2] != 1} == ({f"{b}.conv{k}" for b in SPLIT_BLOCKS for k in (1, 2)} if n > 1 else set())
    assert all(c[2] in (1, n) for c in sconvs.values())
    for b, (shortcut, kpart, v) in sblocks.items():
        assert (shortcut, v) == (blocks[b][0], blocks[b][2])
        assert kpart == (n * 384 * 32 * 16 if n > 1 and b in SPLIT_BLOCKS else 0), b
    if n == 4:
        assert (sconvs, sblocks) == (convs, blocks)
