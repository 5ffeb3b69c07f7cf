"""Host-only: the routes of the deep trunk on a 1024-bin context (ResUNet30 at the 32 kHz geometry, n_fft 2048, and the multi-STFT
model), row by row as tools/route_table.cpp prints them from lass_amd/csrc/conv_route.h.  One level wider than the 16 kHz context,
every trunk block sits on another width class: encoder_block6 / decoder_block1 on the 32-bin level (16 x 32 blocks), conv_block7a on
the 16-bin level (32 x 16 blocks, split-K), encoder_block5 / decoder_block2 on the 64-bin level (8 x 64 blocks).  The frame counts are
those of a 1.3 s, 5 s, 10 s and 20 s clip.  tests/test_gpu_wide_trunk.py runs the launches these rows name; a row that changes here
changes what that file covers."""
import os
import shutil
import subprocess

import pytest

from lass_amd import arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# argument positions of route_table behind T_PAD
ARGS = ("min_cin", "vprep", "splits", "aligned", "windows", "B", "head_fold", "head", "head_sc_fold", "mode", "fuse_catb", "fuse_block",
        "fuse_up", "n_fft", "gemm")
DEFAULTS = dict(min_cin=32, vprep=1, splits=0, aligned=1, windows=0, B=1, head_fold=1, head=1, head_sc_fold=1, mode=0, fuse_catb=1,
                fuse_block=1, fuse_up=1, n_fft=2048, gemm=1)
TRUNK = ("encoder_block5", "encoder_block6", "conv_block7a", "decoder_block1", "decoder_block2")

# (family, kind, splits, v, gemm) of a conv
G1 = ("f4x4", "CONV1_ACT", 1, 1, 1)          # the gemm route: scatter, 36 batched GEMMs, gather (wino4_gemm.hip)
G2 = ("f4x4", "CONV2_IDENT", 1, 1, 1)
N1 = ("f4x4", "CONV1_ACT", 4, 1, 1)          # ... on the narrow 32 x 16 blocks; the fields in front are the split-K launches behind it
N2 = ("f4x4", "CONV2_IDENT", 4, 1, 1)
W1 = ("f2x2", "CONV1_ACT", 1, 0, 0)          # F(2x2,3x3), wino.hip
W2 = ("f2x2", "CONV2_IDENT", 1, 0, 0)
W2S = ("f2x2", "CONV2_SHORTCUT", 1, 0, 0)    # ... with the 1x1 shortcut fused

# t_pad -> block -> (conv1, conv2, shortcut column, up family or None)
TABLE = {
    128: {"encoder_block5": (G1, G2, "gemm", None), "encoder_block6": (W1, W2, "-", None), "conv_block7a": (W1, W2, "-", None),
          "decoder_block1": (W1, W2S, "fused", "gemm"), "decoder_block2": (G1, G2, "gemm", "gemm")},
    512: {"encoder_block5": (G1, G2, "gemm", None), "encoder_block6": (G1, W2, "-", None), "conv_block7a": (W1, W2, "-", None),
          "decoder_block1": (G1, G2, "gemm", "gemm"), "decoder_block2": (G1, G2, "gemm", "gemm")},
    1024: {"encoder_block5": (G1, G2, "gemm", None), "encoder_block6": (G1, W2, "-", None), "conv_block7a": (N1, N2, "-", None),
           "decoder_block1": (G1, G2, "gemm", "gemm"), "decoder_block2": (G1, G2, "gemm", "gemm")},
}
TABLE[2048] = TABLE[1024]   # conv_block7a at 64 x 16: two narrow blocks per plane, the same routes
# block -> (kpart, v, m) floats of workspace at 1024 padded frames, B = 1
SLOTS_1024 = {"encoder_block5": (0, 3538944, 3538944), "encoder_block6": (0, 884736, 884736), "conv_block7a": (786432, 442368, 442368),
              "decoder_block1": (0, 1769472, 884736), "decoder_block2": (0, 7077888, 3538944)}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """run(t_pad, **switches) -> {block: (conv1, conv2, shortcut, up family or None, (kpart, v, m))}"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler in this environment")
    exe = str(tmp_path_factory.mktemp("route_wide") / "route_table")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lass_amd", "csrc"),
                    os.path.join(ROOT, "tools", "route_table.cpp"), "-o", exe], check=True)

    def run(t_pad, **kw):
        a = dict(DEFAULTS, **kw)
        out = subprocess.run([exe, str(t_pad)] + [str(a[k]) for k in ARGS], check=True, capture_output=True, text=True).stdout
        convs, blocks, ups = {}, {}, {}
        for line in out.splitlines():
            f = line.split()
            kv = dict(t.split("=") for t in f if "=" in t)
            if f[0] == "conv":
                convs[f[1]] = (f[2], f[3], int(f[4]), int(f[5]), int(kv["gemm"]))
            elif f[0] == "block":
                blocks[f[1]] = (kv["shortcut"], (int(kv["kpart"]), int(kv["v"]), int(kv["m"])))
            elif f[0] == "up":
                ups[f[1]] = f[2]
        return {b: (convs[b + ".conv1"], convs[b + ".conv2"], blocks[b][0], ups.get(b), blocks[b][1]) for b in TRUNK}
    return run


def _rows(got):
    return {b: r[:4] for b, r in got.items()}


def _slots(got):
    return {b: r[4] for b, r in got.items()}


@pytest.mark.parametrize("t_pad", [128, 512, 1024, 2048])
def test_trunk_routes_at_the_32khz_geometry(table, t_pad):
    got = table(t_pad)
    assert _rows(got) == TABLE[t_pad]
    if t_pad == 1024:
        assert _slots(got) == SLOTS_1024
    if t_pad == 2048:   # twice the rows at every level: every slot doubles
        assert _slots(got) == {b: tuple(2 * x for x in s) for b, s in SLOTS_1024.items()}
    if t_pad == 512:    # conv_block7a has no slot; the others halve
        assert _slots(got) == {b: (0, 0, 0) if b == "conv_block7a" else tuple(x // 2 for x in s) for b, s in SLOTS_1024.items()}


def test_the_multistft_trunk_is_the_same_trunk(table):
    got = table(1024, windows=3)
    assert _rows(got) == TABLE[1024] and _slots(got) == SLOTS_1024


def _fallback(row, v=None, splits=None):
    """a conv off the gemm route: the same family and kind, gemm = 0"""
    return row[:2] + (row[2] if splits is None or row[2] == 1 else splits, row[3] if v is None else min(v, row[3]), 0)


def test_the_switch_falls_back_to_prep_plus_conv_and_split_k(table):
    """WINO4_GEMM = 0: the product image goes, nothing else moves - conv_block7a on the split-K kernels (S = 4) with its V image, the
    others on the V-prep + conv launches of wino4.hip"""
    for t_pad in (512, 1024, 2048):
        got, on = table(t_pad, gemm=0), table(t_pad)
        assert _rows(got) == {b: (_fallback(r[0]), _fallback(r[1]), r[2], r[3]) for b, r in TABLE[t_pad].items()}, t_pad
        assert _slots(got) == {b: (s[0], s[1], 0) for b, s in _slots(on).items()}
    got = table(1024, gemm=0)
    assert got["conv_block7a"][:2] == (("f4x4", "CONV1_ACT", 4, 1, 0), ("f4x4", "CONV2_IDENT", 4, 1, 0))
    assert got["encoder_block6"][:2] == (("f4x4", "CONV1_ACT", 1, 1, 0), W2)
    assert got["decoder_block1"][:2] == (("f4x4", "CONV1_ACT", 1, 1, 0), ("f4x4", "CONV2_IDENT", 1, 1, 0))


@pytest.mark.parametrize("n", [1, 2, 4])
def test_a_forced_split_factor_falls_back_the_same_way(table, n):
    """FORCED_SPLITS = n: every conv leaves the gemm route; only the narrow blocks of conv_block7a take the factor (1: the unsplit
    32 x 16 kernel, no partials)"""
    got = table(1024, splits=n)
    assert _rows(got) == {b: (_fallback(r[0], splits=n), _fallback(r[1], splits=n), r[2], r[3]) for b, r in TABLE[1024].items()}
    assert got["conv_block7a"][0][2] == got["conv_block7a"][1][2] == n
    kpart = n * 384 * 32 * 16 if n > 1 else 0
    assert _slots(got) == {b: (kpart if b == "conv_block7a" else 0, s[1], 0) for b, s in SLOTS_1024.items()}
    if n == 4:
        assert got == table(1024, gemm=0)


def test_without_v_images_the_convs_transform_their_own_input(table):
    """VPREP_MODE = 0: no V from memory, hence no gemm route; conv_block7a stays split-K"""
    got = table(1024, vprep=0)
    assert _rows(got) == {b: (_fallback(r[0], v=0), _fallback(r[1], v=0), r[2], r[3]) for b, r in TABLE[1024].items()}
    assert _slots(got) == {b: (s[0], 0, 0) for b, s in SLOTS_1024.items()}


@pytest.mark.parametrize("t_pad", [128, 512, 1024, 2048])
def test_the_python_mirror_holds_the_same_rows(table, t_pad):
    """lass_amd.arch.conv_layer_table at 1024 bins / wino4_routed: what bench.py's FLOP accounting reads"""
    rows = arch.conv_layer_table(t_pad, arch.MS_F_CROP)
    routed = arch.wino4_routed(rows)
    shape = {r["name"]: (r["h"], r["w"]) for r in rows}
    want = {f"{b}.conv{k + 1}" for b, r in TABLE[t_pad].items() for k in (0, 1) if r[k][0] == "f4x4"}
    assert {n for n in routed if n.rsplit(".", 1)[0] in TRUNK} == want
    assert shape["encoder_block5.conv1"] == shape["decoder_block2.conv2"] == (t_pad // 16, 64)
    assert shape["encoder_block6.conv2"] == shape["decoder_block1.conv1"] == (t_pad // 32, 32)
    assert shape["conv_block7a.conv1"] == (t_pad // 32, 16) and shape["decoder_block1.up"] == (t_pad // 32, 16)
    ms = arch.ms_conv_layer_table(t_pad)
    assert {n for n in arch.wino4_routed(ms) if n.rsplit(".", 1)[0] in TRUNK} == want
