"""Host-only: the gemm route of conv_route.h (ConvRoute::gemm, BlockRoute::m_floats - the f32 F(4x4,3x3) convs with 384 output
channels as scatter, 36 batched split-bf16 GEMMs and gather, wino4_gemm.hip) through tools/route_table.cpp, which prints the two
as trailing columns behind the fields of the launches the switch falls back to."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_CONVS = {f"{b}.conv{k}" for b in ("encoder_block5", "encoder_block6", "decoder_block1", "decoder_block2") for k in (1, 2)}
# argument positions of route_table behind T_PAD
ARGS = ("min_cin", "vprep", "splits", "aligned", "windows", "B", "head_fold", "head", "head_sc_fold", "mode", "fuse_catb", "fuse_block",
        "fuse_up", "n_fft", "gemm")
DEFAULTS = dict(min_cin=32, vprep=1, splits=0, aligned=1, windows=0, B=1, head_fold=1, head=1, head_sc_fold=1, mode=0, fuse_catb=1,
                fuse_block=1, fuse_up=1, n_fft=0, gemm=1)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """run(t_pad, **switches) -> ({conv: dict of its line}, {block: dict of its line})"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler in this environment")
    exe = str(tmp_path_factory.mktemp("route_gemm") / "route_table")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lass_amd", "csrc"),
                    os.path.join(ROOT, "tools", "route_table.cpp"), "-o", exe], check=True)

    def run(t_pad, **kw):
        a = dict(DEFAULTS, **kw)
        out = subprocess.run([exe, str(t_pad)] + [str(a[k]) for k in ARGS], check=True, capture_output=True, text=True).stdout
        convs, blocks = {}, {}
        for line in out.splitlines():
            f = line.split()
            kv = dict(t.split("=") for t in f if "=" in t)
            if f[0] == "conv":
                convs[f[1]] = dict(family=f[2], kind=f[3], splits=int(f[4]), v=int(f[5]), gemm=int(kv["gemm"]))
            elif f[0] == "block":
                blocks[f[1]] = dict(kpart=int(kv["kpart"]), v=int(kv["v"]), m=int(kv["m"]))
        return convs, blocks
    return run


def _routed(convs):
    return {n for n, c in convs.items() if c["gemm"]}


def test_a_10s_clip_routes_exactly_the_eight_384_cout_convs(table):
    convs, blocks = table(1024)
    assert _routed(convs) == GEMM_CONVS
    for n in GEMM_CONVS:   # the fields in front still describe the launches the switch falls back to
        assert convs[n]["family"] == "f4x4" and convs[n]["v"] == 1
        assert convs[n]["splits"] == (4 if n.split(".")[0] in ("encoder_block6", "decoder_block1") else 1)
    assert {b for b, v in blocks.items() if v["m"]} == {n.split(".")[0] for n in GEMM_CONVS}


@pytest.mark.parametrize("B", [1, 8, 16])
def test_m_floats(table, B):
    convs, blocks = table(1024, B=B)
    assert _routed(convs) == GEMM_CONVS   # never a function of B
    assert blocks["encoder_block5"]["m"] == blocks["decoder_block2"]["m"] == B * 384 * 64 * 32 * 9 // 4
    assert blocks["encoder_block6"]["m"] == blocks["decoder_block1"]["m"] == B * 384 * 32 * 16 * 9 // 4
    assert all(v["m"] == 0 for b, v in blocks.items() if b not in ("encoder_block5", "encoder_block6", "decoder_block1", "decoder_block2"))


def test_the_switch_and_its_neighbours_turn_it_off(table):
    on_convs, on_blocks = table(1024)
    for kw in (dict(gemm=0), dict(vprep=0), dict(splits=1), dict(splits=2), dict(splits=4), dict(min_cin=0), dict(mode=1), dict(mode=2)):
        convs, blocks = table(1024, **kw)
        assert _routed(convs) == set(), kw
        assert all(v["m"] == 0 for v in blocks.values()), kw
    # ... and the switch moves nothing else
    convs, blocks = table(1024, gemm=0)
    assert {n: {k: v for k, v in c.items() if k != "gemm"} for n, c in convs.items()} == \
           {n: {k: v for k, v in c.items() if k != "gemm"} for n, c in on_convs.items()}
    assert {b: (v["kpart"], v["v"]) for b, v in blocks.items()} == {b: (v["kpart"], v["v"]) for b, v in on_blocks.items()}
    # vprep mode 2 adds V images to shallower layers; the route still asks for 12 cout groups
    assert _routed(table(1024, vprep=2)[0]) == GEMM_CONVS


def test_other_frame_counts(table):
    # 992 padded frames: 31 rows at the 16-bin level and 62 at the 32-bin level tile into no F(4x4,3x3) block at all
    assert _routed(table(992)[0]) == set()
    # 512: the 32-bin level has 32 rows (16 x 32 blocks), the 16-bin level 16 rows (none)
    assert _routed(table(512)[0]) == {f"{b}.conv{k}" for b in ("encoder_block5", "decoder_block2") for k in (1, 2)}
    assert _routed(table(2048)[0]) == GEMM_CONVS


def test_multistft_table_follows_the_same_shape_rule(table):
    """the multi-STFT model (1024 bins) has the same trunk one level wider: the route is set exactly where a conv has V from memory,
    384 output channels and an unforced split factor"""
    for t_pad in (992, 1024):
        convs, blocks = table(t_pad, windows=4)
        # (vprep mode 1 gives V images to the 384-cout layers only; one level wider, conv_block7a sits at 16 bins and is one of them)
        want = {n for n, c in convs.items() if c["v"] and c["family"] == "f4x4"}
        assert _routed(convs) == want, t_pad
        assert want <= GEMM_CONVS | {"conv_block7a.conv1", "conv_block7a.conv2"}
        assert all((blocks[b]["m"] > 0) == any(convs[f"{b}.conv{k}"]["gemm"] for k in (1, 2)) for b in blocks if f"{b}.conv1" in convs)
    assert _routed(table(1024, windows=4)[0]) != set()
