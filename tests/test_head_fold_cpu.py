"""The folded output head on the CPU: the composition of decoder_block6's conv2 + shortcut with after_conv
(lass_amd/csrc/head_fold.h, held by tools/head_fold_check.cpp under the address and undefined-behaviour sanitizers) and the
route rule that sends the last launch of lass_separate to the folded kernel (lass_amd/csrc/conv_route.h through
tools/route_table.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lass_amd", "csrc")


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    return cxx


def build_route_table(tmp_dir):
    """run(t_pad, min_cin, vprep, splits, aligned, windows, B, head_fold, head) -> {conv name: fold}"""
    exe = os.path.join(str(tmp_dir), "route_table")
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tools", "route_table.cpp"), "-o", exe],
                   check=True)

    def run(t_pad, min_cin=32, vprep=1, splits=0, aligned=1, windows=0, B=1, head_fold=1, head=1):
        out = subprocess.run([exe] + [str(v) for v in (t_pad, min_cin, vprep, splits, aligned, windows, B, head_fold, head)],
                             check=True, capture_output=True, text=True).stdout
        rows = {}
        for line in out.splitlines():
            f = line.split()
            if f[0] == "conv":
                assert f[6].startswith("fold=")
                rows[f[1]] = (f[2], f[3], int(f[6][5:]))
        return rows
    return run


@pytest.fixture(scope="module")
def route_table(tmp_path_factory):
    return build_route_table(tmp_path_factory.mktemp("route_fold"))


def _folded(rows):
    return {n for n, r in rows.items() if r[2]}


def test_composition_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "head_fold_check")
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "head_fold_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
    assert r.stderr == "", r.stderr   # no sanitizer report


# frame counts: 128 = the 16 000-sample clip of the GPU tests, 1024 = the 10 s clip, 992 / 2016 = not a multiple of 32 at the 16-bin
# level, 32 = the shortest plan; every one tiles decoder_block6's 512-bin image into 8 x 64 blocks
@pytest.mark.parametrize("t_pad", [32, 128, 992, 1024, 2016])
def test_only_decoder_block6_conv2_with_a_head_is_folded(route_table, t_pad):
    rows = route_table(t_pad)
    assert _folded(rows) == {"decoder_block6.conv2"}
    assert rows["decoder_block6.conv2"][:2] == ("f4x4", "CONV2_SHORTCUT")
    # the stage call has no head, the switch turns the route off, and so does LASS_WINO4=0; nothing else moves
    for other in (route_table(t_pad, head=0), route_table(t_pad, head_fold=0), route_table(t_pad, min_cin=0)):
        assert _folded(other) == set()
    for off in (route_table(t_pad, head=0), route_table(t_pad, head_fold=0)):
        assert {n: r[:2] for n, r in off.items()} == {n: r[:2] for n, r in rows.items()}


@pytest.mark.parametrize("windows", [1, 3, 4])
def test_multistft_decoder_block6_is_folded(route_table, windows):
    for t_pad in (32, 128, 1024):
        rows = route_table(t_pad, windows=windows)   # 1 024 bins: the 8 x 64 blocks
        assert _folded(rows) == {"decoder_block6.conv2"}
        assert _folded(route_table(t_pad, windows=windows, head_fold=0)) == set()


def test_a_min_cin_above_32_leaves_the_head_unfolded(route_table):
    # decoder_block6.conv2 has 32 input channels: with a higher threshold it is no F(4x4,3x3) launch and cannot fold
    rows = route_table(1024, min_cin=64)
    assert rows["decoder_block6.conv2"][0] != "f4x4" and _folded(rows) == set()
