"""The folded head's shortcut logits at their producers, on the CPU: the composition of lass_amd/csrc/head_fold.h
(compose_head_sc_fold, held by tools/head_sc_fold_check.cpp under the address and undefined-behaviour sanitizers) and the route rule
that sends encoder_block1.conv2, decoder_block6's transposed conv and the head to that route together (plan_head_sc_fold of
lass_amd/csrc/conv_route.h, through the last field of tools/route_table.cpp's conv lines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lass_amd", "csrc")
ENDS = {"encoder_block1.conv2", "decoder_block6.conv2"}   # the two ends of the planes that the table shows


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    return cxx


def build_route_table(tmp_dir):
    """run(t_pad, ..., head_sc_fold) -> {conv name: (family, kind, fold, scfold)}"""
    exe = os.path.join(str(tmp_dir), "route_table")
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tools", "route_table.cpp"), "-o", exe],
                   check=True)

    def run(t_pad, min_cin=32, vprep=1, splits=0, aligned=1, windows=0, B=1, head_fold=1, head=1, head_sc_fold=1):
        args = (t_pad, min_cin, vprep, splits, aligned, windows, B, head_fold, head, head_sc_fold)
        out = subprocess.run([exe] + [str(v) for v in args], check=True, capture_output=True, text=True).stdout
        rows = {}
        for line in out.splitlines():
            f = line.split()
            if f[0] == "conv":
                assert f[6].startswith("fold=") and f[-1].startswith("scfold=")
                rows[f[1]] = (f[2], f[3], int(f[6][5:]), int(f[-1][7:]))
        return rows
    return run


@pytest.fixture(scope="module")
def route_table(tmp_path_factory):
    return build_route_table(tmp_path_factory.mktemp("route_sc_fold"))


def _on(rows):
    return {n for n, r in rows.items() if r[3]}


def test_composition_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "head_sc_fold_check")
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "head_sc_fold_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)   # the measured deviations (bar: 1e-12 relative, in double)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
    assert r.stderr == "", r.stderr   # no sanitizer report


# 128 = the 16 000-sample clip of the GPU tests, 1024 = the 10 s clip of the benchmark
@pytest.mark.parametrize("t_pad", [128, 1024])
def test_the_route_is_on_for_the_resunet30_plan(route_table, t_pad):
    rows = route_table(t_pad)
    assert _on(rows) == ENDS
    assert rows["encoder_block1.conv2"][:3] == ("f4x4", "CONV2_IDENT_PRE", 0)
    assert rows["decoder_block6.conv2"][:3] == ("f4x4", "CONV2_SHORTCUT", 1)
    # the batch does not enter the decision
    assert _on(route_table(t_pad, B=16)) == ENDS


@pytest.mark.parametrize("t_pad", [128, 1024])
def test_the_route_is_off_without_its_preconditions(route_table, t_pad):
    rows = route_table(t_pad)
    for what, other in (("head=0", route_table(t_pad, head=0)), ("head_fold=0", route_table(t_pad, head_fold=0)),
                        ("head_sc_fold=0", route_table(t_pad, head_sc_fold=0)), ("min_cin=64", route_table(t_pad, min_cin=64))):
        assert _on(other) == set(), what
    # the switch moves nothing but its own field
    off = route_table(t_pad, head_sc_fold=0)
    assert {n: r[:3] for n, r in off.items()} == {n: r[:3] for n, r in rows.items()}


@pytest.mark.parametrize("windows", [1, 2, 3, 4])
def test_the_route_is_off_for_every_multistft_window_count(route_table, windows):
    for t_pad in (128, 1024):
        rows = route_table(t_pad, windows=windows)
        assert _on(rows) == set()
        assert rows["decoder_block6.conv2"][2] == 1   # the folded head itself stays


def test_the_trailing_argument_is_optional(tmp_path):
    """nine arguments, as the earlier tests pass them, give the default of the tenth; the fields in front of the new one stay"""
    exe = str(tmp_path / "route_table")
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tools", "route_table.cpp"), "-o", exe],
                   check=True)
    nine = subprocess.run([exe, "1024", "32", "1", "0", "1", "0", "1", "1", "1"], check=True, capture_output=True, text=True).stdout
    ten = subprocess.run([exe, "1024", "32", "1", "0", "1", "0", "1", "1", "1", "1"], check=True, capture_output=True, text=True).stdout
    assert nine == ten
    for line in nine.splitlines():
        f = line.split()
        if f[0] == "conv":
            assert len(f) == 8 and f[6].startswith("fold=") and f[7].startswith("scfold=")
