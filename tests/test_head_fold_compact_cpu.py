"""The compact 4-row weight image of the folded head on the CPU (lass_amd/csrc/head_fold.h: HeadFold::u4, head_fold_u4_index):
tools/head_fold_check.cpp holds it to the 16-row image - the same f32 values, every live element addressed once, row 3 and the tail
of each chunk zero - under the address and undefined-behaviour sanitizers, as a stand-alone host program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lass_amd", "csrc")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    exe = str(tmp_path_factory.mktemp("head_fold_compact") / "head_fold_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "head_fold_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr   # no sanitizer report
    return r.stdout


def test_compact_image_holds_rows_0_to_3_of_the_u_image(check_output):
    # decoder_block6's own shape: 32 input channels x 36 xi x 4 rows, each compared bit for bit with the 16-row image
    lines = [l for l in check_output.splitlines() if "compact image:" in l]
    got = {tuple(int(v) for v in re.match(r"N=(\d+) C=(\d+) K=(\d+) Q=(\d+):", l).groups()): l for l in lines}
    assert set(got) == {(32, 32, 64, 3), (8, 8, 16, 3)}
    assert "%d values equal" % (32 * 36 * 4) in got[(32, 32, 64, 3)] and "row 3 zero" in got[(32, 32, 64, 3)]
    assert "%d values equal" % (8 * 36 * 4) in got[(8, 8, 16, 3)]


def test_no_compact_image_without_a_zero_row(check_output):
    # 16 live logit rows: the 4-row blocks have no zero row to spare, compose_head_fold leaves u4 empty (and lass_finalize the route off)
    assert "N=8 C=16 K=8 Q=16: no compact image" in check_output
    assert check_output.strip().endswith("ok")
