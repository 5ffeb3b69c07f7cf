"""Host-only: lass_amd/csrc/audio_args.h - the operand structs of the audio file entry points and the one statement of each of
their rules - held to tests/golden/audio_refusals.json through tools/audio_args_table.cpp (built here with the host compiler).

The fixture is (entry, case) -> (rc, message) of every argument set of tests/audio_refusal_cases.py, recorded through ctypes from
the entries as they stood before the header existed: their inline checks are the yardstick, never the header itself.  Every case
the header decides must give the recorded message, byte for byte, which also fixes the order of the checks (the two-violation
cases); every good set must give none.  The cases that a device-side predicate decides (lass_resample_true_peak_fits,
lass_loudness_filter) pass the header and are held on the GPU alone (tests/test_audio_refusals_gpu.py)."""
import json
import os
import shutil
import subprocess

import pytest

import audio_refusal_cases as arc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_WORDS = {"lass_resample_true_peak": "do not fit the CU's LDS", "lass_loudness": "coef must be finite",
                "lass_loudness_stats": "coef must be finite"}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """table(entry, args) -> the header's message ("" for accepted)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    exe = str(tmp_path_factory.mktemp("audio_args") / "audio_args_table")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lass_amd", "csrc"),
                    os.path.join(ROOT, "tools", "audio_args_table.cpp"), "-o", exe], check=True)

    def run(entry, args):
        argv = [f"{k}={int(v is not None) if k == 'coef' else v}" for k, v in args.items()]
        out = subprocess.run([exe, entry, *argv], check=True, capture_output=True, text=True).stdout
        assert out.endswith("\n") and out.count("\n") == 1, out
        return out[:-1]
    return run


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "audio_refusals.json")) as f:
        return json.load(f)


def test_the_list_and_the_fixture_cover_each_other(fixture):
    listed = {}
    for entry, cid, _, _ in arc.cases():
        assert cid not in listed.setdefault(entry, set()), (entry, cid)
        listed[entry].add(cid)
    assert set(listed) == set(arc.PARAMS) == set(arc.GOOD) == set(arc.OUTPUTS) and len(listed) == 12
    assert {e: set(v) for e, v in fixture.items()} == listed
    for entry, good in arc.GOOD.items():
        assert set(good) == {n for n, _ in arc.PARAMS[entry]}, entry
    # every recorded refusal is LASS_ERR_ARG under the entry's own name
    for entry, by_case in fixture.items():
        for cid, (rc, msg) in by_case.items():
            assert rc == -1 and msg.startswith(entry + ": "), (entry, cid, rc, msg)


def test_device_side_cases_are_those_two_predicates_and_few(fixture):
    device = [(entry, cid) for entry, cid, _, dev in arc.cases() if dev]
    for entry, cid in device:
        assert DEVICE_WORDS[entry] in fixture[entry][cid][1], (entry, cid)
    # and nothing else was handed to the GPU test alone: every other case with such a message would be a header case gone missing
    for entry, cid, _, dev in arc.cases():
        if not dev:
            assert not any(word in fixture[entry][cid][1] for word in DEVICE_WORDS.values()), (entry, cid)
    assert 0 < len(device) <= 7


def test_header_gives_every_recorded_message(table, fixture):
    checked = 0
    for entry, cid, args, dev in arc.cases():
        got = table(entry, args)
        if dev:
            assert got == "", (entry, cid, got)          # the header passes it on to the predicate
            continue
        assert got == fixture[entry][cid][1], (entry, cid)
        checked += 1
    assert checked >= 380


def test_header_accepts_every_good_set(table):
    for entry, good in arc.GOOD.items():
        assert table(entry, good) == "", entry
    # and the variants the GPU replay runs
    assert table("lass_limit", dict(arc.GOOD["lass_limit"], os=1, os_taps=0, n_os_taps=0, curve=0, envelope=0, min_gain=0, frames=0)) == ""
    assert table("lass_remix_encode", dict(arc.GOOD["lass_remix_encode"], gain=arc.at("gain"))) == ""
