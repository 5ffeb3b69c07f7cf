"""Host-only: the bookkeeping of lass_separate's graph replay (lass_amd/csrc/graph_cache.h) - when a key is worth a capture, which
slot a new key takes, what becomes of an evicted graph - driven through tools/graph_cache_check.cpp (built here with the host
compiler), the exec handle being a plain number.  The HIP calls around it stay in api.hip; tests/test_gpu_workspace_plan.py and
tests/test_gpu_parity.py hold the replays themselves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lass_amd", "csrc")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    exe = os.path.join(str(tmp_path_factory.mktemp("graph_cache")), "graph_cache_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tools", "graph_cache_check.cpp"), "-o", exe],
                   check=True)

    def go(script):
        """One dict per step: {"op": .., field: int} (touch, set, fail) or {"op": .., "execs": [..]} (drained, all)"""
        out = subprocess.run([exe, *script.split()], check=True, capture_output=True, text=True).stdout
        rows = []
        for line in out.splitlines():
            f = line.split()
            if f[0] in ("drained", "all"):
                rows.append({"op": f[0], "execs": [int(x) for x in f[1:]]})
            else:
                rows.append({"op": f[0], **{k: int(v) for k, v in (x.split("=") for x in f[1:])}})
        return rows
    return go


def captured(key, handle):
    """The three sightings of a key and its successful capture"""
    return f"t{key} t{key} t{key} s{handle} "


def test_a_key_is_offered_for_capture_on_its_third_sighting(run):
    r = run("t1 t1 t1 s7 t1 t1")
    assert [x["seen"] for x in r if x["op"] == "touch"] == [1, 2, 3, 4, 5]
    assert [x["capture_due"] for x in r if x["op"] == "touch"] == [0, 0, 1, 0, 0]   # not before, and not again once it has an exec
    assert [x["exec"] for x in r if x["op"] == "touch"] == [0, 0, 0, 7, 7]
    # other keys in between do not reset the count
    r = run("t1 t2 t1 t3 t1")
    assert r[-1]["seen"] == 3 and r[-1]["capture_due"] == 1


def test_a_fifth_key_takes_an_empty_slot_before_one_with_an_exec(run):
    # keys 1 and 2 hold execs and are the least recently used; 3 and 4 are claimed and empty
    r = run(captured(1, 101) + captured(2, 102) + "t3 t4 t5 t1 t2 t4 t3")
    t = [x for x in r if x["op"] == "touch"][-5:]
    assert t[0]["key"] == 5 and t[0]["seen"] == 1 and t[0]["retired"] == 0      # took key 3's slot: the older of the empty ones
    assert (t[1]["exec"], t[2]["exec"]) == (101, 102)                           # both graphs survived
    assert t[3]["key"] == 4 and t[3]["seen"] == 2                               # so did the younger empty slot
    assert t[4]["key"] == 3 and t[4]["seen"] == 1                               # key 3 was evicted: it starts over


def test_with_four_execs_the_least_recently_used_is_evicted_and_retired(run):
    r = run(captured(1, 101) + captured(2, 102) + captured(3, 103) + captured(4, 104) + "t1 t5 d t2 t1 t3 t4")
    t5 = r[-6]
    assert t5["key"] == 5 and t5["seen"] == 1 and t5["exec"] == 0 and t5["retired"] == 1 and t5["drain_due"] == 0
    assert r[-5] == {"op": "drained", "execs": [102]}        # key 1 was used after key 2: key 2's graph went
    t2 = r[-4]
    assert t2["seen"] == 1 and t2["exec"] == 0 and t2["retired"] == 0       # key 2 starts over, in key 5's empty slot
    assert [x["exec"] for x in r[-3:]] == [101, 103, 104]


def test_the_retire_list_asks_to_be_drained_once_it_holds_more_than_eight(run):
    script = "".join(captured(k, 100 + k) for k in range(1, 5))
    script += "".join(captured(k, 100 + k) for k in range(5, 14))     # nine more keys: each first sighting evicts one exec
    r = run(script + "d t13")
    first = [x for x in r if x["op"] == "touch" and x["key"] >= 5 and x["seen"] == 1]
    assert [x["retired"] for x in first] == list(range(1, 10))
    assert [x["drain_due"] for x in first] == [0] * 8 + [1]
    assert r[-2] == {"op": "drained", "execs": [100 + k for k in range(1, 10)]}
    assert r[-1]["exec"] == 113 and r[-1]["retired"] == 0 and r[-1]["drain_due"] == 0
    # take_all hands over what is left, live execs included, and empties the slots
    r = run(captured(1, 101) + captured(2, 102) + captured(3, 103) + captured(4, 104) + "t5 a t1")
    assert sorted(r[-2]["execs"]) == [101, 102, 103, 104] and r[-1]["seen"] == 1 and r[-1]["exec"] == 0


def test_a_failed_capture_leaves_the_slot_claimed_and_empty(run):
    r = run("t1 t1 t1 f t1 t1 s9 t1")
    assert r[3] == {"op": "fail", "exec": 0}
    # the policy offers every later call of the key until one succeeds (lass_separate turns replay off after the first failure)
    assert [(x["seen"], x["exec"], x["capture_due"]) for x in r if x["op"] == "touch"] == [(1, 0, 0), (2, 0, 0), (3, 0, 1), (4, 0, 1), (5, 0, 1), (6, 9, 0)]
    # and the empty slot is the first to go when a new key needs one, although it is the most recently used
    r = run(captured(1, 101) + captured(2, 102) + captured(3, 103) + "t4 t4 t4 f t5 t4")
    assert r[-2]["key"] == 5 and r[-2]["retired"] == 0
    assert r[-1]["key"] == 4 and r[-1]["seen"] == 1 and r[-1]["retired"] == 0       # key 4 starts over, in key 5's empty slot


def test_a_changed_gen_is_a_different_key(run):
    r = run("t1 t1 t1g1 t1 t1g1 t1g1")
    assert [(x["gen"], x["seen"], x["capture_due"]) for x in r] == [(0, 1, 0), (0, 2, 0), (1, 1, 0), (0, 3, 1), (1, 2, 0), (1, 3, 1)]
    r = run(captured(1, 101) + "t1g1")      # lass_finalize bumped gen: the old graph is not replayed for the new weights
    assert r[-1]["exec"] == 0 and r[-1]["seen"] == 1
