"""Host-only: the weight images of a model - which lass_finalize makes, in which layout, from what - as lass_amd/csrc/weight_plan.h
lists them (plan_weights), and the images every planned launch reads (route_images), printed by tools/weight_table.cpp (built here
with the host compiler).  lass_finalize makes the list with the switches at their defaults and the switches can be thrown afterwards:
whatever they say then, a launch must find its images in that list.  That invariant is held here over the grid of frame counts and
switches; the element counts are held against the channel tables of lass_amd/arch.py."""
import itertools
import os
import shutil
import subprocess

import pytest

from lass_amd import arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lass_amd", "csrc")
MODES = {"f32": 0, "bf16": 1, "bf16x3": 2}
# name -> (WINDOWS, FCROP)
MODELS = {"resunet30": (0, 512), "resunet30_32k": (0, 1024), **{f"multistft{n}": (n, 1024) for n in (1, 2, 3, 4)}}
GRID_MODELS = ("resunet30", "resunet30_32k", "multistft3")
T_PADS = (128, 160, 512, 1024, 2048)
F32_SWITCHES = [dict(zip(("vprep", "splits", "head_fold", "head_sc_fold", "wino4_gemm", "pw_split"), v))
                for v in itertools.product((0, 1, 2), (0, 1, 2, 4), (0, 1), (0, 1), (0, 1), (0, 1))]
BF16_SWITCHES = [dict(zip(("fuse_catb", "fuse_block", "fuse_up"), v)) for v in itertools.product((0, 1), repeat=3)]
DECODER_SLOTS = {"UP16", "UP16L", "UP3"}
CONTEXT_SLOTS = {"UP_SC", "UP_SC16", "HS_WT", "HS_WSKIP"}
LO_SLOTS = {"B1L", "B2L", "BSCL", "UP16L"}
F32_ONLY_SLOTS = {"U1", "U2", "USC", "U1F", "U2F", "U1G", "U2G", "WSC3", "U2H", "WSCH", "BH", "UP3", "HS_WT", "HS_WSKIP"}
F4X4_SLOTS = {"U1F", "U2F", "U1G", "U2G", "U2H", "WSCH", "BH", "HS_WT", "HS_WSKIP"}
BF16_SLOTS = {"B1", "B2", "BSC16", "UP16", "UP_SC", "UP_SC16"} | LO_SLOTS
TWO_BYTE_SLOTS = BF16_SLOTS - {"UP_SC"} | {"U1G", "U2G", "WSC3", "UP3"}


def build_weight_table(tmp_dir):
    """run(model, mode, wino4=32, Q=3, t_pads=(), **switches) -> {"items": [item], "images": {(t_pad, site, name): {slot}}}"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler in this environment"
    exe = os.path.join(str(tmp_dir), "weight_table")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tools", "weight_table.cpp"), "-o", exe], check=True)

    def run(model, mode, wino4=32, Q=3, t_pads=(), **switches):
        windows, fcrop = MODELS[model]
        argv = [str(v) for v in (MODES[mode], wino4, windows, fcrop, Q)]
        if t_pads:
            argv += [",".join(str(t) for t in t_pads)] + [f"{k}={v}" for k, v in sorted(switches.items())]
        return parse(subprocess.run([exe, *argv], check=True, capture_output=True, text=True).stdout)
    return run


def parse(out):
    t = {"items": [], "images": {}}
    t_pad = None
    for line in out.splitlines():
        f = line.split()
        if f[0] == "item":
            rows, cols, taps = (int(x) for x in f[5].split("x"))
            t["items"].append({"owner": f[1], "slot": f[2], "form": f[3], "source": f[4], "rows": rows, "cols": cols, "taps": taps,
                               "count": int(f[6]), "bytes": int(f[7])})
        elif f[0] == "frames":
            t_pad = int(f[1])
        elif f[0] == "images":
            assert (t_pad, f[1], f[2]) not in t["images"]
            t["images"][(t_pad, f[1], f[2])] = set() if f[3] == "-" else set(f[3].split(","))
    return t


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return build_weight_table(tmp_path_factory.mktemp("weight_plan"))


def owner_of(name, slot):
    """the owner whose list holds `slot` for the launch line `name` (a block, or up:<decoder>)"""
    if slot in CONTEXT_SLOTS:
        return "context"
    decoder = name.split(":")[-1]
    return "up:" + decoder if slot in DECODER_SLOTS else name


def check_coverage(table, model, mode, wino4, switch_sets):
    owned = {}
    for it in table(model, mode, wino4)["items"]:       # the plan of lass_finalize: the switches at their defaults
        owned.setdefault(it["owner"], set()).add(it["slot"])
    lines = 0
    for sw in switch_sets:
        images = table(model, mode, wino4, t_pads=T_PADS, **sw)["images"]
        for (t_pad, site, name), slots in images.items():
            lines += 1
            for s in slots:
                assert s in owned.get(owner_of(name, s), ()), (model, mode, wino4, sw, t_pad, site, name, s)
            if wino4 == 0:
                assert not slots & F4X4_SLOTS, (model, mode, sw, t_pad, site, name)
    return lines


@pytest.mark.parametrize("wino4", [32, 0])
@pytest.mark.parametrize("model", GRID_MODELS)
def test_every_planned_launch_finds_its_images_f32(table, model, wino4):
    lines = check_coverage(table, model, "f32", wino4, F32_SWITCHES)
    windows = MODELS[model][0]
    # every block twice (the lass_separate walk, the stage call's default site) and every transposed conv twice
    assert lines == len(F32_SWITCHES) * len(T_PADS) * 2 * ((windows or 1) + 12 + 6)


@pytest.mark.parametrize("wino4", [32, 0])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("model", GRID_MODELS)
def test_every_planned_launch_finds_its_images_bf16(table, model, mode, wino4):
    lines = check_coverage(table, model, mode, wino4, BF16_SWITCHES)
    windows = MODELS[model][0]
    assert 0 < lines <= len(BF16_SWITCHES) * len(T_PADS) * 2 * ((windows or 1) + 12 + 6)    # (a transposed conv inside a fused block has no line)


def test_the_default_plans_read_the_images_the_routes_are_named_for(table):
    """the check above is not vacuous: the routes of the default switches ask for the images their kernels are named for"""
    im = table("resunet30", "f32", t_pads=(1024,))["images"]
    assert im[(1024, "separate", "encoder_block6")] == {"U1G", "U2G"}                       # 16 bins: the gemm route
    assert im[(1024, "separate", "decoder_block2")] == {"WSC", "WSC3", "U1G", "U2G"}        # the split shortcut GEMM in front
    assert im[(1024, "separate", "decoder_block6")] == {"U1F", "U2H", "WSCH", "BH"}         # the folded head
    assert im[(1024, "separate", "encoder_block1")] == {"U1F", "U2F", "HS_WSKIP"}
    assert im[(1024, "separate", "up:decoder_block6")] == {"HS_WT"} and im[(1024, "stage", "up:decoder_block6")] == set()
    assert im[(1024, "separate", "up:decoder_block2")] == {"UP3"}
    off = table("resunet30", "f32", t_pads=(1024,), wino4_gemm=0, pw_split=0, head_fold=0)["images"]
    assert off[(1024, "separate", "encoder_block6")] == {"U1F", "U2F"}
    assert off[(1024, "separate", "decoder_block2")] == {"WSC", "U1F", "U2F"}
    assert off[(1024, "separate", "decoder_block6")] == {"WSC", "U1F", "U2F"}
    assert off[(1024, "separate", "up:decoder_block2")] == set()
    bf = table("resunet30", "bf16", t_pads=(1024,))["images"]
    assert bf[(1024, "separate", "decoder_block6")] == {"B1", "B2", "BSC16", "UP16", "UP_SC16"}       # dec6u: the transposed conv inside
    assert (1024, "separate", "up:decoder_block6") not in bf
    x3 = table("resunet30", "bf16x3", t_pads=(1024,))["images"]
    assert x3[(1024, "separate", "decoder_block5")] == {"B1", "B2", "BSC16", "B1L", "B2L", "BSCL"}
    assert x3[(1024, "separate", "up:decoder_block5")] == {"UP16", "UP16L"}


CASES = list(itertools.product(MODELS, MODES, (32, 0)))


@pytest.mark.parametrize("model,mode,wino4", CASES, ids=[f"{m}-{d}-wino4_{w}" for m, d, w in CASES])
def test_consistency(table, model, mode, wino4):
    items = table(model, mode, wino4)["items"]
    made = set()
    for it in items:
        key = (it["owner"], it["slot"])
        assert key not in made, key                                      # no slot twice for one owner
        if it["source"].startswith("slot:"):                             # made from an image that is already there
            assert (it["owner"], it["source"][5:]) in made, key
        made.add(key)
        assert owner_of(it["owner"], it["slot"]) == it["owner"], key     # block, decoder and context slots at their owners
    slots = {s for _, s in made}
    assert {"W1", "W2", "WSC"} <= slots
    if mode != "bf16x3":
        assert not slots & LO_SLOTS
    if mode != "f32":
        assert not slots & F32_ONLY_SLOTS and {"B1", "B2", "BSC16", "UP16"} <= slots
    else:
        assert not slots & BF16_SLOTS and {"U1", "U2", "USC", "UP3", "WSC3"} <= slots
    if wino4 == 0:
        assert not slots & F4X4_SLOTS
    assert ("UP_SC16" in slots) == ("UP_SC" in slots) == (mode == "bf16" and not MODELS[model][0])


def model_channels(model):
    """{block: (cin, cout)}, {decoder: (cin, cout, uh, uw)} from lass_amd/arch.py"""
    windows = MODELS[model][0]
    blocks = {}
    if windows:
        for k in range(windows):
            blocks[f"encoder_block1s.{k}"] = (arch.PRE_CH, arch.PRE_CH)
        encoders = arch.ms_encoders(tuple(range(windows)))
    else:
        encoders = arch.ENCODERS
    blocks.update({e.name: (e.cin, e.cout) for e in encoders})
    skip = {d.name: e.cout for d, e in zip(arch.DECODERS, reversed(arch.ENCODERS[:6]))}
    skip["decoder_block6"] = arch.PRE_CH * (windows or 1)
    blocks.update({d.name: (d.cout + skip[d.name], d.cout) for d in arch.DECODERS})
    return blocks, {d.name: (d.cin, d.cout, *d.up) for d in arch.DECODERS}


def expected_count(blocks, ups, owner, slot, Q):
    d6 = ups["decoder_block6"]
    if owner == "context":
        return {"UP_SC": 4 * blocks["decoder_block6"][1] * d6[0], "UP_SC16": 4 * blocks["decoder_block6"][1] * d6[0],
                "HS_WT": d6[0] * 64, "HS_WSKIP": Q * arch.PRE_CH}[slot]
    if owner.startswith("up:"):
        cin, cout, uh, uw = ups[owner[3:]]
        return (3 if slot == "UP3" else 1) * cin * cout * uh * uw
    ci, co = blocks[owner]
    u4_chunk = -(-(36 * 8 * 4) // 256) * 256        # one 8-channel chunk of the compact folded-head image, in whole 1-KiB pieces
    return {"W1": 9 * co * ci, "W2": 9 * co * co, "WSC": co * ci, "U1": 16 * co * ci, "U2": 16 * co * co, "USC": 4 * co * ci,
            "U1F": 36 * co * ci, "U2F": 36 * co * co, "U1G": 3 * 36 * co * ci, "U2G": 3 * 36 * co * co, "WSC3": 3 * co * ci,
            "B1": 9 * co * ci, "B2": 9 * co * co, "BSC16": co * ci, "B1L": 9 * co * ci, "B2L": 9 * co * co, "BSCL": co * ci,
            "U2H": co // 8 * u4_chunk, "WSCH": ci * 16, "BH": 16}[slot]


def test_sizes(table):
    for model in MODELS:
        blocks, ups = model_channels(model)
        for mode in MODES:
            items = table(model, mode)["items"]
            assert {it["owner"] for it in items} - {"context"} - {"up:" + d for d in ups} == set(blocks)
            for it in items:
                want = expected_count(blocks, ups, it["owner"], it["slot"], 3)
                assert it["count"] == want, (model, mode, it)
                assert it["bytes"] == want * (2 if it["slot"] in TWO_BYTE_SLOTS else 4), (model, mode, it)
            print(f"{model} {mode}: {len(items)} images, {sum(it['bytes'] for it in items)} bytes")


def test_head_sc_weights(table):
    def has(model, mode, wino4=32, Q=3):
        slots = {(it["owner"], it["slot"]) for it in table(model, mode, wino4, Q)["items"]}
        assert (("context", "HS_WT") in slots) == (("context", "HS_WSKIP") in slots)
        return ("context", "HS_WT") in slots

    assert has("resunet30", "f32") and has("resunet30_32k", "f32")
    assert not any(has(f"multistft{n}", "f32") for n in (1, 2, 3, 4))
    assert not has("resunet30", "f32", wino4=0)
    assert not any(has("resunet30", "f32", Q=q) for q in (0, 1, 2, 4, 16, 17))
    assert not has("resunet30", "bf16") and not has("resunet30", "bf16x3")
    # the folded head's own images need conv2's F(4x4,3x3) image and at most 3 logits, whatever the model
    for model in ("resunet30", "multistft2"):
        for Q, want in ((1, True), (3, True), (4, False)):
            assert (("decoder_block6", "U2H") in {(it["owner"], it["slot"]) for it in table(model, "f32", 32, Q)["items"]}) == want


def test_workspace_table_reads_the_same_rule(table, tmp_path):
    """tools/workspace_table.cpp's default head_sc_weights is head_sc_weights(cfg, m, 3): the argument given says nothing new"""
    from test_workspace_plan_cpu import build_workspace_table
    ws = build_workspace_table(tmp_path)
    for model, name in (("resunet30", "resunet30"), ("resunet30_32k", "resunet30_32k"), ("multistft", "multistft3")):
        for mode in MODES:
            for wino4 in (32, 0):
                rule = int(any(it["slot"] == "HS_WT" for it in table(name, mode, wino4)["items"]))
                assert rule == int(mode == "f32" and model != "multistft" and wino4 > 0)
                for B, L in ((1, 16000), (16, 160000)):
                    assert ws(model, mode, B, L, wino4=wino4) == ws(model, mode, B, L, wino4=wino4, head_sc_weights=rule)
                    if rule:
                        assert ws(model, mode, B, L, wino4=wino4) != ws(model, mode, B, L, wino4=wino4, head_sc_weights=0)
