"""The printed plan against what ran: the P_CONV3X3 / P_TCONV profiler scopes one lass_separate opens (one per launch in the bf16
modes) equal the `scopes` line tools/route_table.cpp prints for the same plan (conv_route.h: plan_separate), which
tests/test_bf16_routing_cpu.py pins to the same literals.

ResUNet30 runs B = 1, L = 16 000: 101 frames padded to 128 rows, the smallest plan in which every level still exists and both
fused end kernels are eligible.  The multi-STFT model runs B = 1, L = 5 000 (32 rows), the shortest clip
tests/test_multistft_model.py sends through the model."""
import pytest
import torch

from lass_amd import arch, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("LASS_FUSE_CATB", "LASS_FUSE_BLOCK", "LASS_FUSE_UP")
# (model, compute mode, the switch set to 0, (conv3x3_mfma, tconv_mfma) launches; None: what the tool prints for f32)
CASES = [
    ("resunet30", "bf16", None, (24, 5)),
    ("resunet30", "bf16", "LASS_FUSE_UP", (24, 6)),
    ("resunet30", "bf16", "LASS_FUSE_BLOCK", (26, 6)),
    ("resunet30", "bf16", "LASS_FUSE_CATB", (26, 6)),
    ("resunet30", "bf16x3", None, (26, 6)),
    ("resunet30", "f32", None, None),
    ("multistft", "bf16", None, (27, 6)),
]


@pytest.mark.parametrize("model,mode,off,want", CASES, ids=[f"{c[0]}-{c[1]}-{c[2] or 'default'}" for c in CASES])
def test_the_planned_launches_are_the_ones_that_run(model, mode, off, want, synthetic_sd, monkeypatch, tmp_path):
    from lass_amd.engine import Engine
    from test_bf16_routing_cpu import build_route_table
    for s in SWITCHES:   # the switches are read at lass_create
        monkeypatch.delenv(s, raising=False)
    if off:
        monkeypatch.setenv(off, "0")
    ms = model == "multistft"
    L = 5000 if ms else 16000
    t_pad = (arch.frames_for(L) + 31) // 32 * 32
    assert t_pad == (32 if ms else 128)
    # the tool's line for this plan (built here: no compiler is a failure, not a skip)
    table = build_route_table(tmp_path)
    sw = {"catb": int(off != "LASS_FUSE_CATB"), "block": int(off != "LASS_FUSE_BLOCK"), "up": int(off != "LASS_FUSE_UP")}
    planned = table(t_pad, windows=len(arch.MS_WIN_LENGTHS) if ms else 0, mode=Engine.COMPUTE_MODES[mode], **sw)["scopes"]
    if want is None:
        want = planned
    e = Engine(DEV, multistft=(arch.MS_N_FFT, arch.MS_WIN_LENGTHS, arch.MS_MASK_WINDOW) if ms else None)
    e.load_state_dict(synthetic.make_state_dict_ms() if ms else synthetic_sd, compute_dtype=mode)
    _, mix = synthetic.make_mixtures(1, L)
    mix, cond = torch.from_numpy(mix).to(DEV), torch.from_numpy(synthetic.make_condition(1)).to(DEV)
    e.set_profiling(True)
    out = e.separate(mix, cond)
    torch.cuda.synchronize()
    prof = e.profile()
    e.set_profiling(False)
    ran = (prof["conv3x3_mfma"][1], prof["tconv_mfma"][1])
    print(f"{model} {mode} {off or 'default switches'}: planned {planned}, ran {ran}")
    assert bool(torch.isfinite(out).all())
    assert planned == want
    assert ran == want
