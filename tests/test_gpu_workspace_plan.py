"""The C-ABI against the printed plan: lass_workspace_bytes and every lass_workspace_tensor row equal what tools/workspace_table.cpp
prints for the same call (workspace_plan.h: make_plan, plan_call; tests/test_workspace_plan_cpu.py holds that table's invariants),
and a batch of 8 on caller-kept buffers runs split or whole as the table says for the workspace it is given - replayed from the
captured graph on the fourth call either way, with the same bytes out as an eager run."""
from ctypes import byref, c_int64, c_size_t, c_void_p

import pytest
import torch

from lass_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 8000
SWITCHES = ("LASS_SPLIT", "LASS_GRAPH", "LASS_WINO4", "LASS_WINO4_VPREP", "LASS_HEAD_FOLD", "LASS_HEAD_SC_FOLD", "LASS_PW_SPLIT",
            "LASS_WINO4_GEMM", "LASS_FUSE_CATB", "LASS_FUSE_BLOCK", "LASS_FUSE_UP")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    from test_workspace_plan_cpu import build_workspace_table   # built here: no compiler is a failure, not a skip
    return build_workspace_table(tmp_path_factory.mktemp("workspace_plan_gpu"))


@pytest.fixture
def default_switches(monkeypatch):
    for s in SWITCHES:   # read at lass_create; the tool's defaults are a context's
        monkeypatch.delenv(s, raising=False)
    return monkeypatch


def tensor_row(e, B, name):
    off, shape, strides = c_size_t(), (c_int64 * 4)(), (c_int64 * 4)()
    rc = e.lib.lass_workspace_tensor(e.ctx, B, L, name.encode(), byref(off), shape, strides)
    return rc, (off.value, tuple(shape), tuple(strides))


@pytest.mark.parametrize("mode", ("f32", "bf16"))
def test_the_abi_answers_from_the_printed_plan(mode, table, synthetic_sd, default_switches):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd, compute_dtype=mode)
    for B in (2, 8):
        t = table("resunet30", mode, B, L)
        assert e.workspace_bytes(B, L) == t["call"]["need"]
        assert len(t["tensors"]) >= 31
        for name, want in t["tensors"].items():
            assert tensor_row(e, B, name) == (0, want), name
        assert tensor_row(e, B, "no_such_tensor")[0] == -1
        assert ("head_sc.skip" in t["tensors"]) == (mode == "f32") and tensor_row(e, B, "head_sc.skip")[0] == (0 if mode == "f32" else -1)


def test_a_batch_of_8_splits_or_not_as_its_workspace_allows(table, synthetic_sd, default_switches):
    from lass_amd.engine import Engine
    B = 8
    t = table("resunet30", "f32", B, L)
    need, total = t["call"]["need"], t["plan"]["total"]
    assert table("resunet30", "f32", B, L, capturing=1, workspace_bytes=need)["call"]["split"] == 1
    _, mix = synthetic.make_mixtures(B, L)
    mix, cond = torch.from_numpy(mix).to(DEV), torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: c_void_p(x.data_ptr())  # noqa: E731

    def four_calls(e, ws_bytes):
        """-> the fourth call's output, and the workspace (caller-kept: the same pointers every time)"""
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
        out = torch.full_like(mix, float("nan"))
        for _ in range(4):
            out.fill_(float("nan"))
            assert e.lib.lass_separate(e.ctx, P(mix), P(cond), P(out), B, L, P(ws), ws.numel(), st) == 0, e.lib.lass_last_error(e.ctx)
        torch.cuda.synchronize()
        return out, ws

    def tap(e, ws, name):
        rc, (off, shape, strides) = tensor_row(e, B, name)
        assert rc == 0 and off % 4 == 0
        return ws.view(torch.float32).as_strided(shape, strides, off // 4)

    e = Engine(DEV)
    e.load_state_dict(synthetic_sd, compute_dtype="f32")
    assert e.workspace_bytes(B, L) == need
    # exactly lass_workspace_bytes: captured on the third call as two half-batch branches, replayed on the fourth
    on, cap0, rep0 = e.graph_stats()
    assert on
    out_split, _ = four_calls(e, need)
    _, cap, rep = e.graph_stats()
    assert cap - cap0 == 1 and rep - rep0 >= 1
    assert tensor_row(e, B, "mag")[0] == -3          # LASS_ERR_STATE: the workspace holds two half-batch layouts
    assert bool(torch.isfinite(out_split).all())
    # the whole plan's bytes only: the same four calls run and replay unsplit, taps stay readable
    if total == need:
        pytest.skip(f"B = {B}, L = {L}: the two half-batch plans take exactly the whole plan's {total} bytes")
    assert table("resunet30", "f32", B, L, capturing=1, workspace_bytes=total)["call"] == {"split": 0, "need": total, "accepted": 1}
    out_whole, ws_whole = four_calls(e, total)
    _, cap2, rep2 = e.graph_stats()
    assert cap2 - cap == 1 and rep2 - rep >= 1
    taps = {n: tap(e, ws_whole, n).clone() for n in ("mag", "x0", "encoder_block3", "decoder_block5", "out_real")}
    # ... and an eager engine (LASS_GRAPH=0; eager calls run whole by default)
    default_switches.setenv("LASS_GRAPH", "0")
    e0 = Engine(DEV)
    e0.load_state_dict(synthetic_sd, compute_dtype="f32")
    out_eager, ws_eager = four_calls(e0, need)
    on0, cap_e, rep_e = e0.graph_stats()
    assert not on0 and cap_e == 0 and rep_e == 0
    assert torch.equal(out_split, out_eager) and torch.equal(out_whole, out_eager)
    for n, got in taps.items():
        assert bool(torch.isfinite(got).all()) and torch.equal(got, tap(e0, ws_eager, n)), n
