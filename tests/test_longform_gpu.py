"""Long-form separation on the GPU: windows of one long recording through lass_separate_windows must keep exactly the samples
the gathered window gives through lass_separate, store them at the window's offset of one long output row and touch nothing
else - through the two window kernels, the C entry points (clamping, split, graph replay),
Engine.separate_windows, ResUNet30.separate_long and chunk_inference(resident=True).  Synthetic weights, seeded noise."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from lass_amd import arch, longform, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
# A: W = 4000 (T = 26, Tp = 32), 7 windows, the last start (16011) a multiple of no hop or span; B: W = 7777 (T = 49, odd, Tp = 64)
GEOMETRY = {"A": dict(W=4000, context=640, total=20011), "B": dict(W=7777, context=1000, total=30001)}


def _rms(a):
    return float(torch.as_tensor(a).double().pow(2).mean().sqrt())


def _noise(n, seed):
    return (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))).to(DEV)


def _cond(seed=0):
    return torch.from_numpy(synthetic.make_condition(1, seed=synthetic.SEED + seed)).to(DEV)


def _make_model(sd, cls, mode="f32"):
    m = cls(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).eval().set_compute_dtype(mode)


def _solo(eng, rec, cond, starts, W):
    """Each window gathered and separated alone, as a clip of W samples."""
    return [eng.separate(rec[s:s + W][None].contiguous(), cond)[0].clone() for s in starts]


def _expected(total, plan, solo):
    """NaN everywhere but in the kept ranges, which hold the gathered windows' samples."""
    want = torch.full((total,), NAN, device=DEV)
    for (s, lo, hi), ref in zip(plan, solo):
        want[s + lo:s + hi] = ref[lo:hi]
    return want


def _same(a, b):
    """Bit equality that lets NaN equal NaN."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.fixture(scope="module")
def model(synthetic_sd):
    from lass_amd.resunet import ResUNet30
    return _make_model(synthetic_sd, ResUNet30)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def cases(eng):
    """Per geometry: the recording, its plan, every window separated ALONE, and one separate_windows call over the whole plan
    into a NaN-filled output.  Computed once, read by several tests."""
    out = {}
    for name, g in GEOMETRY.items():
        W, total = g["W"], g["total"]
        rec, cond = _noise(total, 21 + len(out)), _cond(len(out))
        plan = longform.plan_windows(total, W, g["context"])
        solo = _solo(eng, rec, cond, [p[0] for p in plan], W)
        got = torch.full((total,), NAN, device=DEV)
        eng.separate_windows(rec, [p[0] for p in plan], [p[1:] for p in plan], cond, W, out=got)
        out[name] = dict(W=W, total=total, context=g["context"], rec=rec, cond=cond, plan=plan, solo=solo, out=got.clone())
    return out


# ---- 1. kept samples equal the gathered window, f32 --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_kept_samples_equal_gathered_window_f32(cases, name):
    c = cases[name]
    assert len(c["plan"]) == {"A": 7, "B": 5}[name] and c["plan"][-1][0] == c["total"] - c["W"]
    for (s, lo, hi), ref in zip(c["plan"], c["solo"]):
        assert torch.equal(c["out"][s + lo:s + hi], ref[lo:hi]), (name, s, lo, hi)
    assert torch.isfinite(c["out"]).all()   # the keeps tile the recording


# ---- 2. nothing else is written ----------------------------------------------------------------------------------------
def test_nothing_outside_the_keeps_is_written(cases, eng):
    """Keeps with gaps between them: inside one 2560-sample span (span k holds samples [2560 k - 512, 2560 k + 2048)), across a
    span boundary, from / up to a boundary, one sample, and an empty one."""
    c = cases["A"]
    W, total = c["W"], c["total"]
    rows = [(0, 100, 900), (2720, 1000, 1000), (5440, 2000, 2100), (8160, 2048, 2700), (10880, 0, 2048), (16011, 3999, 4000)]
    idx = [[p[0] for p in c["plan"]].index(s) for s, _, _ in rows]
    got = torch.full((total,), NAN, device=DEV)
    eng.separate_windows(c["rec"], [r[0] for r in rows], [r[1:] for r in rows], c["cond"], W, out=got)
    want = _expected(total, rows, [c["solo"][i] for i in idx])
    kept = ~torch.isnan(want)
    assert int(kept.sum()) == sum(hi - lo for _, lo, hi in rows)
    assert torch.isnan(got[~kept]).all()            # every sample outside the keeps is still NaN
    assert torch.isfinite(got[kept]).all()          # every kept sample is finite
    assert _same(got, want)


# ---- 3. clamping -------------------------------------------------------------------------------------------------------
def test_out_of_range_entries_are_clamped(cases, eng):
    c = cases["A"]
    W, total, G = c["W"], c["total"], 1024
    big_in = torch.full((total + 2 * G,), NAN, device=DEV)
    big_in[G:G + total] = c["rec"]
    big_out = torch.full((total + 2 * G,), NAN, device=DEV)
    rec, out = big_in[G:G + total], big_out[G:G + total]
    starts = torch.tensor([-5, total, 5440, 8160], dtype=torch.int64, device=DEV)
    keep = torch.tensor([[-3, W + 9], [3000, W + 9], [W, 0], [640, 3360]], dtype=torch.int32, device=DEV)
    eng.separate_windows(rec, starts, keep, c["cond"], W, out=out, checked=True)    # returns 0: no LassError
    clamped = [(0, 0, W), (total - W, 3000, W), (5440, W, W), (8160, 640, 3360)]
    ctrl = torch.full((total,), NAN, device=DEV)
    eng.separate_windows(c["rec"], [r[0] for r in clamped], [r[1:] for r in clamped], c["cond"], W, out=ctrl)
    assert _same(out, ctrl)
    idx = [[p[0] for p in c["plan"]].index(s) for s, _, _ in clamped]
    assert _same(ctrl, _expected(total, clamped, [c["solo"][i] for i in idx]))
    assert torch.isnan(big_out[:G]).all() and torch.isnan(big_out[G + total:]).all()   # the guards of `out` are untouched
    kept = ~torch.isnan(ctrl)
    assert torch.isfinite(out[kept]).all() and int(kept.sum()) == W + 1000 + 2720      # no NaN of the input guards got in


# ---- 4. oracle parity --------------------------------------------------------------------------------------------------
def test_separate_long_vs_oracle(cases, model, synthetic_sd):
    """separate_long against the CPU oracle's forward on each window, stitched by the same plan: 1e-4 RMS, the waveform bar."""
    from oracle import resunet as orr
    sd = orr.to_torch(synthetic_sd)
    c = cases["A"]
    got = model.separate_long(c["rec"], c["cond"], window=c["W"], context=c["context"], max_batch=8)
    assert got.shape == (c["total"],) and got.dtype == torch.float32 and got.device.type == "cuda"
    assert torch.equal(got, c["out"])
    want = torch.zeros(c["total"], dtype=torch.float64)
    for s, lo, hi in c["plan"]:
        ref = orr.forward(sd, {"mixture": c["rec"][s:s + c["W"]].cpu()[None, None, :], "condition": c["cond"].cpu()})["waveform"]
        want[s + lo:s + hi] = ref[0, 0, lo:hi].double()
    err = _rms(got.cpu().double() - want)
    print("separate_long RMS error vs oracle", err, "signal RMS", _rms(want))
    assert err <= 1e-4, err


# ---- 5. bf16 and bf16x3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_bf16_modes_equal_a_gathered_batch(cases, synthetic_sd, mode):
    """The control gathers the same 8 windows into an (8, W) batch for lass_separate - same B, same row positions, so the
    launches between the two ends are the same - and copies out the keeps."""
    from lass_amd.engine import Engine
    c = cases["A"]
    W, total = c["W"], c["total"]
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd, mode)
    rows = longform.group_windows(c["plan"], 8)[0]
    assert len(rows) == 8 and rows[-1][1] == rows[-1][2]
    got = torch.full((total,), NAN, device=DEV)
    e.separate_windows(c["rec"], [r[0] for r in rows], [r[1:] for r in rows], c["cond"], W, out=got)
    batch = torch.stack([c["rec"][s:s + W] for s, _, _ in rows]).contiguous()
    sep = e.separate(batch, c["cond"].expand(8, -1).contiguous())
    want = _expected(total, rows, list(sep))
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


# ---- 6. graph replay and split -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_batch,total", [(2, 20011), (8, 72011)])
def test_separate_long_graph_replay(model, eng, max_batch, total):
    """>= 4 groups on the same buffers: groups 1-2 eager, group 3 captures, group 4 replays with rewritten index arrays; at
    max_batch = 8 the captured graph runs two half-batches."""
    W, context = 4000, 640
    plan = longform.plan_windows(total, W, context)
    assert len(longform.group_windows(plan, max_batch)) >= 4
    rec, cond = _noise(total, 31), _cond(3)
    _, cap0, rep0 = eng.graph_stats()
    got = model.separate_long(rec, cond, window=W, context=context, max_batch=max_batch).clone()
    on, cap1, rep1 = eng.graph_stats()
    assert on and cap1 >= cap0 + 1 and rep1 >= rep0 + 1, (cap0, cap1, rep0, rep1)
    eng.set_graph_replay(False)
    try:
        eager = model.separate_long(rec, cond, window=W, context=context, max_batch=max_batch).clone()
        assert eng.graph_stats()[1:] == (cap1, rep1)
    finally:
        eng.set_graph_replay(True)
    assert torch.isfinite(got).all() and torch.equal(got, eager)


# ---- 7. multi-STFT context ---------------------------------------------------------------------------------------------
def test_multistft_kept_samples_equal_gathered_window():
    from lass_amd.resunet_with_multistft import ResUNet30 as MsResUNet30
    m = _make_model(synthetic.make_state_dict_ms(), MsResUNet30)
    e = m.engine
    assert e.multistft == (2048, (256, 512, 2048), 512)
    g = GEOMETRY["A"]
    W, total = g["W"], g["total"]
    rec, cond = _noise(total, 41), _cond(4)
    plan = longform.plan_windows(total, W, g["context"], e.n_fft)
    solo = _solo(e, rec, cond, [p[0] for p in plan], W)
    got = torch.full((total,), NAN, device=DEV)
    e.separate_windows(rec, [p[0] for p in plan], [p[1:] for p in plan], cond, W, out=got)
    assert _same(got, _expected(total, plan, solo)) and torch.isfinite(got).all()
    assert torch.equal(m.separate_long(rec, cond, window=W, context=g["context"], max_batch=4), got)


# ---- 8. stage calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_stage_calls(eng, name):
    g = GEOMETRY[name]
    W, total = g["W"], g["total"]
    gen = torch.Generator().manual_seed(7)
    rec = ((torch.rand(total, generator=gen) * 2 - 1) * 0.5).to(DEV)       # as test_istft_vs_oracle_and_roundtrip
    plan = longform.plan_windows(total, W, g["context"])
    starts = [p[0] for p in plan]
    T = arch.frames_for(W)
    mag, cos, sin, x0 = eng.front_end_windows(rec, starts, W)
    assert x0.shape == (len(plan), arch.padded_frames(T), 512) and mag.shape == (len(plan), T, 513)
    ref = eng.front_end(torch.stack([rec[s:s + W] for s in starts]).contiguous())
    for got, want in zip((mag, cos, sin, x0), ref):
        assert torch.equal(got, want)
    back = torch.full((total,), NAN, device=DEV)
    eng.istft_windows(mag * cos, mag * sin, starts, [p[1:] for p in plan], W, back)
    err = float((back - rec).abs().max())
    print(name, "front_end_windows -> istft_windows round trip, max |error|", err)
    assert err < 5e-6                                                      # NaN (a sample not written) fails this too


# ---- 9. chunk_inference(resident=True) ---------------------------------------------------------------------------------
def test_chunk_inference_resident_equals_default(model, golden_dir):
    g = np.load(os.path.join(golden_dir, "g3_chunk.npz"))
    segs = [synthetic.make_mixtures(1, 160000, first=10 + i)[1][0] for i in range(3)]
    long_mix = np.concatenate(segs)[:400000].astype(np.float32)             # the input of test_chunk_inference_vs_golden
    inp = {"mixture": torch.from_numpy(long_mix)[None, None, :].to(DEV), "condition": torch.from_numpy(synthetic.make_condition(1)).to(DEV)}
    default = model.chunk_inference(inp)
    out = model.chunk_inference(inp, resident=True)
    assert out.shape == (1, 400000) and out.dtype == np.float64
    assert np.array_equal(out, default)
    assert np.sqrt(np.mean((out[0, ::25] - g["out_dec"]) ** 2)) < 3e-6
    for s, seam in zip((32000, 128000, 224000, 320000), g["seams"]):
        np.testing.assert_allclose(out[0, s - 64:s + 64], seam, atol=3e-5)
    short = model.chunk_inference({"mixture": torch.zeros(1, 1, 160000, device=DEV), "condition": inp["condition"]}, resident=True)
    assert short.shape == (1, 160000) and short.dtype == np.float64 and not short.any()


# ---- 10. separate_long edges -------------------------------------------------------------------------------------------
def test_separate_long_edges(model, eng):
    W, context = 4000, 640
    cond = _cond(5)
    for total in (W, 600):                                  # one plain forward
        rec = _noise(total, 50 + total)
        got = model.separate_long(rec, cond, window=W, context=context)
        assert got.shape == (total,) and torch.equal(got, eng.separate(rec[None].contiguous(), cond)[0])
    rec = _noise(W + 1, 52)                                 # two windows one sample apart
    plan = longform.plan_windows(W + 1, W, context)
    assert plan == [(0, 0, W - context), (1, W - context - 1, W)]
    solo = _solo(eng, rec, cond, [0, 1], W)
    got = model.separate_long(rec, cond.reshape(-1), window=W, context=context, max_batch=2)
    want = torch.cat([solo[0][:W - context], solo[1][W - context - 1:]])
    assert torch.equal(got, want)
    into = torch.full((W + 1,), NAN, device=DEV)
    assert model.separate_long(rec, cond, window=W, context=context, max_batch=3, out=into) is into and torch.equal(into, want)
    with pytest.raises(ValueError):
        model.separate_long(_noise(512, 53), cond, window=W, context=context)


# ---- 11. error paths ---------------------------------------------------------------------------------------------------
def test_error_paths_launch_nothing(cases, eng):
    from lass_amd import _lib
    lib, c = eng.lib, cases["A"]
    W, total, B = c["W"], c["total"], 2
    big = torch.zeros(2 * total, device=DEV)
    big[:total] = c["rec"]
    rec, out = big[:total], torch.full((total,), 7.0, device=DEV)
    cond = torch.zeros(B, 512, device=DEV)
    starts = torch.tensor([0, 5440], dtype=torch.int64, device=DEV)
    keep = torch.tensor([[0, 3360], [640, 3360]], dtype=torch.int32, device=DEV)
    ws = torch.empty(eng.workspace_bytes(B, W), dtype=torch.uint8, device=DEV)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    Z = c_void_p(0)
    stats0 = eng.graph_stats()

    def call(recording=P(rec), total_=total, starts_=P(starts), keep_=P(keep), cond_=P(cond), out_=P(out), B_=B, W_=W, ws_=P(ws)):
        rc = lib.lass_separate_windows(eng.ctx, recording, total_, starts_, keep_, cond_, out_, B_, W_, ws_, ws.numel(), st)
        assert rc in (0, -1), rc                          # LASS_ERR_ARG
        _lib.check(eng.ctx, rc, "lass_separate_windows")

    for null in ("recording", "starts_", "keep_", "cond_", "out_", "ws_"):
        with pytest.raises(_lib.LassError, match="null pointer"):
            call(**{null: Z})
    with pytest.raises(_lib.LassError, match="B >= 1"):
        call(B_=0)
    with pytest.raises(_lib.LassError, match="reflect padding"):
        call(W_=512)
    with pytest.raises(_lib.LassError, match="shorter than one window"):
        call(total_=W - 1)
    with pytest.raises(_lib.LassError, match="overlap"):
        call(out_=P(big[total - 1:]))                       # the last sample of recording is the first of out
    with pytest.raises(_lib.LassError, match="overlap"):
        call(out_=P(rec))
    assert lib.lass_front_end_windows(eng.ctx, P(rec), total, Z, B, W, None, None, None, P(out), st) == -1
    assert lib.lass_front_end_windows(eng.ctx, P(rec), W - 1, P(starts), B, W, None, None, None, P(out), st) == -1
    assert lib.lass_istft_windows(eng.ctx, P(rec), P(rec), P(starts), Z, total, B, 26, W, 1024, 1024, P(out), st) == -1
    assert lib.lass_istft_windows(eng.ctx, P(rec), P(rec), P(starts), P(keep), total, B, 25, W, 1024, 1024, P(out), st) == -1
    with pytest.raises(ValueError, match="overlap"):
        eng.separate_windows(rec, [0, 2720], [(0, 3360), (639, 3360)], cond[:1], W, out=out)   # overlapping Python keeps
    with pytest.raises(ValueError, match="start"):
        eng.separate_windows(rec, [0, total - W + 1], [(0, 10), (20, 30)], cond[:1], W, out=out)
    with pytest.raises(_lib.LassError, match="checked"):
        eng.separate_windows(rec, starts, keep, cond, W, out=out)                              # device indices need the caller's word
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and eng.graph_stats() == stats0   # nothing ran
    call(out_=P(big[total:]))                                        # adjacent rows do not overlap ... and the engine still works
    torch.cuda.synchronize()
    assert torch.isfinite(big).all() and big[total:total + 3360].any() and not big[total + 3360:total + 5440 + 640].any()
