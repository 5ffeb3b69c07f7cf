"""Cross-faded long-form separation on the GPU: lass_separate_windows_faded must store what
lass_separate_windows stores outside the fade regions and ADD the ramp-weighted samples inside them, so that a zone holds
fl(fl(w_a y_a) + fl(w_b y_b)) whatever the grouping of the windows into calls - through the faded iSTFT form, the C entry points
(clamping, split, graph replay, errors), Engine.separate_windows / istft_windows(fade=, ramp=), ResUNet30.separate_long(fade=)
and separate_long_list.  The model of every test: each window gathered and separated ALONE, blended in numpy float32.
Synthetic weights, seeded noise."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from lass_amd import arch, longform, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPAN = 2560   # samples per iSTFT workgroup, at every geometry the library has
# A: W = 4000 (T = 26, Tp = 32), context 500: 7 windows; the total is chosen so that the last, right-aligned window's fade-in
# straddles the span edge at window sample 2048 for both fade lengths, while the other zones lie inside one span.
# B: W = 7777 (T = 49, Tp = 64): the fade-outs [6049, 7283) straddle the edge at 7168, the fade-ins [494, 1728) none.
GEOMETRY = {"A": dict(W=4000, context=500, total=20411), "B": dict(W=7777, context=1111, total=40009)}
FADES = {"A": (400, 1000), "B": (1234,)}


def _noise(n, seed):
    return (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))).to(DEV)


def _cond(seed=0, n=1):
    return torch.from_numpy(synthetic.make_condition(n, seed=synthetic.SEED + seed)).to(DEV)


def _make_model(sd, cls, mode="f32", **kw):
    m = cls(1, 1, 512, **kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).eval().set_compute_dtype(mode)


def _solo(eng, rec, cond, starts, W):
    """Each window gathered and separated alone, as a clip of W samples (numpy float32)."""
    return [eng.separate(rec[s:s + W][None].contiguous(), cond)[0].cpu().numpy() for s in starts]


def _blend(total, rows, solo, ramp, fill=0.0):
    """The model: an output row holding `fill` where no row reaches and 0 where one does, onto which every row stores its plain
    range and adds np.float32(w) * y, rounded to float32, over its fade regions (cut as the header documents).  Returns
    (row, reached)."""
    F = len(ramp)
    want, reached = np.full(total, fill, dtype=np.float32), np.zeros(total, dtype=bool)
    for (s, lo, hi, fin, fout), _ in zip(rows, solo):
        reached[s + lo:s + hi] = True
    want[reached] = 0.0
    for (s, lo, hi, fin, fout), y in zip(rows, solo):
        assert y.dtype == np.float32 and ramp.dtype == np.float32
        in_end, out_begin = longform.fade_regions(lo, hi, fin, fout, F)
        want[s + in_end:s + out_begin] = y[in_end:out_begin]
        want[s + lo:s + in_end] += ramp[:in_end - lo] * y[lo:in_end]                       # ramp[n - lo]
        want[s + out_begin:s + hi] += ramp[:hi - out_begin][::-1] * y[out_begin:hi]        # ramp[hi - 1 - n]
    return want, reached


def _straddles(plan, F, n_fft=1024):
    """Per fade region of the plan: does it reach across a span edge (window samples k * SPAN - n_fft / 2) of its window?"""
    out = []
    for s, lo, hi, fin, fout in plan:
        in_end, out_begin = longform.fade_regions(lo, hi, fin, fout, F)
        for a, b in ((lo, in_end), (out_begin, hi)):
            if a < b:
                out.append((a + n_fft // 2) // SPAN != (b - 1 + n_fft // 2) // SPAN)
    return out


def _args(rows):
    return [r[0] for r in rows], [r[1:3] for r in rows], [r[3:5] for r in rows]


def _run(eng, rec, rows, cond, W, ramp, out):
    starts, keep, fade = _args(rows)
    return eng.separate_windows(rec, starts, keep, cond, W, out=out, fade=fade, ramp=ramp)


@pytest.fixture(scope="module")
def model(synthetic_sd):
    from lass_amd.resunet import ResUNet30
    return _make_model(synthetic_sd, ResUNet30)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def cases(eng):
    """Per geometry: the recording and every window of its plan separated ALONE (the starts do not depend on the fade)."""
    out = {}
    for name, g in GEOMETRY.items():
        W, total = g["W"], g["total"]
        rec, cond = _noise(total, 61 + len(out)), _cond(len(out))
        starts = [p[0] for p in longform.plan_windows(total, W, g["context"])]
        out[name] = dict(W=W, total=total, context=g["context"], rec=rec, cond=cond, starts=starts, solo=_solo(eng, rec, cond, starts, W))
    return out


# ---- 1. the whole row, bit for bit, f32 --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,F", [("A", 400), ("A", 1000), ("B", 1234)])
@pytest.mark.parametrize("shape", ["linear", "hann"])
def test_whole_row_equals_the_blended_windows_f32(cases, eng, name, F, shape):
    c = cases[name]
    W, total = c["W"], c["total"]
    plan = longform.plan_windows_faded(total, W, c["context"], F)
    assert [p[0] for p in plan] == c["starts"] and len(plan) == {"A": 7, "B": 7}[name]
    across = _straddles(plan, F)
    assert any(across) and not all(across), across       # a zone across a span edge and one inside a span: both paths run
    ramp = longform.fade_ramp(F, shape)
    want, reached = _blend(total, plan, c["solo"], ramp)
    assert reached.all()
    got = _run(eng, c["rec"], plan, c["cond"], W, torch.from_numpy(ramp).to(DEV), torch.zeros(total, device=DEV)).cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert np.array_equal(got, want), (name, F, shape, bad[:8], got[bad[:8]], want[bad[:8]])


# ---- 2. grouping independence, graph replay, the split -----------------------------------------------------------------
def test_any_grouping_gives_the_same_bits(model, eng):
    W, context, F, total = 4000, 640, 400, 72011
    plan = longform.plan_windows_faded(total, W, context, F)
    groups = longform.group_windows_faded(plan, 8)
    assert len(plan) == 27 and len(groups) >= 4           # groups 1-2 eager, group 3 is captured, group 4 replays
    # windows 7 | 8 are neighbours in two calls, windows 3 | 4 neighbours on the two half-batches of one call (B = 8 splits 4 + 4)
    assert groups[0][7][4] and groups[1][0][3] and groups[0][7][0] + groups[0][7][2] == groups[1][0][0] + groups[1][0][1] + F
    assert groups[0][3][4] and groups[0][4][3] and groups[0][3][0] + groups[0][3][2] == groups[0][4][0] + groups[0][4][1] + F
    rec, cond = _noise(total, 71), _cond(3)
    ramp = longform.fade_ramp(F)
    want, reached = _blend(total, plan, _solo(eng, rec, cond, [p[0] for p in plan], W), ramp)
    assert reached.all()
    for max_batch in (1, 2, 8):
        _, cap0, rep0 = eng.graph_stats()
        got = model.separate_long(rec, cond, window=W, context=context, max_batch=max_batch, fade=F).cpu().numpy()
        on, cap1, rep1 = eng.graph_stats()
        assert np.array_equal(got, want), max_batch
        if max_batch == 8:
            assert on and cap1 >= cap0 + 1 and rep1 >= rep0 + 1, (cap0, cap1, rep0, rep1)
    eng.set_graph_replay(False)
    try:
        eager = model.separate_long(rec, cond, window=W, context=context, max_batch=8, fade=F).cpu().numpy()
    finally:
        eng.set_graph_replay(True)
    assert np.array_equal(eager, want)


# ---- 3. nothing else is touched ----------------------------------------------------------------------------------------
def test_nothing_outside_the_reached_samples_is_touched(cases, eng):
    """Windows 0, 1, 3 and 6 of case A: zone 0|1 complete, of zones 1|2, 2|3, 3|4 and 5|6 one half only, gaps between."""
    c = cases["A"]
    W, total, F, SENTINEL = c["W"], c["total"], 400, 7.0
    plan = longform.plan_windows_faded(total, W, c["context"], F)
    pick = [0, 1, 3, 6]
    rows = [plan[i] for i in pick]
    ramp = longform.fade_ramp(F)
    want, reached = _blend(total, rows, [c["solo"][i] for i in pick], ramp, fill=SENTINEL)
    assert 0 < int((~reached).sum()) and int(reached.sum()) == sum(r[2] - r[1] for r in rows) - F
    out = torch.from_numpy(np.where(reached, np.float32(0), np.float32(SENTINEL))).to(DEV)
    got = _run(eng, c["rec"], rows, c["cond"], W, torch.from_numpy(ramp).to(DEV), out).cpu().numpy()
    assert (got[~reached] == SENTINEL).all()
    assert np.array_equal(got, want)


# ---- 4. clamping -------------------------------------------------------------------------------------------------------
def test_wrong_entries_are_clamped(cases, eng):
    """Entries that are wrong but harmless by contract, against their documented clamped meaning.  `out` and `ramp` are interior
    slices of larger allocations whose guards (NaN beside the ramp) must come back unchanged: a missing clamp fails an
    assertion here."""
    c = cases["A"]
    W, total, F = c["W"], c["total"], 400
    G = W + F
    ramp = longform.fade_ramp(F)
    big_ramp = torch.full((F + 2 * G,), float("nan"), device=DEV)
    big_ramp[G:G + F] = torch.from_numpy(ramp).to(DEV)
    big_out = torch.full((total + 2 * G,), 3.0, device=DEV)
    big_out[G:G + total] = 0.0
    out = big_out[G:G + total]
    i5, i6 = c["starts"].index(6000), c["starts"].index(12000)
    starts = torch.tensor([-5, 6000, 12000, total], dtype=torch.int64, device=DEV)
    keep = torch.tensor([[-3, W + 9], [1000, 1300], [2000, 2600], [3700, 100]], dtype=torch.int32, device=DEV)
    fade = torch.tensor([[7, -1], [1, 1], [1, 1], [1, 1]], dtype=torch.int32, device=DEV)
    eng.separate_windows(c["rec"], starts, keep, c["cond"], W, out=out, checked=True, fade=fade, ramp=big_ramp[G:G + F])
    # what the header says these mean: starts into [0, total - W], lo into [0, W], hi into [lo, W], any non-zero flag set; a
    # keep shorter than F is all fade-in; one shorter than 2F has its fade-out cut where the fade-in ends; hi < lo keeps nothing
    meant = [(0, 0, W, 1, 1), (6000, 1000, 1300, 1, 1), (12000, 2000, 2600, 1, 1), (total - W, 3700, 3700, 1, 1)]
    assert [longform.fade_regions(*r[1:], F) for r in meant] == [(400, 3600), (1300, 1300), (2400, 2400), (3700, 3700)]
    want, reached = _blend(total, meant, [c["solo"][0], c["solo"][i5], c["solo"][i6], c["solo"][-1]], ramp)
    got = out.cpu().numpy()
    assert int(reached.sum()) == W + 300 + 600 and np.isfinite(got).all()
    assert np.array_equal(got, want)
    assert bool((big_out[:G] == 3.0).all()) and bool((big_out[G + total:] == 3.0).all())
    assert bool(torch.isnan(big_ramp[:G]).all()) and bool(torch.isnan(big_ramp[G + F:]).all())


# ---- 5. bf16 and bf16x3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_bf16_modes_equal_a_gathered_batch_plus_the_blend(cases, synthetic_sd, mode):
    """The control gathers the same 8 windows into an (8, W) batch for lass_separate - same B, same row positions, so the
    launches between the two ends are the same - and blends its rows."""
    from lass_amd.engine import Engine
    c = cases["A"]
    W, total, F = c["W"], c["total"], 400
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd, mode)
    rows = longform.group_windows_faded(longform.plan_windows_faded(total, W, c["context"], F), 8)[0]
    assert len(rows) == 8 and rows[-1][1:] == (0, 0, 0, 0)
    ramp = longform.fade_ramp(F)
    got = _run(e, c["rec"], rows, c["cond"], W, torch.from_numpy(ramp).to(DEV), torch.zeros(total, device=DEV)).cpu().numpy()
    batch = torch.stack([c["rec"][r[0]:r[0] + W] for r in rows]).contiguous()
    sep = e.separate(batch, c["cond"].expand(8, -1).contiguous()).cpu().numpy()
    want, reached = _blend(total, rows, list(sep), ramp)
    assert reached.all() and np.isfinite(got).all()
    assert np.array_equal(got, want)


# ---- 6. the other contexts ---------------------------------------------------------------------------------------------
def _context_case(m, W, total, context, F, max_batch):
    e = m.engine
    rec, cond = _noise(total, 81), _cond(4)
    plan = longform.plan_windows_faded(total, W, context, F, e.n_fft)
    across = _straddles(plan, F, e.n_fft)
    assert any(across) and not all(across), across
    ramp = longform.fade_ramp(F, "hann")
    want, reached = _blend(total, plan, _solo(e, rec, cond, [p[0] for p in plan], W), ramp)
    assert reached.all()
    got = _run(e, rec, plan, cond, W, torch.from_numpy(ramp).to(DEV), torch.zeros(total, device=DEV)).cpu().numpy()
    assert np.array_equal(got, want)
    long = m.separate_long(rec, cond, window=W, context=context, max_batch=max_batch, fade=F, fade_shape="hann")
    assert np.array_equal(long.cpu().numpy(), want)


def test_multistft_context():
    from lass_amd.resunet_with_multistft import ResUNet30 as MsResUNet30
    m = _make_model(synthetic.make_state_dict_ms(), MsResUNet30)
    assert m.engine.multistft == (2048, (256, 512, 2048), 512)
    _context_case(m, 4000, 11911, 500, 400, 4)        # 4 windows; the last one's fade-in [1389, 1789) crosses the edge at 1536


def test_2048_320_context():
    from lass_amd.resunet import ResUNet30
    m = _make_model(synthetic.make_state_dict(n_fft=2048), ResUNet30, n_fft=2048, hop=320)
    assert (m.engine.n_fft, m.engine.hop) == (2048, 320)
    _context_case(m, 9000, 24003, 1000, 800, 2)       # 4 windows; the last one's fade-in [6597, 7397) crosses the edge at 6656


# ---- 7. the stage call -------------------------------------------------------------------------------------------------
def test_istft_windows_faded_equals_istft_nfft_plus_the_blend(cases, eng):
    c = cases["B"]
    W, total, F = c["W"], c["total"], 1234
    plan = longform.plan_windows_faded(total, W, c["context"], F)
    starts, keep, fade = _args(plan)
    mag, cos, sin, _ = eng.front_end_windows(c["rec"], starts, W)
    re, im = mag * cos, mag * sin
    assert re.shape == (len(plan), arch.frames_for(W), 513)
    alone = eng.istft_nfft(re, im, W, 1024, 1024).cpu().numpy()
    ramp = longform.fade_ramp(F)
    want, reached = _blend(total, plan, list(alone), ramp)
    out = torch.zeros(total, device=DEV)
    assert eng.istft_windows(re, im, starts, keep, W, out, fade=fade, ramp=torch.from_numpy(ramp).to(DEV)) is out
    assert reached.all() and np.array_equal(out.cpu().numpy(), want)
    err = float(np.abs(want - c["rec"].cpu().numpy()).max())
    print("front_end_windows -> istft_windows(fade) round trip, max |error|", err)
    assert err < 5e-6          # complementary weights: the blended round trip is still the recording


# ---- 8. separate_long(fade=F) against the CPU oracle --------------------------------------------------------------------
def test_separate_long_faded_vs_oracle(cases, model, synthetic_sd):
    """separate_long(fade=F) against the CPU oracle's forward on each window, blended in float64 by the same plan and ramp:
    1e-4 RMS, the bar of test_longform_gpu.py::test_separate_long_vs_oracle.  And fade=0 is still the hard-seamed stitch."""
    from oracle import resunet as orr
    sd = orr.to_torch(synthetic_sd)
    c = cases["A"]
    W, total, context, F = c["W"], c["total"], c["context"], 400
    got = model.separate_long(c["rec"], c["cond"], window=W, context=context, max_batch=8, fade=F)
    assert got.shape == (total,) and got.dtype == torch.float32 and got.device.type == "cuda"
    plan = longform.plan_windows_faded(total, W, context, F)
    ramp = longform.fade_ramp(F).astype(np.float64)
    want = np.zeros(total, dtype=np.float64)
    for s, lo, hi, fin, fout in plan:
        ref = orr.forward(sd, {"mixture": c["rec"][s:s + W].cpu()[None, None, :], "condition": c["cond"].cpu()})["waveform"]
        y = ref[0, 0].double().numpy()
        in_end, out_begin = longform.fade_regions(lo, hi, fin, fout, F)
        want[s + in_end:s + out_begin] = y[in_end:out_begin]
        want[s + lo:s + in_end] += ramp[:in_end - lo] * y[lo:in_end]
        want[s + out_begin:s + hi] += ramp[:hi - out_begin][::-1] * y[out_begin:hi]
    err = float(np.sqrt(np.mean((got.cpu().double().numpy() - want) ** 2)))
    print("separate_long(fade) RMS error vs oracle", err, "signal RMS", float(np.sqrt(np.mean(want ** 2))))
    assert err <= 1e-4, err
    into = torch.full((total,), 5.0, device=DEV)       # a caller's `out` is zero-filled, whatever it held
    assert model.separate_long(c["rec"], c["cond"], window=W, context=context, max_batch=8, fade=F, out=into) is into
    assert torch.equal(into, got)
    hard = np.empty(total, dtype=np.float32)
    for (s, lo, hi), y in zip(longform.plan_windows(total, W, context), c["solo"]):
        hard[s + lo:s + hi] = y[lo:hi]
    for kw in (dict(), dict(fade=0), dict(fade=0, fade_shape="hann")):
        assert np.array_equal(model.separate_long(c["rec"], c["cond"], window=W, context=context, max_batch=8, **kw).cpu().numpy(), hard)
    with pytest.raises(ValueError):
        model.separate_long(c["rec"], c["cond"], window=W, context=context, fade=401)


# ---- 9. error paths ----------------------------------------------------------------------------------------------------
def test_error_paths_launch_nothing(cases, eng):
    from lass_amd import _lib
    lib, c = eng.lib, cases["A"]
    W, total, B, F = c["W"], c["total"], 2, 400
    rec, out = c["rec"], torch.full((total,), 7.0, device=DEV)
    cond = torch.zeros(B, 512, device=DEV)
    starts = torch.tensor([0, 3000], dtype=torch.int64, device=DEV)
    keep = torch.tensor([[0, 3700], [300, 3700]], dtype=torch.int32, device=DEV)
    fade = torch.tensor([[0, 1], [1, 1]], dtype=torch.int32, device=DEV)
    ramp = torch.from_numpy(longform.fade_ramp(F)).to(DEV)
    ws = torch.empty(eng.workspace_bytes(B, W), dtype=torch.uint8, device=DEV)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    Z = c_void_p(0)
    stats0 = eng.graph_stats()

    def call(fade_=P(fade), ramp_=P(ramp), F_=F, keep_=P(keep), W_=W, B_=B):
        rc = lib.lass_separate_windows_faded(eng.ctx, P(rec), total, P(starts), keep_, fade_, ramp_, F_, P(cond), P(out), B_, W_,
                                             P(ws), ws.numel(), st)
        assert rc in (0, -1), rc                          # LASS_ERR_ARG
        _lib.check(eng.ctx, rc, "lass_separate_windows_faded")

    for kw in (dict(fade_=Z), dict(ramp_=Z), dict(keep_=Z)):
        with pytest.raises(_lib.LassError, match="null pointer"):
            call(**kw)
    for bad in (0, -1, W + 1):
        with pytest.raises(_lib.LassError, match="fade length"):
            call(F_=bad)
    with pytest.raises(_lib.LassError, match="B >= 1"):    # ... and whatever lass_separate_windows refuses
        call(B_=0)
    with pytest.raises(_lib.LassError, match="reflect padding"):
        call(W_=512, F_=400)
    spec = torch.zeros(B, 26, 513, device=DEV)
    istft = lambda fade_, ramp_, F_: lib.lass_istft_windows_faded(eng.ctx, P(spec), P(spec), P(starts), P(keep), fade_, ramp_, F_,  # noqa: E731
                                                                  total, B, 26, W, 1024, 1024, P(out), st)
    assert istft(Z, P(ramp), F) == -1 and istft(P(fade), Z, F) == -1 and istft(P(fade), P(ramp), 0) == -1
    assert istft(P(fade), P(ramp), W + 1) == -1
    with pytest.raises(ValueError, match="go together"):
        eng.separate_windows(rec, [0], [(0, 10)], cond[:1], W, out=out, fade=[(0, 0)])
    with pytest.raises(ValueError, match="overlap"):        # host rows are checked: a stored range over a fade-in
        eng.separate_windows(rec, [0, 3000], [(0, 3400), (300, 3700)], cond[:1], W, out=out, fade=[(0, 0), (1, 0)], ramp=ramp)
    with pytest.raises(_lib.LassError, match="checked"):    # device rows need the caller's word
        eng.separate_windows(rec, starts, keep, cond, W, out=out, fade=fade, ramp=ramp)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and eng.graph_stats() == stats0   # nothing ran
    out.zero_()
    call()                                                            # ... and the same arguments, valid, do run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(out[:3700].any()) and not bool(out[6700:].any())


# ---- 10. several recordings in one pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [0, 400])
def test_separate_long_list_equals_separate_long_of_each(model, eng, F):
    W, context, lengths = 4000, 500, (20011, 9001, 3000)
    recs = [_noise(n, 90 + i) for i, n in enumerate(lengths)]
    conds = _cond(7, n=3)
    assert not torch.equal(conds[0], conds[1])
    # 7 + 3 windows in groups of 8: the first group holds windows of both long recordings; the third recording is a short one
    plans = [longform.plan_windows(n, W, context) for n in lengths[:2]]
    assert [len(p) for p in plans] == [7, 3] and len(plans[0]) < 8 < len(plans[0]) + len(plans[1]) and lengths[2] <= W
    got = model.separate_long_list(recs, conds, window=W, context=context, max_batch=8, fade=F)
    assert len(got) == 3 and [g.shape[0] for g in got] == list(lengths)
    for i, (rec, g) in enumerate(zip(recs, got)):
        alone = model.separate_long(rec, conds[i], window=W, context=context, max_batch=8, fade=F)
        assert g.dtype == torch.float32 and g.device.type == "cuda" and torch.isfinite(g).all()
        assert torch.equal(g, alone), (i, F)
