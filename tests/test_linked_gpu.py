"""Linked channels on the GPU: one mask from a guide signal, applied to every channel's spectrum.

What is held to what: the mask to the network's own output on the guide (a derived bound), the masked transform to the restated
float32 product (bit equality), the linked calls to their pieces (bit equality), a plane's result to every other way of running it
(bit equality), the whole to the float64 statement of tests/linked_reference.py, and the file pipeline to the public pieces
composed by hand (byte equality).  Synthetic weights, seeded noise."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import linked_reference as lref
from lass_amd import arch, longform, pipeline, synthetic, wavio
from lass_amd import resample as rs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
# tests/test_longform_gpu.py's two geometries: A: W = 4000 (T = 26, Tp = 32: padded rows), B: W = 7777 (T = 49, odd: an unpaired
# last frame, Tp = 64); and one window length at the (2048, 320) geometry: W = 8001 (T = 26, Tp = 32)
GEOMETRY = {"A": dict(W=4000, context=640, total=20011), "B": dict(W=7777, context=1000, total=30001)}
WIDE = dict(W=8001, context=1300, total=20011)


def _noise(shape, seed):
    return (0.1 * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to(DEV)


def _cond(seed=0, n=1):
    return torch.from_numpy(synthetic.make_condition(n, seed=synthetic.SEED + seed)).to(DEV)


def _same(a, b):
    """Bit equality that lets NaN equal NaN."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _make_model(sd, mode="f32", **kw):
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512, **kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).eval().set_compute_dtype(mode)


def _mask(eng, B, W):
    """M as the last linked call of (B, W) left it in the workspace."""
    return eng.workspace_tensor("out_real", B, W)[:, 0].clone(), eng.workspace_tensor("out_imag", B, W)[:, 0].clone()


def _product(re, im, m_re, m_im):
    """The rule restated in torch float32: four products and two sums, each one elementwise op, each rounded once."""
    return re * m_re - im * m_im, re * m_im + im * m_re


@pytest.fixture(scope="module")
def model(synthetic_sd):
    return _make_model(synthetic_sd)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def wide_model():
    return _make_model(synthetic.make_state_dict(n_fft=2048), n_fft=2048, hop=320)


@pytest.fixture(scope="module")
def cases(eng):
    """Per geometry: a guide, three planes, the plan, and ONE linked call over the whole plan (7 and 5 windows: never split) into
    NaN-filled rows, with the mask it left behind.  Computed once, read by several tests."""
    out = {}
    for k, (name, g) in enumerate(GEOMETRY.items()):
        W, total = g["W"], g["total"]
        guide, planes, cond = _noise(total, 60 + k), _noise((3, total), 70 + k), _cond(k)
        plan = longform.plan_windows(total, W, g["context"])
        got = torch.full((3, total), NAN, device=DEV)
        eng.separate_windows_linked(guide, planes, [p[0] for p in plan], [p[1:] for p in plan], cond, W, out=got)
        m_re, m_im = _mask(eng, len(plan), W)
        out[name] = dict(W=W, total=total, context=g["context"], guide=guide, planes=planes, cond=cond, plan=plan, out=got.clone(),
                         m_re=m_re, m_im=m_im)
    return out


# ---- 1. the mask is the network's ---------------------------------------------------------------------------------------
def _mask_against_unlinked(e, c, rows):
    """|out_real - mag (cos M_re - sin M_im)| <= 1e-6 mag per bin, in float64, and likewise the imaginary part.  Derived: the head's
    own product and the one formed here from M differ by at most about six float32 roundings of factors bounded by 1, 3.6e-7 mag."""
    W, B = c["W"], len(rows)
    starts, keeps = [r[0] for r in rows], [r[1:] for r in rows]
    e.separate_windows(c["guide"], starts, keeps, c["cond"], W)
    mag, cos, sin, o_re, o_im = (e.workspace_tensor(n, B, W)[:, 0].double().cpu() for n in ("mag", "cos", "sin", "out_real", "out_imag"))
    e.separate_windows_linked(c["guide"], c["planes"][:2], starts, keeps, c["cond"], W)
    m_re, m_im = (t.double().cpu() for t in _mask(e, B, W))
    assert float(mag.min()) > 0 and float((m_re ** 2 + m_im ** 2).max()) <= 1.0 + 1e-6 and float(m_re.abs().max()) > 0.01
    assert not m_re[..., -1].any() and not m_im[..., -1].any()            # the Nyquist column is 0, as today's out_real there
    d_re = (o_re - mag * (cos * m_re - sin * m_im)).abs() / mag
    d_im = (o_im - mag * (sin * m_re + cos * m_im)).abs() / mag
    print(f"mask vs the unlinked head: worst |difference| / mag = {float(d_re.max()):.3e} (real), {float(d_im.max()):.3e} (imag)")
    assert float(d_re.max()) <= 1e-6 and float(d_im.max()) <= 1e-6


@pytest.mark.parametrize("name", ["A", "B"])
def test_mask_is_the_networks_f32(cases, eng, name):
    _mask_against_unlinked(eng, cases[name], cases[name]["plan"][:3])


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_mask_is_the_networks_bf16_modes(cases, synthetic_sd, mode):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd, mode)
    _mask_against_unlinked(e, cases["A"], cases["A"]["plan"][:3])


# ---- 2. masked_stft is the restated product, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_masked_stft_equals_the_restated_product(cases, eng, name):
    c = cases[name]
    W, plan, plane = c["W"], c["plan"], c["planes"][0]
    starts = [p[0] for p in plan]
    gathered = torch.stack([plane[s:s + W] for s in starts]).contiguous()
    _, _, _, re, im = eng.stft_magphase(gathered, want_complex=True)
    want = _product(re, im, c["m_re"], c["m_im"])
    for got in (eng.masked_stft_windows(plane, starts, W, c["m_re"], c["m_im"]), eng.masked_stft(gathered, c["m_re"], c["m_im"])):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert not got[0][..., -1].any() and not got[1][..., -1].any()     # the Nyquist column is exactly zero
        assert float(got[0].abs().max()) > 1e-3
    # ragged: every clip from its own frames, exact zeros beyond them
    B = 3
    lengths = [W, W - 1500, max(eng.ragged_bucket(W)[0], W - 3223)]
    rows = torch.full((B, W), NAN, device=DEV)
    for b, n in enumerate(lengths):
        rows[b, :n] = gathered[b, :n]
    y_re, y_im = eng.masked_stft(rows, c["m_re"][:B].contiguous(), c["m_im"][:B].contiguous(), lengths=lengths)
    for b, n in enumerate(lengths):
        Tb = 1 + n // eng.hop
        _, _, _, re, im = eng.stft_magphase(rows[b:b + 1, :n].contiguous(), want_complex=True)
        w_re, w_im = _product(re, im, c["m_re"][b:b + 1, :Tb], c["m_im"][b:b + 1, :Tb])
        assert torch.equal(y_re[b, :Tb], w_re[0]) and torch.equal(y_im[b, :Tb], w_im[0]), (b, n)
        assert not y_re[b, Tb:].any() and not y_im[b, Tb:].any()
    assert 1 + lengths[2] // eng.hop < 1 + W // eng.hop


# ---- 3. the linked output composes from the pieces ----------------------------------------------------------------------
def _compose_windows(e, c, rows, C, fade=None, ramp=None, fill=NAN):
    """One linked call on C planes and, from the mask it leaves, masked_stft_windows + istft_windows per plane."""
    W, total = c["W"], c["total"]
    starts, keeps = [r[0] for r in rows], [r[1:3] for r in rows]
    got = torch.full((C, total), fill, device=DEV)
    e.separate_windows_linked(c["guide"], c["planes"][:C].contiguous(), starts, keeps, c["cond"], W, out=got, fade=fade, ramp=ramp)
    m_re, m_im = _mask(e, len(rows), W)
    want = torch.full((C, total), fill, device=DEV)
    for ch in range(C):
        y_re, y_im = e.masked_stft_windows(c["planes"][ch], starts, W, m_re, m_im)
        e.istft_windows(y_re, y_im, starts, keeps, W, want[ch], fade=fade, ramp=ramp)
    return got, want


@pytest.mark.parametrize("name,C", [("A", 3), ("B", 2)])
def test_linked_windows_compose_from_the_pieces(cases, eng, name, C):
    c = cases[name]
    got, want = _compose_windows(eng, c, c["plan"], C)
    assert torch.isfinite(got).all() and torch.equal(got, want) and torch.equal(got, c["out"][:C])
    assert float(got.abs().max()) > 1e-3


def test_linked_windows_touch_nothing_outside_the_keeps(cases, eng):
    """tests/test_longform_gpu.py's keeps with gaps: inside a span, across a span boundary, one sample, an empty one."""
    c = cases["A"]
    rows = [(0, 100, 900), (2720, 1000, 1000), (5440, 2000, 2100), (8160, 2048, 2700), (10880, 0, 2048), (16011, 3999, 4000)]
    got, want = _compose_windows(eng, c, rows, 2)
    kept = torch.zeros(c["total"], dtype=torch.bool, device=DEV)
    for s, lo, hi in rows:
        kept[s + lo:s + hi] = True
    assert int(kept.sum()) == sum(hi - lo for _, lo, hi in rows)
    assert torch.isnan(got[:, ~kept]).all() and torch.isfinite(got[:, kept]).all() and _same(got, want)


@pytest.mark.parametrize("shape", ["linear", "hann"])
def test_linked_faded_seams_compose_from_the_pieces(cases, eng, shape):
    c = cases["A"]
    F = 400
    plan = longform.plan_windows_faded(c["total"], c["W"], c["context"], F)
    ramp = torch.from_numpy(longform.fade_ramp(F, shape)).to(DEV)
    got, want = _compose_windows(eng, c, plan, 2, fade=[p[3:5] for p in plan], ramp=ramp, fill=0.0)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    assert not torch.equal(got, c["out"][:2])                              # (the seams are cross-faded, not switched)
    hard = longform.plan_windows(c["total"], c["W"], c["context"])
    inner = hard[0][2] - F                                                 # before the first fade zone both are the first window's
    assert torch.equal(got[:, :inner], c["out"][:2, :inner])


def test_linked_ragged_composes_and_writes_the_zero_tail(cases, eng):
    c = cases["A"]
    W, B, C = c["W"], 3, 2
    lengths = [W, W - 1500, max(eng.ragged_bucket(W)[0], W - 3223)]
    guide = torch.full((B, W), NAN, device=DEV)
    planes = torch.full((C, B, W), NAN, device=DEV)
    for b, n in enumerate(lengths):
        guide[b, :n] = c["guide"][b * W:b * W + n]
        planes[:, b, :n] = c["planes"][:C, b * W:b * W + n]
    cond = _cond(9, B)
    got = eng.separate_ragged_linked(guide, lengths, planes, cond, out=torch.full((C, B, W), NAN, device=DEV))
    m_re, m_im = _mask(eng, B, W)
    for ch in range(C):
        y_re, y_im = eng.masked_stft(planes[ch], m_re, m_im, lengths=lengths)
        assert torch.equal(got[ch], eng.istft_ragged(y_re, y_im, lengths, W))
    for b, n in enumerate(lengths):
        assert torch.isfinite(got[:, b, :n]).all() and not got[:, b, n:].any()   # the zero tail is written
        # ... and a clip is what it is alone, dense: guide and plane of its own length
        alone = eng.separate_ragged_linked(guide[b:b + 1, :n].contiguous(), None, planes[:, b:b + 1, :n].contiguous(), cond[b:b + 1])
        assert torch.equal(got[:, b, :n], alone[:, 0])


def test_wide_geometry_composes_from_the_pieces(wide_model):
    """(2048, 320): W = 8001 gives T = 26, Tp = 32; B = 3 windows, C = 2."""
    e = wide_model.engine
    assert (e.n_fft, e.hop) == (2048, 320)
    W, total = WIDE["W"], WIDE["total"]
    c = dict(W=W, total=total, guide=_noise(total, 80), planes=_noise((2, total), 81), cond=_cond(7))
    plan = longform.plan_windows(total, W, WIDE["context"], e.n_fft)
    B = len(plan)
    assert 3 <= B < 8 and arch.frames_for(W, e.hop) == 26
    got, want = _compose_windows(e, c, plan, 2)
    assert torch.isfinite(got).all() and torch.equal(got, want) and float(got.abs().max()) > 1e-3
    starts = [p[0] for p in plan]
    m_re, m_im = _mask(e, B, W)
    assert m_re.shape == (B, 26, 1025) and not m_re[..., -1].any() and not m_im[..., -1].any()
    gathered = torch.stack([c["planes"][1][s:s + W] for s in starts]).contiguous()
    _, _, _, re, im = e.stft_magphase(gathered, want_complex=True)
    y = e.masked_stft_windows(c["planes"][1], starts, W, m_re, m_im)
    w = _product(re, im, m_re, m_im)
    assert torch.equal(y[0], w[0]) and torch.equal(y[1], w[1])
    assert torch.equal(wide_model.separate_long_linked(c["planes"], c["cond"], guide=c["guide"], window=W, context=WIDE["context"], max_batch=4), got)


# ---- 4. invariance, f32 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_a_plane_does_not_depend_on_the_other_planes(cases, eng, name):
    c = cases[name]
    starts, keeps = [p[0] for p in c["plan"]], [p[1:] for p in c["plan"]]
    for ch in range(3):
        one = torch.full((1, c["total"]), NAN, device=DEV)
        eng.separate_windows_linked(c["guide"], c["planes"][ch:ch + 1].contiguous(), starts, keeps, c["cond"], c["W"], out=one)
        assert torch.equal(one[0], c["out"][ch]), (name, ch)


def test_a_window_alone_in_a_split_batch_eager_and_replayed(cases, eng):
    """The first group of 8 of geometry A's plan (7 windows and a padding row): every window alone (B = 1), the group eager
    (unsplit) and, from the fourth identical call on, as the replayed graph of two half-batches - the same bits."""
    c = cases["A"]
    W, total = c["W"], c["total"]
    rows = longform.group_windows(c["plan"], 8)[0]
    assert len(rows) == 8 and rows[-1][1] == rows[-1][2]
    starts, keeps = [r[0] for r in rows], [r[1:] for r in rows]
    planes = c["planes"][:2].contiguous()
    out = torch.full((2, total), NAN, device=DEV)
    _, cap0, rep0 = eng.graph_stats()
    eng.separate_windows_linked(c["guide"], planes, starts, keeps, c["cond"], W, out=out)
    eager = out.clone()
    assert torch.equal(eager, c["out"][:2])                                # B = 8 eager against the B = 7 call
    for _ in range(3):
        out.fill_(NAN)
        eng.separate_windows_linked(c["guide"], planes, starts, keeps, c["cond"], W, out=out)
    on, cap1, rep1 = eng.graph_stats()
    assert on and cap1 == cap0 + 1 and rep1 >= rep0 + 1, (cap0, cap1, rep0, rep1)
    assert torch.equal(out, eager)
    from lass_amd import _lib
    with pytest.raises(_lib.LassError, match="half-batches"):
        eng.workspace_tensor("out_real", 8, W)                             # the replayed graph ran split
    for s, lo, hi in c["plan"][:3] + c["plan"][-1:]:
        alone = torch.full((2, total), NAN, device=DEV)
        eng.separate_windows_linked(c["guide"], planes, [s], [(lo, hi)], c["cond"], W, out=alone)
        assert torch.equal(alone[:, s + lo:s + hi], eager[:, s + lo:s + hi])
        assert int(torch.isfinite(alone[0]).sum()) == hi - lo


def test_long_list_equals_each_recording_alone(cases, model):
    c = cases["A"]
    W, ctx = c["W"], c["context"]
    recs = [c["planes"][:2, :total].contiguous() for total in (20011, 3000, 9000, W)]
    guides = [c["guide"][:r.shape[1]].contiguous() for r in recs]
    conds = _cond(11, len(recs))
    for fade, gd in ((0, guides), (400, None)):                            # (None: every recording's own down-mix)
        got = model.separate_long_list_linked(recs, conds, gd, window=W, context=ctx, max_batch=8, fade=fade)
        for k, r in enumerate(recs):
            alone = model.separate_long_linked(r, conds[k], None if gd is None else gd[k], window=W, context=ctx, max_batch=8, fade=fade)
            assert got[k].shape == r.shape and torch.isfinite(got[k]).all() and torch.equal(got[k], alone), (fade, gd is None, k)
        if gd is None:
            assert torch.equal(got[3], model.separate_long_linked(recs[3], conds[3], model.downmix(recs[3]), window=W, context=ctx))
    with pytest.raises(ValueError, match="one channel count"):
        model.separate_long_list_linked([recs[0], recs[1][:1]], conds[:2], window=W, context=ctx)


def test_a_zero_plane_gives_a_zero_output(cases, eng):
    c = cases["A"]
    planes = c["planes"].clone()
    planes[1] = 0.0
    out = torch.full((3, c["total"]), NAN, device=DEV)
    eng.separate_windows_linked(c["guide"], planes, [p[0] for p in c["plan"]], [p[1:] for p in c["plan"]], c["cond"], c["W"], out=out)
    assert not out[1].any() and torch.equal(out[0], c["out"][0]) and torch.equal(out[2], c["out"][2])


# ---- 5. end to end ------------------------------------------------------------------------------------------------------
def test_one_plane_guiding_itself_against_separate_long(cases, model, synthetic_sd):
    """C = 1 with guide = plane computes what `separate_long` computes, by another route: the head forms the mask alone, and the
    plane's spectrum meets it in the masked transform.  Both device paths are measured against the float64 statement of
    tests/linked_reference.py (which for this case IS the oracle's forward: tests/test_linked_cpu.py), and their difference is
    barred at 4 x the larger of the two deviations - the margin this project gives a float32 device result over the
    float32-vs-float64 deviation of the same computation.  Measured on an MI355X (signal RMS 5.1e-2): linked
    1.360e-8 RMS / 6.875e-8 max and separate_long 1.360e-8 / 5.884e-8 from float64; between the two 4.403e-9 / 2.980e-8 under bars
    of 5.439e-8 / 2.750e-7."""
    from oracle import resunet as orr
    sd64 = orr.to_torch(synthetic_sd, torch.float64)
    c = cases["A"]
    W, total, plane = c["W"], c["total"], c["planes"][0]
    linked = model.separate_long_linked(plane[None].contiguous(), c["cond"], window=W, context=c["context"], max_batch=8)[0]
    plain = model.separate_long(plane, c["cond"], window=W, context=c["context"], max_batch=8)
    x, cond = plane.double().cpu().numpy(), c["cond"].double().cpu().numpy()
    wins = [lref.linked_forward(sd64, x[None, s:s + W], x[None, None, s:s + W], cond)[0, 0] for s, _, _ in c["plan"]]
    ref = lref.stitch(total, c["plan"], wins)
    dev = {}
    for name, y in (("linked", linked), ("separate_long", plain)):
        d = y.double().cpu().numpy() - ref
        dev[name] = (float(np.sqrt(np.mean(d ** 2))), float(np.max(np.abs(d))))
    d = (linked.double() - plain.double()).cpu().numpy()
    rms, worst = float(np.sqrt(np.mean(d ** 2))), float(np.max(np.abs(d)))
    bar_rms, bar_max = 4 * max(v[0] for v in dev.values()), 4 * max(v[1] for v in dev.values())
    print(f"vs float64: linked rms {dev['linked'][0]:.3e} max {dev['linked'][1]:.3e}; separate_long rms {dev['separate_long'][0]:.3e} "
          f"max {dev['separate_long'][1]:.3e}; linked - separate_long rms {rms:.3e} (bar {bar_rms:.3e}) max {worst:.3e} (bar {bar_max:.3e}); "
          f"signal rms {float(np.sqrt(np.mean(ref ** 2))):.3e}")
    assert float(np.sqrt(np.mean(ref ** 2))) > 1e-3
    assert rms <= bar_rms and worst <= bar_max


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cases, eng):
    from lass_amd import _lib
    from lass_amd.engine import Engine
    lib, c = eng.lib, cases["A"]
    W, total, B, C = c["W"], c["total"], 2, 2
    big = torch.zeros(4 * total, device=DEV)
    guide, planes = big[:total], big[total:3 * total]
    out = torch.full((C * total + 8,), 7.0, device=DEV)
    cond = torch.zeros(B, 512, device=DEV)
    starts = torch.tensor([0, 5440], dtype=torch.int64, device=DEV)
    keep = torch.tensor([[0, 3360], [640, 3360]], dtype=torch.int32, device=DEV)
    fade = torch.zeros(B, 2, dtype=torch.int32, device=DEV)
    ramp = torch.ones(16, device=DEV)
    ws = torch.empty(eng.workspace_bytes(B, W), dtype=torch.uint8, device=DEV)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    Z = c_void_p(0)
    stats0 = eng.graph_stats()

    def windows(ctx=eng.ctx, guide_=P(guide), total_=total, starts_=P(starts), keep_=P(keep), fade_=Z, ramp_=Z, F_=0, planes_=P(planes),
                ps=total, C_=C, cond_=P(cond), out_=P(out), ops=total, B_=B, W_=W, ws_=P(ws), bytes_=ws.numel()):
        rc = lib.lass_separate_windows_linked(ctx, guide_, total_, starts_, keep_, fade_, ramp_, F_, planes_, ps, C_, cond_, out_, ops, B_,
                                              W_, ws_, bytes_, st)
        return rc, lib.lass_last_error(ctx).decode()

    def ragged(guide_=P(guide), lens=Z, planes_=P(planes), ps=B * W, C_=C, cond_=P(cond), out_=P(out), ops=B * W, B_=B, L_=W, ws_=P(ws),
               bytes_=ws.numel()):
        rc = lib.lass_separate_ragged_linked(eng.ctx, guide_, lens, planes_, ps, C_, cond_, out_, ops, B_, L_, ws_, bytes_, st)
        return rc, lib.lass_last_error(eng.ctx).decode()

    ARG, WS = -1, -4
    for call, name in ((windows, "lass_separate_windows_linked"), (ragged, "lass_separate_ragged_linked")):
        n = total if call is windows else B * W
        new = [(dict(planes_=Z), "null pointer"), (dict(C_=0), "channels"), (dict(C_=9), "channels"), (dict(C_=-1), "channels"),
               (dict(ps=n - 1), "plane stride"), (dict(ops=n - 1), "plane stride"), (dict(ps=0), "plane stride"),
               (dict(out_=P(guide)), "overlaps the guide"), (dict(out_=P(big[n - 1:])), "overlaps"),
               (dict(out_=P(planes)), "overlaps an input plane"), (dict(out_=P(big[total + n - 1:])), "overlaps an input plane"),
               (dict(out_=P(big[total - n:])), "overlaps")]
        old = [(dict(guide_=Z), "null pointer"), (dict(cond_=Z), "null pointer"), (dict(out_=Z), "null pointer"), (dict(ws_=Z), "null pointer")]
        for kw, text in new + old:
            rc, msg = call(**kw)
            assert rc == ARG and msg.startswith(name) and text in msg, (name, kw, rc, msg)
        rc, msg = call(bytes_=4096)
        assert rc == WS and "workspace too small" in msg, (rc, msg)
    for kw, text in [(dict(fade_=P(fade)), "fade and ramp go together"), (dict(ramp_=P(ramp)), "fade and ramp go together"),
                     (dict(fade_=P(fade), ramp_=P(ramp), F_=0), "fade length"), (dict(fade_=P(fade), ramp_=P(ramp), F_=W + 1), "fade length"),
                     (dict(starts_=Z), "null pointer"), (dict(keep_=Z), "null pointer"), (dict(B_=0), "B >= 1"), (dict(W_=512), "reflect padding"),
                     (dict(total_=W - 1, ps=W - 1, ops=W - 1), "shorter than one window")]:
        rc, msg = windows(**kw)
        assert rc == ARG and msg.startswith("lass_separate_windows_linked") and text in msg, (kw, rc, msg)
    for kw in (dict(B_=0), dict(L_=512)):
        rc, msg = ragged(**kw)
        assert rc == ARG and msg.startswith("lass_separate_ragged_linked"), (kw, rc, msg)
    # a multi-STFT context takes none of the four
    ms = Engine(DEV, multistft=(2048, (256, 512, 2048), 512))
    rc, msg = windows(ctx=ms.ctx)
    assert rc == ARG and "multi-STFT" in msg, (rc, msg)
    spec = torch.zeros(B, 26, 513, device=DEV)
    y = torch.full((2, B, 26, 513), 7.0, device=DEV)
    assert lib.lass_masked_stft(ms.ctx, P(guide), None, B, W, P(spec), P(spec), P(y[0]), P(y[1]), st) == ARG
    assert lib.lass_masked_stft_windows(ms.ctx, P(guide), total, P(starts), B, W, P(spec), P(spec), P(y[0]), P(y[1]), st) == ARG
    # the stage calls' own limits
    for a in ((Z, None, B, W, P(spec), P(spec), P(y[0]), P(y[1])), (P(guide), None, B, W, Z, P(spec), P(y[0]), P(y[1])),
              (P(guide), None, B, W, P(spec), P(spec), Z, P(y[1])), (P(guide), None, 0, W, P(spec), P(spec), P(y[0]), P(y[1])),
              (P(guide), None, B, 512, P(spec), P(spec), P(y[0]), P(y[1]))):
        assert lib.lass_masked_stft(eng.ctx, *a, st) == ARG and lib.lass_last_error(eng.ctx).decode().startswith("lass_masked_stft:")
    assert lib.lass_masked_stft_windows(eng.ctx, P(guide), total, Z, B, W, P(spec), P(spec), P(y[0]), P(y[1]), st) == ARG
    assert lib.lass_masked_stft_windows(eng.ctx, P(guide), W - 1, P(starts), B, W, P(spec), P(spec), P(y[0]), P(y[1]), st) == ARG
    # the Python layer's own
    with pytest.raises(ValueError, match="planes must be"):
        eng.separate_windows_linked(guide, torch.zeros(9, total, device=DEV), [0], [(0, 10)], cond[:1], W)
    with pytest.raises(ValueError, match="planes must be"):
        eng.separate_windows_linked(guide, torch.zeros(2, total - 1, device=DEV), [0], [(0, 10)], cond[:1], W)
    with pytest.raises(ValueError, match="overlap"):
        eng.separate_windows_linked(guide, planes.view(2, total), [0, 2720], [(0, 3360), (639, 3360)], cond[:1], W)
    with pytest.raises(_lib.LassError, match="checked"):
        eng.separate_windows_linked(guide, planes.view(2, total), starts, keep, cond, W)
    with pytest.raises(ValueError, match="fade and ramp go together"):
        eng.separate_windows_linked(guide, planes.view(2, total), [0], [(0, 10)], cond[:1], W, fade=[(0, 0)])
    with pytest.raises(_lib.LassError, match="bucket"):
        eng.separate_ragged_linked(torch.zeros(2, W, device=DEV), [W, 100], torch.zeros(2, 2, W, device=DEV), cond)
    with pytest.raises(ValueError, match="mask must be"):
        eng.masked_stft(torch.zeros(2, W, device=DEV), spec[:, :25].contiguous(), spec[:, :25].contiguous())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((y == 7.0).all()) and eng.graph_stats() == stats0   # nothing ran, nothing was written
    rc, msg = windows(C_=1, out_=P(big[3 * total:]))                       # adjacent rows do not overlap: the good call does run
    torch.cuda.synchronize()
    assert rc == 0, msg


# ---- 7. the file pipeline -----------------------------------------------------------------------------------------------
SR, WINDOW, CONTEXT = 16000, 4000, 640
CAPTIONS = ["a dog barking", "rain on a roof", "a dog barking"]
SPECS = [("a.wav", 2, 40000), ("b.wav", 1, 30011), ("c.wav", 2, 35001)]     # 44.1 kHz PCM16, under a second each


@pytest.fixture(scope="module")
def holder(model):
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    return AudioSep(ss_model=model, query_encoder=PrecomputedQueryEncoder())


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("linkedfiles")
    paths = []
    for i, (name, nch, frames) in enumerate(SPECS):
        rng = np.random.Generator(np.random.PCG64([33, i]))
        t = np.arange(frames)[:, None] / 44100
        x = 0.15 * rng.standard_normal((frames, nch)) + 0.3 * np.sin(2 * np.pi * rng.uniform(200, 3000, nch) * t + rng.uniform(0, 6, nch))
        x[:, -1] *= 0.5                                                     # an off-centre image
        paths.append(str(d / name))
        wavio.write_wav_pcm16(paths[-1], (x if nch > 1 else x[:, 0]).astype(np.float32), 44100)
    return d, paths


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _raw_row(path):
    enc, nch, rate, frames, _ = info = wavio.wav_info(path)
    row = np.zeros((frames * nch * rs.SAMPLE_BYTES[enc] + 3) // 4 * 4, dtype=np.uint8)
    assert wavio.read_wav_raw_into(path, info, row[:frames * nch * rs.SAMPLE_BYTES[enc]])
    return info, torch.from_numpy(row)[None].to(DEV)


def _linked_by_hand(holder, paths, captions, fade=0, db=None):
    """The public pieces: decode_resample (the guide), decode_resample_planar (the planes), separate_long_list_linked per channel
    count, resample_encode (remix_encode with a dB), wav_header."""
    eng = holder.ss_model.engine
    per_file = []
    for p, cap in zip(paths, captions):
        (enc, nch, rate, frames, _), raw = _raw_row(p)
        planes = eng.decode_resample_planar(raw, frames, nch, enc, rate, SR)[0]
        guide = eng.decode_resample(raw, frames, nch, enc, rate, SR)[0]
        cond = holder.query_encoder.get_query_embed(modality="text", text=[cap], device=DEV)[0].to(torch.float32)
        per_file.append((enc, nch, rate, frames, raw, planes, guide, cond))
    seps = [None] * len(paths)
    for group in ([k for k, f in enumerate(per_file) if f[1] == n] for n in (2, 1)):
        outs = holder.ss_model.separate_long_list_linked([per_file[k][5] for k in group], torch.stack([per_file[k][7] for k in group]),
                                                         [per_file[k][6] for k in group], window=WINDOW, context=CONTEXT, fade=fade)
        for k, o in zip(group, outs):
            seps[k] = o
    files = []
    for (enc, nch, rate, frames, raw, _, _, _), sep in zip(per_file, seps):
        if db is None:
            payload = eng.resample_encode(sep.contiguous(), SR, rate, enc, frames_out=frames)
        else:
            amount = torch.tensor([float(pipeline.remix_coefficient(db))], dtype=torch.float32, device=DEV)
            payload = eng.remix_encode(sep.contiguous(), SR, rate, enc, raw, enc, amount, frames_out=frames)
        files.append(wavio.wav_header(enc, nch, rate, frames) + bytes(payload[0].cpu().numpy()))
    return files


@pytest.mark.parametrize("fade", [0, 200])
def test_linked_files_equal_the_pieces_by_hand(holder, files, fade):
    d, paths = files
    outs = [str(d / f"linked_{fade}_{k}.wav") for k in range(3)]
    recs = pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs)), SR, channels="linked", window=WINDOW, context=CONTEXT, fade=fade)
    want = _linked_by_hand(holder, paths, CAPTIONS, fade)
    for p, o, rec, w, (_, nch, frames) in zip(paths, outs, recs, want, SPECS):
        assert wavio.wav_info(o) == ("pcm16", nch, 44100, frames, 44)
        assert rec == dict(rate=44100, channels=nch, frames=frames, path="device", linked=True, clipped=rec["clipped"])
        assert _read(o) == w, (p, fade)
        assert float(np.max(np.abs(wavio.read_wav(o)[0]))) > 1e-3           # (a real signal came out)
    # inference is the one-job call, and other passes give the same files
    one = str(d / "one.wav")
    assert pipeline.inference(holder, paths[0], CAPTIONS[0], one, sampling_rate=SR, channels="linked", window=WINDOW, context=CONTEXT,
                              fade=fade) == recs[0]
    assert _read(one) == want[0]
    again = [str(d / f"again_{fade}_{k}.wav") for k in range(3)]
    pipeline.separate_files(holder, list(zip(paths, CAPTIONS, again)), SR, channels="linked", window=WINDOW, context=CONTEXT, fade=fade,
                            max_samples=1000)
    assert [_read(a) for a in again] == want


def test_linked_remix_equals_the_pieces_by_hand(holder, files):
    d, paths = files
    outs = [str(d / f"tgt_{k}.wav") for k in range(3)]
    mixes = [str(d / f"remix_{k}.wav") for k in range(3)]
    recs = pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs, mixes)), SR, channels="linked", window=WINDOW, context=CONTEXT,
                                   target_gain_db=-12.0)
    for o, m, rec, t, r in zip(outs, mixes, recs, _linked_by_hand(holder, paths, CAPTIONS), _linked_by_hand(holder, paths, CAPTIONS, db=-12.0)):
        assert _read(o) == t and _read(m) == r and t != r
        assert rec["linked"] is True and rec["remix"]["linked"] is True and rec["remix"]["target_gain_db"] == -12.0


def test_each_still_writes_what_the_pieces_give(holder, files, tmp_path):
    """channels="each" on the same files, held to tests/test_export_gpu.py's composition (restated): every channel decoded alone,
    `separate_long_list`, `Engine.resample`, the host writer."""
    d, paths = files
    eng = holder.ss_model.engine
    outs = [str(d / f"each_{k}.wav") for k in range(3)]
    recs = pipeline.separate_files(holder, list(zip(paths, CAPTIONS, outs)), SR, channels="each", window=WINDOW, context=CONTEXT)
    planes, conds, metas = [], [], []
    for p, cap in zip(paths, CAPTIONS):
        enc, nch, rate, frames, _ = info = wavio.wav_info(p)
        row = np.zeros(frames * nch * 2, dtype=np.uint8)
        assert wavio.read_wav_raw_into(p, info, row)
        chans = np.frombuffer(row.tobytes(), dtype="<i2").reshape(frames, nch)
        for ch in range(nch):
            one = np.zeros((frames * 2 + 3) // 4 * 4, dtype=np.uint8)
            one[:frames * 2] = np.frombuffer(np.ascontiguousarray(chans[:, ch]).tobytes(), dtype=np.uint8)
            planes.append(eng.decode_resample(torch.from_numpy(one)[None].to(DEV), frames, 1, enc, rate, SR)[0])
            conds.append(holder.query_encoder.get_query_embed(modality="text", text=[cap], device=DEV)[0])
        metas.append((rate, frames, nch))
    seps = holder.ss_model.separate_long_list(planes, torch.stack(conds), window=WINDOW, context=CONTEXT)
    at = 0
    for k, (rate, frames, nch) in enumerate(metas):
        y = np.stack([eng.resample(s, SR, rate)[:frames].cpu().numpy() for s in seps[at:at + nch]], axis=1)
        at += nch
        hand = str(tmp_path / f"hand{k}.wav")
        wavio.write_wav_pcm16(hand, y if nch > 1 else y[:, 0], rate)
        assert _read(outs[k]) == _read(hand), k
        assert "linked" not in recs[k] and recs[k]["channels"] == nch
