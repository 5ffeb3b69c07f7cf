"""ResUNet30 at the 32 kHz STFT geometry (n_fft 2048, hop 320: lass_create_stft) on the GPU: the two ends of the network against
the float64 STFT oracle, the whole model against the CPU oracle in all three compute modes and for every head route, and the
ragged, windowed, evaluator and graph-replay entry points.

The oracle is the suite's own: oracle/stft.py takes (n_fft, hop) and everything in oracle/resunet.py behind the STFT is
shape-generic, so `oracle.resunet.ostft` is patched with the same four functions bound to (2048, 320).  Seeded synthetic
weights with a 1025-bin bn0; inputs (rand * 2 - 1) * 0.5.  Every shape is the smallest that still takes the path it names."""
import os
import types
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from lass_amd import arch, longform, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
N_FFT, HOP = 2048, 320
NB, FC = N_FFT // 2 + 1, N_FFT // 2


@contextmanager
def oracle_at_geometry():
    """oracle.resunet with its STFT pair bound to (2048, 320); magnitude / phase helpers pass through unchanged."""
    from oracle import resunet as orr
    from oracle import stft as S
    ns = types.SimpleNamespace(stft_fft=lambda x: S.stft_fft(x, N_FFT, HOP),
                               istft_fft=lambda r, i, l: S.istft_fft(r, i, l, N_FFT, HOP),
                               spectrogram_phase=S.spectrogram_phase, magphase=S.magphase)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(orr, "ostft", ns)
        yield orr


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def _noise(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * 0.5


@pytest.fixture(scope="module")
def sd():
    return synthetic.make_state_dict(n_fft=N_FFT)


@pytest.fixture(scope="module")
def model(sd):
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512, n_fft=N_FFT, hop=HOP)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def eng(model):
    e = model.engine
    assert (e.n_fft, e.hop) == (N_FFT, HOP)
    return e


@pytest.fixture(scope="module")
def refs(sd):
    """{L: (mixture (2,1,L), condition (2,512), oracle waveform (2,1,L), taps)}: computed once, shared, never modified."""
    out = {}
    with oracle_at_geometry() as orr:
        tsd = orr.to_torch(sd)
        for L in (32000, 20111):
            mix, cond = _noise((2, 1, L), 500 + L), torch.from_numpy(synthetic.make_condition(2))
            taps = {}
            wav = orr.forward(tsd, {"mixture": mix, "condition": cond}, taps=taps)["waveform"]
            out[L] = (mix, cond, wav, taps)
    return out


def _run(model, mix, cond):
    return model({"mixture": mix.to(DEV), "condition": cond.to(DEV)})["waveform"]


# ---- 1. front end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1025, 7001, 20111])   # T = 4 (the minimum), 22 (even), 63 (odd, L no multiple of the hop)
def test_front_end_vs_f64_oracle(eng, sd, L):
    from oracle import stft as S
    x = _noise((3, L), L)
    x[2] = 0.0   # silence: the 1e-10 clamp
    T, Tp = arch.frames_for(L, HOP), arch.padded_frames(arch.frames_for(L, HOP))
    assert T == {1025: 4, 7001: 22, 20111: 63}[L]
    mag, cos, sin, x0 = (t.cpu() for t in eng.front_end(x.to(DEV)))
    assert mag.shape == (3, T, NB) and x0.shape == (3, Tp, FC)
    m_ref, c_ref, s_ref = (t[:, 0] for t in S.spectrogram_phase(*S.stft_fft(x.double(), N_FFT, HOP)))
    scale = float(m_ref.max())
    e_mag = float((mag.double() - m_ref).abs().max())
    e_re = float((mag.double() * cos.double() - m_ref * c_ref).abs().max())
    e_im = float((mag.double() * sin.double() - m_ref * s_ref).abs().max())
    print(f"L={L} scale={scale:.3f} mag {e_mag:.2e} re {e_re:.2e} im {e_im:.2e}")
    assert e_mag < 2e-6 * scale + 1e-6
    assert e_re < 4e-6 * scale + 1e-6 and e_im < 4e-6 * scale + 1e-6
    assert float((mag[2] - 1e-5).abs().max()) < 1e-11 and not cos[2].any() and not sin[2].any()
    assert not x0[:, T:].any()
    s = torch.from_numpy(sd["base.bn0.weight"] / np.sqrt(sd["base.bn0.running_var"] + 1e-5)).double()
    h = torch.from_numpy(sd["base.bn0.bias"]).double() - torch.from_numpy(sd["base.bn0.running_mean"]).double() * s
    want = (m_ref * s + h)[..., :FC]
    assert float((x0[:, :T].double() - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max()))


# ---- 2. iSTFT ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [7001, 20111])   # T = 22, 63
def test_istft_vs_f64_oracle_and_roundtrip(eng, L):
    from oracle import stft as S
    T = arch.frames_for(L, HOP)
    g = torch.Generator().manual_seed(L)
    re, im = torch.randn(2, T, NB, generator=g), torch.randn(2, T, NB, generator=g)
    im[..., 0] = im[..., -1] = 0.0   # a real frame's spectrum: bins 0 and n_fft/2 are real
    ref = S.istft_fft(re.double()[:, None], im.double()[:, None], L, N_FFT, HOP)
    for y in (eng.istft_nfft(re.to(DEV), im.to(DEV), L, N_FFT, N_FFT), eng.istft(re.to(DEV), im.to(DEV), L)):
        err = float((y.cpu().double() - ref).abs().max())
        print(f"L={L} iSTFT max error {err:.2e} (peak {float(ref.abs().max()):.3f})")
        assert y.shape == (2, L) and err < 1e-5
    x = _noise((2, L), 7 + L)
    _, _, _, sre, sim = eng.stft_magphase(x.to(DEV), want_complex=True)
    assert sre.shape == (2, T, NB)
    back = float((eng.istft(sre, sim, L).cpu() - x).abs().max())
    print(f"L={L} STFT -> iSTFT max error {back:.2e}")
    assert back < 1e-5


# ---- 3. whole model, f32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32000, 20111])   # T = 101 -> Tp = 128 (the G1 shape at this hop), T = 63 -> Tp = 64
def test_model_f32_vs_oracle_every_head_route(model, eng, refs, L):
    mix, cond, ref, taps = refs[L]
    sig = _rms(ref)
    assert ref.shape == (2, 1, L) and sig > 1e-3
    assert taps["x0"].shape == (2, 1, arch.padded_frames(arch.frames_for(L, HOP)), FC) and taps["logits"].shape[-1] == NB
    lib, ctx = eng.lib, eng.ctx
    try:
        for fold, sc in ((1, 1), (1, 0), (0, 1), (0, 0)):
            assert lib.lass_set_head_fold(ctx, fold) == 0 and lib.lass_set_head_sc_fold(ctx, sc) == 0
            out = _run(model, mix, cond)
            err = _rms(out.cpu() - ref)
            print(f"L={L} head_fold={fold} head_sc_fold={sc}: RMS error {err:.3e} (signal {sig:.3e})")
            assert out.shape == (2, 1, L) and err <= 1e-5, (fold, sc, err)
            x0 = eng.workspace_tensor("x0", 2, L).cpu()
            assert float((x0 - taps["x0"]).abs().max()) < 2e-5 * max(1.0, float(taps["x0"].abs().max()))
    finally:
        lib.lass_set_head_fold(ctx, 1)
        lib.lass_set_head_sc_fold(ctx, 1)
    both = _run(model, mix, cond)
    one = _run(model, mix[:1], cond[:1])
    assert torch.equal(one[0], both[0])


# ---- 4. bf16x3 and bf16 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_model_bf16_modes_vs_oracle(model, refs, mode):
    mix, cond, ref, _ = refs[20111]
    try:
        model.set_compute_dtype(mode)
        err = _rms(_run(model, mix, cond).cpu() - ref)
    finally:
        model.set_compute_dtype("f32")
    print(f"{mode}: RMS error {err:.3e} (signal {_rms(ref):.3e})")
    if mode == "bf16x3":
        assert err <= 1e-5
    else:
        assert 1e-7 < err <= 5e-2 * _rms(ref)


# ---- 5. ragged ---------------------------------------------------------------------------------------------------------
def test_ragged_rows_equal_each_clip_alone(model, eng):
    from lass_amd._lib import LassError
    L, lengths = 20111, [10240, 14400, 14401, 20111]
    assert eng.ragged_bucket(L) == (10240, 20111)
    clips = [_noise((n,), 900 + n).to(DEV) for n in lengths]
    cond = torch.from_numpy(synthetic.make_condition(len(lengths))).to(DEV)
    rows = torch.full((len(lengths), L), NAN, device=DEV)
    for b, c in enumerate(clips):
        rows[b, :c.numel()] = c
    out = model.separate_ragged(rows, lengths, cond)
    for b, (n, c) in enumerate(zip(lengths, clips)):
        alone = model({"mixture": c[None, None], "condition": cond[b:b + 1]})["waveform"][0, 0]
        assert torch.equal(out[b, :n], alone) and not out[b, n:].any(), n
    with pytest.raises(LassError):
        model.separate_ragged(rows, [10239] + lengths[1:], cond)
    # separate_list plans with the engine's bucket: the three clips of one bucket share a batch, the shorter one runs apart
    got = model.separate_list([clips[0][:10239]] + clips[1:], cond)
    assert [g.numel() for g in got] == [10239] + lengths[1:] and torch.equal(got[3], out[3, :20111])


def test_ragged_stage_calls_equal_each_clip_alone(eng):
    # rows of 1920 samples: T = 7, Tp = 32, bucket [1025, 1920]; frame counts 4, 5, 5, 5, 6, 7.  The iSTFT's span 1 starts at
    # sample 2560 - 1024 = 1536 (either span candidate): wholly beyond a clip of 1025, at the end of one of 1536, inside 1537
    L, lengths = 1920, [1025, 1536, 1537, 1599, 1600, 1920]
    B, T, Tp = len(lengths), arch.frames_for(L, HOP), 32
    assert T == 7 and eng.ragged_bucket(L) == (1025, L)
    assert [arch.frames_for(n, HOP) for n in lengths] == [4, 5, 5, 5, 6, 7]
    clips = [_noise((n,), 100 + n).to(DEV) for n in lengths]
    rows = torch.full((B, L), NAN, device=DEV)
    for b, c in enumerate(clips):
        rows[b, :c.numel()] = c
    mag, cos, sin, x0 = eng.front_end_ragged(rows, lengths)
    assert x0.shape == (B, Tp, FC) and mag.shape == (B, T, NB)
    solo = [eng.front_end(c[None].contiguous()) for c in clips]
    for b, n in enumerate(lengths):
        tb = arch.frames_for(n, HOP)
        m1, c1, s1, x1 = solo[b]
        assert torch.equal(x0[b, :tb], x1[0, :tb]) and not x0[b, tb:].any(), n
        for got, ref in ((mag, m1), (cos, c1), (sin, s1)):
            assert torch.equal(got[b, :tb], ref[0]) and not got[b, tb:].any(), n
    re = torch.full((B, T, NB), NAN, device=DEV)
    im = torch.full_like(re, NAN)
    for b, (m1, c1, s1, _) in enumerate(solo):
        re[b, :m1.shape[1]], im[b, :m1.shape[1]] = (m1 * c1)[0], (m1 * s1)[0]
    wav = eng.istft_ragged(re, im, lengths, L)
    for b, (n, (m1, c1, s1, _)) in enumerate(zip(lengths, solo)):
        alone = eng.istft_nfft(m1 * c1, m1 * s1, n, N_FFT, N_FFT)[0]
        assert torch.equal(wav[b, :n], alone) and not wav[b, n:].any(), n


# ---- 6. windows --------------------------------------------------------------------------------------------------------
def test_istft_windows_keep_exactly_their_ranges(eng):
    # 1536 = 2560 - 1024 and 4096 = 2 * 2560 - 1024 = 5120 - 1024 are span edges for a span of 8 hops and of 16 hops alike
    W, total = 8000, 20003
    starts = [0, 1000, 6000, 3000, 12003]
    keeps = [(0, 1536), (1536, 4096), (4095, 4097), (4096, 6000), (900, 900)]
    rec = _noise((total,), 7).to(DEV)
    gathered = torch.stack([rec[s:s + W] for s in starts]).contiguous()
    got = eng.front_end_windows(rec, starts, W)
    ref = eng.front_end(gathered)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
    mag, cos, sin, _ = ref
    re, im = mag * cos, mag * sin
    alone = eng.istft_nfft(re, im, W, N_FFT, N_FFT)
    out = torch.full((total,), NAN, device=DEV)
    eng.istft_windows(re, im, starts, keeps, W, out)
    written = torch.zeros(total, dtype=torch.bool, device=DEV)
    for b, (s, (lo, hi)) in enumerate(zip(starts, keeps)):
        assert torch.equal(out[s + lo:s + hi], alone[b, lo:hi]), (s, lo, hi)
        written[s + lo:s + hi] = True
    assert int(written.sum()) == 1536 + 2560 + 2 + 1904
    assert torch.isnan(out[~written]).all() and not torch.isnan(out[written]).any()


def test_separate_long_equals_gathered_windows(model, eng):
    total, W, context = 50003, 20111, 3200
    plan = longform.plan_windows(total, W, context, N_FFT)
    assert len(plan) == 4 and plan[-1][0] == total - W
    rec = _noise((total,), 31).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(1)).to(DEV)
    got = model.separate_long(rec, cond, window=W, context=context, max_batch=4)
    assert got.shape == (total,) and torch.isfinite(got).all()
    batch = torch.stack([rec[s:s + W] for s, _, _ in plan])[:, None].contiguous()
    sep = model({"mixture": batch, "condition": cond.expand(len(plan), -1).contiguous()})["waveform"][:, 0]
    covered = 0
    for b, (s, lo, hi) in enumerate(plan):
        assert torch.equal(got[s + lo:s + hi], sep[b, lo:hi]), (s, lo, hi)
        covered += hi - lo
    assert covered == total


# ---- 7. evaluator ------------------------------------------------------------------------------------------------------
def test_evaluator_from_the_32k_config(tmp_path, sd):
    from lass_amd import evaluator as lev
    from lass_amd.audiosep import PrecomputedQueryEncoder
    from oracle import evaluator as oev
    n, L, SR = 4, 32000, 32000
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=n, length=L, sr=SR)
    ckpt = os.path.join(str(tmp_path), "audiosep_32k.ckpt")
    torch.save({"state_dict": {"ss_model." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, ckpt)
    ev = lev.DCASEEvaluator(sampling_rate=SR, eval_indexes=csv_path, audio_dir=os.path.join(str(tmp_path), "lass_validation"),
                            batch_size=3)
    sdr, sdri, sisdr = lev.eval(ev, ckpt, config_yaml="config/audiosep_32k.yaml", device="cuda")
    clips = [synthetic.make_clip(i, L, SR) for i in range(n)]
    conds = PrecomputedQueryEncoder().get_query_embed("text", [f"synthetic tone cluster {i % 4}" for i in range(n)]).numpy()
    with oracle_at_geometry() as orr:
        (o_sisdr, o_sdri, o_sdr), rows = oev.evaluate(orr.to_torch(sd), clips, conds)
    print("rows (sdr, sdri, sisdr)", np.asarray(ev.last_rows).round(4).tolist(), "oracle", rows.round(4).tolist())
    np.testing.assert_allclose(ev.last_rows, rows, atol=0.01)
    assert abs(sdr - o_sdr) < 0.01 and abs(sdri - o_sdri) < 0.01 and abs(sisdr - o_sisdr) < 0.01


# ---- 8. graph replay ---------------------------------------------------------------------------------------------------
def test_separate_into_replays_its_graph(model, eng):
    B, L = 2, 20111
    mix, out = _noise((B, L), 77).to(DEV), torch.empty(B, L, device=DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    on, cap0, rep0 = eng.graph_stats()
    assert on
    first = model.separate_into(mix, cond, out).clone()
    model.separate_into(mix, cond, out)
    out.fill_(NAN)
    third = model.separate_into(mix, cond, out).clone()   # the third call of a key is captured and runs as the graph
    _, cap1, _ = eng.graph_stats()
    out.fill_(NAN)
    fourth = model.separate_into(mix, cond, out).clone()  # ... and every later one is a replay
    _, cap2, rep2 = eng.graph_stats()
    assert cap1 == cap0 + 1 and cap2 == cap1 and rep2 >= rep0 + 1
    assert torch.equal(third, first) and torch.equal(fourth, first)
