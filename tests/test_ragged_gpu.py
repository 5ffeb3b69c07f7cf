"""Ragged batches on the GPU: clips of different lengths of one 32-frame bucket in one lass_separate_ragged call must come out
exactly as each clip separated alone at its own length, with a zero tail, through every layer: the two
per-clip-length kernels, the C entry points (split, graph replay), Engine.separate_ragged, ResUNet30.separate_list and
DCASEEvaluator(ragged=True).  Synthetic weights, seeded noise clips."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from lass_amd import arch, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BUCKET64 = [5120, 5279, 7777, 10079, 10080, 10239]   # Tp = 64: T = 33 (smallest, odd) ... T = 64 = Tp, row length last
BUCKET32 = [513, 800, 3000, 5119]                    # Tp = 32: from the shortest clip the STFT takes


def _rms(a):
    return float(torch.as_tensor(a).double().pow(2).mean().sqrt())


def _clips(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(0.1 * torch.randn(n, generator=g)).to(DEV) for n in lengths]


def _cond(n, seed=0):
    return torch.from_numpy(synthetic.make_condition(n, seed=synthetic.SEED + seed)).to(DEV)


def _rows(clips, fill=0.0):
    row = max(c.shape[0] for c in clips)
    x = torch.full((len(clips), row), fill, dtype=torch.float32, device=DEV)
    for r, c in enumerate(clips):
        x[r, :c.shape[0]] = c
    return x


def _solo(eng, clips, cond):
    return [eng.separate(c[None].contiguous(), cond[i:i + 1].contiguous())[0].clone() for i, c in enumerate(clips)]


def _assert_rows_equal_solo(out, solo, what=""):
    for b, s in enumerate(solo):
        n = s.shape[0]
        assert torch.equal(out[b, :n], s), (what, b, n, float((out[b, :n] - s).abs().max()))
        assert not out[b, n:].any(), (what, b, n, "tail not zero")   # (NaN counts as nonzero)


def _make_model(sd, cls, mode="f32"):
    m = cls(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).eval().set_compute_dtype(mode)


@pytest.fixture(scope="module")
def model(synthetic_sd):
    from lass_amd.resunet import ResUNet30
    return _make_model(synthetic_sd, ResUNet30)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def cases(eng):
    """Per bucket: the clips, their conditions, each clip separated ALONE at its own length, and the ragged call's output on
    zero-padded rows.  Computed once, read by several tests."""
    out = {}
    for name, lengths, seed in (("b64", BUCKET64, 11), ("b32", BUCKET32, 12)):
        clips, cond = _clips(lengths, seed), _cond(len(lengths), seed)
        solo = _solo(eng, clips, cond)
        ragged = eng.separate_ragged(_rows(clips), lengths, cond).clone()
        out[name] = dict(lengths=lengths, clips=clips, cond=cond, solo=solo, ragged=ragged)
    return out


# ---- 1. solo equality, f32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b64", "b32"])
def test_ragged_rows_equal_solo_f32(cases, name):
    c = cases[name]
    assert c["ragged"].shape == (len(c["lengths"]), max(c["lengths"]))
    _assert_rows_equal_solo(c["ragged"], c["solo"], name)


@pytest.mark.parametrize("name", ["b64", "b32"])
def test_ragged_rows_vs_oracle(cases, synthetic_sd, name):
    """Each row against the CPU oracle run on that clip alone: the waveform bar of test_gpu_parity.py, 1e-4 RMS."""
    from oracle import resunet as orr
    sd = orr.to_torch(synthetic_sd)
    c = cases[name]
    for b, n in enumerate(c["lengths"]):
        ref = orr.forward(sd, {"mixture": c["clips"][b].cpu()[None, None, :], "condition": c["cond"][b:b + 1].cpu()})["waveform"]
        err = _rms(c["ragged"][b, :n].cpu() - ref[0, 0])
        print(name, n, "RMS error vs oracle", err)
        assert err <= 1e-4, (n, err)


# ---- 2. nothing beyond a clip's end is read -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b64", "b32"])
def test_ragged_reads_nothing_beyond_a_clip(cases, eng, name):
    c = cases[name]
    out = eng.separate_ragged(_rows(c["clips"], fill=float("nan")), c["lengths"], c["cond"])
    assert torch.equal(out, c["ragged"])


# ---- 3. bf16 and bf16x3 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_ragged_bf16_modes_no_worse_than_batching(cases, synthetic_sd, mode):
    """d_ragged = max |ragged row - the clip alone|; the control d_ctrl is what BATCHING alone does in this mode: the
    equal-length lass_separate on the same six (zero-padded) rows at B = 6 against B = 1.  d_ragged <= d_ctrl; where the mode
    is batch-invariant d_ctrl is 0 and this is bit equality."""
    from lass_amd.engine import Engine
    c = cases["b64"]
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd, mode)
    solo = _solo(e, c["clips"], c["cond"])
    rows = _rows(c["clips"])
    ragged = e.separate_ragged(rows, c["lengths"], c["cond"])
    d_ragged = max(float((ragged[b, :s.shape[0]] - s).abs().max()) for b, s in enumerate(solo))
    assert all(not ragged[b, s.shape[0]:].any() for b, s in enumerate(solo))
    whole = e.separate(rows, c["cond"]).clone()
    d_ctrl = max(float((whole[b] - e.separate(rows[b:b + 1].contiguous(), c["cond"][b:b + 1].contiguous())[0]).abs().max())
                 for b in range(rows.shape[0]))
    print(mode, "d_ragged", d_ragged, "d_ctrl", d_ctrl)
    assert torch.isfinite(ragged).all()
    assert d_ragged <= d_ctrl, (d_ragged, d_ctrl)


# ---- 4. multi-STFT context ----------------------------------------------------------------------------------------------
def test_ragged_multistft_rows_equal_solo():
    from lass_amd.resunet_with_multistft import ResUNet30 as MsResUNet30
    m = _make_model(synthetic.make_state_dict_ms(), MsResUNet30)
    e = m.engine
    assert e.multistft == (2048, (256, 512, 2048), 512)
    lengths = [5120, 6001, 10239]                     # all > n_fft / 2 = 1024, one bucket
    assert e.ragged_bucket(10239) == (5120, 10239) and e.ragged_bucket(4000) == (1025, 4000)
    clips, cond = _clips(lengths, 13), _cond(3, 13)
    solo = _solo(e, clips, cond)
    out = e.separate_ragged(_rows(clips, fill=float("nan")), lengths, cond)
    _assert_rows_equal_solo(out, solo, "multistft")


# ---- 5. split and replay ------------------------------------------------------------------------------------------------
def test_ragged_split_and_graph_replay(cases, eng):
    """B = 8 (an even batch >= 8: the captured graph runs two half-batches, the second reading lengths + 4) on the SAME buffers:
    calls 1-2 eager, call 3 captures, call 4 replays; then the buffers' CONTENTS are permuted in place (same pointers, the
    lengths among them) and the replayed graph must follow."""
    c = cases["b64"]
    pick = [0, 1, 2, 3, 4, 5, 2, 0]
    cond_all = c["cond"][pick].contiguous()
    rows_all = _rows([c["clips"][i] for i in pick])
    lens_all = torch.tensor([c["lengths"][i] for i in pick], dtype=torch.int32)
    mix, cond, out = rows_all.clone(), cond_all.clone(), torch.empty_like(rows_all)
    lens = lens_all.to(DEV)
    _, cap0, rep0 = eng.graph_stats()
    for call in range(4):
        out.fill_(float("nan"))
        eng.separate_ragged(mix, lens, cond, out=out, checked=True)
        _assert_rows_equal_solo(out, [c["solo"][i] for i in pick], f"call {call}")
    _, cap1, rep1 = eng.graph_stats()
    assert cap1 == cap0 + 1 and rep1 == rep0 + 1, (cap0, cap1, rep0, rep1)
    perm = [5, 7, 1, 6, 0, 3, 2, 4]
    mix.copy_(rows_all[perm]); cond.copy_(cond_all[perm]); lens.copy_(lens_all[perm])
    out.fill_(float("nan"))
    eng.separate_ragged(mix, lens, cond, out=out, checked=True)
    _assert_rows_equal_solo(out, [c["solo"][pick[p]] for p in perm], "permuted")
    assert eng.graph_stats()[2] == rep1 + 1


# ---- 6. stage calls -----------------------------------------------------------------------------------------------------
def test_ragged_stage_calls(cases, eng):
    c = cases["b64"]
    lengths, clips = c["lengths"], c["clips"]
    L = max(lengths)
    T, Tp = arch.frames_for(L), arch.padded_frames(arch.frames_for(L))
    mag, cos, sin, x0 = eng.front_end_ragged(_rows(clips, fill=float("nan")), lengths)
    assert x0.shape == (len(lengths), Tp, 512) and mag.shape == (len(lengths), T, 513)
    spectra = []
    for b, n in enumerate(lengths):
        tb = arch.frames_for(n)
        m1, c1, s1, x1 = eng.front_end(clips[b][None].contiguous())
        assert torch.equal(x0[b, :tb], x1[0, :tb]) and not x0[b, tb:].any(), n
        for got, ref in ((mag, m1), (cos, c1), (sin, s1)):
            assert torch.equal(got[b, :tb], ref[0]) and not got[b, tb:].any(), n
        spectra.append(eng.stft_magphase(clips[b][None].contiguous(), want_complex=True)[3:])
    # iSTFT: solo-produced spectra packed into (B, T, 513); what lies beyond a clip's frames must not matter
    re = torch.full((len(lengths), T, 513), float("nan"), device=DEV)
    im = torch.full_like(re, float("nan"))
    for b, (r1, i1) in enumerate(spectra):
        re[b, :r1.shape[1]], im[b, :r1.shape[1]] = r1[0], i1[0]
    wav = eng.istft_ragged(re, im, lengths, L)
    _assert_rows_equal_solo(wav, [eng.istft(r1, i1, n)[0] for (r1, i1), n in zip(spectra, lengths)], "istft")


# ---- 7. separate_list ---------------------------------------------------------------------------------------------------
def test_separate_list_any_lengths_in_input_order(model, eng):
    lengths = [5120, 800, 12000, 7777, 513, 10239, 15359, 3000, 10240, 5119, 10080, 11111]   # three buckets, interleaved
    assert sorted({n // 5120 for n in lengths}) == [0, 1, 2]
    clips, cond = _clips(lengths, 14), _cond(len(lengths), 14)
    solo = _solo(eng, clips, cond)
    got = model.separate_list([c.cpu() if i % 2 else c for i, c in enumerate(clips)], cond, max_batch=3)
    assert len(got) == len(lengths)
    for i, (g, s) in enumerate(zip(got, solo)):
        assert g.shape == (lengths[i],) and torch.equal(g, s), (i, lengths[i])


# ---- 8. evaluator ---------------------------------------------------------------------------------------------------------
def test_evaluator_ragged_equals_clip_by_clip(tmp_path, model, monkeypatch):
    """10 pairs of 4 distinct lengths, interleaved so that grouping consecutive equal lengths yields batches of one.  The
    waveforms are bit-equal either way; the dB rows differ by the order of the f64 sums only: 1e-3 dB."""
    from lass_amd import wavio
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.evaluator import DCASEEvaluator
    lengths = [16000, 12000, 14000, 11000, 16000, 14000, 12000, 11000, 14000, 16000]
    assert len(set(lengths)) == 4 and all(a != b for a, b in zip(lengths, lengths[1:]))
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=len(lengths), length=max(lengths))
    adir = os.path.join(str(tmp_path), "lass_validation")
    for i, n in enumerate(lengths):
        for stem in ("src", "noise"):
            path = os.path.join(adir, f"{stem}_{i:04d}.wav")
            x, _ = wavio.read_wav(path, 16000)
            wavio.write_wav_f32(path, x[:n], 16000)
    pl_model = AudioSep(ss_model=model, query_encoder=PrecomputedQueryEncoder())
    calls = {"forward": 0, "ragged": 0}
    fwd, rag = model._separate, model.separate_ragged
    monkeypatch.setattr(model, "_separate", lambda *a, **k: (calls.__setitem__("forward", calls["forward"] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(model, "separate_ragged", lambda *a, **k: (calls.__setitem__("ragged", calls["ragged"] + 1), rag(*a, **k))[1])
    plain = DCASEEvaluator(16000, csv_path, adir, batch_size=8, resident=False)
    ragged = DCASEEvaluator(16000, csv_path, adir, batch_size=8, resident=False, ragged=True)
    p = plain(pl_model)
    n_plain = dict(calls)
    r = ragged(pl_model)
    assert n_plain == {"forward": len(lengths), "ragged": 0}, n_plain
    n_ragged = calls["ragged"] + calls["forward"] - n_plain["forward"]
    assert calls["forward"] == n_plain["forward"] and 0 < n_ragged < len(lengths), calls
    assert n_ragged == 2   # 16000 -> bucket 3; 11000, 12000, 14000 -> bucket 2
    assert ragged.last_rows.shape == plain.last_rows.shape == (len(lengths), 3)
    print("max |dB| gap", float(np.abs(ragged.last_rows - plain.last_rows).max()))
    np.testing.assert_allclose(ragged.last_rows, plain.last_rows, rtol=0, atol=1e-3)
    assert r == pytest.approx(p, abs=1e-3)


# ---- 9. error paths -------------------------------------------------------------------------------------------------------
def test_ragged_error_paths_launch_nothing(eng):
    from lass_amd import _lib
    lib = eng.lib
    B, L = 2, 10239
    mix, cond = torch.zeros(B, L, device=DEV), torch.zeros(B, 512, device=DEV)
    out = torch.full((B, L), 7.0, device=DEV)
    lens = torch.tensor([6000, 10239], dtype=torch.int32, device=DEV)
    ws = torch.empty(eng.workspace_bytes(B, L), dtype=torch.uint8, device=DEV)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    stats0 = eng.graph_stats()
    assert lib.lass_separate_ragged(eng.ctx, P(mix), c_void_p(0), P(cond), P(out), B, L, P(ws), ws.numel(), st) == -1
    assert b"lengths" in lib.lass_last_error(eng.ctx)
    assert lib.lass_separate_ragged(eng.ctx, P(mix), P(lens), P(cond), P(out), B, 512, P(ws), ws.numel(), st) == -1
    assert lib.lass_front_end_ragged(eng.ctx, P(mix), c_void_p(0), B, L, None, None, None, P(out), st) == -1
    assert lib.lass_istft_ragged(eng.ctx, P(mix), P(mix), c_void_p(0), B, 64, L, 1024, 1024, P(out), st) == -1
    assert lib.lass_istft_ragged(eng.ctx, P(mix), P(mix), P(lens), B, 63, L, 1024, 1024, P(out), st) == -1   # T != 1 + L/160
    with pytest.raises(_lib.LassError, match="bucket"):
        eng.separate_ragged(mix, [5000, 10239], cond, out=out)       # 5000 lies in the bucket below
    with pytest.raises(_lib.LassError, match="bucket"):
        eng.separate_ragged(mix, torch.tensor([6000, 10240]), cond, out=out)   # longer than the row
    with pytest.raises(_lib.LassError, match="checked"):
        eng.separate_ragged(mix, lens, cond, out=out)                # device lengths need the caller's word
    with pytest.raises(_lib.LassError):
        eng.ragged_bucket(512)
    assert eng.ragged_bucket(L) == (5120, L) and eng.ragged_bucket(5119) == (513, 5119)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and eng.graph_stats() == stats0   # nothing ran
    eng.separate_ragged(mix, lens, cond, out=out, checked=True)    # ... and the engine still works
    assert torch.isfinite(out).all() and not out[0, 6000:].any()
