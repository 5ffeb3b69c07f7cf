"""Linked channels without a device: the ABI of the four new entry points, what `pipeline.separate_files`
plans and refuses under channels="linked", and the float64 statement of the semantics (tests/linked_reference.py) against the
oracle's ordinary forward where the two must agree - one plane that is its own guide."""
import os
import re

import numpy as np
import pytest
import torch

import linked_reference as lref
from lass_amd import longform, pipeline, synthetic, wavio
from lass_amd import resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, N_FFT = 16000, 1024
NEW = ("lass_separate_ragged_linked", "lass_separate_windows_linked", "lass_masked_stft", "lass_masked_stft_windows")


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_linked_symbols():
    import __graft_entry__ as g
    g.build()
    from ctypes import c_int, c_int64, c_size_t, c_void_p
    from lass_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    declared = set(re.findall(r"\b(lass_[a-z_0-9]+)\s*\(", hdr))
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    P, I, Q, Z = c_void_p, c_int, c_int64, c_size_t
    # ctx, guide, lengths, planes, plane_stride, channels, condition, out, out_plane_stride, B, L, workspace, bytes, stream
    assert bound["lass_separate_ragged_linked"] == [P, P, P, P, Q, I, P, P, Q, I, I, P, Z, P]
    # ctx, guide, total, starts, keep, fade, ramp, F, planes, plane_stride, channels, condition, out, out_plane_stride, B, W, ws, bytes, stream
    assert bound["lass_separate_windows_linked"] == [P, P, Q, P, P, P, P, I, P, Q, I, P, P, Q, I, I, P, Z, P]
    assert bound["lass_masked_stft"] == [P, P, P, I, I, P, P, P, P, P]
    assert bound["lass_masked_stft_windows"] == [P, P, Q, P, I, I, P, P, P, P, P]
    # the linked calls take their unlinked siblings' arguments plus planes, the two strides and the channel count
    assert len(bound["lass_separate_ragged_linked"]) == len(bound["lass_separate_ragged"]) + 4
    assert len(bound["lass_separate_windows_linked"]) == len(bound["lass_separate_windows_faded"]) + 4
    # ... in the header's order
    for name in NEW:
        proto = re.search(name + r"\(([^;]*)\);", hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == len(bound[name]), name
    assert "#define LASS_MAX_LINKED_CHANNELS 8" in hdr and pipeline.MAX_CHANNELS == 8
    assert lib.lass_version() >= 11000
    assert lib.lass_separate_ragged_linked(None, None, None, None, 0, 0, None, None, 0, 0, 0, None, 0, None) < 0
    assert lib.lass_separate_windows_linked(None, None, 0, None, None, None, None, 0, None, 0, 0, None, None, 0, 0, 0, None, 0, None) < 0
    assert lib.lass_masked_stft(None, None, None, 0, 0, None, None, None, None, None) < 0
    assert lib.lass_masked_stft_windows(None, None, 0, None, 0, 0, None, None, None, None, None) < 0


def test_python_layers_have_the_linked_calls():
    from lass_amd.engine import Engine
    from lass_amd.resunet import ResUNet30
    for name in ("separate_ragged_linked", "separate_windows_linked", "masked_stft", "masked_stft_windows"):
        assert callable(getattr(Engine, name))
    for name in ("separate_long_linked", "separate_long_list_linked", "downmix"):
        assert callable(getattr(ResUNet30, name))
    assert Engine.MAX_LINKED_CHANNELS == pipeline.MAX_CHANNELS


def test_downmix_is_the_float32_mean_in_channel_order():
    from lass_amd.resunet import ResUNet30
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.standard_normal((3, 1001)).astype(np.float32)
    want = ((x[0] + x[1]) + x[2]) / np.float32(3)
    assert np.array_equal(ResUNet30.downmix(torch.from_numpy(x)).numpy(), want)
    one = torch.from_numpy(x[:1])
    assert torch.equal(ResUNet30.downmix(one), one[0])                     # a single plane is its own guide, bit for bit
    two = ResUNet30.downmix(torch.from_numpy(x[:2])).numpy()
    assert np.array_equal(two, (x[0] + x[1]) / np.float32(2))


# ---- planning -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("linkedplan")
    rng = np.random.Generator(np.random.PCG64(31))
    specs = [("pcm16", 2, 44100, 22051), ("f32", 1, 16000, 16000), ("pcm16", 2, 44101, 22052), ("pcm32", 3, 32000, 9000),
             ("pcm16", 2, 16000, 7000)]
    paths = []
    for k, (enc, nch, rate, frames) in enumerate(specs):
        paths.append(str(d / f"in{k}.wav"))
        x = 0.1 * rng.standard_normal((frames, nch) if nch > 1 else frames).astype(np.float32)
        pipeline._WRITERS[enc](paths[-1], x, rate)
    return d, paths, specs


def _options():
    return pipeline.Options(None, None, False, False, False, 0, 0, False)


def _jobs(paths):
    return [(p, "a caption", p + ".out.wav") for p in paths]


def test_linked_plans_keep_the_channels_and_count_the_guide(files):
    _, paths, specs = files
    each = pipeline.plan_files(_jobs(paths), None, _options(), SR, N_FFT, channels="each")
    linked = pipeline.plan_files(_jobs(paths), None, _options(), SR, N_FFT, channels="linked")
    assert linked == each                                                   # the same planes, lengths, routes and outputs
    assert [p.n_planes for p in linked] == [s[1] for s in specs] and [p.how for p in linked] == ["device", "device", "host", "device", "device"]
    for nch in (1, 2, 8):
        assert pipeline.model_samples(nch, 44100, 44100, SR, "linked") == pipeline.model_samples(nch, 44100, 44100, SR, "each") == (nch, 16000)
        assert pipeline.pass_rows(nch, "linked") == nch + 1 and pipeline.pass_rows(nch, "each") == nch and pipeline.pass_rows(1, "mono") == 1
    # C + 1 rows per file: the bound that holds both stereo files as planes alone does not hold them with their guides
    rows = [pipeline.pass_rows(p.n_planes, "linked") * p.length for p in linked]
    assert rows == [(s[1] + 1) * rs.out_len(s[3], *rs.ratio(s[2], SR)) for s in specs]
    planes_only = [p.n_planes * p.length for p in linked]
    bound = planes_only[0] + planes_only[1]
    assert pipeline.plan_passes(planes_only, bound)[0] == [0, 1] and pipeline.plan_passes(rows, bound)[0] == [0]


def test_files_of_a_pass_are_grouped_by_channel_count():
    assert pipeline.group_by_planes([2, 1, 2, 3, 1, 2]) == [[0, 2, 5], [1, 4], [3]]
    assert pipeline.group_by_planes([]) == [] and pipeline.group_by_planes([4]) == [[0]]
    groups = pipeline.group_by_planes([2, 1, 2, 3, 1, 2])
    assert sorted(k for g in groups for k in g) == list(range(6))           # every file once


def test_each_and_mono_plan_as_before(files):
    """The figures of tests/test_pipeline_cpu.py and tests/test_pipeline_plan_cpu.py, restated: "each" and "mono" are untouched."""
    _, paths, specs = files
    assert pipeline.model_samples(2, 44100, 44100, 16000, "each") == (2, 16000)
    assert pipeline.model_samples(2, 44100, 44101, 16000, "mono") == (1, 16001)
    each = pipeline.plan_files(_jobs(paths), None, _options(), SR, N_FFT)
    mono = pipeline.plan_files(_jobs(paths), None, _options(), SR, N_FFT, channels="mono")
    for p, m, (enc, nch, rate, frames) in zip(each, mono, specs):
        length = rs.out_len(frames, *rs.ratio(rate, SR))
        assert (p.n_planes, p.length, m.n_planes, m.length) == (nch, length, 1, length)
        assert (p.enc_o, p.rate_o, p.frames_o) == (m.enc_o, m.rate_o, m.frames_o) == (enc, rate, frames)
        assert pipeline.pass_rows(p.n_planes, "each") * p.length == nch * length


def test_linked_argument_refusals(files, tmp_path):
    _, paths, _ = files
    jobs = _jobs(paths[:1])
    for bad in ("Linked", "link", "stereo", "", None):
        with pytest.raises(ValueError, match='channels must be "each" or "mono"'):
            pipeline.separate_files(None, jobs, SR, channels=bad)
    # check_remix_args keeps refusing only "mono"
    assert pipeline.check_remix_args(-12.0, jobs, "linked", None, None, False, False, "sample") == [-12.0]
    assert pipeline.check_remix_args(-12.0, [jobs[0] + ("remix.wav",)], "linked", None, None, False, False, "sample") == [-12.0]
    with pytest.raises(ValueError, match='channels="each"'):
        pipeline.check_remix_args(-12.0, jobs, "mono", None, None, False, False, "sample")
    # more channels than the linked calls take: refused by name before anything runs
    wide = str(tmp_path / "wide.wav")
    wavio.write_wav_pcm16(wide, np.zeros((8000, 9), dtype=np.float32), 16000)
    with pytest.raises(ValueError, match=r"wide\.wav.*at most 8 channels"):
        pipeline.plan_files(_jobs([wide]), None, _options(), SR, N_FFT, channels="linked")
    assert pipeline.plan_files(_jobs([wide]), None, _options(), SR, N_FFT, channels="each")[0].n_planes == 9
    short = str(tmp_path / "short.wav")
    wavio.write_wav_pcm16(short, np.zeros((1400, 2), dtype=np.float32), 44100)
    with pytest.raises(ValueError, match=r"short\.wav.*not longer than the reflect padding"):
        pipeline.plan_files(_jobs([short]), None, _options(), SR, N_FFT, channels="linked")


# ---- the semantics, in float64 ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd64(synthetic_sd):
    from oracle import resunet as orr
    return orr.to_torch(synthetic_sd, torch.float64)


def test_one_plane_guiding_itself_is_the_ordinary_forward(sd64):
    """Y = X * M with X = mag (cos + i sin) and M = mask_mag (mc + i ms) is the reference's out_mag (out_cos + i out_sin), term by
    term: the float64 statement must give the oracle's waveform to float64 rounding.  W = 4000 (T = 26, padded to 32) and W = 7777
    (T = 49), B = 2."""
    from oracle import resunet as orr
    for W, seed in ((4000, 1), (7777, 2)):
        rng = np.random.Generator(np.random.PCG64(seed))
        x = 0.1 * rng.standard_normal((2, W))
        cond = synthetic.make_condition(2, seed=synthetic.SEED + seed).astype(np.float64)
        want = orr.forward(sd64, {"mixture": torch.from_numpy(x)[:, None, :], "condition": torch.from_numpy(cond)})["waveform"][:, 0].numpy()
        got = lref.linked_forward(sd64, x, x[None], cond)
        assert got.shape == (1, 2, W) and got.dtype == np.float64
        err, scale = float(np.max(np.abs(got[0] - want))), float(np.max(np.abs(want)))
        print(f"W = {W}: max |linked statement - oracle forward| = {err:.3e} at signal peak {scale:.3e}")
        assert scale > 1e-3 and err <= 1e-12 * scale


def test_statement_is_linear_in_the_plane_and_blind_to_the_other_planes(sd64):
    """One mask for every plane: a plane's output does not depend on the other planes, scales with the plane, and the planes of a
    zero plane are zero - while another guide gives another output."""
    W = 4000
    rng = np.random.Generator(np.random.PCG64(5))
    guide, planes = 0.1 * rng.standard_normal((1, W)), 0.1 * rng.standard_normal((3, 1, W))
    planes[2] = 0.0
    cond = synthetic.make_condition(1).astype(np.float64)
    out = lref.linked_forward(sd64, guide, planes, cond)
    assert np.array_equal(out[1], lref.linked_forward(sd64, guide, planes[1:2], cond)[0])
    assert not out[2].any() and float(np.max(np.abs(out[0]))) > 1e-4
    twice = lref.linked_forward(sd64, guide, 2.0 * planes[:1], cond)[0]
    assert np.allclose(twice, 2.0 * out[0], rtol=1e-12, atol=0)
    other = lref.linked_forward(sd64, planes[0], planes[:1], cond)[0]
    assert float(np.max(np.abs(other - out[0]))) > 1e-6
    # the mask itself: inside the unit disc, Nyquist column zero
    from oracle import resunet as orr
    taps = {}
    orr.forward(sd64, {"mixture": torch.from_numpy(guide)[:, None, :], "condition": torch.from_numpy(cond)}, taps)
    m_re, m_im = lref.complex_mask(taps["logits"])
    assert m_re.shape == (1, 26, 513) and float(np.max(m_re ** 2 + m_im ** 2)) <= 1.0 + 1e-12
    assert not m_im[..., -1].any() and not m_re[..., -1].any()   # (the Nyquist LOGITS are padding: sigmoid(0) * phasor(0, 0) = 0)


def test_stitch_follows_the_plan():
    plan = longform.plan_windows(20011, 4000, 640)
    wins = [np.full(4000, float(k + 1)) for k in range(len(plan))]
    row = lref.stitch(20011, plan, wins)
    assert row.min() == 1.0 and row.max() == float(len(plan))              # the keeps tile the row
