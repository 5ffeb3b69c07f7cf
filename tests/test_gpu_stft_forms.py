"""The three clip forms of the two ends of the network (dense rows, a length per clip, windows of one long row: stft.hip) at
n_fft 2048 with three analysis branches and wlen < n_fft: stage calls of a multi-STFT engine only, no conv.  Every form is one
kernel body, so a clip of the ragged or the window form is bit-identical to that clip run alone through the dense form
(DESIGN.md sections 13 and 14): all assertions are bit equality."""
import numpy as np
import pytest
import torch

from lass_amd import arch, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
N_FFT, WIN = 2048, 512                  # the engine's transform and its mask window (the one the iSTFT re-synthesises from)
L = 1920                                # rows and windows: T = 13 frames (odd), Tp = 32, smallest length of the bucket 1025


@pytest.fixture(scope="module")
def model():
    from lass_amd.resunet_with_multistft import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict_ms().items()})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def eng(model):
    e = model.engine
    assert e.multistft[0] == N_FFT and e.multistft[2] == WIN and e.n_branches == 3
    return e


def _noise(n, seed):
    return ((torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * 0.5).to(DEV)


def test_ragged_forms_equal_each_clip_alone(eng):
    # frame counts 7, 10, 10, 10, 11, 13: a pair's second frame lies beyond the clip for some clips and not for others, and some
    # pairs lie wholly beyond it.  The iSTFT's span 1 starts at sample 16 * 160 - 1024 = 1536: wholly beyond a clip of 1025
    # samples, exactly at the end of one of 1536, one sample inside one of 1537.
    lengths = [1025, 1536, 1537, 1599, 1600, 1920]
    B, T, Tp = len(lengths), arch.frames_for(L), arch.padded_frames(arch.frames_for(L))
    assert (T, Tp) == (13, 32) and eng.ragged_bucket(L) == (1025, L)
    assert [arch.frames_for(n) for n in lengths] == [7, 10, 10, 10, 11, 13]
    clips = [_noise(n, 100 + n) for n in lengths]
    rows = torch.full((B, L), NAN, device=DEV)
    for b, c in enumerate(clips):
        rows[b, :c.numel()] = c
    mag, cos, sin, x0 = eng.front_end_ragged(rows, lengths)
    assert x0.shape == (3, B, Tp, N_FFT // 2) and mag.shape == (B, T, N_FFT // 2 + 1)
    solo = [eng.front_end(c[None].contiguous()) for c in clips]
    for b, n in enumerate(lengths):
        tb = arch.frames_for(n)
        m1, c1, s1, x1 = solo[b]
        assert torch.equal(x0[:, b, :tb], x1[:, 0, :tb]) and not x0[:, b, tb:].any(), n
        for got, ref in ((mag, m1), (cos, c1), (sin, s1)):
            assert torch.equal(got[b, :tb], ref[0]) and not got[b, tb:].any(), n
    # iSTFT: solo-produced spectra packed into NaN-filled rows; what lies beyond a clip's frames must not matter
    re = torch.full((B, T, N_FFT // 2 + 1), NAN, device=DEV)
    im = torch.full_like(re, NAN)
    for b, (m1, c1, s1, _) in enumerate(solo):
        re[b, :m1.shape[1]], im[b, :m1.shape[1]] = (m1 * c1)[0], (m1 * s1)[0]
    wav = eng.istft_ragged(re, im, lengths, L, n_fft=N_FFT, win_length=WIN)
    for b, (n, (m1, c1, s1, _)) in enumerate(zip(lengths, solo)):
        alone = eng.istft_nfft(m1 * c1, m1 * s1, n, N_FFT, WIN)[0]
        assert torch.equal(wav[b, :n], alone) and not wav[b, n:].any(), n


def test_window_forms_equal_each_gathered_window(eng):
    # keeps that run up to the iSTFT's span boundary (sample 1536), start at it, straddle it, and are empty
    W, total = L, 5003
    starts = [0, 517, 1081, 3083]
    keeps = [(0, 1536), (1536, 1920), (1535, 1537), (700, 700)]
    T = arch.frames_for(W)
    rec = _noise(total, 7)
    gathered = torch.stack([rec[s:s + W] for s in starts]).contiguous()
    got = eng.front_end_windows(rec, starts, W)
    ref = eng.front_end(gathered)
    assert got[3].shape == (3, len(starts), arch.padded_frames(T), N_FFT // 2)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
    mag, cos, sin, _ = ref
    re, im = mag * cos, mag * sin
    alone = eng.istft_nfft(re, im, W, N_FFT, WIN)
    out = torch.full((total,), NAN, device=DEV)
    eng.istft_windows(re, im, starts, keeps, W, out, n_fft=N_FFT, win_length=WIN)
    written = torch.zeros(total, dtype=torch.bool, device=DEV)
    for b, (s, (lo, hi)) in enumerate(zip(starts, keeps)):
        assert torch.equal(out[s + lo:s + hi], alone[b, lo:hi]), (s, lo, hi)
        written[s + lo:s + hi] = True
    assert int(written.sum()) == 1536 + 384 + 2
    assert torch.isnan(out[~written]).all() and not torch.isnan(out[written]).any()
