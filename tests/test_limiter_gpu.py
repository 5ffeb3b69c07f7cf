"""The look-ahead limiter on the GPU (`lass_limit`, `Engine.limit`), stage by stage.

Yardsticks: the envelope by equality with the composition of the public pieces (`Engine.resample` of every plane at (os, 1), the
absolute value, the maximum with |x| and over the channels) and its maximum by equality with `Engine.resample_true_peak`; the
required gain r and its look-ahead minimum m by equality with numpy float32 on the device's own envelope (through `frames`, and
through the curve wherever the definition makes it exactly 1, with curve <= r everywhere); the curve against the float64 definition on the
device's envelope with the float32 taps, within (2H + 2) * 2^-24 - the rounding of a (2H + 1)-term fmaf chain whose terms sum to
at most 1, beside the two roundings of r; the output by equality with (g * curve) * x in torch float32.

Every row has one short burst over a quiet bed, and across the cases it sits on the seams of every power-of-two tile from 256 to
4096 - frames T - 1, T, T + 1, T - 2H - 10 and T + 2H + 10 - and on the row's first and last frame, so the test needs no
knowledge of the kernel's tile: a tile that forgets its halo, takes it short, or reads what a neighbour wrote lands on one."""
import numpy as np
import pytest
import torch

from lass_amd import _alloc
from lass_amd import loudness as ld

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, C, L = 3, 2, 9000
RATES = (16000, 32000)
REACHES = (1, 24, 512)
CEILING = 0.5
GAINS = (1.5, 2.0, 3.0)


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


def _cases(H):
    """Batches of B positions: the row's two ends and, for every power-of-two tile T, its first seam (T is a seam of every smaller
    tile too) - and 8192, the last seam of a row of 9000 for the tiles up to 2048."""
    at = {0, L - 1}
    for k in (256, 512, 1024, 2048, 4096, 8192):
        at.update(p for p in (k - 1, k, k + 1, k - 2 * H - 10, k + 2 * H + 10) if 0 <= p < L)
    keep = sorted(at)
    while len(keep) % B:
        keep.append(keep[-2])
    return [keep[i:i + B] for i in range(0, len(keep), B)]


def _rows(positions, seed):
    """(B, C, L) float32: a bed of noise at 0.01 and, in channel b % C of row b, five samples of alternating sign at 0.8 starting
    at the row's position (cut at the row's end)."""
    x = 0.01 * np.random.Generator(np.random.PCG64([31, seed])).standard_normal((len(positions), C, L))
    for b, p in enumerate(positions):
        n = min(5, L - p)
        x[b, b % C, p:p + n] = 0.8 * (-1.0) ** np.arange(n)
    return x.astype(np.float32)


def _gain(n=B):
    return torch.tensor(GAINS[:n], dtype=torch.float32, device=DEV)


def _composed_envelope(eng, x, rate, os_):
    """(B, L) from the public pieces: |resample(plane, rate, os * rate)| off phase 0, the maximum with |x| and over the channels."""
    Bx, Cx, Lx = x.shape
    e = x.abs()
    if os_ > 1:
        z = eng.resample(x.reshape(Bx * Cx, Lx).contiguous(), rate, os_ * rate)
        assert z.shape == (Bx * Cx, os_ * Lx)
        e = torch.maximum(e, z.view(Bx, Cx, Lx, os_)[..., 1:].abs().amax(3))
    return e.amax(1)


def _required32(e, g, c):
    a = np.float32(g) * e.astype(np.float32)
    with np.errstate(divide="ignore"):
        return np.where(a <= np.float32(c), np.float32(1), np.float32(c) / np.where(a <= np.float32(c), np.float32(1), a)).astype(np.float32)


def _window_min(r, H):
    """min r[k] over |k - n| <= H inside the row, every window looked at in full."""
    pad = np.concatenate([np.full(H, np.inf, dtype=r.dtype), r, np.full(H, np.inf, dtype=r.dtype)])
    return np.lib.stride_tricks.sliding_window_view(pad, 2 * H + 1).min(axis=1)


def _check(eng, x_np, rate, H, peak, positions):
    x = torch.from_numpy(x_np).to(DEV)
    g = _gain(x.shape[0])
    out, info = eng.limit(x, rate, g, CEILING, H, peak=peak, return_curve=True)
    env, curve = info["envelope"], info["curve"]
    os_ = ld.oversampling(rate) if peak == "true" else 1
    # the envelope
    assert torch.equal(env, _composed_envelope(eng, x, rate, os_)), (rate, H, peak, positions)
    if peak == "true":
        assert torch.equal(env.amax(1), eng.resample_true_peak(x, rate, rate))
    else:
        assert torch.equal(env, x.abs().amax(1))
    # r and m from the device's envelope, numpy float32
    e_np, G_np = env.cpu().numpy(), curve.cpu().numpy()
    w = ld.limiter_window(H)
    for b in range(x.shape[0]):
        gb = np.float32(GAINS[b])
        r = _required32(e_np[b], gb, CEILING)
        m = _window_min(r, H)
        assert int(info["frames"][b]) == int(np.count_nonzero(m < 1)) > 0, (rate, H, peak, positions, b)
        assert np.all(G_np[b] <= r)
        free = _window_min(m, H) == 1
        assert np.all(G_np[b][free] == 1.0) and np.all(G_np[b] <= 1.0) and float(G_np[b][~free].min()) < 1.0
        G64 = ld.limiter_curve(e_np[b].astype(np.float64), gb, CEILING, H, window=w)[0]
        err = float(np.abs(G_np[b].astype(np.float64) - G64).max())
        assert err <= (2 * H + 2) * 2.0 ** -24, (rate, H, peak, positions, b, err)
        assert float(info["min_gain"][b]) == float(G_np[b].min()) < 1.0
    assert torch.equal(info["min_gain"], curve.amin(1))
    # the output
    assert torch.equal(out, (g[:, None] * curve)[:, None, :] * x)
    assert float(out.abs().max()) <= CEILING * (1 + 2.0 ** -22)
    return out, info


@pytest.mark.parametrize("H", REACHES)
@pytest.mark.parametrize("rate", RATES)
def test_every_stage_on_every_seam(eng, rate, H):
    for k, positions in enumerate(_cases(H)):
        _check(eng, _rows(positions, k), rate, H, "true", positions)


@pytest.mark.parametrize("H", REACHES)
def test_sample_peak_envelope(eng, H):
    for k, positions in enumerate(_cases(H)[::4]):
        _check(eng, _rows(positions, 100 + k), 16000, H, "sample", positions)


def test_quiet_silent_and_nan_rows(eng):
    x = torch.from_numpy(_rows([100, 4000, 8000], 7)).to(DEV)
    x[0] *= 0.1                                         # under the ceiling at every gain
    x[1] = 0.0
    x[2, 1, 3000:3010] = float("nan")
    g = _gain()
    out, info = eng.limit(x, 16000, g, CEILING, 24, return_curve=True)
    assert info["frames"].tolist()[:2] == [0, 0] and info["min_gain"].tolist()[:2] == [1.0, 1.0]
    assert torch.equal(info["curve"][:2], torch.ones(2, L, device=DEV))
    assert torch.equal(out[:2], g[:2, None, None] * x[:2])
    # a NaN counts as 0 in the envelope (it spreads over the interpolator's reach there too), and stays a NaN in the output
    env = info["envelope"]
    assert not bool(torch.isnan(env).any()) and not bool(torch.isnan(info["curve"]).any())
    assert bool((env[2, 3000:3010] > 0).all())           # (the other channel's bed)
    assert bool(torch.isnan(out[2, 1, 3000:3010]).all()) and int(info["frames"][2]) > 0
    assert torch.equal(out[2, 0], (g[2] * info["curve"][2]) * x[2, 0])


def _bits(out, info):
    return [out, info["curve"], info["envelope"], info["min_gain"], info["frames"]]


def _same(a, b, rows=slice(None)):
    return all(torch.equal(s[rows] if isinstance(rows, slice) else s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("rate, H", [(16000, 24), (32000, 512)])
def test_a_rows_bits_do_not_depend_on_the_batch_the_strides_or_the_fill(eng, rate, H):
    x_np = _rows([1023, 2048 - 2 * H - 10, L - 1], 9)
    x = torch.from_numpy(x_np).to(DEV)
    g = _gain()
    want = _bits(*eng.limit(x, rate, g, CEILING, H, return_curve=True))
    assert all(int(f) > 0 for f in want[4])
    for b in (2, 0, 1):                                  # alone, (C, L), another call
        got = _bits(*eng.limit(x[b], rate, g[b:b + 1].contiguous(), CEILING, H, return_curve=True))
        assert all(torch.equal(s, t[b:b + 1]) for s, t in zip(got, want)), b
    got = _bits(*eng.limit(x.flip(0), rate, g.flip(0).contiguous(), CEILING, H, return_curve=True))          # rows flipped
    assert all(torch.equal(s.flip(0), t) for s, t in zip(got, want))
    big = torch.randn(B, C + 1, L + 3, generator=torch.Generator().manual_seed(32)).to(DEV)              # strided views with gaps
    big[:, :C, :L] = x
    view = big[:, :C, :L]
    assert view.stride(0) == (C + 1) * (L + 3) and view.stride(1) == L + 3
    assert _same(_bits(*eng.limit(view, rate, g, CEILING, H, return_curve=True)), want)
    for byte in (0x00, 0x7F, 0xFF):
        with _alloc.poisoned(byte):
            assert _same(_bits(*eng.limit(x, rate, g, CEILING, H, return_curve=True)), want), hex(byte)
    # without the optional outputs the planes are the same
    assert torch.equal(eng.limit(x, rate, g, CEILING, H)[0], want[0])


def test_refusals_launch_nothing(eng):
    from lass_amd import _lib
    from lass_amd import resample as rs
    from lass_amd.engine import _ptr, _stream
    Lr = 600
    x = torch.full((2, 2, Lr), 0.9, device=DEV)
    taps4 = rs.device_taps(4, 1, DEV)
    win = torch.from_numpy(ld.limiter_window(24)).to(DEV)
    g = torch.ones(2, device=DEV)
    sentinel = 123.0
    out = torch.full((2, 2, Lr), sentinel, device=DEV)
    curve, env = torch.full((2, Lr), sentinel, device=DEV), torch.full((2, Lr), sentinel, device=DEV)
    mg, fr = torch.full((2,), sentinel, device=DEV), torch.full((2,), 77, dtype=torch.int32, device=DEV)

    def call(planes=x, rs_=2 * Lr, ps=Lr, Bn=2, ch=2, Ln=Lr, os_=4, t=taps4, n_os=81, gain=g, c=0.5, H=24, w=win, o=out, ors=2 * Lr, ops=Lr,
             cv=curve, ev=env, crs=Lr, m=mg, f=fr):
        ptr = lambda v: v if isinstance(v, int) else _ptr(v)
        rc = eng.lib.lass_limit(eng.ctx, ptr(planes), rs_, ps, Bn, ch, Ln, os_, ptr(t), n_os, ptr(gain), c, H, ptr(w), ptr(o), ors, ops,
                                ptr(cv), ptr(ev), crs, ptr(m), ptr(f), _stream(eng.device))
        return rc, (eng.lib.lass_last_error(eng.ctx) or b"").decode()

    bad = [
        (dict(ch=0), "channels"), (dict(ch=9), "channels"), (dict(Ln=0), "L >= 1"), (dict(H=0), "H must"), (dict(H=513), "H must"),
        (dict(os_=3), "os must"), (dict(os_=0), "os must"), (dict(n_os=80), "n_os_taps"), (dict(os_=2), "n_os_taps"),
        (dict(t=None), "os_taps"), (dict(os_=1, t=None, n_os=5), "n_os_taps"),
        (dict(c=0.0), "ceiling"), (dict(c=-1.0), "ceiling"), (dict(c=float("inf")), "ceiling"), (dict(c=float("nan")), "ceiling"),
        (dict(ps=Lr - 1), "plane_stride"), (dict(rs_=2 * Lr - 1), "row_stride"), (dict(ops=Lr - 1), "out_plane_stride"),
        (dict(ors=2 * Lr - 1), "out_row_stride"), (dict(crs=Lr - 1), "curve_row_stride"),
        (dict(o=x), "overlap"), (dict(o=x.data_ptr() + 4 * (4 * Lr - 1)), "overlap"), (dict(o=x.data_ptr() - 4 * (4 * Lr - 1)), "overlap"),
        (dict(planes=x.data_ptr() + 2), "aligned"), (dict(o=out.data_ptr() + 2), "aligned"), (dict(cv=curve.data_ptr() + 1), "aligned"),
        (dict(m=mg.data_ptr() + 2), "aligned"), (dict(f=fr.data_ptr() + 2), "aligned"), (dict(gain=g.data_ptr() + 2), "aligned"),
        (dict(w=win.data_ptr() + 2), "aligned"),
        (dict(planes=None), "non-NULL"), (dict(gain=None), "non-NULL"), (dict(w=None), "non-NULL"), (dict(o=None), "non-NULL"),
        (dict(Bn=0), "B"), (dict(Bn=65536), "B"),
    ]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("lass_limit: ") and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for t in (out, curve, env, mg):
        assert bool((t == sentinel).all())
    assert fr.tolist() == [77, 77]
    # and the same arguments, unbroken, run: with and without the optional outputs, and at os == 1 with no taps
    assert call()[0] == 0
    assert call(os_=1, t=None, n_os=0, cv=None, ev=None, m=None, f=None)[0] == 0
    torch.cuda.synchronize()
    assert fr.tolist() == [Lr, Lr] and float(mg.max()) < 1.0 and float(out.abs().max()) <= 0.5 * (1 + 2.0 ** -22)
    with pytest.raises(_lib.LassError, match="lookahead"):
        eng.limit(x, 16000, g, 0.5, 513)
    with pytest.raises(_lib.LassError, match="gain"):
        eng.limit(x, 16000, torch.ones(3, device=DEV), 0.5, 24)
    with pytest.raises(_lib.LassError, match="peak"):
        eng.limit(x, 16000, g, 0.5, 24, peak="rms")
