"""GPU parity tests: every HIP stage and the whole hot path, through the C-ABI, against the CPU oracle and the golden
fixtures (which were produced by the reference's own resunet.py).  Tolerances are absolute float32 figures stated per
test; the north_star bar for the waveform is 1e-4 RMS."""
import os

import numpy as np
import pytest
import torch

from lass_amd import arch, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rms(a):
    return float(torch.as_tensor(a).double().pow(2).mean().sqrt())


def _relerr(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return _rms(got - ref) / max(_rms(ref), 1e-30)


@pytest.fixture(scope="module")
def oracle_sd(synthetic_sd):
    from oracle import resunet as orr
    return orr.to_torch(synthetic_sd)


@pytest.fixture(scope="module")
def eng(synthetic_sd):
    from lass_amd.engine import Engine
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd)
    return e


@pytest.fixture(scope="module")
def model(synthetic_sd):
    from lass_amd.resunet import ResUNet30
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    return m.to(DEV).eval()


def test_library_loaded_is_in_tree():
    from lass_amd import _lib
    lib = _lib.load()
    assert os.path.samefile(lib._name, _lib.LIB_PATH)
    maps = open("/proc/self/maps").read()
    assert "liblass_hip.so" in maps


# ---- STFT / iSTFT ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16000, 160000, 8000 + 77])
def test_stft_magphase_vs_oracle(eng, L):
    from oracle import stft as ost
    g = torch.Generator().manual_seed(L)
    x = (torch.rand(3, L, generator=g) * 2 - 1) * 0.5
    x[1] = torch.from_numpy(synthetic.make_mixtures(1, L)[1][0])
    x[2, : L // 2] = 0.0  # silence: exercises the 1e-10 clamp (cos = sin = 0, mag = 1e-5)
    mag, cos, sin, re, im = eng.stft_magphase(x.to(DEV), want_complex=True)
    r64, i64 = ost.stft_fft(x.double())
    scale = float(r64.abs().max())
    assert float((re.cpu().double() - r64[:, 0]).abs().max()) < 2e-6 * scale + 1e-6
    assert float((im.cpu().double() - i64[:, 0]).abs().max()) < 2e-6 * scale + 1e-6
    m_ref, c_ref, s_ref = ost.spectrogram_phase(*ost.stft_fft(x))
    assert float((mag.cpu() - m_ref[:, 0]).abs().max()) < 2e-6 * scale + 1e-6
    # phase is ill-conditioned where |X| ~ 0: compare re-synthesised real/imag parts instead of cos/sin directly
    assert float((mag.cpu() * cos.cpu() - m_ref[:, 0] * c_ref[:, 0]).abs().max()) < 4e-6 * scale + 1e-6
    assert float((mag.cpu() * sin.cpu() - m_ref[:, 0] * s_ref[:, 0]).abs().max()) < 4e-6 * scale + 1e-6
    strong = m_ref[:, 0] > 1e-2 * scale
    assert float((cos.cpu() - c_ref[:, 0])[strong].abs().max()) < 2e-4
    assert float((sin.cpu() - s_ref[:, 0])[strong].abs().max()) < 2e-4
    # exact silence frames
    T_sil = (L // 2 - 512) // 160 - 1
    assert float((mag[2, :T_sil] - 1e-5).abs().max()) < 1e-11
    assert torch.all(cos[2, :T_sil] == 0) and torch.all(sin[2, :T_sil] == 0)


@pytest.mark.parametrize("L", [16000, 160000])
def test_istft_vs_oracle_and_roundtrip(eng, L):
    from oracle import stft as ost
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(2, L, generator=g) * 2 - 1) * 0.5
    _, _, _, re, im = eng.stft_magphase(x.to(DEV), want_complex=True)
    y = eng.istft(re, im, L)
    assert float((y.cpu() - x).abs().max()) < 5e-6          # STFT -> iSTFT identity
    # arbitrary (inconsistent) spectrogram vs the oracle
    T = arch.frames_for(L)
    sr = torch.randn(2, T, 513, generator=g)
    si = torch.randn(2, T, 513, generator=g)
    y = eng.istft(sr.to(DEV), si.to(DEV), L)
    y_ref = ost.istft_fft(sr[:, None].double(), si[:, None].double(), L)
    assert float((y.cpu().double() - y_ref).abs().max()) < 1e-5


def test_stft_istft_roundtrip_full_batch(eng):
    """BASELINE config-2 size (B=16, 10 s): size-independent property instead of a CPU comparison."""
    _, mix = synthetic.make_mixtures(16, 160000)
    x = torch.from_numpy(mix).to(DEV)
    _, _, _, re, im = eng.stft_magphase(x, want_complex=True)
    y = eng.istft(re, im, 160000)
    assert float((y - x).abs().max()) < 1e-5


# ---- FiLM ----------------------------------------------------------------------------------------------------------
def test_film_vs_oracle_and_golden(eng, oracle_sd, golden_dir):
    from oracle import resunet as orr
    cond = torch.from_numpy(synthetic.make_condition(2))
    raw = eng.film(cond.to(DEV), raw=True).cpu()
    ref = orr.film_all(oracle_sd, cond)
    g = np.load(os.path.join(golden_dir, "g1_tiny.npz"))
    n_checked = 0
    for site, c, used in arch.film_sites():
        off = eng.film_offset(site)
        if not used:
            assert off == -1
            continue
        got = raw[:, off:off + c]
        np.testing.assert_allclose(got.numpy(), ref[site].numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(got.numpy(), g["film/" + site], rtol=0, atol=2e-6)
        n_checked += 1
    assert n_checked == 32 and eng.film_width() == 9856 - 1600


# ---- residual blocks / transposed convs ---------------------------------------------------------------------------
BLOCKS = [  # (module prefix, film site stem, cin, cout, H, W)
    ("base.encoder_block1.conv_block1", "encoder_block1->conv_block1", 32, 32, 40, 64),   # identity, PW=32, N=32
    ("base.encoder_block2.conv_block1", "encoder_block2->conv_block1", 32, 64, 24, 32),   # 1x1 shortcut, N=64
    ("base.encoder_block5.conv_block1", "encoder_block5->conv_block1", 256, 384, 8, 32),
    ("base.encoder_block6.conv_block1", "encoder_block6->conv_block1", 384, 384, 12, 16),  # PW=16, ragged H
    ("base.conv_block7a.conv_block1", "conv_block7a->conv_block1", 384, 384, 4, 8),       # PW=8, H < tile
    ("base.decoder_block1.conv_block2", "decoder_block1->conv_block2", 768, 384, 4, 16),
    ("base.decoder_block6.conv_block2", "decoder_block6->conv_block2", 64, 32, 17, 96),   # ragged H, 3 x-tiles
]


@pytest.mark.parametrize("prefix,stem,cin,cout,H,W", BLOCKS)
def test_convblock_vs_oracle(eng, oracle_sd, prefix, stem, cin, cout, H, W):
    from oracle import resunet as orr
    g = torch.Generator().manual_seed(H * 1000 + W)
    B = 2
    x = torch.randn(B, cin, H, W, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    shift = eng.film(cond.to(DEV))
    y = eng.convblock(prefix, x.to(DEV), shift, cout).cpu()
    ref = orr.conv_block_res(oracle_sd, prefix, x, orr.film(oracle_sd, cond, stem + "->beta1"),
                             orr.film(oracle_sd, cond, stem + "->beta2"))
    assert y.shape == ref.shape
    assert _relerr(y, ref) < 5e-6, _relerr(y, ref)
    assert float((y - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))


UPS = [("decoder_block1", 384, 384, (1, 2), 4, 8), ("decoder_block2", 384, 384, (2, 2), 4, 16),
       ("decoder_block5", 128, 64, (2, 2), 9, 64), ("decoder_block6", 64, 32, (2, 2), 16, 32)]


@pytest.mark.parametrize("name,cin,cout,up,h,w", UPS)
def test_upconv_vs_oracle(eng, oracle_sd, name, cin, cout, up, h, w):
    import torch.nn.functional as F
    from oracle import resunet as orr
    g = torch.Generator().manual_seed(h * 100 + w)
    B = 2
    x = torch.randn(B, cin, h, w, generator=g)
    cond = torch.from_numpy(synthetic.make_condition(B))
    shift = eng.film(cond.to(DEV))
    y = eng.upconv("base." + name, x.to(DEV), shift, cout, up).cpu()
    hh = F.leaky_relu(orr._bn(oracle_sd, f"base.{name}.bn1", x) + orr.film(oracle_sd, cond, f"{name}->beta1"), 0.01)
    ref = F.conv_transpose2d(hh, oracle_sd[f"base.{name}.conv1.weight"], stride=up)
    assert y.shape == ref.shape
    assert _relerr(y, ref) < 2e-6, _relerr(y, ref)


# ---- mask ----------------------------------------------------------------------------------------------------------
def test_mask_apply_vs_oracle(eng, oracle_sd):
    import torch.nn.functional as F
    from oracle import stft as ost
    g = torch.Generator().manual_seed(3)
    B, T, Tp = 2, 101, 128
    x12 = torch.randn(B, 32, Tp, 512, generator=g)
    re = torch.randn(B, 1, T, 513, generator=g)
    im = torch.randn(B, 1, T, 513, generator=g)
    mag, cos, sin = ost.spectrogram_phase(re, im)
    o_re, o_im = eng.mask_apply(x12.to(DEV), mag[:, 0].contiguous().to(DEV), cos[:, 0].contiguous().to(DEV),
                                sin[:, 0].contiguous().to(DEV))
    lg = F.conv2d(x12, oracle_sd["base.after_conv.weight"], oracle_sd["base.after_conv.bias"])
    lg = F.pad(lg, (0, 1))[:, :, 0:T, :]
    mm = torch.sigmoid(lg[:, 0:1])
    _, mc, ms = ost.magphase(torch.tanh(lg[:, 1:2]), torch.tanh(lg[:, 2:3]))
    om = F.relu(mag * mm)
    ref_re = om * (cos * mc - sin * ms)
    ref_im = om * (sin * mc + cos * ms)
    assert float((o_re.cpu() - ref_re[:, 0]).abs().max()) < 5e-6
    assert float((o_im.cpu() - ref_im[:, 0]).abs().max()) < 5e-6
    assert torch.all(o_re[:, :, 512] == 0) and torch.all(o_im[:, :, 512] == 0)   # Nyquist bin exactly zero


# ---- whole path ------------------------------------------------------------------------------------------------------
def test_separate_tiny_vs_oracle_and_golden(model, oracle_sd, golden_dir):
    from oracle import resunet as orr
    _, mix = synthetic.make_mixtures(2, 16000)
    cond = synthetic.make_condition(2)
    inp = {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(cond).to(DEV)}
    out = model(inp)["waveform"]
    assert out.shape == (2, 1, 16000) and out.dtype == torch.float32 and out.device.type == "cuda"
    ref = orr.forward(oracle_sd, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": torch.from_numpy(cond)})[
        "waveform"]
    err = _rms(out.cpu() - ref)
    assert err < 2e-6, err                         # north_star bar: 1e-4 RMS
    g = np.load(os.path.join(golden_dir, "g1_tiny.npz"))
    assert _rms(out.cpu() - torch.from_numpy(g["waveform"])) < 2e-6   # the reference's own output


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_separate_10s_vs_golden(synthetic_sd, golden_dir, mode):
    """G2 = the reference's own output and SDR / SDRi / SI-SDR triple on a 10 s clip (tools/gen_golden.py).  Every compute
    mode is pinned to it: the triple within north_star's 0.05 dB (f32: 0.01), the waveform within 3e-6 RMS for f32,
    1e-5 RMS for the split-operand mode (f32 tolerance class), 0.69 % relative for plain bf16 (8-bit mantissa operands: 3 x the
    0.227 % measured; tests/test_gpu_bf16_exact.py holds every launch to its own model)."""
    from lass_amd.resunet import ResUNet30
    from oracle import metrics as om
    g = np.load(os.path.join(golden_dir, "g2_clip10s.npz"))
    src, mix = synthetic.make_mixtures(1, 160000, first=3)
    cond = synthetic.make_condition(1)
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    m = m.to(DEV).eval().set_compute_dtype(mode)
    out = m({"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(cond).to(DEV)})[
        "waveform"][0, 0].cpu().numpy()
    err = float(np.sqrt(np.mean((out[::16] - g["waveform_dec"]) ** 2)))
    ref_rms = float(np.sqrt(np.mean(g["waveform_dec"] ** 2)))
    print(mode, "waveform RMS error vs the reference's own 10 s output", err, "relative", err / ref_rms)
    if mode == "f32":
        assert err < 3e-6
        np.testing.assert_allclose(out[:2048], g["head"], atol=3e-5)
        np.testing.assert_allclose(out[-2048:], g["tail"], atol=3e-5)
    elif mode == "bf16x3":
        assert err <= 1e-5
    else:
        assert 1e-7 < err < 6.9e-3 * ref_rms   # really the bf16 kernels; 3 x the 2.27e-3 measured (was 5e-2)
    sdr = om.calculate_sdr(src[0], out)
    sdr0 = om.calculate_sdr(src[0], mix[0])
    sisdr = om.calculate_sisdr(src[0], out)
    got = np.asarray([sdr, sdr - sdr0, sisdr])
    print(mode, "SDR / SDRi / SI-SDR", got, "reference", g["sdr_triple"])
    np.testing.assert_allclose(got, g["sdr_triple"], atol=0.01 if mode == "f32" else 0.05)   # bar: +-0.05 dB


def test_separate_batch_invariance_full_size(model):
    """Config-2 size (B=16 x 10 s): clips are independent, so row i of a batched run must equal a batch-1 run of clip i
    bit for bit; also finite and deterministic across two launches."""
    _, mix = synthetic.make_mixtures(16, 160000)
    cond = synthetic.make_condition(16)
    m = torch.from_numpy(mix)[:, None, :].to(DEV)
    c = torch.from_numpy(cond).to(DEV)
    out = model({"mixture": m, "condition": c})["waveform"]
    out2 = model({"mixture": m, "condition": c})["waveform"]
    assert torch.isfinite(out).all()
    assert torch.equal(out, out2)
    for i in (0, 7, 15):
        one = model({"mixture": m[i:i + 1], "condition": c[i:i + 1]})["waveform"]
        assert torch.equal(one[0], out[i]), i


def test_silence_and_edge_lengths(model, oracle_sd):
    from oracle import resunet as orr
    cond = torch.from_numpy(synthetic.make_condition(1))
    for L in (1024, 5000, 16001):   # T = 7 / 32 / 101 -> Tpad = 32 / 32 / 128
        x = torch.zeros(1, 1, L)
        x[0, 0, L // 3] = 0.5       # a click in silence
        out = model({"mixture": x.to(DEV), "condition": cond.to(DEV)})["waveform"]
        ref = orr.forward(oracle_sd, {"mixture": x, "condition": cond})["waveform"]
        assert out.shape == (1, 1, L)
        assert _rms(out.cpu() - ref) < 2e-6


def test_c_abi_error_paths(eng, synthetic_sd):
    """Every misuse returns a negative code with a message (no crash, no silent fallback): include/lass_hip.h contract."""
    from ctypes import byref, c_size_t, c_void_p
    from lass_amd import _lib
    from lass_amd.engine import Engine
    lib = eng.lib
    mix = torch.zeros(2, 4000, device=DEV)
    cond = torch.zeros(2, 512, device=DEV)
    out = torch.empty_like(mix)
    ws = torch.empty(eng.workspace_bytes(2, 4000), dtype=torch.uint8, device=DEV)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    # workspace too small / null pointers / clip shorter than the reflect padding
    assert lib.lass_separate(eng.ctx, P(mix), P(cond), P(out), 2, 4000, P(ws), 1024, st) < 0
    assert b"workspace" in lib.lass_last_error(eng.ctx)
    assert lib.lass_separate(eng.ctx, c_void_p(0), P(cond), P(out), 2, 4000, P(ws), ws.numel(), st) < 0
    assert lib.lass_separate(eng.ctx, P(mix), P(cond), P(out), 2, 512, P(ws), ws.numel(), st) < 0
    n = c_size_t()
    assert lib.lass_workspace_bytes(eng.ctx, 0, 4000, byref(n)) < 0
    # a context that was never finalized refuses to compute
    raw = Engine(DEV)
    assert raw.lib.lass_separate(raw.ctx, P(mix), P(cond), P(out), 2, 4000, P(ws), ws.numel(), st) < 0
    assert raw.lib.lass_last_error(raw.ctx)
    # unknown names / wrong shapes at upload; unknown blocks at the stage entry points
    w = torch.zeros(3, 3)
    shp = (__import__("ctypes").c_int64 * 2)(3, 3)
    assert raw.lib.lass_set_param(raw.ctx, b"base.encoder_block1.conv_block1.conv1.weight", P(w), shp, 2, 0) < 0
    assert raw.lib.lass_set_param(raw.ctx, b"not.a.parameter", P(w), shp, 2, 0) < 0
    assert raw.lib.lass_set_param(raw.ctx, b"base.stft.conv_real.weight", P(w), shp, 2, 0) == 1  # ignored, by contract
    with pytest.raises(_lib.LassError):
        eng.convblock("base.no_such_block", torch.zeros(1, 32, 8, 32, device=DEV), eng.film(cond[:1]), 32)
    # multi-window front end: unsupported window, too many windows
    with pytest.raises(_lib.LassError):
        eng.multi_stft(mix, [300])
    with pytest.raises(_lib.LassError):
        eng.multi_stft(mix, [256, 512, 1024, 2048, 256])
    # the engine still works afterwards
    assert torch.isfinite(eng.separate(mix, cond)).all()


def test_bf16_and_f32_wino_contexts_coexist(synthetic_sd, monkeypatch):
    """no kernel of the library carries packed-f32 arithmetic, so a bf16 context and an f32 context on the
    F(2x2,3x3) route (LASS_WINO4=0) may be alive in one process together - and the f32 one computes exactly what it computes
    alone."""
    import gc
    from lass_amd.resunet import ResUNet30
    _, mix = synthetic.make_mixtures(2, 24000)
    inp = {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(synthetic.make_condition(2)).to(DEV)}

    def make(mode):
        m = ResUNet30(1, 1, 512)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
        m = m.to(DEV).eval().set_compute_dtype(mode)
        m.engine   # lass_create (reads the switches) + lass_finalize happen here
        return m

    gc.collect()
    monkeypatch.setenv("LASS_WINO4", "0")
    alone = make("f32")
    ref = alone(inp)["waveform"].cpu()
    del alone
    gc.collect()
    monkeypatch.delenv("LASS_WINO4")
    bf = make("bf16")
    monkeypatch.setenv("LASS_WINO4", "0")
    f32 = make("f32")
    assert torch.isfinite(bf(inp)["waveform"]).all()
    assert torch.equal(f32(inp)["waveform"].cpu(), ref)


def test_integration_md_ctypes_stub_runs_verbatim(tmp_path, synthetic_sd, oracle_sd):
    """INTEGRATION.md section B shows the binding a maintainer adds on the reference side (a ctypes `HipSeparator` around the
    five C-ABI calls).  The code block is taken out of the document and executed as written - only the library's file name is
    made absolute - against the oracle: documentation that cannot rot."""
    import importlib.util
    import re
    from lass_amd import _lib
    from lass_amd.resunet import ResUNet30
    from oracle import resunet as orr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    sec_b = text[text.index("## B. Bind the C-ABI directly"):]
    code = re.search(r"```python\n(.*?)```", sec_b, re.S).group(1)
    assert "class HipSeparator" in code and 'ctypes.CDLL("liblass_hip.so")' in code
    code = code.replace('ctypes.CDLL("liblass_hip.so")', f'ctypes.CDLL({_lib.LIB_PATH!r})')
    path = os.path.join(str(tmp_path), "resunet_hip.py")
    open(path, "w").write(code)
    spec = importlib.util.spec_from_file_location("resunet_hip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # `m`: a module with the reference's state_dict (keys, shapes, extra torchlibrosa buffers included); weights on the HOST
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    sd = dict(m.state_dict())
    sd["base.stft.conv_real.weight"] = torch.zeros(513, 1, 1024)
    holder = type("RefModule", (), {"state_dict": lambda self: sd})()
    hip_sep = mod.HipSeparator(holder, 0)
    _, mix = synthetic.make_mixtures(2, 20000)
    cond = torch.from_numpy(synthetic.make_condition(2))
    out = hip_sep({"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": cond.to(DEV)})["waveform"]
    assert out.shape == (2, 1, 20000)
    ref = orr.forward(oracle_sd, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": cond})["waveform"]
    assert _rms(out.cpu() - ref) <= 1e-5
    with pytest.raises(RuntimeError):   # the stub's error path: lass_separate's message comes back through lass_last_error
        hip_sep({"mixture": torch.zeros(1, 1, 100, device=DEV), "condition": cond[:1].to(DEV)})


def test_random_shapes_against_oracle(model, oracle_sd):
    """Seeded random (batch, length) pairs - lengths that are no multiple of the hop, frame counts that leave odd heights
    down the U-Net, batch sizes that do not fill a tile - against the CPU oracle."""
    from oracle import resunet as orr
    rng = np.random.default_rng(2024)
    for _ in range(6):
        B = int(rng.integers(1, 5))
        L = int(rng.integers(513, 30000))
        x = torch.from_numpy((rng.standard_normal((B, 1, L)) * 0.1).astype(np.float32))
        cond = torch.from_numpy(synthetic.make_condition(B))
        out = model({"mixture": x.to(DEV), "condition": cond.to(DEV)})["waveform"].cpu()
        ref = orr.forward(oracle_sd, {"mixture": x, "condition": cond})["waveform"]
        assert out.shape == ref.shape == (B, 1, L)
        assert _rms(out - ref) < 1e-5 * max(_rms(ref), 1e-3) + 2e-6, (B, L)


def test_long_form_clip_config5(model, oracle_sd):
    """BASELINE configs[4] input shape: one 30 s clip at 32 kHz (L = 960000, T = 6001 -> 6016) through the same
    single-STFT trunk (the reference's multi-STFT model is not runnable).  Whole-clip forward vs the oracle."""
    from oracle import resunet as orr
    L = 960000
    segs = [synthetic.make_mixtures(1, 160000, first=20 + i)[1][0] for i in range(6)]
    mix = torch.from_numpy(np.concatenate(segs)[:L].astype(np.float32))[None, None, :]
    cond = torch.from_numpy(synthetic.make_condition(1))
    out = model({"mixture": mix.to(DEV), "condition": cond.to(DEV)})["waveform"]
    assert out.shape == (1, 1, L) and torch.isfinite(out).all()
    ref = orr.forward(oracle_sd, {"mixture": mix, "condition": cond})["waveform"]
    assert _rms(out.cpu() - ref) < 3e-6


def test_chunk_inference_vs_golden(model, golden_dir):
    g = np.load(os.path.join(golden_dir, "g3_chunk.npz"))
    segs = [synthetic.make_mixtures(1, 160000, first=10 + i)[1][0] for i in range(3)]
    long_mix = np.concatenate(segs)[:400000].astype(np.float32)
    cond = synthetic.make_condition(1)
    out = model.chunk_inference({"mixture": torch.from_numpy(long_mix)[None, None, :].to(DEV),
                                 "condition": torch.from_numpy(cond).to(DEV)})
    assert out.shape == (1, 400000) and out.dtype == np.float64
    assert np.sqrt(np.mean((out[0, ::25] - g["out_dec"]) ** 2)) < 3e-6
    for s, seam in zip((32000, 128000, 224000, 320000), g["seams"]):
        np.testing.assert_allclose(out[0, s - 64:s + 64], seam, atol=3e-5)
    short = model.chunk_inference({"mixture": torch.zeros(1, 1, 160000, device=DEV),
                                   "condition": torch.from_numpy(cond).to(DEV)})
    assert short.shape == (1, 160000) and not short.any()


# ---- metrics / evaluator ---------------------------------------------------------------------------------------------
def test_sdr_stats_vs_oracle():
    from lass_amd import metrics
    from oracle import metrics as om
    rng = np.random.default_rng(5)
    ref = rng.standard_normal(160000).astype(np.float32) * 0.1
    for est in (ref.copy(), 0.5 * ref, ref + 0.01 * rng.standard_normal(160000).astype(np.float32),
                np.zeros_like(ref), rng.standard_normal(160000).astype(np.float32)):
        assert abs(metrics.calculate_sdr(ref, est) - om.calculate_sdr(ref, est)) < 1e-3
        a, b = metrics.calculate_sisdr(ref, est), om.calculate_sisdr(ref, est)
        assert abs(a - b) < 1e-2 or (a > 80 and b > 80)   # est == a*ref: both are "infinite", float32 eps-limited
    assert abs(metrics.calculate_sdr(ref, 0.5 * ref) - 6.0206) < 1e-3


@pytest.mark.parametrize("L", [32000, 160000])
def test_evaluator_matches_oracle(tmp_path, model, oracle_sd, L):
    """BASELINE configs[0]: dcase_evaluator on 8 synthetic mixtures - once at its stated size (10 s @ 16 kHz) and once
    at 2 s per clip (faster CPU oracle, different frame count)."""
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.evaluator import DCASEEvaluator
    from oracle import evaluator as oev
    n = 8
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=n, length=L)
    qe = PrecomputedQueryEncoder()
    pl_model = AudioSep(ss_model=model, query_encoder=qe)
    ev = DCASEEvaluator(sampling_rate=16000, eval_indexes=csv_path, audio_dir=os.path.join(str(tmp_path), "lass_validation"),
                        batch_size=3)   # ragged last batch on purpose
    sisdr, sdri, sdr = ev(pl_model)
    clips = [synthetic.make_clip(i, L) for i in range(n)]
    conds = qe.get_query_embed("text", [f"synthetic tone cluster {i % 4}" for i in range(n)]).numpy()
    (o_sisdr, o_sdri, o_sdr), rows = oev.evaluate(oracle_sd, clips, conds)
    np.testing.assert_allclose(ev.last_rows, rows, atol=0.01)
    assert abs(sdr - o_sdr) < 0.01 and abs(sdri - o_sdri) < 0.01 and abs(sisdr - o_sisdr) < 0.01
    # default path = device-side mixing + prefetch + caption cache; the reference's host-side numpy mixing must agree
    calls = []
    orig = qe.get_query_embed
    qe.get_query_embed = lambda *a, **k: (calls.append(list(k.get("text") or a[1])), orig(*a, **k))[1]
    host = DCASEEvaluator(sampling_rate=16000, eval_indexes=csv_path, audio_dir=os.path.join(str(tmp_path), "lass_validation"),
                          batch_size=3, device_mixing=False)
    assert host(pl_model) == pytest.approx((sisdr, sdri, sdr), abs=2e-3)
    np.testing.assert_allclose(host.last_rows, ev.last_rows, atol=2e-3)
    assert sorted(sum(calls, [])) == sorted({f"synthetic tone cluster {i}" for i in range(4)})  # once per caption


def test_evaluator_resident_path_equals_generic_path(tmp_path, model):
    """dcase_evaluator.py:65-122, round 5: the resident data path (decode threads fill pinned slot rows directly, two persistent
    device batches, recurring pointers -> lass_separate replays its hipGraph with the two overlapping half-batches) returns
    per-clip rows equal to the generic path's (fresh tensors per batch, eager launches) to 1e-9 dB; a clip of another length sends
    only its batch through the generic route; later calls replay graphs from their first batch."""
    from lass_amd import wavio
    from lass_amd.audiosep import AudioSep, PrecomputedQueryEncoder
    from lass_amd.evaluator import DCASEEvaluator
    n, L, B = 41, 24000, 8      # five full batches + a ragged tail of 1
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=n, length=L)
    adir = os.path.join(str(tmp_path), "lass_validation")
    pl_model = AudioSep(ss_model=model, query_encoder=PrecomputedQueryEncoder())
    gen = DCASEEvaluator(16000, csv_path, adir, batch_size=B, resident=False)
    res = DCASEEvaluator(16000, csv_path, adir, batch_size=B)
    g = gen(pl_model)
    assert gen.last_path == "generic"
    _, cap0, rep0 = model.engine.graph_stats()
    for call in range(3):
        r = res(pl_model)
        assert res.last_path == "resident" and res.resident_batches == 6 and res.generic_batches == 0
        # (same kernels on the same data; the f64 statistics are accumulated with atomics, whose order is not fixed: 1e-9 dB)
        np.testing.assert_allclose(res.last_rows, gen.last_rows, rtol=0, atol=1e-9, err_msg=str(call))
        assert r == pytest.approx(g, abs=1e-9)
    _, cap1, rep1 = model.engine.graph_stats()
    assert cap1 > cap0 and rep1 - rep0 >= 8, (cap0, cap1, rep0, rep1)   # the slots' pointers recur: captured, then replayed
    # a PCM16 file and a clip of another length in the set: that batch (and only that one) takes the generic route
    x, _ = wavio.read_wav(os.path.join(adir, "src_0003.wav"), 16000)
    wavio.write_wav_pcm16(os.path.join(adir, "src_0003.wav"), x, 16000)          # still fits a slot row (decoded in place)
    y, _ = wavio.read_wav(os.path.join(adir, "src_0010.wav"), 16000)
    wavio.write_wav_f32(os.path.join(adir, "src_0010.wav"), y[:20000], 16000)
    z, _ = wavio.read_wav(os.path.join(adir, "noise_0010.wav"), 16000)
    wavio.write_wav_f32(os.path.join(adir, "noise_0010.wav"), z[:20000], 16000)
    g2 = gen(pl_model)
    r2 = res(pl_model)
    assert res.last_path == "resident" and res.generic_batches == 1 and res.resident_batches == 5
    np.testing.assert_allclose(res.last_rows, gen.last_rows, rtol=0, atol=1e-9)
    assert r2 == pytest.approx(g2, abs=1e-9)


def test_eval_from_checkpoint_default_config(tmp_path, synthetic_sd, oracle_sd, capsys, monkeypatch):
    """SURVEY §8 a14 / f2 end to end on the GPU: a Lightning-shaped `.ckpt` (`state_dict['ss_model.*']` next to
    `query_encoder.*` keys and the torchlibrosa buffers a reference checkpoint carries, utils.py:387-398) goes through
    `eval(evaluator, checkpoint_path)` with the reference's own call signature and DEFAULT `config_yaml`
    (dcase_evaluator.py:126-145) into the HIP path; the returned triple equals the CPU oracle's evaluator and the printed
    line is the reference's (`SDR: x, SDRi: y, SISDR: z`, dcase_evaluator.py:141-143)."""
    import re
    from lass_amd import evaluator as lev
    from lass_amd.audiosep import PrecomputedQueryEncoder
    from lass_amd.resunet import ResUNet30
    from lass_amd.utils import get_ss_model
    from oracle import evaluator as oev
    n, L = 8, 32000
    csv_path = synthetic.write_validation_set(str(tmp_path), n_clips=n, length=L)
    ck = {"state_dict": {"ss_model." + k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()},
          "epoch": 7, "global_step": 200000, "pytorch-lightning_version": "2.1.0"}
    ck["state_dict"]["query_encoder.model.logit_scale_a"] = torch.zeros(())
    ck["state_dict"]["query_encoder.model.text_projection.0.weight"] = torch.zeros(512, 768)
    ck["state_dict"]["ss_model.base.stft.conv_real.weight"] = torch.zeros(513, 1, 1024)
    ck["state_dict"]["ss_model.base.istft.conv_imag.weight"] = torch.zeros(1024, 1024, 1)
    ckpt = os.path.join(str(tmp_path), "audiosep_16k,baseline,step=200000.ckpt")
    torch.save(ck, ckpt)
    monkeypatch.chdir(tmp_path)   # a working directory WITHOUT config/: the shipped config/audiosep_base.yaml must be found
    ev = lev.DCASEEvaluator(sampling_rate=16000, eval_indexes=csv_path,
                            audio_dir=os.path.join(str(tmp_path), "lass_validation"), batch_size=5)
    sdr, sdri, sisdr = lev.eval(ev, ckpt, device="cuda")
    out = capsys.readouterr().out
    m = re.search(r"^SDR: (-?\d+\.\d{3}), SDRi: (-?\d+\.\d{3}), SISDR: (-?\d+\.\d{3})$", out, re.M)
    assert m, out
    assert [float(g) for g in m.groups()] == [round(sdr, 3), round(sdri, 3), round(sisdr, 3)]
    assert "Evaluation on DCASE T9 synthetic validation set." in out and "Start Evaluation" in out
    clips = [synthetic.make_clip(i, L) for i in range(n)]
    conds = PrecomputedQueryEncoder().get_query_embed("text", [f"synthetic tone cluster {i % 4}" for i in range(n)]).numpy()
    (o_sisdr, o_sdri, o_sdr), rows = oev.evaluate(oracle_sd, clips, conds)
    np.testing.assert_allclose(ev.last_rows, rows, atol=0.01)
    assert abs(sdr - o_sdr) < 0.01 and abs(sdri - o_sdri) < 0.01 and abs(sisdr - o_sisdr) < 0.01
    # utils.py:326-353: the bare separator from the same default config; the checkpoint's weights load into it key for key
    ss = get_ss_model("config/audiosep_base.yaml")
    assert isinstance(ss, ResUNet30)
    ss.load_state_dict({k[len("ss_model."):]: v for k, v in ck["state_dict"].items() if k.startswith("ss_model.")},
                       strict=True)
    ss = ss.to("cuda").eval()
    _, mix = synthetic.make_mixtures(2, L)
    cond = torch.from_numpy(synthetic.make_condition(2)).cuda()
    wav = ss({"mixture": torch.from_numpy(mix)[:, None, :].cuda(), "condition": cond})["waveform"]
    from oracle import resunet as orr
    ref = orr.forward(oracle_sd, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": cond.cpu()})["waveform"]
    assert _rms(wav.cpu() - ref) <= 1e-5


def test_mix_at_snr_vs_reference_formula(eng):
    """lass_mix_at_snr against dcase_evaluator.py:77-89 restated in numpy float32, incl. clips that need declipping."""
    rng = np.random.default_rng(3)
    B, L = 6, 48000
    src = (rng.standard_normal((B, L)) * rng.uniform(0.02, 0.6, (B, 1))).astype(np.float32)
    noise = (rng.standard_normal((B, L)) * rng.uniform(0.01, 0.5, (B, 1))).astype(np.float32)
    snrs = np.array([-15, -10, 0, 5, 15, -15], dtype=np.float32)
    src[5] *= 3.0  # loud source at -15 dB SNR: certainly clips
    exp_src, exp_mix = [], []
    for b in range(B):
        s, n = src[b].copy(), noise[b]
        sf = np.sqrt((np.mean(s ** 2) / (10 ** (float(snrs[b]) / 10))) / np.mean(n ** 2))
        m = s + n * np.float32(sf)
        mx = np.max(np.abs(m))
        if mx > 1:
            s *= np.float32(0.9 / mx)
            m *= np.float32(0.9 / mx)
        exp_src.append(s)
        exp_mix.append(m)
    d_src = torch.from_numpy(src).to(DEV)
    mix = eng.mix_at_snr(d_src, torch.from_numpy(noise).to(DEV), torch.from_numpy(snrs).to(DEV)).cpu().numpy()
    got_src = d_src.cpu().numpy()
    clipped = [float(np.max(np.abs(m))) for m in exp_mix]
    assert any(abs(c - 0.9) < 1e-5 for c in clipped) and any(c < 0.9 for c in clipped)  # both branches exercised
    for b in range(B):
        scale = float(np.max(np.abs(exp_mix[b])))
        assert float(np.max(np.abs(mix[b] - exp_mix[b]))) < 2e-6 * max(scale, 1.0)
        assert float(np.max(np.abs(got_src[b] - exp_src[b]))) < 2e-6 * max(scale, 1.0)


def test_wino4_routes_agree(synthetic_sd, monkeypatch):
    """The shipped F(4x4,3x3) routes against F(2x2,3x3) everywhere (LASS_WINO4=0) and against F(4x4,3x3) on the deep
    layers only (LASS_WINO4=64): same waveform to f32 summation-order noise.  The switch is read at lass_create."""
    from lass_amd.resunet import ResUNet30
    _, mix = synthetic.make_mixtures(2, 24000)
    inp = {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(synthetic.make_condition(2)).to(DEV)}

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = ResUNet30(1, 1, 512)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
        out = m.to(DEV).eval()(inp)["waveform"].cpu()
        for k in env:
            monkeypatch.delenv(k)
        return out

    ref = run({})
    scale = float(ref.pow(2).mean().sqrt())
    for env in ({"LASS_WINO4": "0"}, {"LASS_WINO4": "64"}):
        got = run(env)
        assert float((got - ref).pow(2).mean().sqrt()) < 2e-5 * scale, env


# ---- BASELINE configs[2]: bf16-MFMA convolutions (reduced precision by design; its own tolerances) --------------------
def test_bf16_mode_convblock_and_waveform(synthetic_sd, oracle_sd, monkeypatch):
    """Operands of the 3x3 convs are rounded to bf16 (8-bit mantissa, ~4e-3 relative each): per-block outputs must
    agree with the f32 oracle to ~1e-2 relative RMS and the end-to-end waveform to ~5e-2 relative RMS; SDR against the
    oracle's waveform must exceed 25 dB.  (The f32 path is held to 2e-6.)"""
    from lass_amd.engine import Engine
    from lass_amd.resunet import ResUNet30
    from oracle import resunet as orr
    e = Engine(DEV)
    e.load_state_dict(synthetic_sd, "bf16")
    g = torch.Generator().manual_seed(11)
    B = 2
    cond = torch.from_numpy(synthetic.make_condition(B))
    shift = e.film(cond.to(DEV))
    for prefix, stem, cin, cout, H, W in [("base.encoder_block1.conv_block1", "encoder_block1->conv_block1", 32, 32, 40, 64),
                                          ("base.encoder_block3.conv_block1", "encoder_block3->conv_block1", 64, 128, 16, 32),
                                          ("base.decoder_block5.conv_block2", "decoder_block5->conv_block2", 128, 64, 24, 96)]:
        x = torch.randn(B, cin, H, W, generator=g)
        y = e.convblock(prefix, x.to(DEV), shift, cout).cpu()
        ref = orr.conv_block_res(oracle_sd, prefix, x, orr.film(oracle_sd, cond, stem + "->beta1"),
                                 orr.film(oracle_sd, cond, stem + "->beta2"))
        rel = _relerr(y, ref)
        print("bf16", prefix, "relative RMS error vs the f32 oracle", rel)
        assert 1e-5 < rel < 8.1e-3, (prefix, rel)   # > 1e-5: the bf16 kernels really ran; 3 x the largest measured, 2.67e-3 (was 2e-2)
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    m = m.to(DEV).eval().set_compute_dtype("bf16")
    _, mix = synthetic.make_mixtures(2, 16000)
    c2 = synthetic.make_condition(2)
    out = m({"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(c2).to(DEV)})["waveform"]
    ref = orr.forward(oracle_sd, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": torch.from_numpy(c2)})[
        "waveform"]
    rel = _relerr(out, ref)
    print("bf16 waveform relative RMS error", rel)
    assert rel < 7.4e-3, rel   # 3 x the 2.46e-3 measured (was 5e-2)
    # decoder_block6's transposed conv inside its fused kernel (default) composes the shortcut with it - weights rounded once,
    # bf16 noise apart from the three-launch form (test_bf16_fused_upconv_vs_separate_launch); the exact A/B pairs below are
    # taken against the three-launch form
    monkeypatch.setenv("LASS_FUSE_UP", "0")
    m1 = ResUNet30(1, 1, 512)
    m1.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    out_fu = out
    out = m1.to(DEV).eval().set_compute_dtype("bf16")(
        {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(c2).to(DEV)})["waveform"]
    monkeypatch.delenv("LASS_FUSE_UP")
    assert _relerr(out, ref) < 5e-2 and _relerr(out_fu, out) < 1.5e-2
    # the blocked bf16 concat copies (default) round exactly what the f32-concat path rounds while staging: same waveform
    monkeypatch.setenv("LASS_FUSE_CATB", "0")
    m2 = ResUNet30(1, 1, 512)
    m2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    out2 = m2.to(DEV).eval().set_compute_dtype("bf16")(
        {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(c2).to(DEV)})["waveform"]
    monkeypatch.delenv("LASS_FUSE_CATB")
    # (round 5: with the blocked copies the 1x1 shortcut is contracted INSIDE the 3x3 chunk loop, with f32 tensors behind it -
    # another f32 summation order, so roundings of the bf16 hand-overs flip here and there: bf16 noise, not 1e-5 any more)
    print("blocked bf16 hand-overs vs f32 hand-overs (bf16): relative RMS difference", _relerr(out2, out))
    assert _relerr(out2, out) < 2e-3   # measured 8.9e-4: 3 x that would be looser than this bar, which stays
    # encoder_block1 and decoder_block6 as ONE kernel each (conv_bf16_fused.hip: the 32-channel intermediate stays in LDS) is the default; the
    # two-launch form rounds the same f32 accumulators to the same bf16 intermediate: same waveform
    monkeypatch.setenv("LASS_FUSE_BLOCK", "0")
    m3 = ResUNet30(1, 1, 512)
    m3.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    out3 = m3.to(DEV).eval().set_compute_dtype("bf16")(
        {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(c2).to(DEV)})["waveform"]
    monkeypatch.delenv("LASS_FUSE_BLOCK")
    print("fused vs two-launch encoder_block1 / decoder_block6 (bf16): relative RMS difference", _relerr(out3, out))
    assert _relerr(out3, out) < 1e-5


def test_bf16_fused_upconv_vs_separate_launch(synthetic_sd, oracle_sd, monkeypatch):
    """decoder_block6's transposed conv inside the fused decoder kernel (default; the up-sampled half of the concat is never
    written) against the three-launch form (LASS_FUSE_UP=0: transposed conv -> blocked copies -> fused block).  The fused
    form composes the 1x1 shortcut with the transposed conv (weights rounded once), so the two agree to bf16 rounding
    noise, not bit for bit: compared on the separated spectrum (workspace tap, every bin - tile borders and image edges
    included) and on the waveform; both forms against the f32 oracle as in test_bf16_mode_convblock_and_waveform.
    L = 25 600 -> 161 frames -> 192 padded rows: 24 row tiles, masked rows beyond the last frame."""
    from lass_amd.resunet import ResUNet30
    from oracle import resunet as orr
    B, L = 2, 25600
    _, mix = synthetic.make_mixtures(B, L)
    cond = synthetic.make_condition(B)
    inp = {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(cond).to(DEV)}
    res = {}
    for tag, env in (("fused", None), ("separate", "0")):
        if env is not None:
            monkeypatch.setenv("LASS_FUSE_UP", env)
        m = ResUNet30(1, 1, 512)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
        m = m.to(DEV).eval().set_compute_dtype("bf16")
        out = m(inp)["waveform"].cpu()
        T = 1 + L // 160
        spec = [m.engine.workspace_tensor(n, B, L)[:, :, :T].clone().cpu() for n in ("out_real", "out_imag")]
        res[tag] = (out, spec)
        if env is not None:
            monkeypatch.delenv("LASS_FUSE_UP")
    ref = orr.forward(oracle_sd, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": torch.from_numpy(cond)})["waveform"]
    for tag in res:
        assert _relerr(res[tag][0], ref) < 5e-2, tag
    d = _relerr(res["fused"][0], res["separate"][0])
    print("bf16: transposed conv inside decoder_block6's kernel vs its own launch, waveform relative RMS difference", d)
    assert 1e-7 < d < 1.5e-2, d   # not identical (composed shortcut weights), bf16 noise
    for a, bq in zip(res["fused"][1], res["separate"][1]):
        scale = float(bq.abs().max())
        err = (a - bq).abs()
        # a wrong pixel mapping / border rule shows as an isolated large error: bound the maximum over all bins
        assert float(err.max()) < 0.08 * scale, float(err.max()) / scale
        assert float(err.pow(2).mean().sqrt()) < 1e-2 * float(bq.pow(2).mean().sqrt())


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_bf16_modes_ragged_shapes(synthetic_sd, mode):
    """Frame counts that leave odd heights at the bottom of the U-Net (T = 151 -> 160 -> H = 5 at encoder_block6) and a
    batch of 3: the bf16 hand-over paths must track the f32 path (same weights, same inputs)."""
    from lass_amd.resunet import ResUNet30
    _, mix = synthetic.make_mixtures(3, 24000)
    inp = {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(synthetic.make_condition(3)).to(DEV)}
    outs = {}
    for m_ in ("f32", mode):
        m = ResUNet30(1, 1, 512)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
        outs[m_] = m.to(DEV).eval().set_compute_dtype(m_)(inp)["waveform"].cpu()
    rel = _relerr(outs[mode], outs["f32"])
    assert rel < (5e-2 if mode == "bf16" else 1e-4), rel


def test_bf16x3_split_mode_is_f32_accurate(synthetic_sd, oracle_sd, golden_dir):
    """LASS_COMPUTE_BF16X3: operands split hi+lo (two bf16), products hi*hi + hi*lo + lo*hi on the bf16 MFMA with f32
    accumulation.  ~16 mantissa bits per operand: must stay within the f32 path's own tolerance class (bar 1e-4)."""
    from lass_amd.resunet import ResUNet30
    from oracle import resunet as orr
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    m = m.to(DEV).eval().set_compute_dtype("bf16x3")
    _, mix = synthetic.make_mixtures(2, 16000)
    c2 = synthetic.make_condition(2)
    out = m({"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(c2).to(DEV)})["waveform"]
    g = np.load(os.path.join(golden_dir, "g1_tiny.npz"))
    err = _rms(out.cpu() - torch.from_numpy(g["waveform"]))
    print("bf16x3 waveform RMS error vs the reference's own output", err, "relative", err / _rms(g["waveform"]))
    assert err < 1e-5, err


def test_bf16_modes_full_size_metrics_vs_f32(synthetic_sd):
    """BASELINE configs[2] at its stated size (B=16, 10 s @ 16 kHz): bf16 and bf16x3 waveforms against the f32 path on the
    same inputs.  north_star's bar is SDR within +-0.05 dB; SDR / SDRi / SI-SDR of every clip (reference = the synthetic
    source) must agree to that, and the split mode must stay inside the f32 tolerance class (1e-5 RMS)."""
    from lass_amd.metrics import stats_to_db
    from lass_amd.resunet import ResUNet30
    B, L = 16, 160000
    src, mix = synthetic.make_mixtures(4, L)
    src = np.concatenate([src] * 4)[:B]
    mix = np.concatenate([mix] * 4)[:B]
    inp = {"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": torch.from_numpy(synthetic.make_condition(B)).to(DEV)}
    source = torch.from_numpy(src).to(DEV)
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    m = m.to(DEV).eval()
    rows, outs = {}, {}
    for mode in ("f32", "bf16", "bf16x3"):
        out = m.set_compute_dtype(mode)(inp)["waveform"][:, 0].contiguous()
        eng = m.engine
        sdr, sisdr = stats_to_db(eng.sdr_stats(source, out).cpu().numpy(), L)
        sdr0, _ = stats_to_db(eng.sdr_stats(source, inp["mixture"][:, 0].contiguous()).cpu().numpy(), L)
        rows[mode] = np.stack([sdr, sdr - sdr0, sisdr], axis=1)
        outs[mode] = out.cpu()
    assert np.isfinite(rows["f32"]).all()
    for mode in ("bf16", "bf16x3"):
        d = np.abs(rows[mode] - rows["f32"]).max()
        print(mode, "max |dB difference| vs f32 over 16 clips x (SDR, SDRi, SI-SDR):", d)
        assert d < (0.0434 if mode == "bf16" else 1.3e-4), (mode, d)   # 3 x the 1.444e-2 / 4.14e-5 dB measured (was 0.05 for both)
    assert _rms(outs["bf16x3"] - outs["f32"]) <= 1e-5
    assert 1e-6 < _rms(outs["bf16"] - outs["f32"]) < 5e-2 * _rms(outs["f32"])   # really the bf16 kernels, and sane


@pytest.mark.parametrize("mode", ["bf16", "f32", "bf16x3"])
def test_half_batch_overlap_is_bit_identical(synthetic_sd, monkeypatch, mode):
    """lass_separate's two overlapping half-batches (the captured graph's default for an even batch of >= 8 clips) against
    the unsplit run on the same 16 clips: the same bits, call after call, launched eagerly and as a replayed graph."""
    from lass_amd.resunet import ResUNet30
    B, L = 16, 160000
    _, mix = synthetic.make_mixtures(4, L)
    mix = np.concatenate([mix * g for g in (1.0, 0.8, 0.6, 0.4)])[:B]
    x = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    engines = {}
    for split in ("1", "0"):
        monkeypatch.setenv("LASS_SPLIT", "2" if split == "1" else "0")   # 2: eager launches split too (default: graphs only)
        m = ResUNet30(1, 1, 512)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
        engines[split] = m.to(DEV).eval().set_compute_dtype(mode).engine
    monkeypatch.delenv("LASS_SPLIT")
    assert engines["1"].workspace_bytes(B, L) >= engines["0"].workspace_bytes(B, L)
    ref = engines["0"].separate(x, cond).clone()
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 1e-3
    out = torch.empty_like(ref)   # one output buffer: the same (pointers, shape) key every call, so the graph is replayed
    for graph in (False, True):
        engines["1"].set_graph_replay(graph)
        for call in range(6):
            out.zero_()
            engines["1"].separate(x, cond, out=out)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (mode, "graph" if graph else "eager", call)
    _, captures, replays = engines["1"].graph_stats()
    assert captures >= 1 and replays >= 1, (captures, replays)   # the two-stream form captures as one graph with two branches
    with pytest.raises(Exception, match="half-batches"):   # the workspace holds two half-batch layouts, not the B = 16 one
        engines["1"].workspace_tensor("out_real", B, L)
    # ... and only then: the default schedule (LASS_SPLIT=1) splits the REPLAYED graph only, so after eager calls of the same
    # batch the whole-batch layout is in the workspace and its taps are readable
    if mode == "f32":
        m = ResUNet30(1, 1, 512)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
        e1 = m.to(DEV).eval().engine
        e1.set_graph_replay(False)
        o1 = e1.separate(x, cond)
        tap = e1.workspace_tensor("out_real", B, L)
        assert tap.shape[0] == B and torch.isfinite(tap).all() and float(tap.abs().max()) > 0
        assert torch.equal(o1, ref)
        e1.set_graph_replay(True)
        for _ in range(4):                                   # third identical call captures, fourth replays: split from then on
            e1.separate(x, cond, out=out)
        with pytest.raises(Exception, match="half-batches"):
            e1.workspace_tensor("out_real", B, L)


# (the ids keep the part count these cases were written with; every even batch >= 8 now runs as two halves)
@pytest.mark.parametrize("B,L", [(8, 25600), (10, 40000), (16, 16000), (9, 25600)],
                         ids=["8-25600-2", "10-40000-2", "16-16000-4", "9-25600-2"])
def test_part_batches_at_ragged_shapes(synthetic_sd, monkeypatch, B, L):
    """The half-batch schedule at batch sizes whose halves are odd / minimal, at short clips, and at an odd
    batch (which must simply run unsplit): eager two-stream launches (LASS_SPLIT=2) and the replayed graph against LASS_SPLIT=0,
    bit for bit, in bf16 mode (every blocked-layout hand-over is in play there)."""
    from lass_amd.resunet import ResUNet30
    _, mix = synthetic.make_mixtures(B, L)
    x = torch.from_numpy(mix).to(DEV)
    cond = torch.from_numpy(synthetic.make_condition(B)).to(DEV)
    engines = {}
    for split in ("2", "0"):
        monkeypatch.setenv("LASS_SPLIT", split)
        m = ResUNet30(1, 1, 512)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
        engines[split] = m.to(DEV).eval().set_compute_dtype("bf16").engine
    ref = engines["0"].separate(x, cond).clone()
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 1e-3
    out = torch.empty_like(ref)
    for graph in (False, True):
        engines["2"].set_graph_replay(graph)
        for call in range(4):
            out.zero_()
            engines["2"].separate(x, cond, out=out)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (B, L, "graph" if graph else "eager", call)


def test_front_end_is_exact_beside_a_bf16_separation():
    """Regression check for the co-residency hazard of DESIGN.md 5b: STFT front-end launches on one stream while lass_separate
    (bf16) runs on another.  With packed-f32 instructions in stft.hip about one launch in six came out wrong; as built by
    __graft_entry__.build() (-fno-slp-vectorize for the kernels without matrix instructions) every one is exact."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("coresident_stress", os.path.join(os.path.dirname(__file__), "..", "tools",
                                                                                   "coresident_stress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    wrong, overlapped = mod.run("bf16", nrep=60, trials=2, verbose=False, return_overlap=True)
    assert wrong == 0
    # the guard must not pass by not overlapping: output sets are pre-allocated and stream A separates for the whole window,
    # so most of the 2 x 60 front-end launches end while it is still busy (events on both streams)
    assert overlapped >= 60, overlapped
