"""ResUNet30 at the 32 kHz STFT geometry (n_fft 2048, hop 320), host side: parameter table, frame and bucket arithmetic, the
module's constructor and state-dict checks, the shipped configuration, the seeded weights and the C-ABI's two new symbols.
No GPU: the device side is tests/test_gpu_geometry.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lass_amd import arch, ragged, synthetic
from lass_amd.resunet import ResUNet30

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_param_specs_follow_n_fft():
    base, wide = arch.param_specs(), arch.param_specs(n_fft=2048)
    assert arch.param_specs(n_fft=1024) == base
    assert [n for n, _, _ in base] == [n for n, _, _ in wide]
    for (name, s0, k0), (_, s1, k1) in zip(base, wide):
        assert k0 == k1
        if name.startswith("base.bn0.") and not name.endswith("num_batches_tracked"):
            assert s0 == (513,) and s1 == (1025,), name
        else:
            assert s0 == s1, name


def test_frames_and_buckets():
    assert arch.frames_for(20111, 320) == 63
    assert arch.frames_for(32000, 320) == 101 and arch.padded_frames(101) == 128
    assert ragged.bucket_of(20111, 2048, hop=320) == 64
    assert ragged.bucket_range(20111, 2048, hop=320) == (10240, 20111)
    assert ragged.bucket_range(1920, 2048, hop=320) == (1025, 1920)
    assert ragged.bucket_of(10239, 2048, hop=320) == 32 and ragged.bucket_of(10240, 2048, hop=320) == 64
    plan = ragged.plan_batches([10240, 14400, 10239, 20111], 16, 2048, hop=320)
    assert plan == [([0, 1, 3], 20111), ([2], 10239)]
    with pytest.raises(ValueError):
        ragged.bucket_of(1024, 2048, hop=320)


def test_defaults_unchanged():
    """The default-argument results are the values the suite asserted before the arguments existed."""
    assert arch.frames_for(160000) == 1001 and arch.frames_for(16000) == 101 and arch.frames_for(6000) == 38
    for L in (513, 5119, 5120, 16000, 160000):
        assert ragged.bucket_of(L) == 32 * -(-(1 + L // 160) // 32), L
    assert ragged.bucket_of(5119) == 32 and ragged.bucket_of(5120) == 64
    assert ragged.bucket_of(1025, n_fft=2048) == 32
    assert ragged.bucket_range(16000) == (15360, 16000) and ragged.bucket_range(2000) == (513, 2000)
    assert ragged.bucket_range(2000, 2048) == (1025, 2000)
    assert ragged.plan_batches([4000, 5200, 4100], 2) == [([0, 2], 4100), ([1], 5200)]
    assert ragged.BUCKET_SAMPLES == 5120


def test_constructor_takes_the_two_geometries_only():
    for bad in ((1024, 320), (2048, 160), (512, 160)):
        with pytest.raises(ValueError) as ei:
            ResUNet30(1, 1, 512, n_fft=bad[0], hop=bad[1])
        assert "n_fft=" in str(ei.value) and "hop=" in str(ei.value)
    m = ResUNet30(1, 1, 512, n_fft=2048, hop=320)
    assert (m.n_fft, m.hop) == (2048, 320)
    assert m.state_dict()["base.bn0.weight"].shape == (1025,)
    d = ResUNet30(1, 1, 512)
    assert (d.n_fft, d.hop) == (1024, 160) and d.state_dict()["base.bn0.weight"].shape == (513,)
    assert list(d.state_dict()) == list(m.state_dict())


def test_config_reaches_the_geometry():
    from lass_amd.utils import get_ss_model, parse_yaml

    m = get_ss_model("config/audiosep_32k.yaml")
    assert m.state_dict()["base.bn0.weight"].shape == (1025,)
    assert (m.n_fft, m.hop) == (2048, 320)
    cfg = parse_yaml("config/audiosep_32k.yaml")
    assert cfg["data"]["sampling_rate"] == 32000 and cfg["model"]["n_fft"] == 2048 and cfg["model"]["hop"] == 320
    base = get_ss_model("config/audiosep_base.yaml")   # no keys: the class default
    assert (base.n_fft, base.hop) == (1024, 160) and base.state_dict()["base.bn0.weight"].shape == (513,)


def _torch_sd(**kw):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict(**kw).items()}


def test_cross_geometry_state_dict_names_the_keywords():
    wide, base = _torch_sd(n_fft=2048), _torch_sd()
    with pytest.raises(ValueError) as ei:
        ResUNet30(1, 1, 512).load_state_dict(wide)
    assert "n_fft=2048" in str(ei.value) and "hop=320" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        ResUNet30(1, 1, 512, n_fft=2048, hop=320).load_state_dict(base, strict=False)
    assert "n_fft=1024" in str(ei.value) and "hop=160" in str(ei.value)
    ResUNet30(1, 1, 512, n_fft=2048, hop=320).load_state_dict(wide)   # and the matching pairs load
    ResUNet30(1, 1, 512).load_state_dict(base)


def test_seeded_stream_of_the_default_is_untouched():
    a, b = synthetic.make_state_dict(), synthetic.make_state_dict(n_fft=1024)
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    w = synthetic.make_state_dict(n_fft=2048)
    assert w["base.bn0.running_var"].shape == (1025,) and w["base.pre_conv.weight"].shape == a["base.pre_conv.weight"].shape


def test_header_declares_the_geometry_symbols():
    """As tests/test_host_cpu.py checks the ABI: declared in the header, bound in _lib.SYMBOLS, exported by the library."""
    import __graft_entry__ as g
    g.build()
    from lass_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lass_hip.h")).read()
    declared = set(re.findall(r"\b(lass_[a-z_0-9]+)\s*\(", hdr))
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("lass_create_stft", "lass_stft_geometry"):
        assert name in declared and name in bound and hasattr(lib, name), name
    assert lib.lass_version() >= 10600
    # the pair is checked before anything touches a device: the message names both accepted pairs
    h = ctypes.c_void_p()
    for n_fft, hop in ((1024, 320), (2048, 160), (4096, 640)):
        assert lib.lass_create_stft(ctypes.byref(h), 0, n_fft, hop) == -1 and not h.value
        msg = lib.lass_last_error(None).decode()
        assert "(1024, 160)" in msg and "(2048, 320)" in msg, msg
    assert lib.lass_stft_geometry(None, None, None) < 0
