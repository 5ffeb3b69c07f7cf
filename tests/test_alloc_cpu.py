"""Host-only: lass_amd._alloc, the seam every workspace, scratch buffer and library-written output of the package is allocated
through.  By default it is torch.empty and nothing more; inside `poisoned(byte)` every byte of every such buffer is that byte
(tests/test_gpu_poison.py runs the kernels on such buffers)."""
import numpy as np
import pytest
import torch

from lass_amd import _alloc


@pytest.fixture(autouse=True)
def no_process_wide_fill(monkeypatch):
    """These tests state the default; a hand run with LASS_POISON in the environment must not change what they see."""
    monkeypatch.setattr(_alloc, "_byte", None)


@pytest.fixture
def spies(monkeypatch):
    """Counts of torch.empty / torch.empty_like calls and of Tensor.fill_ calls made while the fixture is live."""
    calls = {"empty": 0, "empty_like": 0, "fill_": 0}

    def spy(owner, name):
        real = getattr(owner, name)

        def wrapped(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, wrapped)
    spy(torch, "empty")
    spy(torch, "empty_like")
    spy(torch.Tensor, "fill_")
    return calls


def all_bytes(t):
    return np.frombuffer(t.contiguous().numpy().tobytes(), dtype=np.uint8)


def test_default_is_torch_empty_and_nothing_else(spies):
    assert _alloc.poison_byte() is None
    t = _alloc.empty(3, 5, dtype=torch.float64, device="cpu")
    assert t.shape == (3, 5) and t.dtype == torch.float64 and spies == {"empty": 1, "empty_like": 0, "fill_": 0}
    u = _alloc.empty((2, 7), dtype=torch.uint8, device="cpu")
    assert u.shape == (2, 7) and u.dtype == torch.uint8 and spies == {"empty": 2, "empty_like": 0, "fill_": 0}
    v = _alloc.empty_like(t)
    assert v.shape == t.shape and v.dtype == t.dtype and spies == {"empty": 2, "empty_like": 1, "fill_": 0}
    keep = torch.arange(6, dtype=torch.float32)
    assert _alloc.refill(keep) is keep and spies["fill_"] == 0 and torch.equal(keep, torch.arange(6, dtype=torch.float32))


@pytest.mark.parametrize("byte", (0x00, 0xFF, 0x7F, 0xA5))
@pytest.mark.parametrize("dtype", (torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16))
def test_poisoned_buffers_hold_the_byte_in_every_byte(byte, dtype):
    with _alloc.poisoned(byte):
        assert _alloc.poison_byte() == byte
        made = [_alloc.empty(3, 5, dtype=dtype, device="cpu"), _alloc.empty((7,), dtype=dtype, device="cpu"),
                _alloc.empty((), dtype=dtype, device="cpu"), _alloc.empty(0, dtype=dtype, device="cpu"),
                _alloc.empty_like(torch.zeros(4, 3, dtype=dtype)), _alloc.empty_like(torch.zeros(4, 3, dtype=dtype).t()),
                _alloc.refill(torch.zeros(2, 9, dtype=dtype))]
    assert [tuple(t.shape) for t in made] == [(3, 5), (7,), (), (0,), (4, 3), (3, 4), (2, 9)]
    for t in made:
        assert t.dtype == dtype
        got = all_bytes(t.view(torch.int16) if dtype == torch.bfloat16 else t)
        assert got.size == t.numel() * t.element_size() and bool((got == byte).all())
    assert _alloc.poison_byte() is None


def test_the_fills_mean_what_the_gpu_tests_take_them_to_mean():
    with _alloc.poisoned(0xFF):
        assert bool(torch.isnan(_alloc.empty(4, dtype=torch.float32, device="cpu")).all())
        assert bool(torch.isnan(_alloc.empty(4, dtype=torch.bfloat16, device="cpu").float()).all())
        assert bool(torch.isnan(_alloc.empty(4, dtype=torch.float64, device="cpu")).all())
    with _alloc.poisoned(0x7F):
        f = _alloc.empty(4, dtype=torch.float32, device="cpu")
        assert bool(torch.isfinite(f).all()) and float(f[0]) > 3.39e38
        assert int(_alloc.empty(1, dtype=torch.int32, device="cpu")[0]) == 0x7F7F7F7F


def test_nesting_restores_the_outer_setting():
    with _alloc.poisoned(0xFF):
        with _alloc.poisoned(0x7F):
            assert _alloc.poison_byte() == 0x7F and int(_alloc.empty(1, dtype=torch.uint8, device="cpu")[0]) == 0x7F
            with pytest.raises(RuntimeError):
                with _alloc.poisoned(0x00):
                    assert int(_alloc.empty(1, dtype=torch.uint8, device="cpu")[0]) == 0
                    raise RuntimeError("leaves through an exception")
            assert _alloc.poison_byte() == 0x7F
        assert _alloc.poison_byte() == 0xFF and int(_alloc.empty(1, dtype=torch.uint8, device="cpu")[0]) == 0xFF
    assert _alloc.poison_byte() is None
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            with _alloc.poisoned(bad):
                pass
    assert _alloc.poison_byte() is None


def test_the_environment_switch_is_one_hex_byte():
    assert _alloc._parse(None) is None and _alloc._parse("") is None
    assert _alloc._parse("ff") == 0xFF and _alloc._parse("7F") == 0x7F and _alloc._parse("0") == 0 and _alloc._parse("0xa5") == 0xA5
    for bad in ("100", "-1", "poison"):
        with pytest.raises(ValueError):
            _alloc._parse(bad)
