"""The twelve audio file entry points of the C layer, replayed through ctypes over tests/audio_refusal_cases.py: every refused
argument set must give the (rc, message) of tests/golden/audio_refusals.json - recorded from the entries as they stood before
lass_amd/csrc/audio_args.h existed, so whole messages and the order of the checks are held, not prefixes - and must leave every
output buffer as it was; every good set runs once."""
import json
import os

import pytest
import torch

import audio_refusal_cases as arc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def eng():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_refusals.json")) as f:
        return json.load(f)


def _buffers():
    """One allocation per buffer of the list, twice its size (an overlap case points past a buffer's own end), inputs zero."""
    bufs = {name: torch.zeros(2 * size + 256, dtype=torch.uint8, device=DEV) for name, size in arc.BUFFERS.items()}
    assert all(t.data_ptr() % 256 == 0 for t in bufs.values())
    return bufs, {name: t.data_ptr() for name, t in bufs.items()}


@pytest.mark.parametrize("entry", sorted(arc.BAD))
def test_every_refusal_is_the_recorded_one_and_launches_nothing(eng, fixture, entry):
    bufs, base = _buffers()
    for name in arc.OUTPUTS[entry]:
        bufs[name].fill_(SENTINEL)
    stream = torch.cuda.current_stream().cuda_stream
    n = 0
    for e, cid, args, _ in arc.cases():
        if e != entry:
            continue
        rc, msg = arc.call(eng.lib, eng.ctx, entry, args, base, stream)
        assert [rc, msg] == fixture[entry][cid], (entry, cid, rc, msg)
        n += 1
    assert n == len(fixture[entry]) >= 10
    torch.cuda.synchronize()
    for name in arc.OUTPUTS[entry]:
        assert bool((bufs[name] == SENTINEL).all()), (entry, name)


def test_every_good_set_runs(eng):
    bufs, base = _buffers()
    stream = torch.cuda.current_stream().cuda_stream
    good = list(arc.GOOD.items()) + [
        ("lass_limit", dict(arc.GOOD["lass_limit"], os=1, os_taps=0, n_os_taps=0, curve=0, envelope=0, min_gain=0, frames=0)),
        ("lass_remix_encode", dict(arc.GOOD["lass_remix_encode"], gain=arc.at("gain")))]
    for entry, args in good:
        rc, msg = arc.call(eng.lib, eng.ctx, entry, args, base, stream)
        assert rc == 0, (entry, rc, msg)
    torch.cuda.synchronize()
    # silence in, silence out (what the kernels compute is the other tests' business)
    assert int(bufs["out_bytes"].sum()) == 0 and int(bufs["clipped"].sum()) == 0 and int(bufs["peak"].sum()) == 0
