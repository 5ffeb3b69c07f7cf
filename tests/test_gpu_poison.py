"""No result depends on what a workspace, a scratch buffer or an output held before the call (include/lass_hip.h, conventions).

Nothing zeroes a workspace: a separation is right only if every kernel writes all that a later one reads - padded frames, channel
padding, the slots that blocks share in turn.  Elsewhere in the suite stale bytes are finite floats of an earlier test, so a kernel
that multiplies an unwritten element by zero, or reads one row past its producer, passes.  Here every such buffer is filled with
0x00, 0xFF (a NaN as f32 and as bf16: arithmetic on stale data shows) and 0x7F (3.39e38: fmaxf, integer maxima on the bits and
comparisons show, which skip a NaN), and everything the call is documented to write must come out bit-identical under the three.
Caller-kept buffers sit between guards of 0xA5, which must survive; `out` is prefilled so that a sample the call skips is seen.

Shapes of the C-ABI cases come from tools/workspace_table.cpp (tests/test_workspace_plan_cpu.py builds and parses it).  The stage,
tower and meter cases go through lass_amd._alloc.poisoned, the seam the package allocates through."""
import os
import random
from ctypes import byref, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from lass_amd import _alloc, arch, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
FILLS = (0x00, 0xFF, 0x7F)
NAN = float("nan")
SWITCHES = ("LASS_SPLIT", "LASS_GRAPH", "LASS_WINO4", "LASS_WINO4_VPREP", "LASS_HEAD_FOLD", "LASS_HEAD_SC_FOLD", "LASS_PW_SPLIT",
            "LASS_WINO4_GEMM", "LASS_FUSE_CATB", "LASS_FUSE_BLOCK", "LASS_FUSE_UP")
TINY = (2, 8077)       # 51 frames padded to 64: 13 rows of padding, odd length
P = lambda x: c_void_p(x.data_ptr())  # noqa: E731


class Guarded:
    """`nbytes` of device memory between two guards of 0xA5; `inner` starts 256-aligned."""

    def __init__(self, nbytes, fill=None):
        self.nbytes = int(nbytes)
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.inner = self.buf[GUARD:GUARD + self.nbytes]
        assert self.inner.data_ptr() % 256 == 0 and self.inner.numel() == self.nbytes
        if fill is not None:
            self.inner.fill_(fill)

    @classmethod
    def of(cls, t):
        """a guarded copy of the float32 tensor t -> (guarded, view of t's shape)"""
        g = cls(t.numel() * 4)
        v = g.inner.view(torch.float32).view(t.shape)
        v.copy_(t)
        return g, v

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.nbytes:] == 0xA5).all())


def bits(t):
    """the tensor as integers: equality of these is equality of bits (a NaN equals itself, -0.0 is not 0.0)"""
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def across_fills(call, fills=FILLS):
    """call() under each fill of lass_amd._alloc -> the results of the first fill, after asserting every other fill gave the same
    bits.  call returns a tensor or a tuple / list / dict of tensors (None entries allowed)."""
    def flat(r):
        if isinstance(r, dict):
            return [x for k in sorted(r, key=str) for x in flat(r[k])]
        if isinstance(r, (tuple, list)):
            return [x for v in r for x in flat(v)]
        return [r]
    first = None
    for byte in fills:
        with _alloc.poisoned(byte):
            got = call()
        torch.cuda.synchronize()
        if first is None:
            first, first_flat = got, flat(got)
            continue
        now = flat(got)
        assert len(now) == len(first_flat)
        for i, (a, b) in enumerate(zip(first_flat, now)):
            assert (a is None) == (b is None)
            if a is not None:
                assert same(a, b), f"result {i} differs between fill {fills[0]:#04x} and fill {byte:#04x}"
    return first


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    from test_workspace_plan_cpu import build_workspace_table   # built here: no compiler is a failure, not a skip
    return build_workspace_table(tmp_path_factory.mktemp("workspace_plan_poison"))


@pytest.fixture
def default_switches(monkeypatch):
    for s in SWITCHES:   # read at lass_create; the tool's defaults are a context's
        monkeypatch.delenv(s, raising=False)
    return monkeypatch


def make_engine(sd, mode="f32", **kw):
    from lass_amd.engine import Engine
    e = Engine(DEV, **kw)
    e.load_state_dict(sd, compute_dtype=mode)
    return e


@pytest.fixture(scope="module")
def eng_f32(synthetic_sd):
    """A default f32 context (switches as the table tool's defaults) shared by the cases that keep no state in it."""
    with pytest.MonkeyPatch.context() as mp:
        for s in SWITCHES:
            mp.delenv(s, raising=False)
        return make_engine(synthetic_sd)


@pytest.fixture(scope="module")
def meter():
    from lass_amd.engine import get_engine
    return get_engine(DEV)


def tiny_inputs(B, L, first=0):
    _, mix = synthetic.make_mixtures(B, L, first=first)
    return torch.from_numpy(mix).to(DEV), torch.from_numpy(synthetic.make_condition(B)).to(DEV)


@pytest.fixture(scope="module")
def oracle_tiny(synthetic_sd):
    """oracle.resunet.forward of the TINY inputs, computed once"""
    from oracle import resunet as orr
    B, L = TINY
    _, mix = synthetic.make_mixtures(B, L)
    cond = synthetic.make_condition(B)
    return orr.forward(orr.to_torch(synthetic_sd), {"mixture": torch.from_numpy(mix)[:, None, :],
                                                    "condition": torch.from_numpy(cond)})["waveform"][:, 0]


# ---- a. lass_separate on caller-kept, guarded buffers ------------------------------------------------------------------------
# f32: the 10 s plan is the only small batch that holds kpart, vprep and mgemm together (32 slots); the bf16 plans have the same
# 27 slots at 2.5 s as at 10 s (asserted), so they take the 268 MB shape.
SHAPES = {"f32": (TINY, (2, 160000), (8, 8077)), "bf16": (TINY, (2, 40077), (8, 8077)), "bf16x3": (TINY, (2, 40077), (8, 8077))}


def guarded_call(e, B, L, need):
    """-> (ws, run): run(byte) fills the guarded workspace with `byte`, prefills the guarded `out` with NaN, calls lass_separate on
    the same pointers and returns a copy of `out`, after checking every guard."""
    mix, cond = tiny_inputs(B, L)
    g_mix, mix = Guarded.of(mix)
    g_cond, cond = Guarded.of(cond)
    g_out, out = Guarded.of(torch.full((B, L), NAN))
    ws = Guarded(need)
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    mix0, cond0 = mix.clone(), cond.clone()

    def run(byte):
        ws.inner.fill_(byte)
        out.fill_(NAN)
        rc = e.lib.lass_separate(e.ctx, P(mix), P(cond), P(out), B, L, P(ws.inner), need, st)
        assert rc == 0, e.lib.lass_last_error(e.ctx)
        torch.cuda.synchronize()
        for name, g in (("workspace", ws), ("out", g_out), ("mixture", g_mix), ("condition", g_cond)):
            assert g.intact(), f"B = {B}, L = {L}, fill {byte:#04x}: a guard byte of {name} changed"
        assert same(mix, mix0) and same(cond, cond0)
        return out.clone()
    return ws, run


@pytest.mark.parametrize("mode", tuple(SHAPES))
def test_separate_on_guarded_poisoned_buffers(mode, table, synthetic_sd, default_switches, oracle_tiny):
    if mode == "f32":
        assert len(table("resunet30", "f32", *TINY)["slots"]) == 29
        assert len(table("resunet30", "f32", 2, 160000)["slots"]) == 32   # a route change that drops a shared slot fails here
        assert table("resunet30", "f32", 8, 8077)["call"]["need"] == 256503808
    else:
        assert len(table("resunet30", mode, 2, 40077)["slots"]) == len(table("resunet30", mode, 2, 160000)["slots"]) == 27
    e = make_engine(synthetic_sd, mode)
    for B, L in SHAPES[mode]:
        t = table("resunet30", mode, B, L)
        need = t["call"]["need"]
        assert e.workspace_bytes(B, L) == need and (t["plan"]["T"], t["plan"]["Tp"]) == \
            {8077: (51, 64), 40077: (251, 256), 160000: (1001, 1024)}[L]
        ws, run = guarded_call(e, B, L, need)
        outs = [run(byte) for byte in FILLS]
        del ws
        assert bool(torch.isfinite(outs[0]).all()), (B, L)
        for byte, o in zip(FILLS[1:], outs[1:]):
            assert same(o, outs[0]), f"{mode} B = {B}, L = {L}: out under fill {byte:#04x} differs from out under 0x00"
        if mode == "f32" and (B, L) == TINY:   # "equal" must not come to mean "equally wrong"
            err = float((outs[0].cpu() - oracle_tiny).pow(2).mean().sqrt())
            print("f32 TINY, fill 0x00: RMS error against the oracle", err)
            assert err < 2e-6, err


# ---- b. graph replay under fresh poison --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (2, 8))
def test_replayed_graph_meets_fresh_poison(B, table, synthetic_sd, default_switches):
    L = TINY[1]
    need = table("resunet30", "f32", B, L)["call"]["need"]
    if B == 8:   # the captured call runs as two half-batch plans side by side
        assert table("resunet30", "f32", B, L, capturing=1, workspace_bytes=need)["call"]["split"] == 1
    e = make_engine(synthetic_sd)
    on, cap0, rep0 = e.graph_stats()
    assert on and e.workspace_bytes(B, L) == need
    ws, run = guarded_call(e, B, L, need)
    outs = [run(byte) for byte in (0xFF, 0x7F, 0x00, 0xFF, 0x7F)]   # eager, eager, capture, replay, replay
    _, cap, rep = e.graph_stats()
    assert (cap - cap0, rep - rep0) == (1, 2), (cap - cap0, rep - rep0)
    assert bool(torch.isfinite(outs[0]).all())
    for i, o in enumerate(outs[1:], 1):
        assert same(o, outs[0]), f"B = {B}: call {i} differs from call 0"


def test_the_engine_refills_its_workspace_in_front_of_a_replay(synthetic_sd, default_switches):
    """The same through Engine.separate: under poison the engine's one workspace is refilled on the call's stream before every
    call, the replayed ones included."""
    B, L = TINY
    e = make_engine(synthetic_sd)
    _, cap0, rep0 = e.graph_stats()
    mix, cond = tiny_inputs(B, L)
    out = torch.empty(B, L, device=DEV)
    outs = []
    for byte in (0xFF, 0x7F, 0x00, 0xFF, 0x7F):
        out.fill_(NAN)
        with _alloc.poisoned(byte):
            e.separate(mix, cond, out=out)
        torch.cuda.synchronize()
        outs.append(out.clone())
        assert bool(torch.isfinite(e.workspace_tensor("encoder_block3", B, L)).all())
    _, cap, rep = e.graph_stats()
    assert e.ws_allocations == 1 and (cap - cap0, rep - rep0) == (1, 2)
    with _alloc.poisoned(0xFF):
        assert bool((_alloc.refill(e._ws_buf) == 0xFF).all())   # what `separate` does in front of its call
    for i, o in enumerate(outs[1:], 1):
        assert same(o, outs[0]), f"call {i} differs from call 0"


# ---- c. named intermediates --------------------------------------------------------------------------------------------------
def test_every_named_intermediate_is_written_whole_or_not_at_all(table, synthetic_sd, default_switches):
    """After a call on a 0xFF workspace and after one on a 0x00 workspace every tensor lass_workspace_tensor names is bit-equal, or
    still 0xFF in every byte (this route never writes it: decoder_block6 under the fused head).  Written in part is the failure."""
    B, L = TINY
    default_switches.setenv("LASS_GRAPH", "0")
    e = make_engine(synthetic_sd)
    assert not e.graph_stats()[0]
    names = sorted(table("resunet30", "f32", B, L)["tensors"])
    assert len(names) >= 31
    mix, cond = tiny_inputs(B, L)
    taps = {}
    for byte in (0xFF, 0x00):
        with _alloc.poisoned(byte):
            out = e.separate(mix, cond)
        torch.cuda.synchronize()
        taps[byte] = {n: e.workspace_tensor(n, B, L).clone() for n in names}
        taps[byte]["out"] = out
    untouched = []
    for n in names + ["out"]:
        a, z = taps[0xFF][n], taps[0x00][n]
        if n != "out" and bool((bits(a).view(torch.uint8) == 0xFF).all()):
            untouched.append(n)
            continue
        assert same(a, z), f"{n}: differs between a 0xFF and a 0x00 workspace (written in part, or computed from stale bytes)"
        assert bool(torch.isfinite(a).all()), n
    print("never written on this route:", untouched)
    must = ["mag", "cos", "sin", "x0", "out_real", "out_imag", "conv_block7a"] + [f"encoder_block{i}" for i in range(1, 7)] + \
        [f"decoder_block{i}" for i in range(1, 6)]
    assert not set(must) & set(untouched) and set(must) <= set(names)
    T, Tp = arch.frames_for(L), arch.padded_frames(arch.frames_for(L))
    x0 = taps[0xFF]["x0"]
    assert Tp in x0.shape and (T, Tp) == (51, 64)
    pad = x0.reshape(B, Tp, -1)[:, T:]
    assert pad.numel() == B * (Tp - T) * 512 and bool((bits(pad) == 0).all())   # exactly 0.0f, not -0.0f


def test_default_makes_no_fill(eng_f32, monkeypatch):
    """LASS_POISON unset, outside `poisoned`: Engine.separate fills nothing (the benchmark's path is torch.empty as before)."""
    assert _alloc.poison_byte() is None or os.environ.get("LASS_POISON")
    if _alloc.poison_byte() is not None:
        monkeypatch.setattr(_alloc, "_byte", None)
    mix, cond = tiny_inputs(*TINY)
    fills = []
    real = torch.Tensor.fill_
    monkeypatch.setattr(torch.Tensor, "fill_", lambda self, *a, **k: (fills.append(tuple(self.shape)), real(self, *a, **k))[1])
    for _ in range(2):   # the first call allocates the workspace, the second reuses it
        out = eng_f32.separate(mix, cond)
    torch.cuda.synchronize()
    assert fills == [] and bool(torch.isfinite(out).all())


# ---- d. the other separator entries ------------------------------------------------------------------------------------------
def test_ragged(eng_f32):
    B, L = 3, 8077
    lo, hi = eng_f32.ragged_bucket(L)
    lens = [lo, (lo + hi) // 2 + 1, hi]
    assert hi == L and lo < lens[1] < hi
    mix, cond = tiny_inputs(B, L)
    for b, n in enumerate(lens):
        mix[b, n:] = NAN   # the rest of a row is never read
    out = torch.empty(B, L, device=DEV)

    def call():
        out.fill_(NAN)
        return eng_f32.separate_ragged(mix, lens, cond, out=out).clone()
    got = across_fills(call)
    assert bool(torch.isfinite(got).all())
    for b, n in enumerate(lens):
        assert bool((bits(got[b, n:]) == 0).all()), b   # the zero tail is written, as 0.0f
        assert float(got[b, :n].abs().max()) > 0


WIN_B, WIN_W, WIN_TOTAL = 3, 8000, 20000
WIN_STARTS = [0, 6000, 12000]   # overlapping windows


def _recording():
    src, _, _ = synthetic.make_clip(5, WIN_TOTAL)
    return torch.from_numpy(np.asarray(src, dtype=np.float32)).to(DEV), torch.from_numpy(synthetic.make_condition(WIN_B)).to(DEV)


def test_windows(eng_f32):
    keep = [(0, 7000), (1000, 6500), (1000, 7500)]   # disjoint: [0, 7000), [7000, 12500), [13000, 19500)
    rec, cond = _recording()
    out = torch.empty(WIN_TOTAL, device=DEV)

    def call():
        out.fill_(NAN)
        return eng_f32.separate_windows(rec, WIN_STARTS, keep, cond, WIN_W, out=out).clone()
    got = across_fills(call)
    kept = torch.zeros(WIN_TOTAL, dtype=torch.bool, device=DEV)
    for s, (lo, hi) in zip(WIN_STARTS, keep):
        kept[s + lo:s + hi] = True
    assert int((~kept).sum()) == 1000
    assert bool(torch.isfinite(got[kept]).all()) and bool(torch.isnan(got[~kept]).all())   # outside the keeps: the prefill


def test_windows_faded(eng_f32):
    from lass_amd import longform
    F = 400
    keep = [(0, 7200), (800, 7200), (800, 7500)]     # zones [6800, 7200) and [12800, 13200), each one fade-out on one fade-in
    fade = [(0, 1), (1, 1), (1, 0)]
    ramp = torch.from_numpy(longform.fade_ramp(F)).to(DEV)
    rec, cond = _recording()
    out = torch.empty(WIN_TOTAL, device=DEV)

    def call():
        out.zero_()   # the contract of the faded form: zero-filled by the caller
        return eng_f32.separate_windows(rec, WIN_STARTS, keep, cond, WIN_W, out=out, fade=fade, ramp=ramp).clone()
    got = across_fills(call)
    assert bool(torch.isfinite(got).all()) and bool((bits(got[19500:]) == 0).all()) and float(got[6800:7200].abs().max()) > 0
    # the plainly stored samples are those of the unfaded call, bit for bit
    plain = torch.full((WIN_TOTAL,), NAN, device=DEV)
    eng_f32.separate_windows(rec, WIN_STARTS, [(0, 6800), (1200, 6800), (1200, 7500)], cond, WIN_W, out=plain)
    stored = ~torch.isnan(plain)
    assert int(stored.sum()) == 19500 - 2 * F and same(got[stored], plain[stored])


def test_multistft_context(default_switches):
    B, L = TINY
    wins = tuple(arch.MS_WIN_LENGTHS)
    assert (arch.MS_N_FFT, wins) == (2048, (256, 512, 2048))
    e = make_engine(synthetic.make_state_dict_ms(), multistft=(arch.MS_N_FFT, wins, arch.MS_MASK_WINDOW))
    mix, cond = tiny_inputs(B, L)
    out = torch.empty(B, L, device=DEV)

    def separate():
        out.fill_(NAN)
        return e.separate(mix, cond, out=out).clone()
    got = across_fills(separate)
    assert bool(torch.isfinite(got).all())

    def components():
        comp = e.stft_components(mix, arch.MS_N_FFT, wins)   # outputs of the library too: poisoned by the seam
        mags = [comp[w][0][:, 0].contiguous() for w in wins]
        cos, sin = (comp[arch.MS_MASK_WINDOW][k][:, 0].contiguous() for k in (1, 2))
        return e.separate_components(mags, cos, sin, cond, L), mags, cos, sin
    wave = across_fills(components)[0]
    assert bool(torch.isfinite(wave).all()) and wave.shape == (B, L)


def test_32k_geometry_context(default_switches):
    B, L = 2, 16077
    e = make_engine(synthetic.make_state_dict(n_fft=2048), stft=(2048, 320))
    mix, cond = tiny_inputs(B, L)
    out = torch.empty(B, L, device=DEV)

    def call():
        out.fill_(NAN)
        return e.separate(mix, cond, out=out).clone()
    assert bool(torch.isfinite(across_fills(call)).all())


# ---- e. stage calls: poisoned y, pool, scratch and (V from memory) the caller's V image --------------------------------------
from test_gpu_stages import ENC_CASES, UPS_REST, W4_BLOCKS  # noqa: E402

# One per kind of launch sequence tools/route_table.cpp tells apart for the stage calls: F(4x4,3x3) with the shortcut fused
# (decoder_block5), with the shortcut as a GEMM (decoder_block3), the 768 -> 384 block (decoder_block2) and a conv1 that widens
# (encoder_block4); the pre-activated first block with its fused 2x2 pool, a 2x2 pool behind F(2x2,3x3), the 1x2 pool of
# encoder_block6 at the 16-bin split-K level, the stand-alone pool of an odd height, and the pool-less bottom block; a GEMM
# transposed conv and the odd-height one.
CONV_CASES = [W4_BLOCKS[i] for i in (0, 2, 3, 4)]
ENC_PICK = [c for c in ENC_CASES if c in ((0, 16, 64), (4, 8, 32), (5, 12, 16), (1, 9, 32), (6, 4, 8))]
UP_PICK = [UPS_REST[0], UPS_REST[2]]


def _stage_inputs(cin, H, W, B=2, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + H * 100 + W)
    return torch.randn(B, cin, H, W, generator=g).to(DEV), torch.from_numpy(synthetic.make_condition(B)).to(DEV)


@pytest.mark.parametrize("prefix,stem,cin,cout,H,W", CONV_CASES)
def test_convblock_stage(eng_f32, prefix, stem, cin, cout, H, W):
    x, cond = _stage_inputs(cin, H, W)
    y = across_fills(lambda: eng_f32.convblock(prefix, x, eng_f32.film(cond), cout))
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("ei,H,W", ENC_PICK)
def test_encoder_block_stage(eng_f32, ei, H, W):
    e = arch.ENCODERS[ei]
    x, cond = _stage_inputs(e.cin, H, W, seed=ei)
    y, pool = across_fills(lambda: eng_f32.encoder_block("base." + e.name, x, eng_f32.film(cond), e.cout, e.down))
    assert bool(torch.isfinite(y).all()) and (pool is None) == (tuple(e.down) == (1, 1))
    assert pool is None or bool(torch.isfinite(pool).all())


@pytest.mark.parametrize("name,cin,cout,up,h,w", UP_PICK)
def test_upconv_stage(eng_f32, name, cin, cout, up, h, w):
    x, cond = _stage_inputs(cin, h, w)
    y = across_fills(lambda: eng_f32.upconv("base." + name, x, eng_f32.film(cond), cout, up))
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("case", ("enc5_32x32", "enc6_32x16", "dec2_32x32"))
def test_v_from_memory_stage_with_a_poisoned_v_image(synthetic_sd, default_switches, case):
    """The layers that read their transformed input from an image one prep launch writes (lass_set_wino4_vprep mode 2: every layer
    whose kind admits it), the image in a poisoned buffer of the caller's (lass_set_wino4_vprep_buffer)."""
    from lass_amd import _lib
    e = make_engine(synthetic_sd)
    name, hw = case.split("_")
    H, W = (int(v) for v in hw.split("x"))
    B = 2
    n = int(name[3])
    if name.startswith("enc"):
        x, cond = _stage_inputs(256 if n == 5 else 384, H, W, B)
        down = (2, 2) if n == 5 else (1, 2)
        run = lambda: e.encoder_block(f"base.encoder_block{n}", x, e.film(cond), 384, down)  # noqa: E731
        cmax = 384
    else:
        x, cond = _stage_inputs(768, H, W, B)
        run = lambda: e.convblock(f"base.decoder_block{n}.conv_block2", x, e.film(cond), 384)  # noqa: E731
        cmax = 768
    v = torch.empty(B * cmax * H * W * 9 // 4, dtype=torch.float32, device=DEV)
    written = []

    def call():
        _alloc.fill_bytes(v, _alloc.poison_byte())
        got = run()
        torch.cuda.synchronize()
        written.append(int((bits(v).view(torch.uint8) != _alloc.poison_byte()).sum()))
        return got
    try:
        _lib.check(e.ctx, e.lib.lass_set_wino4_vprep(e.ctx, 2), "lass_set_wino4_vprep")
        assert e.lib.lass_set_wino4_vprep_buffer(e.ctx, v.data_ptr(), v.numel()) == 0
        got = across_fills(call)
    finally:
        e.lib.lass_set_wino4_vprep_buffer(e.ctx, None, 0)
    print(case, "bytes of the V image written under each fill:", written, "of", v.numel() * 4)
    assert min(written) > 0, "the layer did not take the V-from-memory route: the case compares nothing"
    for t in got if isinstance(got, tuple) else (got,):
        assert bool(torch.isfinite(t).all())


# ---- f. the towers -----------------------------------------------------------------------------------------------------------
# Their workspaces hold index arrays next to the floats.  Read in text.hip / audio_clap.hip before this was run: lass_text_encode
# copies src[0, M) and cap[0, N] up on the call's stream before its first launch, and the kernels read src[r] for r < M and
# cap[n], cap[n + 1] for n < N only; begin_encode copies all 2 B lengths up and the kernels read lens[b], b < B.  No index element
# is read that the same call did not write, so the whole workspace is poisoned, index regions included.
def _keep_tower_workspace(enc, need):
    g = Guarded(need)
    enc._ws = g.inner   # lass_amd._lib.grow_workspace reuses (and, under poison, refills) a cached workspace that is large enough
    return g


def test_text_tower(golden_dir):
    from test_clap_text_gpu import _encoder, _text_sd
    g5 = dict(np.load(os.path.join(golden_dir, "clap_text_g5.npz")))
    enc = _encoder(_text_sd(g5, 2), 2)
    rows = [int(np.nonzero(g5["lengths"] == n)[0][0]) for n in (2, 31, 77)]
    ids, mask = g5["input_ids"][rows, :77], g5["attention_mask"][rows, :77]
    assert [int(n) for n in g5["lengths"][rows]] == [2, 31, 77] and ids.shape == (3, 77) and int(mask[2].sum()) == 77
    ctx = enc._context()
    n = c_size_t()
    assert ctx.lib.lass_text_workspace_bytes(ctx.ctx, 3, 77, byref(n)) == 0
    g = _keep_tower_workspace(enc, n.value)

    def call():
        r = enc.encode_ids(ids, mask, return_pooler=True)
        assert enc._ws.data_ptr() == g.inner.data_ptr()
        return r
    emb, pool = across_fills(call)
    assert g.intact()
    assert np.abs(emb.cpu().numpy() - g5["embed_l2"][rows]).max() <= 2e-5 and bool(torch.isfinite(pool).all())


def test_audio_tower(golden_dir):
    from test_clap_audio_gpu import _batch, _encoder
    g6 = dict(np.load(os.path.join(golden_dir, "clap_audio_g6.npz")))
    assert tuple(int(d) for d in g6["depths"][1]) == (2, 2, 2, 2)
    enc = _encoder(g6, 1)
    wave, lens = _batch([synthetic.make_clap_audio_clip(i) for i in (0, 1)])
    ctx = enc._context()
    n = c_size_t()
    assert ctx.lib.lass_audioq_workspace_bytes(ctx.ctx, 2, byref(n)) == 0
    g = _keep_tower_workspace(enc, n.value)

    def call():
        r = enc.encode_wave48k(wave, lens, return_taps=True)
        assert enc._ws.data_ptr() == g.inner.data_ptr()
        return r
    emb, taps = across_fills(call)
    assert g.intact()
    assert np.abs(emb.cpu().double().numpy() - g6["embed_s1"][:2]).max() <= max(2e-5, 4 * float(g6["embed_dev_s1"][:2].max()))
    assert all(bool(torch.isfinite(t).all()) for t in [taps["logmel"], taps["tokens"], taps["embedding"]] + taps["stages"])


# ---- g. accumulators and meters ----------------------------------------------------------------------------------------------
def test_sample_peak_on_a_prefilled_peak(meter):
    """`peak` is an integer maximum on the float's bits: a prefill of 3.39e38 shows a missing reset, which a NaN does not."""
    from test_r128_gpu import FEATURES, _padded, _pair_rows
    rate_in, rate_out = 16000, 44100
    view = _padded(_pair_rows(rate_in, rate_out, 2, FEATURES[0], 0))
    got = across_fills(lambda: meter.resample_peak(view, rate_in, rate_out), fills=(0x00, 0x7F, 0xFF))
    assert got.shape == (3,) and bool(((got > 0.3) & (got < 1.0)).all())


def test_true_peak_on_a_prefilled_peak(meter):
    from test_r128_gpu import FEATURES, _padded, _pair_rows
    rate_in, rate_out = 32000, 48000
    view = _padded(_pair_rows(rate_in, rate_out, 2, FEATURES[1], 0))
    got = across_fills(lambda: meter.resample_true_peak(view, rate_in, rate_out), fills=(0x00, 0x7F, 0xFF))
    assert got.shape == (3,) and bool(((got > 0.3) & (got < 1.0)).all())


def _programme(B, C, L, rate):
    rng = np.random.Generator(np.random.PCG64([31, L]))
    t = np.arange(L) / rate
    x = 0.05 * rng.standard_normal((B, C, L)) + 0.2 * np.sin(2 * np.pi * 440.0 * t) * (1 + np.arange(B)[:, None, None])
    return torch.from_numpy(x.astype(np.float32)).to(DEV)


def test_loudness_on_poisoned_scratch_and_blocks(meter):
    from lass_amd import loudness as ld
    B, C, L, rate = 2, 2, 16037, 16000
    x = _programme(B, C, L, rate)
    lens = [L, L - 3300]
    lufs, blocks, counts = across_fills(lambda: meter.loudness(x, rate, lengths=lens, return_blocks=True, return_counts=True))
    assert blocks.shape == (B, ld.n_blocks(L, rate)) and bool(torch.isfinite(lufs).all())
    for b, n in enumerate(lens):
        nb = ld.n_blocks(n, rate)
        assert 0 < nb and int(counts[b, 0]) == nb and bool((blocks[b, :nb] > 0).all())
        assert bool((bits(blocks[b, nb:]) == 0).all()), b   # zeros past the recording's own count
    assert ld.n_blocks(lens[1], rate) < ld.n_blocks(lens[0], rate)


def test_loudness_stats_on_poisoned_scratch_and_short_term(meter):
    from lass_amd import loudness as ld
    B, C, L, rate = 2, 2, 52837, 16000
    assert L // (rate // 10) >= 30
    x = _programme(B, C, L, rate)
    lens = [L, L - 3300]
    res = across_fills(lambda: meter.loudness_stats(x, rate, lengths=lens, return_short_term=True))
    short = res["short_term"]
    assert short.shape == (B, ld.n_short_term(L, rate)) and bool(torch.isfinite(res["loudness"]).all())
    for b, n in enumerate(lens):
        ns = ld.n_short_term(n, rate)
        assert 0 < ns and int(res["short_term_blocks"][b]) == ns and bool((short[b, :ns] > 0).all())
        assert bool((bits(short[b, ns:]) == 0).all()), b
    assert ld.n_short_term(lens[1], rate) < ld.n_short_term(lens[0], rate)


EPS32 = float(np.finfo(np.float32).eps)


def _fused_residual(e, a, r):
    """fl(e - a * r) with ONE rounding, for float64 arrays e, r that hold float32 values and a float64 a: what sdr_pass2 computes
    (the compiler contracts the product into the subtraction: v_fma_f64).  a is split into two 26-bit halves, whose products with a
    24-bit r are exact in float64; the two subtractions run in extended precision, where the one that cancels is exact."""
    t = 134217729.0 * a   # 2^27 + 1 (Dekker)
    a_hi = t - (t - a)
    a_lo = a - a_hi
    ld = np.longdouble
    return ((e.astype(ld) - (a_hi * r).astype(ld)) - (a_lo * r).astype(ld)).astype(np.float64)


def _sdr_rows(L, special):
    """(ref, est) (3, L) float32: a noisy estimate, a scaled one, and the special row"""
    rng = np.random.Generator(np.random.PCG64([17, L]))
    ref = (0.1 * rng.standard_normal((3, L))).astype(np.float32)
    ref[1] *= np.float32(3.0)
    est = ref.copy()
    est[0] = ref[0] + (0.01 * rng.standard_normal(L)).astype(np.float32)
    est[1] = np.float32(0.5) * ref[1]
    if special == "est == 0":
        est[2] = 0
    elif special == "ref == 0":
        est[2] = (0.1 * rng.standard_normal(L)).astype(np.float32)
        ref[2] = 0
    else:
        assert special == "est == ref"
    return ref, est


@pytest.mark.parametrize("byte", FILLS, ids=[f"{b:02x}" for b in FILLS])
@pytest.mark.parametrize("L", (1, 255, 4097, 262145))
def test_sdr_stats_on_a_prefilled_stats(meter, L, byte):
    """lass_sdr_stats at B = 3 and at lengths of one thread, less than a workgroup, two workgroups and - above 64 workgroups x 4096
    - the second trip of the grid-stride loop, `stats` prefilled with the fill.

    The bound is derived, not measured.  A product of two float32 is exact in float64, so a term of the first three sums carries no
    error, and a term of the others is a square of a float64 that numpy forms with the same roundings - est - ref, a x ref, and
    est - a x ref as ONE rounded operation (`_fused_residual`: the kernel's fused multiply-add; rounding a x ref first would leave
    the reference, not the kernel, without a correct digit wherever est is a multiple of ref, every row of L = 1 included) - up to
    the rounding of the square itself, which the kernel's fused accumulation skips: 2^-53 of the term.  Summing L float64 terms in any order is within (L - 1) * 2^-53 * sum|terms| of their exact sum.  So each
    of the six sums is within L * 2^-53 * sum|terms| of the sum of numpy's float64 terms, which is taken in extended precision
    (64-bit mantissa, pairwise: 2^-59 * sum|terms| at the most, and exact for L = 1) so that the reference spends none of the
    bound.  The projection coefficient a of the last two sums is formed from the call's own first and third sum, as the kernel
    forms it; those two are held to numpy's directly.  The sums come from float64 atomics across workgroups and are not bit-reproducible, so each fill
    is held to the reference and not to the other fills."""
    assert (L > 64 * 4096) == (L == 262145) and np.finfo(np.longdouble).nmant >= 63
    total = lambda t: float(np.sum(t.astype(np.longdouble)))  # noqa: E731
    u = 2.0 ** -53
    for special in ("est == ref", "est == 0", "ref == 0"):
        ref, est = _sdr_rows(L, special)
        r, e = ref.astype(np.float64), est.astype(np.float64)
        d_ref, d_est = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
        with _alloc.poisoned(byte):
            got = meter.sdr_stats(d_ref, d_est).cpu().numpy()
        assert got.shape == (3, 6) and got.dtype == np.float64
        for b in range(3):
            a = (EPS32 + got[b, 2]) / (got[b, 0] + EPS32)
            if special == "ref == 0" and b == 2:
                assert a == 1.0   # eps / eps
            tr = a * r[b]
            terms = (r[b] * r[b], e[b] * e[b], r[b] * e[b], (e[b] - r[b]) ** 2, tr * tr, _fused_residual(e[b], a, r[b]) ** 2)
            for k, t in enumerate(terms):
                want, bound = total(t), L * u * total(np.abs(t))
                err = abs(got[b, k] - want)
                assert err <= bound, f"{special}, L = {L}, fill {byte:#04x}, row {b}, sum {k}: {got[b, k]!r} vs {want!r}, " \
                                     f"off by {err:.3e}, bound {bound:.3e}"


def test_mix_at_snr_on_a_prefilled_scratch(meter):
    """The bars of test_gpu_parity.py::test_mix_at_snr_vs_reference_formula, under each prefill of `scratch` (its third entry is an
    integer maximum on float bits)."""
    rng = np.random.default_rng(3)
    B, L = 3, 4097
    src = (rng.standard_normal((B, L)) * np.array([[0.05], [0.3], [1.8]])).astype(np.float32)
    noise = (rng.standard_normal((B, L)) * np.array([[0.3], [0.05], [0.5]])).astype(np.float32)
    snrs = np.array([5, 0, -15], dtype=np.float32)
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
    peaks = [float(np.max(np.abs(m))) for m in exp_mix]
    assert any(abs(p - 0.9) < 1e-5 for p in peaks) and any(p < 0.9 for p in peaks)   # both branches
    for byte in FILLS:
        d_src = torch.from_numpy(src).to(DEV)
        with _alloc.poisoned(byte):
            mix = meter.mix_at_snr(d_src, torch.from_numpy(noise).to(DEV), torch.from_numpy(snrs).to(DEV)).cpu().numpy()
        got_src = d_src.cpu().numpy()
        for b in range(B):
            scale = float(np.max(np.abs(exp_mix[b])))
            assert float(np.max(np.abs(mix[b] - exp_mix[b]))) < 2e-6 * max(scale, 1.0), (byte, b)
            assert float(np.max(np.abs(got_src[b] - exp_src[b]))) < 2e-6 * max(scale, 1.0), (byte, b)


def test_segment_mix_on_a_prefilled_scratch(meter):
    """The bars of test_segment_mixer.py::test_segment_mix_vs_oracle, under each prefill of `scratch`."""
    from oracle import waveform_mixers as owm
    B, L, max_mix = 3, 4097, 4
    clips = np.stack([synthetic.make_clip(i, L)[i % 2] for i in range(B)]).astype(np.float32)
    clips[0] *= 6.0    # a loud primary: its mixture clips
    clips[2] *= 1e-4   # a faint clip: both ratio clamps
    random.seed(99)
    draws = owm.draws_like_reference(B, max_mix, -10, 10)
    x = torch.from_numpy(clips)
    o_mix, o_seg = owm.segment_mix(x, *draws)
    peaks = [float(m.abs().max()) for m in o_mix]
    assert any(abs(p - 0.9) < 1e-5 for p in peaks) and any(p < 0.9 for p in peaks)
    for byte in FILLS:
        with _alloc.poisoned(byte):
            mix, seg = meter.segment_mix(x.to(DEV), *(torch.from_numpy(d) for d in draws))
        for b in range(B):
            scale = max(float(o_mix[b].abs().max()), 1e-3)
            assert float((mix[b].cpu() - o_mix[b]).abs().max()) < 2e-6 * max(scale, 1.0) + 2e-6 * scale, (byte, b)
            assert float((seg[b].cpu() - o_seg[b]).abs().max()) < 2e-6 * max(scale, 1.0), (byte, b)
