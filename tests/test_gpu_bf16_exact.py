"""The bf16 and bf16x3 conv launches against oracle/bf16.py: a float64 model of each launch with the kernels' rounding points
(DESIGN.md "bf16 MFMA modes"), given the inputs the launch really read ("teacher forcing").  Errors are |got - ref| / S with S
the same contraction over |operands| and |weights|, as maximum and as RMS; the bar of every case is 4 x D, D being what the
SAME model computed in float32 differs from float64 by - computed here, on the CPU, for the case's own inputs, and printed.
(4: the MFMA's summation order and its 16-term inner sum are not ATen's; the CLAP tests use the same margin for that.)

A. the stage calls (lass_convblock, lass_encoder_block, lass_upconv), modes bf16 and bf16x3: every block of the model table and
   all six transposed convs at the smallest images at which the tiling can go wrong (row tile 8 at W >= 16, 32 at W = 8; column
   tile 32): H = 11 at W = 32, 64 (a halo crossing a column-tile border) and 16, H = 35 at W = 8.  A block runs at the widths of
   its level's class (a multiple of 32, 16 or 8 bins); lass_bf16_shape holds for every such pair, so none is left out.
   A block is two launches: the intermediate conv1's launch left in the caller's scratch is held to the model element by element
   and conv2 is modelled on it (hold_intermediate says why).
B. inside lass_separate, mode bf16: every hand-over form (blocked copies, fused kernels) exists only there.  After an unsplit run
   the workspace still holds every hand-over tensor; each launch's model is fed what was read and compared with what was written.
   The intermediate of a block is not among them (its slot is shared); where a two-launch block reads an f32 tensor, conv1's
   launch is repeated through the stage call and held as in A (replay_conv1).
C. bf16x3 through the 26 workspace taps of test_hip_taps_vs_oracle_every_element.

tests/test_bf16_oracle_cpu.py holds the model itself, the hand-over table below against tools/route_table.cpp, and shows that
these bars separate a right kernel from eight wrong ones."""
import functools
import hashlib
from ctypes import byref, c_int64, c_size_t

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lass_amd import arch, synthetic
from oracle import bf16 as ob
from oracle import resunet as orr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2
MARGIN = 4       # bar = MARGIN x D
FLOOR = 16       # a wrong model (and, in mode bf16, the unrounded oracle) must be further than FLOOR x D from the model
PIECES = {"bf16": 1, "bf16x3": 2}


@functools.lru_cache(maxsize=None)
def oracle_sd():
    return orr.to_torch(synthetic.make_state_dict())


# ---- A: the cases -----------------------------------------------------------------------------------------------------------
def _wide(w):      # the image widths a block of a level `w` bins wide is run at
    return ((11, 32), (11, 64)) if w % 32 == 0 else ((11, 16),) if w == 16 else ((35, 8),)


def block_cases():
    """(id, kind, name, cin, cout, H, W).  kind 'enc': lass_encoder_block (with its pool; H = 11 runs the separate pool kernel,
    H = 12 the fused 2 x 2 pool; encoder_block6's 1 x 2 pool is always fused), 'dec': lass_convblock on the decoder's ConvBlockRes."""
    out = []
    for i, e in enumerate(arch.ENCODERS):
        shapes = _wide(512 >> i) + (((12, 32),) if i < 5 else ())
        out += [(f"{e.name}-{H}x{W}", "enc", e.name, e.cin, e.cout, H, W) for H, W in shapes]
    for d, s in enumerate(arch.DECODERS):
        out += [(f"{s.name}-{H}x{W}", "dec", s.name, 2 * s.cout, s.cout, H, W) for H, W in _wide(512 >> (5 - d))]
    return out


def up_cases():
    """(id, 'up', name, cin, cout, h, w): the transposed conv's input is the level below its block's."""
    out = []
    for d, s in enumerate(arch.DECODERS):
        out += [(f"{s.name}.up-{h}x{w}", "up", s.name, s.cin, s.cout, h, w) for h, w in _wide((512 >> (5 - d)) // s.up[1])]
    return out


CASES = {c[0]: c for c in block_cases() + up_cases()}


def case_inputs(cid):
    _, _kind, _name, cin, _cout, H, W = CASES[cid]
    g = torch.Generator().manual_seed(int(hashlib.sha256(cid.encode()).hexdigest()[:8], 16))
    return torch.randn(B, cin, H, W, generator=g), torch.from_numpy(synthetic.make_condition(B))   # two different conditions


class CpuShifts:
    """site -> the (B, C) shift of that FiLM site, computed on the CPU (oracle.bf16.shift)"""

    def __init__(self, cond):
        self.cond = cond

    @functools.lru_cache(maxsize=None)
    def __call__(self, site):
        return ob.shift(oracle_sd(), self.cond, site)


class EngineShifts:
    """... as the engine's own lass_film wrote it for `cond`: the vector every launch of that engine reads"""

    def __init__(self, eng, cond):
        self.eng, self.full = eng, eng.film(cond.to(DEV)).cpu()

    def __call__(self, site):
        off, n = self.eng.film_offset(site), oracle_sd()[f"film.{site}.bias"].numel()
        assert off >= 0, site
        return self.full[:, off:off + n].clone()


@functools.lru_cache(maxsize=None)
def cpu_shifts():
    return CpuShifts(torch.from_numpy(synthetic.make_condition(B)))


def case_model(cid, pieces, dtype, mutate=None, shifts=None, mid=None):
    """-> {"y": (value, S)} and, for an encoder with a pool, {"pool": (value, S)}; with `mid` (the intermediate the kernel wrote,
    (hi,) or (hi, lo)) conv2 is modelled on it and {"mid": (the model's own unrounded intermediate, its scale)} comes back too"""
    sd = oracle_sd()
    shifts = shifts or cpu_shifts()
    _, kind, name, _cin, _cout, _H, _W = CASES[cid]
    x, _cond = case_inputs(cid)
    if kind == "up":
        up = next(s.up for s in arch.DECODERS if s.name == name)
        y, S = ob.upconv(sd, "base." + name, x, shifts(f"{name}->beta1"), up, pieces, dtype, mutate=mutate)
        return {"y": (y, S)}
    blk = "conv_block1" if kind == "enc" else "conv_block2"
    y, S, m = ob.block(sd, f"base.{name}.{blk}", x, shifts(f"{name}->{blk}->beta1"), shifts(f"{name}->{blk}->beta2"), pieces, dtype,
                       mutate=mutate, mid_copy=mid)
    out = {"y": (y, S)}
    if mid is not None:
        out["mid"] = m
    down = next((e.down for e in arch.ENCODERS if e.name == name), (1, 1)) if kind == "enc" else (1, 1)
    if down != (1, 1):
        out["pool"] = (ob.pool(y, down), ob.pool(S, down))
    return out


def case_plain(cid):
    """oracle.resunet's unrounded block / transposed conv (float32) for the case's inputs"""
    sd = oracle_sd()
    _, kind, name, _cin, _cout, _H, _W = CASES[cid]
    x, cond = case_inputs(cid)
    if kind == "up":
        up = next(s.up for s in arch.DECODERS if s.name == name)
        h = F.leaky_relu(orr._bn(sd, f"base.{name}.bn1", x) + orr.film(sd, cond, f"{name}->beta1"), 0.01)
        return F.conv_transpose2d(h, sd[f"base.{name}.conv1.weight"], stride=up)
    blk = "conv_block1" if kind == "enc" else "conv_block2"
    return orr.conv_block_res(sd, f"base.{name}.{blk}", x, orr.film(sd, cond, f"{name}->{blk}->beta1"),
                              orr.film(sd, cond, f"{name}->{blk}->beta2"))


@functools.lru_cache(maxsize=None)
def case_reference(cid, pieces, shifts=None):
    """The float64 model and D = err(float32 model, float64 model) per output, computed once and shared."""
    ref = case_model(cid, pieces, torch.float64, shifts=shifts)
    m32 = case_model(cid, pieces, torch.float32, shifts=shifts)
    return ref, {k: ob.err(m32[k][0], ref[k][0], ref[k][1]) for k in ref}


# ---- A: the stage calls ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(synthetic_sd):
    from lass_amd.engine import Engine
    es = {}
    for mode in PIECES:
        eng = Engine(DEV)
        eng.load_state_dict(synthetic_sd, mode)
        es[mode] = (eng, EngineShifts(eng, cpu_shifts().cond))   # every case runs under the same two conditions
    yield es
    case_reference.cache_clear()
    es.clear()


def _hold(tag, got, ref, S, D):
    e = ob.err(got, ref, S)
    print(f"{tag}: max {e[0]:.3e} (D {D[0]:.3e})  rms {e[1]:.3e} (D {D[1]:.3e})")
    assert e[0] <= MARGIN * D[0] and e[1] <= MARGIN * D[1], (tag, e, D)
    return e


def run_block(eng, kind, name, x, shift, cout, down, pieces):
    """lass_encoder_block / lass_convblock with a scratch of our own: -> (y, pool or None, the blocked bf16 intermediate conv1's
    launch left in the scratch: (hi,) or (hi, lo) - the lo plane B C H W 2 bytes behind the hi plane, api.hip: run_resblock)"""
    from lass_amd import _lib
    from lass_amd.engine import _ptr, _stream
    xd = x.contiguous().to(DEV)
    Bn, _cin, H, W = xd.shape
    y = torch.empty(Bn, cout, H, W, dtype=torch.float32, device=DEV)
    scratch = torch.zeros_like(y)
    pool = torch.empty(Bn, cout, H // down[0], W // down[1], dtype=torch.float32, device=DEV) if tuple(down) != (1, 1) else None
    if kind == "enc":
        rc = eng.lib.lass_encoder_block(eng.ctx, ("base." + name).encode(), _ptr(xd), Bn, H, W, _ptr(shift), _ptr(y), _ptr(pool), _ptr(scratch),
                                        _stream(eng.device))
    else:
        rc = eng.lib.lass_convblock(eng.ctx, f"base.{name}.conv_block2".encode(), _ptr(xd), Bn, H, W, _ptr(shift), _ptr(y), _ptr(scratch),
                                    _stream(eng.device))
    _lib.check(eng.ctx, rc, "stage call")
    raw = scratch.cpu().view(torch.uint8).reshape(-1)
    n = Bn * cout * H * W * 2
    mid = tuple(ob.unblock(raw[k * n:(k + 1) * n], Bn, cout, H, W) for k in range(pieces))
    return y.cpu(), None if pool is None else pool.cpu(), mid


def hold_intermediate(tag, mid, t64, St, t32, pieces):
    """The intermediate conv1's launch wrote against the model's r(act2(conv1)).  f32 accumulation noise moves a value across a
    bf16 rounding boundary now and then - in a tensor of 1e4-1e5 elements a handful of times, in the float32 model as in the
    kernel, and one such rounding changes the block's output by 30-500 x D - so the block is held in two steps: every element
    written must be the model's rounded value, or the neighbouring one with the model's unrounded value within MARGIN x D1 of the
    written one (D1: the float32 model's own intermediate against the float64 one, in units of its scale St; + half a bf16 step
    for the rounding itself); and conv2 is then modelled on the intermediate that was written."""
    D1 = ob.err(t32, t64, St)
    got = sum(m.double() for m in mid)
    want = sum(ob._q(t64, pieces))
    step = 2.0 ** (-8 * pieces) * got.abs()
    differ = got != want
    bad = differ & ((got - t64).abs() > MARGIN * D1[0] * St + step)
    print(f"{tag}: {int(differ.sum())} of {differ.numel()} elements differ from the rounded model (D1 max {D1[0]:.2e}); beyond the bound: {int(bad.sum())}")
    assert int(bad.sum()) == 0, (tag, int(bad.sum()))

@pytest.mark.parametrize("mode", list(PIECES))
@pytest.mark.parametrize("cid", list(CASES))
def test_stage_call_vs_model(engines, cid, mode):
    _, kind, name, _cin, cout, _H, _W = CASES[cid]
    eng, shifts = engines[mode]
    pieces = PIECES[mode]
    x, cond = case_inputs(cid)
    shift = eng.film(cond.to(DEV))
    assert torch.equal(shift.cpu(), shifts.full)
    got = {}
    if kind == "up":
        got["y"] = eng.upconv("base." + name, x.to(DEV), shift, cout, next(s.up for s in arch.DECODERS if s.name == name)).cpu()
        ref, D = case_reference(cid, pieces, shifts)
    else:
        down = next(e.down for e in arch.ENCODERS if e.name == name) if kind == "enc" else (1, 1)
        got["y"], pool, mid = run_block(eng, kind, name, x, shift, cout, down, pieces)
        if pool is not None:
            got["pool"] = pool
        ref = case_model(cid, pieces, torch.float64, shifts=shifts, mid=mid)
        m32 = case_model(cid, pieces, torch.float32, shifts=shifts, mid=mid)
        hold_intermediate(f"{cid} {mode} intermediate", mid, ref["mid"][0], ref["mid"][1], m32["mid"][0], pieces)
        del ref["mid"]
        # D is the whole block's: the float32 model against the float64 one, each on its own intermediate.  (Given the written
        # intermediate the two differ by conv2's accumulation alone, 3e-8 ... 6e-8 of S, printed for the record: ATen's blocked
        # GEMM sums 3 456 terms more accurately than one accumulator does, and 4 x THAT misses by 4.6 and 4.9 x on two 384-channel
        # bf16x3 cases.)
        D = case_reference(cid, pieces, shifts)[1]
        print(f"{cid} {mode}: D of conv2 alone, given the intermediate:", {k: ob.err(m32[k][0], ref[k][0], ref[k][1]) for k in ref})
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k][0].shape
        _hold(f"{cid} {mode} {k}", got[k], ref[k][0], ref[k][1], D[k])
    if mode == "bf16":  # really the bf16 kernels: the unrounded oracle is far from what they compute
        free, Dfree = case_reference(cid, 1, shifts)
        e = ob.err(got["y"], case_plain(cid), free["y"][1])
        print(f"{cid} vs the unrounded oracle: max {e[0]:.3e} rms {e[1]:.3e}")
        assert e[0] > FLOOR * Dfree["y"][0] or e[1] > FLOOR * Dfree["y"][1], (cid, e, Dfree["y"])


# ---- B: inside lass_separate -----------------------------------------------------------------------------------------------
SEP_L = 6000   # 38 frames in 64 padded rows: every level down to 2 x 16 and 2 x 8, one unsplit run
FORMS = {"default": {}, "fuse_up=0": {"LASS_FUSE_UP": "0"}, "fuse_block=0": {"LASS_FUSE_BLOCK": "0"}, "fuse_catb=0": {"LASS_FUSE_CATB": "0"}}


def _blk(form, cat_in=0, skip_out=0, pool_copies=0, act_out=0):
    return dict(form=form, cat_in=cat_in, skip_out=skip_out, pool_copies=pool_copies, act_out=act_out)


def handover_plan(form):
    """Which tensors this test reads as blocked bf16 copies, per block and transposed conv (ResUNet30, mode bf16), in the words of
    tools/route_table.cpp's `bf16` and `up` lines; tests/test_bf16_oracle_cpu.py holds it to that tool's output."""
    enc = [f"encoder_block{k}" for k in range(1, 7)] + ["conv_block7a"]
    dec = [f"decoder_block{k}" for k in range(1, 7)]
    if form == "fuse_catb=0":   # f32 everywhere, two launches per block
        return {"bf16": {n: _blk("two") for n in enc + dec}, "up": {n: ("bf16", 0, 0) for n in dec}}
    b = {"encoder_block1": _blk("enc1", skip_out=1, pool_copies=1),
         "encoder_block2": _blk("two", cat_in=1, skip_out=1, pool_copies=1),
         "encoder_block3": _blk("two", cat_in=1, skip_out=1, pool_copies=1),
         "encoder_block4": _blk("two", cat_in=1, skip_out=1, pool_copies=1),
         "encoder_block5": _blk("two", cat_in=1, skip_out=1),
         "encoder_block6": _blk("two"),
         "conv_block7a": _blk("two"),
         "decoder_block1": _blk("two", act_out=1),
         "decoder_block2": _blk("two", cat_in=1, act_out=1),
         "decoder_block3": _blk("two", cat_in=1, act_out=1),
         "decoder_block4": _blk("two", cat_in=1, act_out=1),
         "decoder_block5": _blk("two", cat_in=1, act_out=1),
         "decoder_block6": _blk("dec6u", cat_in=1)}
    up = {"decoder_block1": ("bf16", 0, 0), "decoder_block2": ("bf16", 1, 1), "decoder_block3": ("bf16", 1, 1),
          "decoder_block4": ("bf16", 1, 1), "decoder_block5": ("bf16", 1, 1), "decoder_block6": ("inside", 1, 0)}
    if form in ("fuse_up=0", "fuse_block=0"):
        b["decoder_block6"]["form"] = "dec6"
        up["decoder_block6"] = ("bf16", 1, 1)
    if form == "fuse_block=0":
        b["encoder_block1"]["form"] = b["decoder_block6"]["form"] = "two"
    return {"bf16": b, "up": up}


# the launches the chain must contain, by name, per form
MUST_COVER = {
    "default": ["encoder_block1 (enc1)", "decoder_block6 (dec6u)"],
    "fuse_up=0": ["encoder_block1 (enc1)", "decoder_block6.up", "decoder_block6 (dec6)"],
    "fuse_block=0": ["encoder_block1 (two)", "decoder_block6.up", "decoder_block6 (two)"],
    "fuse_catb=0": [],
}
for _f in MUST_COVER:
    MUST_COVER[_f] += [f"encoder_block{k} (two)" for k in range(2, 7)] + ["conv_block7a (two)"] + \
                      [f"decoder_block{k} (two)" for k in range(1, 6)] + [f"decoder_block{k}.up" for k in range(1, 6)]


def sep_inputs():
    """The seeded clips and conditions of test_hip_taps_vs_oracle_every_element, cut to SEP_L samples.  (With first = 4, seed = 7
    the float32 model of decoder_block2 sat 15.1 x D below 'intermediate left unrounded' in the f32-hand-over form - under the 16
    tests/test_bf16_oracle_cpu.py asks for; these inputs leave 49 x at the tightest launch.)"""
    _, mix = synthetic.make_mixtures(B, SEP_L, first=8)
    return torch.from_numpy(mix), torch.from_numpy(synthetic.make_condition(B, seed=5))


class WorkspaceStore:
    """The hand-over tensors of the last lass_separate, decoded from ONE host copy of the workspace: f32 tensors through
    lass_workspace_tensor's offsets and strides, blocked copies through oracle.bf16.unblock (the activated copy at the slot's
    offset, the raw copy B C H W 2 bytes behind it - api.hip: separate_impl's cb[d], pc[i])."""

    def __init__(self, eng, L):
        self.eng, self.L = eng, L
        self.buf = eng._ws_buf.cpu()
        self.lv = ob.levels(arch.padded_frames(arch.frames_for(L)))
        self.cache = {}

    def _where(self, name):
        off, shape, strides = c_size_t(), (c_int64 * 4)(), (c_int64 * 4)()
        rc = self.eng.lib.lass_workspace_tensor(self.eng.ctx, B, self.L, name.encode(), byref(off), shape, strides)
        assert rc == 0, (name, rc)
        return off.value, tuple(shape), tuple(strides)

    def _f32(self, name, C=None):
        off, shape, strides = self._where(name)
        if C is not None:
            shape = (shape[0], C) + shape[2:]
        return self.buf.view(torch.float32).as_strided(shape, strides, off // 4).clone()

    def _blocked(self, slot, C, H, W, raw):
        off = self._where(slot)[0] + (B * C * H * W * 2 if raw else 0)
        return ob.unblock(self.buf[off:off + B * C * H * W * 2], B, C, H, W)

    def get(self, key):
        if key not in self.cache:
            self.cache[key] = self._get(key)
        return self.cache[key]

    def _get(self, key):
        stem, _, kind = key.partition(".")
        if stem.startswith("cat") and kind in ("act", "raw", "f32"):
            d = int(stem[3:])
            s = arch.DECODERS[d]
            H, W = self.lv[5 - d]
            if kind == "f32":
                return self._f32(s.name + ".up", C=2 * s.cout)
            return self._blocked(s.name + ".up", 2 * s.cout, H, W, kind == "raw")
        if stem.startswith("pool") and kind in ("act", "raw"):
            i = int(stem[4:])
            e = arch.ENCODERS[i]
            H, W = self.lv[i + 1]
            return self._blocked(e.name + ".pool", e.cout, H, W, kind == "raw")
        if stem.startswith("decout") and kind == "act":
            d = int(stem[6:])
            H, W = self.lv[5 - d]
            return self._blocked(arch.DECODERS[d].name, arch.DECODERS[d].cout, H, W, False)
        t = self._f32(key)
        return t[:, None] if key == "x0" and t.dim() == 3 else t


def shares(got, out, o32):
    """A written blocked copy against the rounded float64 model: (share of the distinct computed values that differ, the float32
    model's share, number of differing elements that are not the neighbouring bf16 value and lie further than MARGIN x D from
    the float64 model's unrounded value - where a value is so close to zero that its bf16 spacing is below the f32 noise of its
    own sum, the neighbour rule has nothing to hold on to: the float32 model itself breaks it there, see
    tests/test_bf16_oracle_cpu.py).  Shares count each distinct value of the model once (oracle.bf16.distinct)."""
    k64, k32, kg = ob.bf16_key(ob.rne_bf16(out.value)), ob.bf16_key(ob.rne_bf16(o32.value)), ob.bf16_key(got)
    D = ob.err(o32.value, out.value, out.S)
    groups = ob.distinct(out.value)
    far = (kg - k64).abs() > 1
    beyond = (got.double() - out.value).abs() > (MARGIN * D[0]) * out.S + 2.0 ** -8 * got.double().abs()   # + half a bf16 step
    return ob.share_differing(kg, k64, groups), ob.share_differing(k32, k64, groups), int((far & beyond).sum()), D


@functools.lru_cache(maxsize=None)
def _launch_models(name, key):   # the same launch on the same bytes (most launches of the four forms): modelled once
    launch, mid = _launch_models.pending
    kw = {} if mid is None else {"mid": mid}
    return launch.model(torch.float64, **kw), launch.model(torch.float32, **kw)


def _reads_key(launch, mid=None):
    h = hashlib.blake2b(digest_size=16)
    for k in sorted(launch.reads):
        h.update(k.encode())
        h.update(launch.reads[k].contiguous().numpy().tobytes())
    for m in mid or ():
        h.update(m.contiguous().numpy().tobytes())
    return h.hexdigest()


def replay_conv1(eng, launch, shift):
    """The intermediate of a block that lass_separate ran as two launches on an f32 input.  Inside lass_separate it lies in a
    slot every block shares, overwritten by the time the run ends, and ONE of its elements rounded to the other neighbour by f32
    noise moves 9 pixels x all couts of the block's output by 30-500 x D (hold_intermediate) - on decoder_block1's 2 x 16 image
    a seventh of the tensor, where the float32 model, by chance, has no such element.  conv1's launch does not depend on how
    conv2 hands over, so the stage call of the same block on the tensor that was read repeats it, into a scratch of ours."""
    kind, name, cout, down = launch.replay
    return run_block(eng, kind, name, launch.reads["x"], shift, cout, down, 1)[2]


@pytest.mark.parametrize("form", list(FORMS))
def test_separate_launch_by_launch(synthetic_sd, monkeypatch, form):
    """Every launch of one lass_separate against its model, given what it read.  Measured on an MI355X: every launch of every
    form is inside its bar - encoder_block1 fused and as two launches, encoder_block2-5 with cat_in / skip_out / pool_copies
    (0.016 - 0.14 % of the values differ, the float32 model 0.020 - 0.17 %), the transposed convs with in_act / out_copies (0.004 -
    0.013 % against 0.008 - 0.018 %), decoder_block2-5 with cat_in / act_out (0.08 - 0.41 % against 0.09 - 0.21 %), dec6u_fused,
    dec6_fused and the three-launch decoder_block6 (out_real / out_imag at 1.00 x D).
    A block that runs as two launches on an f32 input (encoder_block6, conv_block7a, decoder_block1; every block with
    LASS_FUSE_CATB=0) is held in two steps, as in A: conv1's launch is repeated through the stage call on the tensor that was
    read (replay_conv1), the intermediate it leaves is held element by element (hold_intermediate), and conv2 is modelled on
    it.  Modelled on the MODEL's intermediate instead, decoder_block1 (768 -> 384 on a 2 x 16 image) missed: 0.62 % of its
    activated copy differed against the float32 model's 0.008 %, 1.40e-6 / 2.40e-7 against D = 4.1e-8 / 4.4e-9 with f32
    hand-overs.  Its intermediate differs from the rounded model at 4 of 24 576 elements (9 with LASS_FUSE_CATB=0), each the
    neighbouring bf16 value and within 4 x D1 of the boundary, and given them the block is at 0.033 % against 0.012 %, and
    6.2e-8 / 8.2e-9 against D = 4.1e-8 / 4.3e-9.  Were the repeated launch not the one lass_separate made, conv2's model would be
    built on the wrong intermediate and the block would miss its bar, so the step can fail a right kernel but not pass a wrong
    one.  The blocks that read blocked copies have no stage call and are modelled whole."""
    from lass_amd.engine import Engine
    mix, cond = sep_inputs()
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    eng = Engine(DEV)   # the switches are read when the context is created
    eng.load_state_dict(synthetic_sd, "bf16")
    eng.separate(mix.to(DEV), cond.to(DEV))
    torch.cuda.synchronize()
    for k in FORMS[form]:
        monkeypatch.delenv(k)
    store = WorkspaceStore(eng, SEP_L)
    T = arch.frames_for(SEP_L)
    seen, failed = [], []
    shifts = EngineShifts(eng, cond)
    shift = eng.film(cond.to(DEV))
    assert torch.equal(shift.cpu(), shifts.full)
    for launch in ob.separate_launches(oracle_sd(), shifts, handover_plan(form), store, arch.padded_frames(T), T):
        mid = replay_conv1(eng, launch, shift) if launch.replay else None
        _launch_models.pending = (launch, mid)
        m64, m32 = _launch_models(launch.name + launch.form, _reads_key(launch, mid))
        seen.append(launch.name)
        for out, o32 in zip(m64, m32):
            if out.key == "mid":   # conv1's launch, held element by element as in A; conv2 is modelled on what it wrote
                try:
                    hold_intermediate(f"{form} {launch.name} intermediate", mid, out.value, out.S, o32.value, 1)
                except AssertionError as e:
                    failed.append(e.args[0])
                continue
            C = out.value.shape[1]
            got = store.get(out.key)[:, out.ch0:out.ch0 + C]
            if out.key in ("out_real", "out_imag"):
                got = got[:, :, :T]
            assert got.shape == out.value.shape, (launch.name, out.key, got.shape, out.value.shape)
            tag = f"{form} {launch.name} -> {out.key}[{out.ch0}:{out.ch0 + C}]"
            if not out.bf16:
                D = ob.err(o32.value, out.value, out.S)
                e = ob.err(got, out.value, out.S)
                print(f"{tag}: max {e[0]:.3e} (D {D[0]:.3e})  rms {e[1]:.3e} (D {D[1]:.3e})")
                if not (e[0] <= MARGIN * D[0] and e[1] <= MARGIN * D[1]):
                    failed.append((tag, e, D))
                continue
            share, share32, wrong, D = shares(got, out, o32)
            print(f"{tag}: {share:.3%} of the values differ (float32 model {share32:.3%}); not neighbours and beyond {MARGIN} D: {wrong}")
            if not (share <= MARGIN * share32 and wrong == 0):
                failed.append((tag, share, share32, wrong))
    assert set(MUST_COVER[form]) <= set(seen), set(MUST_COVER[form]) - set(seen)
    assert not failed, failed   # (every launch is modelled on what was really written, so the chain goes on behind a miss)


# ---- C: bf16x3 through the workspace taps ----------------------------------------------------------------------------------
TAPS = ([f"encoder_block{i}" for i in range(1, 7)] + [f"encoder_block{i}.pool" for i in range(1, 7)] + ["conv_block7a"] +
        [f"decoder_block{i}.up" for i in range(1, 7)] + [f"decoder_block{i}" for i in range(1, 6)] + ["out_real", "out_imag"])


def test_bf16x3_taps_vs_oracle_every_element(synthetic_sd):
    """test_hip_taps_vs_oracle_every_element's 26 tensors (L = 25 600) in mode bf16x3 against the plain oracle, in that test's
    measure (maximum deviation over the tensor's largest magnitude): at most 4 x what the pieces = 2 model itself deviates."""
    from lass_amd.resunet import ResUNet30
    L = 25600
    _, mix = synthetic.make_mixtures(B, L, first=8)
    cond = torch.from_numpy(synthetic.make_condition(B, seed=5))
    m = ResUNet30(1, 1, 512)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_sd.items()})
    m = m.to(DEV).eval().set_compute_dtype("bf16x3")
    m({"mixture": torch.from_numpy(mix)[:, None, :].to(DEV), "condition": cond.to(DEV)})
    torch.cuda.synchronize()
    got = {n: m.engine.workspace_tensor(n, B, L).clone().cpu() for n in TAPS}
    sd = oracle_sd()
    taps = {}
    orr.forward(sd, {"mixture": torch.from_numpy(mix)[:, None, :], "condition": cond}, taps=taps)
    model = ob.forward_taps(sd, taps, EngineShifts(m.engine, cond), 2, torch.float64)
    T = arch.frames_for(L)
    for n in TAPS:
        t, ref, mod = got[n], taps[n], model[n]
        if n in ("out_real", "out_imag"):
            t = t[:, :, :T]
        ref, mod = ref.reshape(t.shape), mod.reshape(t.shape)
        scale = float(ref.abs().max())
        dev, own = float((t - ref).abs().max()) / scale, float((mod - ref).abs().max()) / scale
        print(f"{n}: bf16x3 {dev:.3e}, the pieces = 2 model {own:.3e}")
        assert dev <= MARGIN * own, (n, dev, own)
