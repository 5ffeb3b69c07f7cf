"""Host-only: oracle/bf16.py - the model the GPU tests of the bf16 modes are held to (tests/test_gpu_bf16_exact.py) - checked
without a GPU: (a) its rounding helpers against torch's own conversion, the model against oracle.resunet where rounding changes
nothing, and the decoder of the blocked hand-over layout; (b) the hand-over table of the GPU test against the plan
tools/route_table.cpp prints; (c) for every case of the GPU test, that its bar (4 x D) lies far below what each of eight wrong
models does (more than 16 x D in the maximum or the RMS measure), and that the float32 model alone flips under 2 % of the
elements of a written bf16 copy."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import bf16 as ob
from oracle import resunet as orr
from test_bf16_routing_cpu import build_route_table
import test_gpu_bf16_exact as gx


# ---- (a) the helpers and the model itself -------------------------------------------------------------------------------------
def test_rne_bf16_is_torchs_conversion():
    g = torch.Generator().manual_seed(1)
    # ties (to even, both ways), both signs, a value that rounds up into the next binade, zeros, and 1e5 random values
    edge = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875, 1.998046875, -1.998046875, 255.5, 0.0, -0.0,
                         1.0039062, 1.0039064, 3.0e-5, -7.1e8])
    rnd = torch.cat((torch.randn(50000, generator=g), torch.randn(50000, generator=g) * torch.exp(4 * torch.randn(50000, generator=g))))
    for t in (edge, rnd):
        want = t.to(torch.bfloat16).float()
        assert torch.equal(ob.rne_bf16(t), want)
        assert torch.equal(ob.rne_bf16(t.double()), want.double())   # the float64 path rounds on the same grid
    assert float(ob.rne_bf16(torch.tensor([1.998046875]))) == 2.0 and float(ob.rne_bf16(torch.tensor([1.00390625]))) == 1.0
    tr = ob.trunc_bf16(rnd)
    assert torch.all(tr.abs() <= rnd.abs()) and torch.equal(tr.to(torch.bfloat16).float(), tr)
    assert not torch.equal(tr, ob.rne_bf16(rnd))
    key = ob.bf16_key(torch.tensor([1.0, 1.0078125, 0.99609375, -1.0, -1.0078125, 0.0, -0.0]))
    assert key[1] - key[0] == 1 and key[0] - key[2] == 1 and key[3] == -key[0] and key[4] == -key[1] and key[5] == key[6] == 0


def test_split2_reconstructs_to_16_bits():
    g = torch.Generator().manual_seed(2)
    for t in (torch.randn(100000, generator=g), torch.randn(100000, generator=g).double()):
        hi, lo = ob.split2(t)
        assert torch.equal(hi, ob.rne_bf16(t)) and torch.equal(lo, ob.rne_bf16(t - hi))
        assert float(((hi + lo - t).abs() / t.abs()).max()) <= 2.0 ** -16


def _exact_sd(cin, cout, g):
    """A float64 ConvBlockRes whose operands are bf16-exact at every rounding point: BN is the identity (var + eps = 1), the
    inputs, weights and shifts are small integers and every activation stays positive (the leaky branch would scale by 0.01)."""
    sd = {}
    for bn, c in (("bn1", cin), ("bn2", cout)):
        sd[f"p.{bn}.weight"] = torch.ones(c, dtype=torch.float64)
        sd[f"p.{bn}.bias"] = torch.zeros(c, dtype=torch.float64)
        sd[f"p.{bn}.running_mean"] = torch.zeros(c, dtype=torch.float64)
        sd[f"p.{bn}.running_var"] = torch.full((c,), 1.0 - 1e-5, dtype=torch.float64)
    sparse = lambda *shape: (torch.randint(-1, 2, shape, generator=g) * (torch.rand(shape, generator=g) < 0.1)).double()
    sd["p.conv1.weight"] = sparse(cout, cin, 3, 3)
    sd["p.conv2.weight"] = sparse(cout, cout, 3, 3)
    if cin != cout:
        sd["p.shortcut.weight"] = sparse(cout, cin, 1, 1)
        sd["p.shortcut.bias"] = torch.randint(-3, 4, (cout,), generator=g).double()
    return sd


@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 32)])
def test_model_is_the_plain_block_where_rounding_changes_nothing(cin, cout):
    g = torch.Generator().manual_seed(cin)
    sd = _exact_sd(cin, cout, g)
    x = torch.randint(-1, 2, (2, cin, 7, 9), generator=g).double()
    f1 = torch.full((2, cin), 2.0)
    f2 = torch.randint(100, 120, (2, cout), generator=g).float()
    ref = orr.conv_block_res(sd, "p", x, f1.double()[:, :, None, None], f2.double()[:, :, None, None])
    y, S, mid = ob.block(sd, "p", x, f1, f2, 1, torch.float64)
    assert float(mid.min()) > 0 and float(mid.max()) < 256 and float(y.abs().max()) > 10   # positive, bf16-exact, not trivial
    assert float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((S - y.abs()).min()) >= -1e-9
    # given as copies, the same operands give the same block
    y2, _, _ = ob.block(sd, "p", x if cin == cout else None, f1, f2, 1, torch.float64, act_copy=x + 2.0, raw_copy=x)
    assert torch.equal(y2, y)
    # ... and the split mode has nothing left to add
    y3, _, _ = ob.block(sd, "p", x, f1, f2, 2, torch.float64)
    assert float((y3 - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_transposed_conv_model_is_the_plain_one_where_rounding_changes_nothing():
    g = torch.Generator().manual_seed(5)
    cin, cout = 16, 8
    sd = {"p.bn1.weight": torch.ones(cin, dtype=torch.float64), "p.bn1.bias": torch.zeros(cin, dtype=torch.float64),
          "p.bn1.running_mean": torch.zeros(cin, dtype=torch.float64), "p.bn1.running_var": torch.full((cin,), 1.0 - 1e-5, dtype=torch.float64),
          "p.conv1.weight": torch.randint(-2, 3, (cin, cout, 2, 2), generator=g).double()}
    x = torch.randint(-1, 2, (2, cin, 5, 6), generator=g).double()
    f = torch.full((2, cin), 2.0)
    for up in ((2, 2), (1, 2)):
        w = sd["p.conv1.weight"][:, :, :up[0], :up[1]].contiguous()
        y, S = ob.upconv(dict(sd, **{"p.conv1.weight": w}), "p", x, f, up, 1, torch.float64)
        ref = F.conv_transpose2d(F.leaky_relu(orr._bn(sd, "p.bn1", x) + f.double()[:, :, None, None], 0.01), w, stride=up)
        assert float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max()) and float((S - y.abs()).min()) >= -1e-9


def _blocked_bytes(t):
    """(B, C, H, W) bf16-exact floats -> the bytes of [B][C/8][H][W][8 x bf16], written here from the layout's definition"""
    Bn, C, H, W = t.shape
    u = t.reshape(Bn, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)
    return u.view(torch.int16).reshape(-1).view(torch.uint8)


def test_unblock_inverts_the_blocked_layout():
    g = torch.Generator().manual_seed(3)
    Bn, C, H, W = 2, 24, 5, 7
    act, raw = (ob.rne_bf16(torch.randn(Bn, C, H, W, generator=g)) for _ in range(2))
    slot = torch.cat((_blocked_bytes(act), _blocked_bytes(raw), torch.zeros(64, dtype=torch.uint8)))   # the activated copy first
    n = Bn * C * H * W * 2
    assert torch.equal(ob.unblock(slot, Bn, C, H, W), act)
    assert torch.equal(ob.unblock(slot[n:], Bn, C, H, W), raw)
    assert torch.equal(ob.unblock(bytes(slot[n:2 * n].numpy().tobytes()), Bn, C, H, W), raw)
    # channel c of clip b at (y, x) is element c % 8 of the 16-byte unit ((b * C/8 + c / 8) * H + y) * W + x
    b, c, y, x = 1, 13, 2, 4
    unit = ((b * (C // 8) + c // 8) * H + y) * W + x
    two = slot[n + unit * 16 + 2 * (c % 8): n + unit * 16 + 2 * (c % 8) + 2]
    assert float((two.view(torch.int16).to(torch.int32) << 16).view(torch.float32)) == float(raw[b, c, y, x])


# ---- (b) the hand-over table ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return build_route_table(tmp_path_factory.mktemp("route_bf16_exact"))


@pytest.mark.parametrize("form,switches", [("default", {}), ("fuse_up=0", {"up": 0}), ("fuse_block=0", {"block": 0}), ("fuse_catb=0", {"catb": 0})])
def test_handover_table_is_the_planned_one(table, form, switches):
    from lass_amd import arch
    t_pad = arch.padded_frames(arch.frames_for(gx.SEP_L))
    assert t_pad == 64 and arch.frames_for(gx.SEP_L) == 38
    t = table(t_pad, mode=1, **switches)
    plan = gx.handover_plan(form)
    assert plan["bf16"] == t["bf16"]
    assert plan["up"] == t["up"]
    assert set(gx.FORMS[form]) == {"LASS_FUSE_" + k.upper() for k in switches}


# ---- (c) the bars can tell right from wrong ---------------------------------------------------------------------------------------
def _applicable(kind, has_raw=True, has_shortcut=True):
    muts = list(ob.MUTATIONS)
    if kind == "up":
        muts = [m for m in muts if m not in ("mid_unrounded", "replicate_pad")]   # no intermediate, no padding
    if not has_raw:
        muts.remove("raw_for_act")   # the launch is handed the activated copy alone
    return muts


def _row(tag, D, muts):
    worst = min(max(e[0] / D[0], e[1] / D[1]) for e in muts.values())
    print(f"{tag}: D max {D[0]:.2e} rms {D[1]:.2e} | " + " ".join(f"{m} {e[0] / D[0]:.0f}x/{e[1] / D[1]:.0f}x" for m, e in muts.items()))
    return worst


@pytest.mark.parametrize("cid", list(gx.CASES))
def test_stage_case_bars_separate_right_from_wrong(cid):
    kind = gx.CASES[cid][1]
    for pieces in (1, 2):
        ref, D = gx.case_reference(cid, pieces)
        assert all(d[0] > 0 and d[1] > 0 for d in D.values())
        if pieces == 2:   # the mutations are those of the bf16 mode; the split mode's D is printed for the record
            print(f"{cid} bf16x3: D max {D['y'][0]:.2e} rms {D['y'][1]:.2e}")
            continue
        muts = {}
        for m in _applicable(kind):
            y = gx.case_model(cid, 1, torch.float64, mutate=m)["y"][0]
            muts[m] = ob.err(y, ref["y"][0], ref["y"][1])
        assert _row(cid, D["y"], muts) > gx.FLOOR, cid
        e = ob.err(gx.case_plain(cid), ref["y"][0], ref["y"][1])   # the GPU test's lower bound has room
        assert max(e[0] / D["y"][0], e[1] / D["y"][1]) > gx.FLOOR, (cid, e, D["y"])


class ModelStore:
    """The hand-over tensors as the float64 model itself writes them: the free-running chain."""

    def __init__(self, taps):
        self.t = {k: taps[k] for k in ("x0", "mag", "cos", "sin")}

    def get(self, key):
        if key.startswith("cat") and key.endswith(".f32"):
            name = gx.arch.DECODERS[int(key[3])].name
            return torch.cat((self.t[name + ".up"], self.t["encoder_block%d" % (6 - int(key[3]))]), 1)
        return self.t[key]

    def put(self, out):
        v = (ob.rne_bf16(out.value) if out.bf16 else out.value).float()
        if out.key.startswith("cat"):
            if out.key not in self.t:
                self.t[out.key] = torch.zeros(v.shape[0], 2 * gx.arch.DECODERS[int(out.key[3])].cout, *v.shape[2:])
            self.t[out.key][:, out.ch0:out.ch0 + v.shape[1]] = v
        else:
            self.t[out.key] = v


@functools.lru_cache(maxsize=None)
def _sep_taps():
    mix, cond = gx.sep_inputs()
    taps = {}
    orr.forward(gx.oracle_sd(), {"mixture": mix[:, None, :], "condition": cond}, taps=taps)
    return taps, cond


_seen = {}


@pytest.mark.parametrize("form", list(gx.FORMS))
def test_separate_launch_bars_separate_right_from_wrong(form):
    from lass_amd import arch
    taps, cond = _sep_taps()
    T = arch.frames_for(gx.SEP_L)
    store = ModelStore(taps)
    names = []
    for launch in ob.separate_launches(gx.oracle_sd(), gx.CpuShifts(cond), gx.handover_plan(form), store, arch.padded_frames(T), T):
        names.append(launch.name)
        m64 = launch.model(torch.float64)
        for out in m64:
            store.put(out)
        key = (launch.name + launch.form, gx._reads_key(launch))
        if key in _seen:   # the same launch on the same bytes in an earlier form
            continue
        _seen[key] = True
        m32 = launch.model(torch.float32)
        kind = "up" if launch.name.endswith(".up") else "block"
        muts = _applicable(kind, has_raw=not (kind == "up" and "act" in launch.reads))
        Ds = [ob.err(o32.value, out.value, out.S) for out, o32 in zip(m64, m32)]
        for out, o32, D in zip(m64, m32, Ds):
            assert D[0] > 0 and D[1] > 0
            if out.bf16:
                k64, k32 = ob.bf16_key(ob.rne_bf16(out.value)), ob.bf16_key(ob.rne_bf16(o32.value))
                share = ob.share_differing(k32, k64, ob.distinct(out.value))
                print(f"{form} {launch.name} -> {out.key}: the float32 model flips {share:.3%}, {int(((k64 - k32).abs() > 1).sum())} of them "
                      "further than the neighbouring bf16 value")
                assert 0 < share < 0.02, (launch.name, out.key, share)
        # a wrong launch must show in at least one tensor it writes
        res = {}
        for m in muts:
            om = launch.model(torch.float64, m)
            best = max(range(len(m64)), key=lambda k: max(a / d for a, d in zip(ob.err(om[k].value, m64[k].value, m64[k].S), Ds[k])))
            e = ob.err(om[best].value, m64[best].value, m64[best].S)
            res[m] = (e[0] * Ds[0][0] / Ds[best][0], e[1] * Ds[0][1] / Ds[best][1])   # in units of the first tensor's D, for the table
        assert _row(f"{form} {launch.name} ({', '.join(o.key for o in m64)})", Ds[0], res) > gx.FLOOR, launch.name
    assert set(gx.MUST_COVER[form]) <= set(names), set(gx.MUST_COVER[form]) - set(names)
