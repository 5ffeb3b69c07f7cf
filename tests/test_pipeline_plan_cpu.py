"""What `pipeline.separate_files` decides before a pass and computes on the host, without a device: the
layout of the numbers that travel behind a payload (`pipeline.Tail`), the per-file plan (`pipeline.plan_files`) and the
host-route stages (`pipeline.host_target`, `pipeline.host_remix`) against the expressions written out here from
`lass_amd.loudness`, `wavio._resample` and numpy - the arithmetic the GPU host-route tests reach through a whole pass."""
import itertools

import numpy as np
import pytest
import torch

from lass_amd import loudness as ld
from lass_amd import pipeline, wavio
from lass_amd import resample as rs

SR, N_FFT = 16000, 1024


def _options(loudness=None, ceiling_db=None, true_peak=False, meter=False, limiter=False, remix=False):
    return pipeline.Options(loudness, ceiling_db, true_peak, meter, limiter, ld.reach(1.5, SR) if limiter else 0, 2 if limiter else 0, remix)


# ---- the tail -----------------------------------------------------------------------------------------------------------
# every admissible combination: a true peak and a limiter need a ceiling
COMBOS = [c for c in itertools.product((None, -23.0), (None, -1.0), (False, True), (False, True), (False, True))
          if c[1] is not None or not (c[2] or c[4])]
PAYLOADS = [0, 1, 3, 4, 5, 7, 8, 9, 88200]
DTYPES = {"clipped": torch.int32, "limited": torch.int32, "gain": torch.float32, "peak": torch.float32, "loudness": torch.float64,
          "stats": torch.float64, "loudness_in": torch.float64, "limiter_gain": torch.float32, "min_gain": torch.float32,
          "limiter_frames": torch.int32}
# distinct per field, so that a swapped pair fails; -23.1 and the thirds are no float32, and a silent file's loudness is -inf
SENTINELS = {"clipped": 7, "limited": 1, "gain": 0.30000001192092896, "peak": 1.7000000476837158, "loudness": -23.1,
             "stats": [-1.0 / 3.0 - k for k in range(10)], "loudness_in": -np.inf, "limiter_gain": 2.5999999046325684,
             "min_gain": 0.05000000074505806, "limiter_frames": 123456}


def _expected_fields(loudness, ceiling_db, true_peak, meter, limiter):
    level = loudness is not None or ceiling_db is not None
    return (["clipped"] + (["limited", "gain", "loudness"] if level else []) + (["peak"] if true_peak else [])
            + (["stats"] if meter else []) + (["loudness_in", "limiter_gain", "min_gain", "limiter_frames"] if limiter else []))


def _check_tail(tail, nbytes, names):
    assert sorted(tail.where) == sorted(names + ["payload"])
    spans = sorted((lo, hi, name) for name, (lo, hi, _) in tail.where.items())
    assert tail.where["payload"][:2] == (0, nbytes) and tail.nbytes == nbytes
    for (lo, hi, name), (nxt, _, other) in zip(spans, spans[1:]):
        assert hi <= nxt, (name, other)                                 # no field overlaps another or the payload
    for name in names:
        lo, hi, dtype = tail.where[name]
        item = torch.empty(0, dtype=DTYPES[name]).element_size()
        assert getattr(torch, dtype) == DTYPES[name] and lo % item == 0 and hi - lo == item * (10 if name == "stats" else 1)
    assert tail.size >= max(hi for _, hi, _ in spans)                   # what is asked of the pool covers the last field
    payload = torch.from_numpy(np.random.Generator(np.random.PCG64(nbytes)).integers(0, 256, nbytes, dtype=np.uint8))
    buf = torch.full((tail.size,), 0xA5, dtype=torch.uint8)
    tail.put(buf, "payload", payload)
    for name in names:
        tail.put(buf, name, torch.tensor(SENTINELS[name], dtype=DTYPES[name]).reshape(-1))
    for name in names:
        got = tail.get(buf, name)
        if name == "stats":
            assert got.dtype == torch.float64 and got.tolist() == SENTINELS[name]
        else:
            assert got == SENTINELS[name] and type(got) is type(SENTINELS[name]), name
    assert bytes(buf[:nbytes].numpy()) == bytes(payload.numpy())         # the payload is untouched


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "-".join(str(v) for v in c))
def test_target_tail(combo):
    o = _options(*combo)
    for nbytes in PAYLOADS:
        _check_tail(pipeline.Tail.target(nbytes, o), nbytes, _expected_fields(*combo))


@pytest.mark.parametrize("gained", [False, True])
def test_remix_tail(gained):
    for nbytes in PAYLOADS:
        _check_tail(pipeline.Tail.remix(nbytes, gained), nbytes, ["clipped"] + (["limited", "gain"] if gained else []))


def test_tail_sizes_and_offsets():
    """Without options the row is the payload rounded up to 4 and the clip counter; the largest layout keeps the offsets the
    records of every earlier release were read from."""
    for nbytes in PAYLOADS:
        assert pipeline.Tail.target(nbytes, _options()).size == (nbytes + 3) // 4 * 4 + 4
        assert pipeline.Tail.remix(nbytes, True).size == (nbytes + 3) // 4 * 4 + 12
        full = pipeline.Tail.target(nbytes, _options(-23.0, -1.0, True, True, True))
        base = (nbytes + 7) // 8 * 8
        assert {name: lo - base for name, (lo, _, _) in full.where.items() if name != "payload"} == {
            "clipped": 0, "limited": 4, "gain": 8, "peak": 12, "loudness": 16, "stats": 24, "loudness_in": 104, "limiter_gain": 112,
            "min_gain": 116, "limiter_frames": 120}


def test_tail_record_names_the_meter_columns():
    from lass_amd.engine import Engine
    assert {name: Engine.STATS_COLUMNS.index(name) for name in ("loudness_range", "max_momentary", "max_short_term")} == pipeline._STATS
    o = _options(-23.0, -1.0, True, True, True)
    tail = pipeline.Tail.target(5, o)
    buf = torch.zeros(tail.size, dtype=torch.uint8)
    for name in _expected_fields(-23.0, -1.0, True, True, True):
        tail.put(buf, name, torch.tensor(SENTINELS[name], dtype=DTYPES[name]).reshape(-1))
    rec = tail.record(buf, {"path": "device"})
    want = {"path": "device", "clipped": 7}
    want.update(pipeline._level_record(-23.1, np.float32(SENTINELS["gain"]), True, np.float32(SENTINELS["peak"])))
    want.update(pipeline._meter_record(SENTINELS["stats"][5], SENTINELS["stats"][3], SENTINELS["stats"][4]))
    want.update(pipeline._limiter_record(-np.inf, np.float32(SENTINELS["limiter_gain"]), np.float32(SENTINELS["min_gain"]), 123456))
    assert rec == want
    tail = pipeline.Tail.remix(5, True)
    for name in ("clipped", "limited", "gain"):
        tail.put(buf, name, torch.tensor(SENTINELS[name], dtype=DTYPES[name]).reshape(-1))
    assert tail.record(buf, {"target_gain_db": -12.0}) == pipeline._remix_record({"clipped": 7}, -12.0, np.float32(SENTINELS["gain"]), True)


# ---- the planner --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("planfiles")
    rng = np.random.Generator(np.random.PCG64(29))
    paths = [str(d / f"in{k}.wav") for k in range(4)]
    wavio.write_wav_f32(paths[0], 0.1 * rng.standard_normal(16000).astype(np.float32), 16000)
    wavio.write_wav_pcm16(paths[1], 0.1 * rng.standard_normal((22051, 2)).astype(np.float32), 44100)
    wavio.write_wav_pcm16(paths[2], 0.1 * rng.standard_normal((22052, 2)).astype(np.float32), 44101)
    wavio.write_wav_pcm32(paths[3], 0.1 * rng.standard_normal((8000, 9)).astype(np.float32), 16000)
    return d, paths


SHAPES = [("f32", 1, 16000, 16000), ("pcm16", 2, 44100, 22051), ("pcm16", 2, 44101, 22052), ("pcm32", 9, 16000, 8000)]


def _jobs(paths, n=3):
    return [(p, "a caption", p + ".out.wav") + ((p + ".remix.wav",) if n == 4 else ()) for p in paths]


def test_plan_routes_sizes_and_output(files):
    plans = pipeline.plan_files(_jobs(files[1]), None, _options(), SR, N_FFT)
    assert [p.how for p in plans] == ["device", "device", "host", "host"]
    for p, path, (enc, nch, rate, frames) in zip(plans, files[1], SHAPES):
        assert p.info == wavio.wav_info(path) and p.meta == (enc, nch, rate, frames)
        assert (p.n_planes, p.length) == (nch, rs.out_len(frames, *rs.ratio(rate, SR))) == pipeline.model_samples(nch, rate, frames, SR, "each")
        assert (p.enc_o, p.rate_o, p.frames_o, p.ceiling) == (enc, rate, frames, None)      # out_rate=None: the input's frame count
        assert (p.in_path, p.out_path, p.remix_path, p.db, p.amount) == (path, path + ".out.wav", None, None, None)
    mono = pipeline.plan_files(_jobs(files[1]), None, _options(), SR, N_FFT, channels="mono")
    assert [p.n_planes for p in mono] == [1, 1, 1, 1] and [p.length for p in mono] == [p.length for p in plans]


def test_plan_overrides(files):
    plans = pipeline.plan_files(_jobs(files[1]), None, _options(ceiling_db=0.0), SR, N_FFT, encoding="pcm16", out_rate=48000)
    for p, (enc, nch, rate, frames) in zip(plans, SHAPES):
        assert (p.enc_o, p.rate_o) == ("pcm16", 48000)
        assert p.frames_o == rs.out_len(p.length, *rs.ratio(SR, 48000)) and p.frames_o != frames
        assert p.ceiling == ld.ceiling_for(0.0, "pcm16") and p.ceiling < 1.0 and p.ceiling.dtype == np.float32   # capped: PCM16 cannot hold 1
    assert [p.how for p in plans] == ["device", "device", "host", "host"]
    same = pipeline.plan_files(_jobs(files[1][:1]), None, _options(ceiling_db=0.0), SR, N_FFT, encoding="f32", out_rate=16000)[0]
    assert same.frames_o == 16000 and same.ceiling == np.float32(1.0)
    # a true peak narrows the device route to the pairs Engine.resample_true_peak takes
    for out_rate in (None, 48000, 11025):
        tp = pipeline.plan_files(_jobs(files[1]), None, _options(ceiling_db=-1.0, true_peak=True), SR, N_FFT, out_rate=out_rate)
        assert [p.how for p in tp] == [pipeline.route(wavio.wav_info(f), SR, out_rate, True) for f in files[1]]


def test_plan_remix_paths_and_amounts(files):
    paths = files[1][:3]
    dbs = [-np.inf, -12.0, 6.0]
    three = pipeline.plan_files(_jobs(paths), dbs, _options(remix=True), SR, N_FFT)
    four = pipeline.plan_files(_jobs(paths, 4), dbs, _options(remix=True), SR, N_FFT)
    for k, path in enumerate(paths):
        assert (three[k].out_path, three[k].remix_path) == (None, path + ".out.wav")       # the remix is the job's one file
        assert (four[k].out_path, four[k].remix_path) == (path + ".out.wav", path + ".remix.wav")
        for p in (three[k], four[k]):
            assert p.db == dbs[k] and p.amount == pipeline.remix_coefficient(dbs[k]) and p.amount.dtype == np.float32
    assert [p.amount for p in three] == [np.float32(-1.0), np.float32(10.0 ** (-12.0 / 20.0) - 1.0), np.float32(10.0 ** (6.0 / 20.0) - 1.0)]


def test_plan_refuses_a_file_not_longer_than_the_padding(files, tmp_path):
    short, edge = str(tmp_path / "short.wav"), str(tmp_path / "edge.wav")
    wavio.write_wav_pcm16(short, np.zeros(512 * 44100 // 16000, dtype=np.float32), 44100)       # 512 samples at the model rate
    wavio.write_wav_pcm16(edge, np.zeros(513, dtype=np.float32), 16000)
    assert pipeline.plan_files([(edge, "x", "out.wav")], None, _options(), SR, N_FFT)[0].length == 513
    with pytest.raises(ValueError, match=r"short\.wav: a recording of 512 samples is not longer than the reflect padding \(n_fft/2 = 512\)"):
        pipeline.plan_files(_jobs(files[1]) + [(short, "x", "out.wav")], None, _options(), SR, N_FFT)
    with pytest.raises(ValueError, match=r"edge\.wav: .*n_fft/2 = 1024"):
        pipeline.plan_files([(edge, "x", "out.wav")], None, _options(), SR, 2048)


# ---- the host stages ----------------------------------------------------------------------------------------------------
TARGET, CEILING_DB = -14.0, -6.0


@pytest.fixture(scope="module")
def separated(tmp_path_factory):
    """A 1.5 s stereo 44 101 Hz PCM16 file (the host route), its decoded planes and a stand-in for its separated planes at the
    model rate: a bed of noise with clicks, so that a ceiling binds."""
    path = str(tmp_path_factory.mktemp("hoststage") / "in.wav")
    rng = np.random.Generator(np.random.PCG64(31))
    frames = 66152
    wavio.write_wav_pcm16(path, (0.05 * rng.standard_normal((frames, 2))).astype(np.float32), 44101)
    L = rs.out_len(frames, *rs.ratio(44101, SR))
    x = 0.02 * rng.standard_normal((2, L))
    x[:, 3000::4000] += 0.7
    return path, pipeline._host_decode(path, wavio.wav_info(path), "each"), x.astype(np.float32)


def _plan(path, o, dbs=None, **kw):
    plan = pipeline.plan_files([(path, "x", path + ".out.wav")], dbs, o, SR, N_FFT, **kw)[0]
    assert plan.how == "host"
    return plan


def _resampled(x, plan):
    return np.stack([wavio._resample(p, SR, plan.rate_o) for p in x])[:, :plan.frames_o]


def test_host_target_plain(separated):
    path, _, x = separated
    plan = _plan(path, _options())
    y, rec = pipeline.host_target(x, plan, _options(), SR)
    want = _resampled(x, plan)
    assert y.dtype == np.float32 and y.shape == (2, 66152) and np.array_equal(y, want)
    assert rec == {"clipped": pipeline.host_clip_count(want, "pcm16")}


@pytest.mark.parametrize("true_peak", [False, True])
def test_host_target_level(separated, true_peak):
    path, _, x = separated
    o = _options(TARGET, CEILING_DB, true_peak)
    plan = _plan(path, o)
    y, rec = pipeline.host_target(x, plan, o, SR)
    r = _resampled(x, plan)
    measured = ld.integrated_loudness(x, SR)
    pk = np.float32(ld.true_peak(r, 44101)) if true_peak else float(np.abs(r).max())
    g, bit = ld.gain_for(measured, pk, TARGET, ld.ceiling_for(CEILING_DB, "pcm16"))
    assert bit                                                          # the clicks hold the gain down
    want = (g * r.astype(np.float32)).astype(np.float32)
    assert y.dtype == np.float32 and np.array_equal(y, want)
    entries = {"loudness_out": measured, "gain": float(g), "gain_db": float(20.0 * np.log10(np.float64(g))), "peak_limited": True, "clipped": 0}
    if true_peak:
        entries["true_peak_db"] = float(20.0 * np.log10(np.float64(g) * np.float64(pk)))
    assert rec == entries and list(rec)[-1] == "clipped"


def test_host_target_meter(separated):
    path, _, x = separated
    o = _options(meter=True)
    plan = _plan(path, o, encoding="f32", out_rate=SR)
    y, rec = pipeline.host_target(x, plan, o, SR)
    assert np.array_equal(y, x[:, :plan.frames_o]) and plan.frames_o == x.shape[1]       # the meter writes nothing into a file
    p, q = ld.block_powers(x, SR), ld.short_term_powers(x, SR)
    assert rec == {"loudness_range": ld.loudness_range(q)[0], "max_momentary": ld.max_momentary(p), "max_short_term": ld.max_short_term(q),
                   "clipped": 0}


@pytest.mark.parametrize("meter", [False, True])
def test_host_target_limiter(separated, meter):
    path, _, x = separated
    o = _options(TARGET, CEILING_DB, True, meter, True)
    plan = _plan(path, o)
    y, rec = pipeline.host_target(x, plan, o, SR)
    ceiling, H = ld.ceiling_for(CEILING_DB, "pcm16"), ld.reach(1.5, SR)
    l_in = ld.integrated_loudness(x, SR)
    g = ld.gain_for(l_in, None, TARGET, None)[0]
    v = ld.limit(x, SR, g, ceiling, H)[0].astype(np.float32)
    g = np.float32(g * ld.gain_for(ld.integrated_loudness(v, SR), None, TARGET, None)[0])
    v, G, e = ld.limit(x, SR, g, ceiling, H)
    v = v.astype(np.float32)
    r = _resampled(v, plan)
    measured, pk = ld.integrated_loudness(v, SR), np.float32(ld.true_peak(r, 44101))
    trim, bit = ld.gain_for(measured, pk, TARGET, ceiling)
    assert np.array_equal(y, (trim * r.astype(np.float32)).astype(np.float32))
    want = {"loudness_in": l_in, "limiter_gain_db": float(20.0 * np.log10(np.float64(g))), "limiter_reduction_db": float(20.0 * np.log10(G.min())),
            "limiter_frames": int(np.count_nonzero(ld.limiter_curve(e, g, ceiling, H)[2] < 1.0)),
            "loudness_out": measured, "gain": float(trim), "gain_db": float(20.0 * np.log10(np.float64(trim))), "peak_limited": bool(bit),
            "true_peak_db": float(20.0 * np.log10(np.float64(trim) * np.float64(pk)))}
    if meter:                                                           # the figures of the LIMITED planes
        p, q = ld.block_powers(v, SR), ld.short_term_powers(v, SR)
        want.update(loudness_range=ld.loudness_range(q)[0], max_momentary=ld.max_momentary(p), max_short_term=ld.max_short_term(q))
    want["clipped"] = 0
    assert rec == want and rec["limiter_frames"] > 0 and rec["limiter_reduction_db"] < 0.0


@pytest.mark.parametrize("db,ceiling_db", [(-12.0, None), (-np.inf, None), (12.0, -3.0), (0.0, 0.0)])
def test_host_remix(separated, db, ceiling_db):
    path, dry, x = separated
    o = _options(ceiling_db=ceiling_db, remix=True)
    plan = _plan(path, o, [db])
    v, rec = pipeline.host_remix(x, dry, plan, SR)
    want = pipeline.remix_host(dry, _resampled(x, plan), pipeline.remix_coefficient(db))
    if ceiling_db is None:
        assert rec == {"clipped": pipeline.host_clip_count(want, "pcm16")}
    else:
        g, bit = ld.gain_for(-np.inf, np.float32(np.abs(want).max()), None, ld.ceiling_for(ceiling_db, "pcm16"))
        want = (g * want).astype(np.float32)
        assert bit == (db == 12.0)                                      # the boost meets its ceiling; the file given back does not
        assert rec == {"target_gain_db": db, "gain": float(g), "gain_db": float(20.0 * np.log10(np.float64(g))), "peak_limited": bit,
                       "clipped": 0}
    assert v.dtype == np.float32 and np.array_equal(v, want)
    if db == 0.0:
        assert np.array_equal(v, dry)                                   # at 0 dB the file comes back as it went in
