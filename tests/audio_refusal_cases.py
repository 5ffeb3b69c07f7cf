"""The argument sets that the twelve audio file entry points of the C layer must refuse, and one set each that they accept.

One list drives three things: the recording of tests/golden/audio_refusals.json (made once, on the commit before
lass_amd/csrc/audio_args.h existed), tests/test_audio_args_cpu.py (the header alone, through tools/audio_args_table.cpp) and
tests/test_audio_refusals_gpu.py (the library, through ctypes).

Pointers are integers of a made-up address space: buffer k of BUFFERS starts at (k + 1) << 28, so a value says which buffer it
lies in and how far, 0 is NULL, and alignment and overlap are what they would be in memory.  The GPU replay maps each value into
a real allocation of the buffer's size (`translate`); the CPU tool takes the integers as they are.

Shapes are the smallest the refusal tests of these entries use: B = 2, 2 channels, L = 1000, the ratio 441/160 (and 160/441 for
the decoder).  Every mutation is refused before anything is launched."""

B, CH, L, UP, DOWN = 2, 2, 1000, 441, 160
N_TAPS = 8821                       # lass_amd.resample.n_taps(441, 160) == n_taps(160, 441)
CEIL = 2757                         # ceil(1000 * 441 / 160)
L_DEC = 363                         # ceil(1000 * 160 / 441)
PS, RS = L + 3, 2 * (L + 3)         # plane and row stride of the planes, in floats
ROW16, ROW32 = CEIL * CH * 2, CEIL * CH * 4
RAW_ROW = L * CH * 2
HOP = 25                            # 40 hop bins: 37 blocks, 11 short-term blocks
NB, NS = 37, 11
SCRATCH, SCRATCH_STATS = 5 * B * CH * 40 * 8, (5 * CH + 1) * B * 40 * 8
PCM16, PCM32, F32 = 0, 1, 2
K48 = [1.5351828863637502, -2.691804030199196, 1.198426263333146, -1.6906995865986896, 0.7325047060963897,
       0.9950442970178917, -1.9900885940357833, 0.9950442970178917, -1.990076284018423, 0.9901009040531438]

# name -> bytes (each at least what the good call of any entry touches)
BUFFERS = {
    "planes": B * RS * 4, "taps": 16385 * 4, "out_bytes": B * (ROW32 + 8), "dry": B * (ROW32 + 8), "amount": B * 4, "gain": B * 4,
    "clipped": B * 4, "peak": B * 4, "raw": B * (RAW_ROW + 8), "dec": B * CH * (L_DEC + 1) * 4, "os_taps": 81 * 4,
    "lengths": B * 4, "weights": CH * 4, "meter_out": B * 10 * 8, "blocks": B * NB * 8, "short_term": B * NS * 8,
    "scratch": SCRATCH_STATS, "loudness": B * 3 * 8, "limited": B * 4, "window": 2 * (2 * 512 + 2) * 4, "lim_out": B * CH * L * 4,
    "curve": B * L * 4, "envelope": B * L * 4, "min_gain": B * 4, "frames": B * 4,
}
_BASE = {name: (k + 1) << 28 for k, name in enumerate(BUFFERS)}


def at(name, offset=0):
    """The made-up address of byte `offset` of buffer `name`."""
    return _BASE[name] + offset


def translate(value, real_base):
    """The real address for a made-up one: real_base maps a buffer's name to where its allocation starts."""
    if value == 0:
        return 0
    name = min(_BASE, key=lambda n: abs(value - _BASE[n]))
    return real_base[name] + (value - _BASE[name])


# kinds: p device pointer, i int, q int64, z size_t, f float, d double, coef ten host doubles (or None).  The stream comes last in
# every signature and is not listed.
_PLANES = [("planes", "p"), ("row_stride", "q"), ("plane_stride", "q"), ("B", "i"), ("channels", "i")]
_FILTER = [("up", "i"), ("down", "i"), ("taps", "p"), ("n_taps", "i")]
_DRY = [("dry", "p"), ("dry_row_stride_bytes", "q"), ("dry_encoding", "i"), ("amount", "p")]
_OUT = [("out_bytes", "p"), ("out_row_stride_bytes", "q"), ("frames_out", "i"), ("clipped", "p")]
_DECODE = ([("raw", "p"), ("row_stride_bytes", "q"), ("B", "i"), ("frames", "i"), ("channels", "i"), ("encoding", "i")] + _FILTER +
           [("out", "p"), ("L_out", "i")])
_METER = _PLANES + [("L", "i"), ("lengths", "p"), ("hop", "i"), ("coef", "coef"), ("weights", "p"), ("out", "p"), ("blocks", "p"),
                    ("nb_max", "i")]
PARAMS = {
    "lass_decode_resample": _DECODE,
    "lass_decode_resample_planar": _DECODE,
    "lass_resample_encode": _PLANES + [("L_in", "i")] + _FILTER + [("encoding", "i")] + _OUT,
    "lass_resample_encode_gain": _PLANES + [("L_in", "i")] + _FILTER + [("encoding", "i"), ("gain", "p")] + _OUT,
    "lass_resample_peak": _PLANES + [("L_in", "i")] + _FILTER + [("frames_out", "i"), ("peak", "p")],
    "lass_remix_encode": _PLANES + [("L_in", "i")] + _FILTER + _DRY + [("encoding", "i"), ("gain", "p")] + _OUT,
    "lass_remix_peak": _PLANES + [("L_in", "i")] + _FILTER + _DRY + [("frames_out", "i"), ("peak", "p")],
    "lass_resample_true_peak": _PLANES + [("L_in", "i")] + _FILTER + [("frames_out", "i"), ("os", "i"), ("os_taps", "p"),
                                                                     ("n_os_taps", "i"), ("peak", "p")],
    "lass_loudness": _METER + [("scratch", "p"), ("scratch_bytes", "z")],
    "lass_loudness_stats": _METER + [("short_term", "p"), ("ns_max", "i"), ("scratch", "p"), ("scratch_bytes", "z")],
    "lass_loudness_gain": [("loudness", "p"), ("peak", "p"), ("B", "i"), ("target_lufs", "d"), ("ceiling", "f"), ("gain", "p"),
                           ("limited", "p")],
    "lass_limit": _PLANES + [("L", "i"), ("os", "i"), ("os_taps", "p"), ("n_os_taps", "i"), ("gain", "p"), ("ceiling", "f"), ("H", "i"),
                             ("window", "p"), ("out", "p"), ("out_row_stride", "q"), ("out_plane_stride", "q"), ("curve", "p"),
                             ("envelope", "p"), ("curve_row_stride", "q"), ("min_gain", "p"), ("frames", "p")],
}

_G_PLANES = dict(planes=at("planes"), row_stride=RS, plane_stride=PS, B=B, channels=CH)
_G_FILTER = dict(up=UP, down=DOWN, taps=at("taps"), n_taps=N_TAPS)
_G_DRY = dict(dry=at("dry"), dry_row_stride_bytes=ROW32 + 8, dry_encoding=PCM32, amount=at("amount"))
_G_OUT = dict(encoding=PCM16, out_bytes=at("out_bytes"), out_row_stride_bytes=ROW16 + 8, frames_out=CEIL, clipped=at("clipped"))
_G_PEAK = dict(_G_PLANES, L_in=L, **_G_FILTER, frames_out=CEIL, peak=at("peak"))
_G_DECODE = dict(raw=at("raw"), row_stride_bytes=RAW_ROW + 8, B=B, frames=L, channels=CH, encoding=PCM16, up=DOWN, down=UP,
                 taps=at("taps"), n_taps=N_TAPS, out=at("dec"), L_out=L_DEC)
_G_METER = dict(_G_PLANES, L=L, lengths=at("lengths"), hop=HOP, coef=K48, weights=at("weights"), out=at("meter_out"),
                blocks=at("blocks"), nb_max=NB, scratch=at("scratch"))
GOOD = {
    "lass_decode_resample": _G_DECODE,
    "lass_decode_resample_planar": _G_DECODE,
    "lass_resample_encode": dict(_G_PLANES, L_in=L, **_G_FILTER, **_G_OUT),
    "lass_resample_encode_gain": dict(_G_PLANES, L_in=L, **_G_FILTER, **_G_OUT, gain=at("gain")),
    "lass_resample_peak": _G_PEAK,
    "lass_remix_encode": dict(_G_PLANES, L_in=L, **_G_FILTER, **_G_DRY, **_G_OUT, gain=0),
    "lass_remix_peak": dict(_G_PEAK, **_G_DRY),
    "lass_resample_true_peak": dict(_G_PEAK, os=4, os_taps=at("os_taps"), n_os_taps=81),
    "lass_loudness": dict(_G_METER, scratch_bytes=SCRATCH),
    "lass_loudness_stats": dict(_G_METER, short_term=at("short_term"), ns_max=NS, scratch_bytes=SCRATCH_STATS),
    "lass_loudness_gain": dict(loudness=at("loudness"), peak=at("peak"), B=B, target_lufs=-23.0, ceiling=0.5, gain=at("gain"),
                               limited=at("limited")),
    "lass_limit": dict(_G_PLANES, L=L, os=4, os_taps=at("os_taps"), n_os_taps=81, gain=at("gain"), ceiling=0.5, H=24,
                       window=at("window"), out=at("lim_out"), out_row_stride=CH * L, out_plane_stride=L, curve=at("curve"),
                       envelope=at("envelope"), curve_row_stride=L, min_gain=at("min_gain"), frames=at("frames")),
}
# the buffers whose bytes no refused call may change, per entry
OUTPUTS = {
    "lass_decode_resample": ["dec"], "lass_decode_resample_planar": ["dec"], "lass_resample_encode": ["out_bytes", "clipped"],
    "lass_resample_encode_gain": ["out_bytes", "clipped"], "lass_resample_peak": ["peak"], "lass_remix_encode": ["out_bytes", "clipped"],
    "lass_remix_peak": ["peak"], "lass_resample_true_peak": ["peak"], "lass_loudness": ["meter_out", "blocks", "scratch"],
    "lass_loudness_stats": ["meter_out", "blocks", "short_term", "scratch"], "lass_loudness_gain": ["gain", "limited"],
    "lass_limit": ["lim_out", "curve", "envelope", "min_gain", "frames"],
}

# What lass_decode_resample's limits refuse, in the order of the checks (each entry that shares them names the operands its way).
_FILTER_BAD = [dict(channels=9), dict(channels=0), dict(up=0), dict(down=0), dict(up=-3), dict(up=65537), dict(taps=0), dict(n_taps=0),
               dict(n_taps=8820), dict(n_taps=16385), dict(up=30000, down=1, n_taps=3)]
_PLANES_BAD = [dict(frames_out=CEIL + 1), dict(frames_out=0), dict(plane_stride=L - 1), dict(row_stride=PS + L - 1)]
_DRY_BAD = [dict(dry=0), dict(amount=0), dict(dry_encoding=3), dict(dry_encoding=-1), dict(dry_row_stride_bytes=ROW32 - 4),
            dict(dry_row_stride_bytes=ROW32 + 2), dict(dry_encoding=PCM16, dry_row_stride_bytes=ROW16 - 4), dict(dry=at("dry", 2)),
            dict(amount=at("amount", 2))]
_OUT_BAD = [dict(encoding=3), dict(encoding=-1), dict(out_bytes=0), dict(out_bytes=at("out_bytes", 2)),
            dict(out_row_stride_bytes=ROW16 + 2), dict(out_row_stride_bytes=ROW16 - 4), dict(clipped=at("clipped", 2))]
_FIRST_BAD = [dict(planes=0), dict(B=0), dict(B=65536), dict(L_in=0)]
_PEAK_BAD = _FIRST_BAD + [dict(peak=0)] + _FILTER_BAD + _PLANES_BAD + [dict(planes=at("planes", 2)), dict(peak=at("peak", 2))]
_ENCODE_ORDER = [dict(B=0, encoding=3), dict(encoding=3, channels=9), dict(channels=9, up=0), dict(up=0, taps=0),
                 dict(n_taps=8820, frames_out=0), dict(frames_out=0, plane_stride=L - 1),
                 dict(plane_stride=L - 1, out_row_stride_bytes=ROW16 + 2), dict(out_row_stride_bytes=ROW16 + 2, out_bytes=at("out_bytes", 2)),
                 dict(out_bytes=at("out_bytes", 2), planes=at("planes", 2))]
_PEAK_ORDER = [dict(peak=0, channels=9), dict(channels=9, up=0), dict(up=0, n_taps=8820), dict(n_taps=8820, frames_out=0),
               dict(frames_out=0, plane_stride=L - 1), dict(row_stride=PS + L - 1, peak=at("peak", 2))]
_DRY_ORDER = [dict(plane_stride=L - 1, dry=0), dict(amount=0, dry_encoding=3), dict(dry_encoding=3, dry_row_stride_bytes=ROW32 + 2),
              dict(dry_row_stride_bytes=ROW32 + 2, dry=at("dry", 2))]
_METER_BAD = [dict(planes=0), dict(coef=None), dict(out=0), dict(B=0), dict(L=0), dict(channels=0), dict(channels=9), dict(B=32768),
              dict(hop=0), dict(hop=38401), dict(plane_stride=L - 1), dict(row_stride=PS + L - 1), dict(nb_max=NB - 1), dict(scratch=0),
              dict(scratch_bytes=SCRATCH - 8), dict(planes=at("planes", 2)), dict(lengths=at("lengths", 2)),
              dict(weights=at("weights", 2)), dict(out=at("meter_out", 4)), dict(blocks=at("blocks", 4)), dict(scratch=at("scratch", 4))]
_METER_ORDER = [dict(L=0, channels=9), dict(channels=9, hop=0), dict(hop=0, plane_stride=L - 1), dict(plane_stride=L - 1, nb_max=NB - 1),
                dict(nb_max=NB - 1, scratch=0), dict(scratch_bytes=8, out=at("meter_out", 4))]
# decided by lass_loudness_filter, not by the header: a pole on the unit circle, a coefficient that is not finite
_COEF_BAD = [dict(coef=K48[:3] + [-2.0, 1.0] + K48[5:]), dict(coef=[float("nan")] + K48[1:]), dict(coef=K48[:9] + [float("inf")])]

# entry -> [(mutation, decided by a device-side predicate)]
BAD = {
    "lass_decode_resample": [(m, False) for m in [
        dict(raw=0), dict(out=0), dict(B=0), dict(B=65536), dict(frames=0), dict(encoding=3), dict(encoding=-1)] + _FILTER_BAD + [
        dict(L_out=L_DEC + 1), dict(L_out=L_DEC - 1), dict(L_out=0), dict(row_stride_bytes=RAW_ROW - 4), dict(row_stride_bytes=RAW_ROW + 2),
        dict(raw=at("raw", 2)), dict(up=1, down=7, n_taps=3, L_out=143, encoding=5), dict(up=30000, down=1, n_taps=3, L_out=L * 30000),
        # order
        dict(frames=0, encoding=3), dict(encoding=3, channels=9), dict(channels=9, up=0), dict(up=0, taps=0), dict(n_taps=8820, L_out=0),
        dict(L_out=0, row_stride_bytes=RAW_ROW + 2), dict(row_stride_bytes=RAW_ROW + 2, raw=at("raw", 2))]],
    "lass_decode_resample_planar": [(m, False) for m in [
        dict(raw=0), dict(B=65536), dict(channels=9), dict(encoding=3), dict(n_taps=8820), dict(L_out=L_DEC + 1),
        dict(row_stride_bytes=RAW_ROW - 4), dict(raw=at("raw", 2)), dict(frames=0, encoding=3), dict(channels=9, L_out=0),
        dict(L_out=0, row_stride_bytes=RAW_ROW + 2)]],
    "lass_resample_encode": [(m, False) for m in _FIRST_BAD + _FILTER_BAD + _PLANES_BAD + _OUT_BAD + [
        dict(planes=at("planes", 2)), dict(up=30000, down=1, n_taps=3, frames_out=5)] + _ENCODE_ORDER],
    "lass_resample_encode_gain": [(m, False) for m in [
        dict(gain=0), dict(gain=at("gain", 2)), dict(gain=0, planes=0), dict(gain=at("gain", 2), B=0)] + _FIRST_BAD + [
        dict(channels=9), dict(n_taps=8820), dict(frames_out=0), dict(plane_stride=L - 1), dict(encoding=3),
        dict(out_row_stride_bytes=ROW16 - 4), dict(out_bytes=at("out_bytes", 2)), dict(clipped=at("clipped", 2))] + _ENCODE_ORDER],
    "lass_resample_peak": [(m, False) for m in _PEAK_BAD + _PEAK_ORDER],
    "lass_remix_encode": [(m, False) for m in _FIRST_BAD + _FILTER_BAD + _PLANES_BAD + _DRY_BAD + _OUT_BAD + [
        dict(gain=at("gain", 2)), dict(planes=at("planes", 2))] + _ENCODE_ORDER[:6] + _DRY_ORDER + [
        dict(dry=at("dry", 2), out_row_stride_bytes=ROW16 + 2), dict(out_bytes=at("out_bytes", 2), gain=at("gain", 2))]],
    "lass_remix_peak": [(m, False) for m in _PEAK_BAD + _DRY_BAD + _PEAK_ORDER[:5] + _DRY_ORDER + [
        dict(amount=at("amount", 2), peak=at("peak", 2))]],
    "lass_resample_true_peak": [(m, False) for m in _PEAK_BAD + [
        dict(os=3), dict(os=1), dict(os=0), dict(n_os_taps=80), dict(os=2), dict(os_taps=0), dict(os_taps=at("os_taps", 2)),
        dict(up=1, down=50000, n_taps=1000001, frames_out=1)] + _PEAK_ORDER[:5] + [
        dict(plane_stride=L - 1, os=3), dict(os=3, os_taps=0), dict(n_os_taps=80, peak=at("peak", 2))]] + [
        # the ratio's 21 frames do not fit the LDS: lass_resample_true_peak_fits
        (dict(up=1, down=800, n_taps=16001, frames_out=2), True),
        (dict(up=1, down=800, n_taps=16001, frames_out=2, peak=at("peak", 2)), False)],
    "lass_loudness": [(m, False) for m in _METER_BAD + _METER_ORDER] + [(m, True) for m in _COEF_BAD] + [
        (dict(_COEF_BAD[0], scratch=at("scratch", 4)), False)],
    "lass_loudness_stats": [(m, False) for m in _METER_BAD[:14] + [
        dict(scratch_bytes=SCRATCH_STATS - 8), dict(scratch_bytes=SCRATCH), dict(ns_max=NS - 1), dict(short_term=at("short_term", 4)),
        dict(out=at("meter_out", 4))] + _METER_ORDER + [dict(blocks=at("blocks", 4), ns_max=NS - 1)]] + [
        (m, True) for m in _COEF_BAD] + [(dict(_COEF_BAD[1], ns_max=NS - 1), False)],
    "lass_loudness_gain": [(m, False) for m in [
        dict(loudness=0), dict(gain=0), dict(B=0), dict(B=-1), dict(ceiling=-1.0), dict(ceiling=float("nan")), dict(ceiling=float("inf")),
        dict(peak=0), dict(target_lufs=float("inf")), dict(target_lufs=float("-inf")), dict(loudness=at("loudness", 4)),
        dict(peak=at("peak", 2)), dict(gain=at("gain", 2)), dict(limited=at("limited", 2)),
        dict(B=0, ceiling=-1.0), dict(ceiling=-1.0, peak=0), dict(peak=0, target_lufs=float("inf")),
        dict(target_lufs=float("inf"), gain=at("gain", 2))]],
    "lass_limit": [(m, False) for m in [
        dict(planes=0), dict(gain=0), dict(window=0), dict(out=0), dict(B=0), dict(B=65536), dict(channels=0), dict(channels=9), dict(L=0),
        dict(H=0), dict(H=513), dict(os=3), dict(os=0), dict(n_os_taps=80), dict(os=2), dict(os_taps=0), dict(os=1, os_taps=0, n_os_taps=5),
        dict(os=1, n_os_taps=0), dict(ceiling=0.0), dict(ceiling=-1.0), dict(ceiling=float("inf")), dict(ceiling=float("nan")),
        dict(plane_stride=L - 1), dict(row_stride=PS + L - 1), dict(out_plane_stride=L - 1), dict(out_row_stride=2 * L - 1),
        dict(curve_row_stride=L - 1), dict(curve=0, curve_row_stride=L - 1), dict(out=at("planes")),
        dict(out=at("planes", 4 * (RS + PS + L - 1))), dict(planes=at("lim_out", 4 * (2 * CH * L - 1)), row_stride=CH * L, plane_stride=L),
        dict(planes=at("planes", 2)), dict(out=at("lim_out", 2)), dict(curve=at("curve", 1)), dict(envelope=at("envelope", 2)),
        dict(min_gain=at("min_gain", 2)), dict(frames=at("frames", 2)), dict(gain=at("gain", 2)), dict(window=at("window", 2)),
        dict(os_taps=at("os_taps", 2)),
        # order
        dict(B=0, channels=9), dict(channels=9, L=0), dict(L=0, H=0), dict(H=0, os=3), dict(os=3, n_os_taps=80),
        dict(n_os_taps=80, ceiling=0.0), dict(ceiling=0.0, plane_stride=L - 1), dict(plane_stride=L - 1, out_plane_stride=L - 1),
        dict(out_row_stride=2 * L - 1, curve_row_stride=L - 1), dict(curve_row_stride=L - 1, out=at("planes")),
        dict(out=at("planes", 2))]],
}


def case_id(mutation):
    """A mutation's key in the fixture: its items in order, pointers as buffer+offset."""
    def show(k, v):
        if isinstance(v, list):
            return "[" + ",".join(repr(float(x)) for x in v) + "]"
        if isinstance(v, int) and v >= 1 << 28:
            name = min(_BASE, key=lambda n: abs(v - _BASE[n]))
            return f"{name}{v - _BASE[name]:+d}"
        return repr(v)
    return " ".join(f"{k}={show(k, v)}" for k, v in mutation.items())


def cases():
    """(entry, case id, the full argument set, decided by a device-side predicate) of every refusal."""
    for entry, bad in BAD.items():
        for mutation, device in bad:
            yield entry, case_id(mutation), dict(GOOD[entry], **mutation), device


def call(lib, ctx, entry, args, real_base, stream):
    """Run one argument set through the library: (rc, lass_last_error's text)."""
    import ctypes
    conv = {"p": lambda v: ctypes.c_void_p(translate(v, real_base)), "i": int, "q": int, "z": int, "f": float, "d": float,
            "coef": lambda v: None if v is None else (ctypes.c_double * 10)(*v)}
    rc = getattr(lib, entry)(ctx, *[conv[kind](args[name]) for name, kind in PARAMS[entry]], ctypes.c_void_p(stream))
    return rc, (lib.lass_last_error(ctx) or b"").decode()
