"""ctypes binding of liblass_hip.so (include/lass_hip.h).  No CPU fallback: a missing library is a hard error."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_long, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LASS_HIP_LIB") or os.path.join(_HERE, "csrc", "liblass_hip.so")  # env: another build (A/B)

_lib = None

# every symbol include/lass_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("lass_version", c_int, []),
    ("lass_create", c_int, [POINTER(c_void_p), c_int]),
    ("lass_create_stft", c_int, [POINTER(c_void_p), c_int, c_int, c_int]),
    ("lass_stft_geometry", c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    ("lass_create_multistft", c_int, [POINTER(c_void_p), c_int, c_int, c_int, POINTER(c_int), c_int]),
    ("lass_destroy", c_int, [c_void_p]),
    ("lass_last_error", c_char_p, [c_void_p]),
    ("lass_set_param", c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int, c_int]),
    ("lass_finalize", c_int, [c_void_p, c_int]),
    ("lass_workspace_bytes", c_int, [c_void_p, c_int, c_int, POINTER(c_size_t)]),
    ("lass_separate", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    ("lass_separate_ragged", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t,
                                     c_void_p]),
    ("lass_ragged_bucket", c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int)]),
    ("lass_front_end_ragged", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    ("lass_istft_ragged", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                  c_void_p]),
    ("lass_separate_windows", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                      c_size_t, c_void_p]),
    ("lass_front_end_windows", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    ("lass_istft_windows", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p]),
    ("lass_separate_windows_faded", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                            c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    ("lass_istft_windows_faded", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64,
                                         c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("lass_separate_ragged_linked", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int,
                                            c_int, c_void_p, c_size_t, c_void_p]),
    ("lass_separate_windows_linked", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                             c_int64, c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    ("lass_masked_stft", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("lass_masked_stft_windows", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    ("lass_stft_magphase", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    ("lass_mix_at_snr", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ("lass_decode_resample", c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                     c_void_p, c_int, c_void_p]),
    ("lass_decode_resample_planar", c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                            c_void_p, c_int, c_void_p]),
    ("lass_resample_encode", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                     c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    ("lass_loudness", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_double), c_void_p,
                              c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    ("lass_resample_peak", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                   c_void_p, c_void_p]),
    ("lass_loudness_gain", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, c_float, c_void_p, c_void_p, c_void_p]),
    ("lass_resample_encode_gain", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                          c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    ("lass_resample_true_peak", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                        c_int, c_void_p, c_int, c_void_p, c_void_p]),
    ("lass_loudness_stats", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_double),
                                    c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    ("lass_limit", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_float, c_int,
                           c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    ("lass_remix_encode", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                  c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    ("lass_remix_peak", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    ("lass_segment_mix", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    ("lass_multi_stft", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_void_p),
                                POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    ("lass_graph_stats", c_int, [c_void_p, POINTER(c_long), POINTER(c_long)]),
    ("lass_set_graph_replay", c_int, [c_void_p, c_int]),
    ("lass_set_wino4_splits", c_int, [c_void_p, c_int]),
    ("lass_set_wino4_vprep", c_int, [c_void_p, c_int]),
    ("lass_set_wino4_vprep_buffer", c_int, [c_void_p, c_void_p, c_size_t]),
    ("lass_set_head_fold", c_int, [c_void_p, c_int]),
    ("lass_set_head_sc_fold", c_int, [c_void_p, c_int]),
    ("lass_set_pw_split", c_int, [c_void_p, c_int]),
    ("lass_set_wino4_gemm", c_int, [c_void_p, c_int]),
    ("lass_separate_components", c_int, [c_void_p, POINTER(c_void_p), c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                         c_int, c_void_p, c_size_t, c_void_p]),
    ("lass_stft_components", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_int),
                                     POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    ("lass_istft_nfft", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("lass_istft", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("lass_film", c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    ("lass_film_width", c_int, [c_void_p]),
    ("lass_film_offset", c_int, [c_void_p, c_char_p]),
    ("lass_film_raw", c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    ("lass_convblock", c_int, [c_void_p, c_char_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    ("lass_encoder_block", c_int, [c_void_p, c_char_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    ("lass_front_end", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("lass_workspace_tensor", c_int, [c_void_p, c_int, c_int, c_char_p, POINTER(c_size_t), POINTER(c_int64),
                                      POINTER(c_int64)]),
    ("lass_upconv", c_int, [c_void_p, c_char_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("lass_mask_apply", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                c_void_p, c_void_p]),
    ("lass_sdr_stats", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ("lass_text_create", c_int, [POINTER(c_void_p), c_int]),
    ("lass_text_destroy", c_int, [c_void_p]),
    ("lass_text_last_error", c_char_p, [c_void_p]),
    ("lass_text_set_param", c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    ("lass_text_finalize", c_int, [c_void_p]),
    ("lass_text_layers", c_int, [c_void_p]),
    ("lass_text_workspace_bytes", c_int, [c_void_p, c_int, c_int, POINTER(c_size_t)]),
    ("lass_text_encode", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    ("lass_audioq_create", c_int, [POINTER(c_void_p), c_int]),
    ("lass_audioq_destroy", c_int, [c_void_p]),
    ("lass_audioq_last_error", c_char_p, [c_void_p]),
    ("lass_audioq_set_param", c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    ("lass_audioq_finalize", c_int, [c_void_p]),
    ("lass_audioq_stages", c_int, [c_void_p]),
    ("lass_audioq_workspace_bytes", c_int, [c_void_p, c_int, POINTER(c_size_t)]),
    ("lass_audioq_encode_wave48k", c_int, [c_void_p, c_void_p, POINTER(c_int), c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
    ("lass_audioq_encode_wave32k", c_int, [c_void_p, c_void_p, POINTER(c_int), c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
    ("lass_set_profiling", c_int, [c_void_p, c_int]),
    ("lass_profile_count", c_int, [c_void_p]),
    ("lass_profile_get", c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_double), POINTER(c_int)]),
    ("lass_profile_reset", c_int, [c_void_p]),
]


class LassError(RuntimeError):
    pass


def load():
    """Load liblass_hip.so (once).  torch is imported first so the library binds to the HIP runtime torch loaded."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (must precede the dlopen: one libamdhip64 per process)

    if not os.path.exists(LIB_PATH):
        raise LassError(
            f"{LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  lass_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(ctx, rc: int, what: str):
    if rc < 0:
        msg = load().lass_last_error(ctx)
        raise LassError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
    return rc


class TowerContext:
    """Owns one context of a CLAP tower with its weights uploaded: the lass_text_ctx / lass_audioq_ctx behind the symbols
    <family>_create, _destroy, _last_error, _set_param and _finalize (family "lass_text" or "lass_audioq")."""

    def __init__(self, family: str, dev, tensors):
        """tensors: the (name, tensor) pairs the tower's kernels read, on the torch device `dev`."""
        import torch

        self.lib, self.family = load(), family
        h = c_void_p()
        rc = self.fn("create")(ctypes.byref(h), dev.index if dev.index is not None else torch.cuda.current_device())
        if rc < 0:
            raise LassError(f"{family}_create failed ({rc}): {self.fn('last_error')(None).decode()}")
        self.ctx = h
        self.key = self.key_of(dev, tensors)
        torch.cuda.current_stream(dev).synchronize()  # <family>_set_param copies on the NULL stream
        for name, p in tensors:
            t = p.detach().to(torch.float32).contiguous()
            shape = (c_int64 * t.dim())(*t.shape)
            self.check(self.fn("set_param")(self.ctx, name.encode(), c_void_p(t.data_ptr()), shape, t.dim()),
                       f"{family}_set_param({name})")
        self.check(self.fn("finalize")(self.ctx), f"{family}_finalize")

    @staticmethod
    def key_of(dev, tensors):
        """What an upload is valid for: the device, and every tensor's storage and version."""
        return (dev, tuple((p.data_ptr(), p._version) for _, p in tensors))

    def fn(self, name: str):
        return getattr(self.lib, f"{self.family}_{name}")

    def check(self, rc: int, what: str) -> int:
        if rc < 0:
            raise LassError(f"{what} failed ({rc}): {self.fn('last_error')(self.ctx).decode()}")
        return rc

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.fn("destroy")(self.ctx)
                self.ctx = None
        except Exception:
            pass


def grow_workspace(owner, nbytes: int, dev):
    """owner._ws: a uint8 tensor of at least nbytes on `dev`; a smaller one is released before the larger one is allocated.
    Under poison (lass_amd._alloc) a cached one is filled again, on the current stream of `dev`."""
    import torch

    from . import _alloc

    if owner._ws is None or owner._ws.device != dev or owner._ws.numel() < nbytes:
        owner._ws = None
        owner._ws = _alloc.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        _alloc.refill(owner._ws)
    return owner._ws
