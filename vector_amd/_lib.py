"""ctypes binding of libvsig.so (include/vsig.h) and per-device contexts.

The product path has no CPU fallback: if the library is missing or no HIP
device is present, every compute call raises ``VsigUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np
import torch  # loaded first: libvsig.so then binds torch's HIP runtime (same soname)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvsig.so")

VSIG_OK = 0
MODES = {"valid": 0, "full": 1, "same": 2}
DTYPES = {"c128": 0, "c64": 1, "f64": 2, "f32": 3}
# the element types the |a| kernels take -> their name in DTYPES
TORCH_CODES = {torch.complex128: "c128", torch.complex64: "c64", torch.float64: "f64", torch.float32: "f32"}
NP_CODES = {np.dtype(np.complex128): "c128", np.dtype(np.complex64): "c64", np.dtype(np.float64): "f64",
            np.dtype(np.float32): "f32"}


def upload_native(x, ctx):
    """(contiguous CUDA tensor, dtype name) of a numpy array or a tensor of any
    shape: the four dtypes of DTYPES are kept, anything else is widened to
    float64 / complex128 (as numpy's promotion would for np.abs)."""
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.to(f"cuda:{ctx.device}")
        if t.dtype not in TORCH_CODES:
            t = t.to(torch.complex128 if t.is_complex() else torch.float64)
    else:
        a = np.asarray(x)
        if a.dtype not in NP_CODES:
            a = a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{ctx.device}")
    t = t.contiguous()
    return t, TORCH_CODES[t.dtype]


class VsigUnavailable(RuntimeError):
    """libvsig.so is not built or no HIP device is visible."""


class VsigError(RuntimeError):
    pass


class VsigInvalid(VsigError, ValueError):
    """VSIG_E_INVALID: the library refused an argument before enqueuing any
    work (a ValueError, as numpy raises for a bad argument)."""


class RefineFault(VsigError):
    """The exact-argmax refine faulted on the device (its watchdog fired,
    vsig.h VSIG_E_REFINE / refine status 3): the peak record is invalid.
    Raised, never warned: the lag / |c| contract is numpy's exact answer."""


class Peak(C.Structure):
    _fields_ = [("peak", C.c_double), ("index", C.c_int64),
                ("sum_abs", C.c_double), ("sum_abs2", C.c_double)]


P = C.c_void_p
I32, I64, F32 = C.c_int32, C.c_int64, C.c_float


class ChainConfig(C.Structure):
    """vsig_chain_config (include/vsig.h)."""
    _fields_ = [("n_local", I64), ("taps", P), ("ntaps", I32), ("decim", I32), ("nfft", I32),
                ("window", P), ("psd_scale", F32), ("tmpl", P), ("L", I64)]


SENDRECV = C.CFUNCTYPE(C.c_int, P, P, I64, I32, P, I64, I32, P)
ALLGATHER = C.CFUNCTYPE(C.c_int, P, P, P, I64, P)


class Transport(C.Structure):
    """vsig_transport (include/vsig.h)."""
    _fields_ = [("user", P), ("sendrecv", SENDRECV), ("allgather", ALLGATHER)]


class PacketPlace(C.Structure):
    """vsig_packet_place (include/vsig.h)."""
    _fields_ = [("y", P), ("len", I64), ("start", I64), ("period", I64), ("count", I64)]


class Instance(C.Structure):
    """vsig_instance_t (include/vsig.h)."""
    _fields_ = [("index", I64), ("value", C.c_double)]


class PeaksInfo(C.Structure):
    """vsig_peaks_info_t (include/vsig.h)."""
    _fields_ = [("count", I64), ("argmax", I64), ("max", C.c_double), ("thr_used", C.c_double)]


class Run(C.Structure):
    """vsig_run_t (include/vsig.h)."""
    _fields_ = [("start", I64), ("end", I64), ("argmax", I64), ("max", C.c_double), ("sum", C.c_double)]


class RunsInfo(C.Structure):
    """vsig_runs_info_t (include/vsig.h)."""
    _fields_ = [("count", I64), ("covered", I64), ("argmax", I64), ("max", C.c_double),
                ("thr_used", C.c_double)]


class TraceInfo(C.Structure):
    """vsig_trace_info_t (include/vsig.h)."""
    _fields_ = [("argmin", I64), ("argmax", I64), ("min", C.c_double), ("max", C.c_double)]


TRACE_ABS, TRACE_DB20 = 0, 1


class Segment(C.Structure):
    """vsig_segment_t (include/vsig.h)."""
    _fields_ = [("start", I64), ("len", I64)]


class Band(C.Structure):
    """vsig_band_t (include/vsig.h)."""
    _fields_ = [("power", C.c_double), ("centroid", C.c_double), ("peak", C.c_double),
                ("peak_bin", I32), ("lo_bin", I32), ("hi_bin", I32), ("flags", I32)]


class IsolateSeg(C.Structure):
    """vsig_isolate_seg_t (include/vsig.h)."""
    _fields_ = [("start", I64), ("len", I64), ("freq", C.c_double), ("filter", I32), ("pad", I32)]


class CombineMember(C.Structure):
    """vsig_combine_member_t (include/vsig.h)."""
    _fields_ = [("a_re", C.c_double), ("a_im", C.c_double), ("freq", C.c_double), ("m", C.c_double),
                ("rho", C.c_double), ("Ep", C.c_double), ("Ev", C.c_double), ("res", C.c_double),
                ("n", I64), ("used", I32), ("pad", I32)]


# the same record as a numpy dtype: a device buffer of K records read back in one copy
COMBINE_MEMBER = np.dtype([("a_re", "<f8"), ("a_im", "<f8"), ("freq", "<f8"), ("m", "<f8"), ("rho", "<f8"),
                           ("Ep", "<f8"), ("Ev", "<f8"), ("res", "<f8"), ("n", "<i8"), ("used", "<i4"),
                           ("pad", "<i4")])


# name -> (restype, argtypes); every symbol include/vsig.h declares.
SIGNATURES = {
    "vsig_version": (C.c_int, []),
    "vsig_build_id": (C.c_char_p, []),
    "vsig_refine_status": (C.c_int, [P, C.POINTER(I32), C.POINTER(I64)]),
    "vsig_errstr": (C.c_char_p, [C.c_int]),
    "vsig_init": (C.c_int, [C.c_int, C.POINTER(P)]),
    "vsig_free": (None, [P]),
    "vsig_last_error": (C.c_char_p, [P]),
    "vsig_set_stream": (C.c_int, [P, P]),
    "vsig_get_stream": (P, [P]),
    "vsig_copy_dev": (C.c_int, [P, P, P, I64]),
    "vsig_synchronize": (C.c_int, [P]),
    "vsig_set_option": (C.c_int, [P, C.c_char_p, C.c_int]),
    "vsig_get_option": (C.c_int, [P, C.c_char_p, C.POINTER(C.c_int)]),
    "vsig_timing_enable": (C.c_int, [P, C.c_int]),
    "vsig_timing_read": (C.c_int, [P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(I64)]),
    "vsig_timing_reset": (C.c_int, [P]),
    "vsig_clock_enable": (C.c_int, [P, C.c_int]),
    "vsig_refine_stream": (P, [P]),
    "vsig_refine_join": (C.c_int, [P]),
    "vsig_clock_read": (C.c_int, [P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(I64)]),
    "vsig_psd_c64_dev": (C.c_int, [P, P, I64, I64, P, I32, I64, I32, F32, I32, P, I64]),
    "vsig_psd_c64": (C.c_int, [P, P, I64, P, I32, I64, I32, F32, I32, P, I64]),
    "vsig_psd_traces_c64_dev": (C.c_int, [P, P, I64, I64, P, I32, I64, I32, F32, I32, I64, P, P, P]),
    "vsig_psd_traces_c64": (C.c_int, [P, P, I64, P, I32, I64, I32, F32, I32, I64, P, P, P]),
    "vsig_psd_traces_plan": (C.c_int, [I32, I64, C.POINTER(I64), C.POINTER(I64), C.POINTER(I64)]),
    "vsig_psd_segments_create": (C.c_int, [P, C.POINTER(Segment), I64, I64, I32, I64, I32, C.POINTER(P)]),
    "vsig_psd_segments_free": (None, [P]),
    "vsig_psd_segments_info": (C.c_int, [P, C.POINTER(I64), C.POINTER(I64), C.POINTER(I64), C.POINTER(I64)]),
    "vsig_psd_segments_run": (C.c_int, [P, P, P, F32, I32, P, P, P]),
    "vsig_band_measure_run": (C.c_int, [P, P, I64, I32, I64, C.c_double, P]),
    "vsig_isolate_create": (C.c_int, [P, C.POINTER(IsolateSeg), I64, I64, C.POINTER(F32), I32, I32, C.c_double,
                                      C.POINTER(P)]),
    "vsig_isolate_free": (None, [P]),
    "vsig_isolate_info": (C.c_int, [P, C.POINTER(I64), C.POINTER(I64), C.POINTER(I64), C.POINTER(I64)]),
    "vsig_isolate_offsets": (C.c_int, [P, C.POINTER(I64)]),
    "vsig_isolate_run": (C.c_int, [P, P, P]),
    "vsig_fir_create": (C.c_int, [P, P, I32, I32, C.POINTER(P)]),
    "vsig_fir_free": (None, [P]),
    "vsig_fir_exec_dev": (C.c_int, [P, P, I64, P, I64]),
    "vsig_fir_exec_hist_dev": (C.c_int, [P, P, I64, I64, P, I64]),
    "vsig_fir_c64": (C.c_int, [P, P, I64, P, I32, I32, P, I64]),
    "vsig_fir_block": (C.c_int, [P]),
    "vsig_fir_exec_mix_dev": (C.c_int, [P, P, I64, I64, P, I64, C.c_double, C.c_double, I64]),
    "vsig_xcorr_create": (C.c_int, [P, P, I64, C.POINTER(P)]),
    "vsig_xcorr_free": (None, [P]),
    "vsig_xcorr_exec_dev": (C.c_int, [P, P, I64, I32, P, P]),
    "vsig_xcorr_bank_create": (C.c_int, [P, P, I32, I64, C.POINTER(P)]),
    "vsig_xcorr_bank_create_dev": (C.c_int, [P, P, I32, I64, C.POINTER(P)]),
    "vsig_xcorr_bank_free": (None, [P]),
    "vsig_xcorr_bank_exec_dev": (C.c_int, [P, P, I64, I32, P, P]),
    "vsig_xcorr_bank_plan": (C.c_int, [P, I64, I32, C.POINTER(I32), C.POINTER(I64), C.POINTER(I64),
                                       C.POINTER(I64)]),
    "vsig_match_create": (C.c_int, [P, C.POINTER(I64), I32, C.POINTER(P)]),
    "vsig_match_free": (None, [P]),
    "vsig_match_info": (C.c_int, [P, C.POINTER(I32), C.POINTER(I64), C.POINTER(I64), C.POINTER(I64),
                                  C.POINTER(I64)]),
    "vsig_match_run": (C.c_int, [P, P, P, P, P]),
    "vsig_combine_create": (C.c_int, [P, C.POINTER(I64), C.POINTER(I32), C.POINTER(I64), I32, C.POINTER(I32), I32,
                                      C.POINTER(P)]),
    "vsig_combine_free": (None, [P]),
    "vsig_combine_info": (C.c_int, [P, C.POINTER(I64), C.POINTER(I32), C.POINTER(I64), C.POINTER(I64),
                                    C.POINTER(I64)]),
    "vsig_combine_offsets": (C.c_int, [P, C.POINTER(I64)]),
    "vsig_combine_estimate": (C.c_int, [P, P, P, P, C.c_double, P]),
    "vsig_combine_sum": (C.c_int, [P, P, P, P]),
    "vsig_correlate_dev": (C.c_int, [P, I32, P, I64, P, I64, I32, I32, P, P]),
    "vsig_correlate": (C.c_int, [P, I32, P, I64, P, I64, I32, I32, P, P]),
    "vsig_correlate_c64_dev": (C.c_int, [P, P, I64, P, I64, I32, P, P]),
    "vsig_correlate_c64": (C.c_int, [P, P, I64, P, I64, I32, P, P]),
    "vsig_dft_dev": (C.c_int, [P, I32, P, I64, I64, I32, I32, P]),
    "vsig_resample_dev": (C.c_int, [P, I32, P, I64, I64, I32, P]),
    "vsig_filter_channel_dev": (C.c_int, [P, I32, P, I64, C.c_double, C.c_double, C.c_double, P]),
    "vsig_peak_dev": (C.c_int, [P, I32, P, I64, P]),
    "vsig_peak": (C.c_int, [P, I32, P, I64, P]),
    "vsig_peaks_tile": (C.c_int, []),
    "vsig_peaks_dev": (C.c_int, [P, I32, P, I64, C.c_double, I32, I64, P, I64, P]),
    "vsig_peaks": (C.c_int, [P, I32, P, I64, C.c_double, I32, I64, P, I64, P]),
    "vsig_runs_tile": (C.c_int, []),
    "vsig_runs_dev": (C.c_int, [P, I32, P, I64, C.c_double, I32, I64, P, I64, P]),
    "vsig_runs": (C.c_int, [P, I32, P, I64, C.c_double, I32, I64, P, I64, P]),
    "vsig_abs_stats_dev": (C.c_int, [P, I32, P, I64, P]),
    "vsig_correlate_stats_dev": (C.c_int, [P, I32, P, I64, P, I64, I32, P]),
    "vsig_region_power_dev": (C.c_int, [P, P, P, I64, P]),
    "vsig_trace_envelope_dev": (C.c_int, [P, I32, P, I64, I32, I64, I64, I64, I32, C.c_double, P, P, P]),
    "vsig_mix_c64_dev": (C.c_int, [P, P, I64, C.c_double, C.c_double, I64, P]),
    "vsig_scale_c64_dev": (C.c_int, [P, P, I64, C.c_float, P]),
    "vsig_wv_quantize_dev": (C.c_int, [P, P, I64, C.c_float, P]),
    "vsig_planar_to_c64_dev": (C.c_int, [P, I32, P, P, I64, P]),
    "vsig_c64_to_planar_dev": (C.c_int, [P, P, I64, P, P]),
    "vsig_vector_build_dev": (C.c_int, [P, C.POINTER(PacketPlace), I32, P, I64, P]),
    "vsig_normalize_c64_dev": (C.c_int, [P, P, I64, P, P]),
    "vsig_pfb_c64_dev": (C.c_int, [P, P, I64, P, I32, I32, P, I64]),
    "vsig_pfb_plan": (C.c_int, [I32, I32, I64, C.POINTER(I64), C.POINTER(I64), C.POINTER(I64)]),
    "vsig_select_dev": (C.c_int, [P, I32, P, I64, C.POINTER(I64), I32, C.POINTER(C.c_double)]),
    "vsig_threshold_dev": (C.c_int, [P, I32, P, I64, C.c_double, C.POINTER(I64), C.POINTER(I64),
                                     C.POINTER(I64), C.POINTER(C.c_double)]),
    "vsig_boxcar_energy_dev": (C.c_int, [P, I32, P, I64, I64, P]),
    "vsig_db_dev": (C.c_int, [P, I32, P, I64, C.c_double, P]),
    "vsig_abs_c64_dev": (C.c_int, [P, I32, P, I64, P]),
    "vsig_abs_c128_dev": (C.c_int, [P, I32, P, I64, P]),
    "vsig_spectrogram_image_dev": (C.c_int, [P, I32, P, I64, I64, I32, I64, C.c_double, C.c_double,
                                             C.c_double, I32, I32, I32, I32, P, P]),
    "vsig_chain_create": (C.c_int, [P, C.POINTER(ChainConfig), I32, I32, C.POINTER(Transport),
                                    C.POINTER(P)]),
    "vsig_chain_free": (None, [P]),
    "vsig_chain_last_error": (C.c_char_p, [P]),
    "vsig_chain_input": (P, [P]),
    "vsig_chain_step": (C.c_int, [P]),
    "vsig_chain_result": (C.c_int, [P, C.POINTER(Peak), C.POINTER(I64)]),
    "vsig_chain_filtered": (P, [P, C.POINTER(I64)]),
    "vsig_chain_spectra": (P, [P, C.POINTER(I64)]),
    "vsig_rccl_available": (C.c_int, []),
    "vsig_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "vsig_rccl_comm_init": (C.c_int, [I32, I32, C.c_char_p, I32, C.POINTER(P)]),
    "vsig_rccl_comm_destroy": (C.c_int, [P]),
    "vsig_rccl_transport": (C.c_int, [P, C.POINTER(Transport)]),
    "vsig_loopback_create": (C.c_int, [I32, C.POINTER(P)]),
    "vsig_loopback_free": (None, [P]),
    "vsig_loopback_transport": (C.c_int, [P, I32, C.POINTER(Transport)]),
}

_lib = None
_lib_lock = threading.Lock()


def load_library(path: str | None = None):
    """Load libvsig.so and declare every entry point; no device needed.
    (VSIG_LIB selects an A/B build of the same sources, for the tuning tools.)
    The library's build id must equal the hash of the kernel sources next to
    it (vector_amd/csrc, include/vsig.h): a stale binary is refused."""
    global _lib
    path = path or os.environ.get("VSIG_LIB") or LIB_PATH
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise VsigUnavailable(
                f"{path} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950)")
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        from ._build import source_hash
        want, got = source_hash(), lib.vsig_build_id().decode()
        if want is not None and got != want:
            raise VsigUnavailable(f"{path} was built from other sources (build id {got}, sources "
                                  f"{want}): rebuild with `python -m vector_amd._build`")
        _lib = lib
        return lib


_warned_no_threadpoolctl = False
_blas_ctl = None            # threadpoolctl controller of numpy's OpenBLAS (found once)


def numpy_blas_threads() -> int:
    """The thread count of the OpenBLAS behind this process's numpy (its zdotu
    splits a complex128 dot of more than 10000 terms into that many chunks,
    which decides the rounding of np.correlate's long sums); read at every call
    (threadpool_limits / OPENBLAS_NUM_THREADS may change it) through a
    controller found once (threadpool_info() rescans every loaded library:
    ~5 ms a call; the controller's get_num_threads is one C call into
    OpenBLAS).  1 if unknown -- with a warning when threadpoolctl is missing:
    correlations with more than 10000 overlap terms then match numpy only if
    its OpenBLAS runs one thread."""
    global _warned_no_threadpoolctl, _blas_ctl
    if _blas_ctl is None:
        try:
            import numpy  # noqa: F401  (its OpenBLAS is loaded with it)
            from threadpoolctl import ThreadpoolController
        except ImportError:
            if not _warned_no_threadpoolctl:
                import warnings
                warnings.warn("threadpoolctl is not importable: numpy's OpenBLAS thread count is "
                              "taken as 1 for the exact argmax of correlations over 10000 terms",
                              RuntimeWarning, stacklevel=2)
                _warned_no_threadpoolctl = True
            return 1
        try:
            ctl = [lc for lc in ThreadpoolController().lib_controllers if lc.internal_api == "openblas"]
        except Exception:
            ctl = []
        _blas_ctl = ctl[0] if ctl else False
    if not _blas_ctl:
        return 1
    try:
        return max(1, min(1024, int(_blas_ctl.get_num_threads())))
    except Exception:
        return 1


class Context:
    """One vsig_ctx on one device (the library's stream state lives here)."""

    def __init__(self, device: int):
        lib = load_library()
        h = P()
        rc = lib.vsig_init(device, C.byref(h))
        if rc != VSIG_OK:
            raise VsigUnavailable(f"vsig_init(device={device}) failed: "
                                  f"{lib.vsig_errstr(rc).decode()}")
        self.lib, self.h, self.device = lib, h, device
        self.blas_threads = None
        self.sync_blas_threads()

    def sync_blas_threads(self):
        """The refine matches numpy's complex128 sums operation for operation;
        OpenBLAS splits those over 10000 terms across its threads: hand the
        library numpy's current thread count (called before each correlation)."""
        t = numpy_blas_threads()
        if t != self.blas_threads:
            self.check(self.lib.vsig_set_option(self.h, b"blas_threads", t), "blas_threads")
            self.blas_threads = t

    def check(self, rc: int, what: str):
        if rc != VSIG_OK:
            msg = self.lib.vsig_last_error(self.h).decode()
            err = self.lib.vsig_errstr(rc).decode()
            if rc == -1:
                raise VsigInvalid(f"{what}: {err}: {msg}")
            if rc == -4:
                raise NotImplementedError(f"{what}: {err}: {msg}")
            if rc == -6:
                raise RefineFault(f"{what}: {err}: {msg}")
            raise VsigError(f"{what}: {err}: {msg}")

    def bind_stream(self):
        """Enqueue on torch's current stream (so torch events time our kernels)."""
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.check(self.lib.vsig_set_stream(self.h, P(s)), "vsig_set_stream")

    def __del__(self):
        try:
            if self.h:
                self.lib.vsig_free(self.h)
                self.h = None
        except Exception:
            pass


_ctx_tls = threading.local()


def get_context(device: int | None = None) -> Context:
    """Per-thread, per-device context bound to torch's current stream."""
    if not torch.cuda.is_available():
        raise VsigUnavailable("vector_amd needs a HIP device (torch.cuda.is_available() is False); "
                              "there is no CPU fallback")
    if device is None:
        device = torch.cuda.current_device()
    cache = getattr(_ctx_tls, "ctx", None)
    if cache is None:
        cache = _ctx_tls.ctx = {}
    ctx = cache.get(device)
    if ctx is None:
        with torch.cuda.device(device):
            ctx = cache[device] = Context(device)
    ctx.bind_stream()
    return ctx
