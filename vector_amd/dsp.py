"""Python front end of the hot path — the reference's call signatures, the
MI355X kernels underneath (libvsig.so through ctypes, no CPU fallback).

Reference functions mirrored (ramiyako/vector utils.py):
  create_spectrogram        utils.py:161-353  (parameter logic restated in spectrogram.py)
  cross_correlate_signals   utils.py:1258-1295
  find_correlation_peak     utils.py:1298-1342
  find_packet_location_in_vector  utils.py:1372-1434
and the north-star front-end names:
  spectrum(x, fs, window, nperseg, noverlap, nfft)  == scipy.signal.spectrogram as called
                                                       at utils.py:281-291
  filter(x, taps, decim)    == np.convolve(x, taps, 'full')[:len(x)][::decim]
  correlate(signal1, signal2, mode) == cross_correlate_signals
  correlate_peak(...)       == find_correlation_peak(*correlate(...)) fused on the GPU

Inputs may be numpy arrays (results come back as numpy, with the reference's
dtypes) or CUDA torch tensors (results stay on the device, fp32/complex64,
nothing is synchronised).  Every computation runs in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import warnings
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib
from .windows import get_window

__all__ = ["spectrum", "averaged_spectrum", "SpectrumTraces", "filter", "fir_filter", "correlate", "correlate_peak",
           "cross_correlate_signals", "find_correlation_peak",
           "find_packet_location_in_vector", "FirFilter", "Correlator", "peak_stats",
           "refine_status", "check_refine", "find_peaks", "find_packet_instances", "find_runs", "Runs",
           "CorrelatorBank", "FrequencySearch", "frequency_search", "find_packet_location_with_offset"]

PEAK_BYTES = 32  # sizeof(vsig_peak_t)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _is_dev(x) -> bool:
    return isinstance(x, torch.Tensor)


def _device_c64(x, ctx):
    """1-D complex64 contiguous CUDA tensor of x (host arrays are uploaded)."""
    if _is_dev(x):
        t = x
        if t.dim() != 1:
            raise ValueError("vector_amd works on 1-D signals")
        if not t.is_cuda:
            t = t.to(f"cuda:{ctx.device}")
        if t.dtype != torch.complex64:
            t = t.to(torch.complex64)
        return t.contiguous()
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError("vector_amd works on 1-D signals")
    a = np.ascontiguousarray(a, dtype=np.complex64)
    return torch.from_numpy(a).to(f"cuda:{ctx.device}")


def _ptr(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


def _check_dev(t: torch.Tensor, n: int, dtype, what: str, device=None):
    """Host-side shape check before a kernel writes / reads a caller buffer."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what}: expected a CUDA tensor")
    if t.dtype != dtype:
        raise ValueError(f"{what}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous")
    if t.numel() < n:
        raise ValueError(f"{what}: {t.numel()} elements, need {n}")
    if device is not None and t.device.index != device:
        raise ValueError(f"{what}: on {t.device}, expected cuda:{device}")


def _peak_buffer(ctx):
    return torch.empty(PEAK_BYTES // 8, dtype=torch.float64, device=f"cuda:{ctx.device}")


def _read_peak(buf: torch.Tensor):
    """(max, index, sum_abs, sum_abs2) from a device vsig_peak_t."""
    h = buf.cpu()
    raw = h.numpy()
    idx = int(h.view(torch.int64)[1].item())
    return float(raw[0]), idx, float(raw[2]), float(raw[3])


def _confidence_np(peak, mean, std, threshold_ratio):
    """find_correlation_peak's confidence (utils.py:1328-1340) from numpy's
    mean_corr / std_corr, with the reference's arithmetic."""
    if std > 0:
        conf = np.clip(((np.float64(peak) - mean) / std) / 10.0, 0.0, 1.0)
    else:
        conf = 0.0
    if peak < threshold_ratio * peak:   # utils.py:1339: peak == max(|c|)
        conf = 0.0
    return conf


# The fused correlators sum fp32 |c| values; their single-pass variance
# var = s2/n - mean^2 carries the sums' relative error e (~1e-7: fp32 FFT
# outputs, fp32 per-thread sums, double beyond) amplified by (s2/n) / var.
# Above _FUSED_VAR_FLOOR of the mean square the amplification is <= 20 and the
# std is within ~1e-6 of numpy's (confidence to the 1e-5 bar, tests); below it
# -- a flat |c| (a tone: std of rounding noise), or a tone under weak noise --
# the statistics are recomputed from numpy-order values
# (vsig_correlate_stats_dev: every output re-evaluated as np.correlate forms
# it, then numpy's two-pass mean / std).  Rayleigh-like |c| of noise sits at
# var / (s2/n) = 1 - pi/4 = 0.21 and keeps the fused sums.
_FUSED_VAR_FLOOR = 0.05


def _fused_stats(peak, s1, s2, n):
    """(mean, std, resolved) from the fused record's sums."""
    mean = s1 / n
    ms = s2 / n
    var = ms - mean * mean
    std = float(np.sqrt(var)) if var > 0 else 0.0
    return mean, std, var > _FUSED_VAR_FLOOR * ms


def _confidence(peak, s1, s2, n, threshold_ratio):
    """The confidence from a fused record's sums (single pass; see _FUSED_VAR_FLOOR)."""
    mean, std, _ = _fused_stats(peak, s1, s2, n)
    return _confidence_np(peak, mean, std, threshold_ratio)


def _abs_stats(t: torch.Tensor, code: str, ctx):
    """numpy's (np.mean, np.std) of |t| on the GPU (vsig_abs_stats_dev)."""
    out = torch.empty(2, dtype=torch.float64, device=t.device)
    ctx.check(ctx.lib.vsig_abs_stats_dev(ctx.h, _lib.DTYPES[code], _ptr(t), int(t.numel()), _ptr(out)),
              "abs stats")
    m, sd = out.cpu().tolist()
    return np.float64(m), np.float64(sd)


# ---------------------------------------------------------------------------
# spectrum — scipy.signal.spectrogram(..., return_onesided=False, detrend=False,
# scaling='spectrum') (utils.py:281-291)
# ---------------------------------------------------------------------------
def _triage(window, nperseg, n):
    """scipy.signal._spectral_py._triage_segments for a 1-D input of length n."""
    if isinstance(window, (str, tuple)):
        if nperseg is None:
            nperseg = 256
        if nperseg > n:
            warnings.warn(f"nperseg = {nperseg:d} is greater than input length  = {n:d}, "
                          f"using nperseg = {n:d}", stacklevel=3)
            nperseg = n
        win = get_window(window, nperseg)
    else:
        win = np.asarray(window)
        if win.ndim != 1:
            raise ValueError("window must be 1-D")
        if n < win.shape[-1]:
            raise ValueError("window is longer than input signal")
        if nperseg is None:
            nperseg = win.shape[0]
        elif nperseg != win.shape[0]:
            raise ValueError("value specified for nperseg is different from length of window")
    return win, int(nperseg)


def _out_real_dtype(x):
    dt = x.dtype if not _is_dev(x) else None
    if dt is None:
        return None
    return np.float64 if np.result_type(dt, np.complex64) == np.complex128 else np.float32


def spectrum(x, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, *,
             fftshift=False, _stride=1, _nsamples=None):
    """(f, t, Sxx) of ``scipy.signal.spectrogram(x, fs, window, nperseg, noverlap,
    nfft, detrend=False, return_onesided=False, scaling='spectrum')``.

    Sxx has shape (nfft, nframes) (a transposed view of the frame-major output
    the kernel writes, like scipy's own strided result).  fftshift=True
    returns Sxx already np.fft.fftshift-ed along frequency (f is not shifted).
    """
    if _is_dev(x):
        n = int(_nsamples if _nsamples is not None else x.shape[0])
    else:
        x = np.asarray(x)
        if x.ndim != 1:
            raise ValueError("vector_amd works on 1-D signals")
        n = x.shape[0]
    if n == 0:
        e = np.empty((0,))
        return e, e, e
    win, nperseg = _triage(window, nperseg, n)
    if nfft is None:
        nfft = nperseg
    elif nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    nfft = int(nfft)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    hop = nperseg - noverlap
    nframes = (n - nperseg) // hop + 1
    win32 = win.astype(np.float32)
    scale = float(1.0 / float(np.sum(win32, dtype=np.float64)) ** 2)

    ctx = _lib.get_context()
    dev = f"cuda:{ctx.device}"
    if _is_dev(x):
        xd = x if x.dtype == torch.complex64 else x.to(torch.complex64)
        if not xd.is_contiguous():
            xd = xd.contiguous()
    else:
        xd = _device_c64(x, ctx)
    wd = torch.from_numpy(win32).to(dev)
    out = torch.empty((nframes, nfft), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.vsig_psd_c64_dev(ctx.h, _ptr(xd), n, int(_stride), _ptr(wd), nperseg, hop,
                                       nfft, scale, 1 if fftshift else 0, _ptr(out), nframes),
              "spectrum")
    freqs = np.fft.fftfreq(nfft, 1 / fs)
    times = np.arange(nperseg / 2, n - nperseg / 2 + 1, hop) / float(fs)
    if _is_dev(x):
        return freqs, times, out.T
    S = out.cpu().numpy().T
    odt = _out_real_dtype(x)
    if odt == np.float64:
        S = S.astype(np.float64)
    return freqs, times, S


# ---------------------------------------------------------------------------
# averaged_spectrum — the mean / max-hold / min-hold of spectrum()'s Sxx over
# its frames, reduced inside the transform kernel (vsig_psd_traces_c64_dev)
# ---------------------------------------------------------------------------
SpectrumTraces = namedtuple("SpectrumTraces", "f mean max min nframes")

_DETECTORS = ("mean", "max", "min")


def _check_detectors(detectors):
    detectors = (detectors,) if isinstance(detectors, str) else tuple(detectors)
    for d in detectors:
        if d not in _DETECTORS:
            raise ValueError(f"unknown detector {d!r}: expected some of {_DETECTORS}")
    if not detectors:
        raise ValueError("no detector asked for")
    return detectors


def _averaged_spectrum_dev(x, window, nperseg, noverlap, nfft, fftshift, detectors, stride, nsamples):
    """averaged_spectrum's work: (mean, max, min) device tensors in the output
    dtype (None where not asked for), nfft and nframes; None for an empty
    input.  Every argument error is raised before the device is touched."""
    if _is_dev(x):
        if x.dim() != 1:
            raise ValueError("vector_amd works on 1-D signals")
        n = int(nsamples if nsamples is not None else x.shape[0])
    else:
        if x.ndim != 1:
            raise ValueError("vector_amd works on 1-D signals")
        n = x.shape[0]
    if n == 0:
        return None
    win, nperseg = _triage(window, nperseg, n)
    if nfft is None:
        nfft = nperseg
    elif nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    nfft = int(nfft)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    hop = nperseg - noverlap
    nframes = (n - nperseg) // hop + 1
    win32 = win.astype(np.float32)
    scale = float(1.0 / float(np.sum(win32, dtype=np.float64)) ** 2)

    ctx = _lib.get_context()
    dev = f"cuda:{ctx.device}"
    if _is_dev(x):
        xd = x if x.dtype == torch.complex64 else x.to(torch.complex64)
        if not xd.is_contiguous():
            xd = xd.contiguous()
        wide = x.dtype in (torch.complex128, torch.float64)
    else:
        xd = _device_c64(x, ctx)
        wide = _out_real_dtype(x) == np.float64
    wd = torch.from_numpy(win32).to(dev)
    mean = torch.empty(nfft, dtype=torch.float64, device=dev) if "mean" in detectors else None
    mx = torch.empty(nfft, dtype=torch.float32, device=dev) if "max" in detectors else None
    mn = torch.empty(nfft, dtype=torch.float32, device=dev) if "min" in detectors else None
    ctx.check(ctx.lib.vsig_psd_traces_c64_dev(
        ctx.h, _ptr(xd), n, int(stride), _ptr(wd), nperseg, hop, nfft, scale, 1 if fftshift else 0, nframes,
        _ptr(mean) if mean is not None else None, _ptr(mx) if mx is not None else None,
        _ptr(mn) if mn is not None else None), "averaged_spectrum")
    real = torch.float64 if wide else torch.float32
    return [None if t is None else t.to(real) for t in (mean, mx, mn)], nfft, nframes


def averaged_spectrum(x, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, *,
                      fftshift=False, detectors=("mean", "max", "min"), _stride=1, _nsamples=None):
    """Per-bin traces of ``spectrum(x, fs, window, nperseg, noverlap, nfft)``'s
    Sxx over its frames -> SpectrumTraces(f, mean, max, min, nframes), without
    the (nfft, nframes) array ever being stored:

      mean  ``Sxx.mean(axis=1)``: ``scipy.signal.welch(x, fs, window, nperseg,
            noverlap, nfft, detrend=False, return_onesided=False,
            scaling='spectrum', average='mean')[1]``; summed in double
      max   ``Sxx.max(axis=1)``   a spectrum analyser's max-hold
      min   ``Sxx.min(axis=1)``   its min-hold

    detectors: the traces to compute; the others are None.  A NaN in a frame
    makes that bin NaN in every trace, as numpy's reductions do.
    fftshift=True returns the traces np.fft.fftshift-ed (f is not shifted, as
    in spectrum()).  complex64 / float32 input gives float32 arrays (the
    double mean rounded once), inputs that promote to complex128 float64.
    numpy in -> numpy out; a CUDA tensor in -> device tensors, nothing
    synchronised.  Argument errors are spectrum()'s; an empty input returns
    empty arrays and nframes 0."""
    detectors = _check_detectors(detectors)
    dev_in = _is_dev(x)
    if not dev_in:
        x = np.asarray(x)
    r = _averaged_spectrum_dev(x, window, nperseg, noverlap, nfft, fftshift, detectors, _stride, _nsamples)
    if r is None:
        e = np.empty((0,))
        return SpectrumTraces(e, *(e if d in detectors else None for d in _DETECTORS), 0)
    out, nfft, nframes = r
    if not dev_in:
        out = [None if t is None else t.cpu().numpy() for t in out]
    return SpectrumTraces(np.fft.fftfreq(nfft, 1 / fs), *out, nframes)


# ---------------------------------------------------------------------------
# filter — np.convolve(x, taps, 'full')[:len(x)][::decim]
# ---------------------------------------------------------------------------
class FirFilter:
    """Causal FIR + decimation on the GPU: ``y = np.convolve(x, taps)[:len(x)][::decim]``
    (overlap-save; the filter spectrum is computed once at construction)."""

    def __init__(self, taps, decim: int = 1, device: int | None = None):
        taps = np.ascontiguousarray(np.asarray(taps).ravel(), dtype=np.complex64)
        if taps.size == 0:
            raise ValueError("v cannot be empty")
        if int(decim) < 1:
            raise ValueError("decim must be >= 1")
        self.ctx = _lib.get_context(device)
        self.ntaps, self.decim = int(taps.size), int(decim)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.vsig_fir_create(self.ctx.h, taps.ctypes.data_as(C.c_void_p),
                                                    self.ntaps, self.decim, C.byref(h)),
                       "vsig_fir_create")
        self.h = h

    def out_len(self, n: int) -> int:
        return (n + self.decim - 1) // self.decim

    def __call__(self, x: torch.Tensor, out: torch.Tensor | None = None,
                 nhist: int = 0, freq_shift: float = 0.0, sample_rate: float = 1.0,
                 i0: int = 0) -> torch.Tensor:
        """x: 1-D complex64 CUDA tensor -> complex64 CUDA tensor (async).
        The first nhist samples of x are history (a left halo): only the
        remaining samples produce outputs.  freq_shift != 0 filters
        apply_frequency_shift(x, freq_shift, sample_rate) instead (the NCO
        mixer fused into the filter's loads; x[0] is global sample i0)."""
        self.ctx.bind_stream()
        _check_dev(x, 1, torch.complex64, "filter input", self.ctx.device)
        n = int(x.shape[0]) - int(nhist)
        if n < 1 or nhist < 0:
            raise ValueError("filter: need len(x) > nhist >= 0")
        ny = self.out_len(n)
        if out is None:
            out = torch.empty(ny, dtype=torch.complex64, device=x.device)
        _check_dev(out, ny, torch.complex64, "filter output", self.ctx.device)
        if freq_shift and self.block != 1024:
            # long filters (M > 1024): the standalone mixer first, same phase origin
            xm = torch.empty_like(x)
            w = (2j * np.pi * freq_shift).imag
            self.ctx.check(self.ctx.lib.vsig_mix_c64_dev(self.ctx.h, _ptr(x), int(x.shape[0]),
                                                         float(w), float(sample_rate), int(i0),
                                                         _ptr(xm)), "mix")
            x, freq_shift = xm, 0.0
        if freq_shift:
            self.ctx.check(self.ctx.lib.vsig_fir_exec_mix_dev(
                self.h, _ptr(x), int(nhist), n, _ptr(out), ny, float(freq_shift),
                float(sample_rate), int(i0)), "filter (mixed)")
        else:
            self.ctx.check(self.ctx.lib.vsig_fir_exec_hist_dev(self.h, _ptr(x), int(nhist), n,
                                                               _ptr(out), ny), "filter")
        return out

    @property
    def block(self) -> int:
        """Overlap-save block size the library chose for these taps."""
        return int(self.ctx.lib.vsig_fir_block(self.h))

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.vsig_fir_free(self.h)
                self.h = None
        except Exception:
            pass


_fir_cache: "OrderedDict[tuple, FirFilter]" = OrderedDict()


def _cached_fir(taps_c64: np.ndarray, decim: int, device: int) -> FirFilter:
    key = (taps_c64.tobytes(), decim, device)
    f = _fir_cache.get(key)
    if f is None:
        f = FirFilter(taps_c64, decim, device)
        _fir_cache[key] = f
        if len(_fir_cache) > 16:
            _fir_cache.popitem(last=False)
    else:
        _fir_cache.move_to_end(key)
    return f


def fir_filter(x, taps, decim: int = 1, freq_shift: float = 0.0, sample_rate: float = 1.0):
    """Causal FIR then stride decimation: ``np.convolve(x, taps, 'full')[:len(x)][::decim]``
    (the reference's idioms, utils.py:802,816 and utils.py:194).  With
    ``freq_shift`` the input is first mixed as ``apply_frequency_shift(x,
    freq_shift, sample_rate)`` (utils.py:120-127) inside the same kernel."""
    if freq_shift and float(sample_rate) == 0.0:
        raise ZeroDivisionError("float division by zero")
    taps_np = np.asarray(taps)
    if taps_np.size == 0:
        raise ValueError("v cannot be empty")
    n = int(x.shape[0]) if _is_dev(x) else np.asarray(x).shape[0]
    if n == 0:
        raise ValueError("a cannot be empty")
    ctx = _lib.get_context()
    f = _cached_fir(np.ascontiguousarray(taps_np.ravel(), dtype=np.complex64), int(decim), ctx.device)
    xd = _device_c64(x, ctx)
    y = f(xd, freq_shift=freq_shift, sample_rate=sample_rate)
    if _is_dev(x):
        return y
    xa = np.asarray(x)
    odt = np.result_type(xa.dtype, taps_np.dtype)
    yh = y.cpu().numpy()
    if not np.issubdtype(odt, np.complexfloating):
        yh = yh.real
    return yh.astype(odt, copy=False)


filter = fir_filter  # noqa: A001  (north-star name)


# ---------------------------------------------------------------------------
# correlation
# ---------------------------------------------------------------------------
def _lags(mode, l1, l2):
    """utils.py:1288-1293 (incl. the 'same'-mode length quirk)."""
    if mode == "full":
        return np.arange(-l1 + 1, l2)
    if mode == "same":
        return np.arange(-l1 // 2, l1 // 2 + l1 % 2)
    return np.arange(l2 - l1 + 1)


def _corr_len(mode, na, nv):
    if mode == "full":
        return na + nv - 1
    if mode == "valid":
        return max(na, nv) - min(na, nv) + 1
    return max(na, nv)


def _check_mode(mode):
    if mode not in _lib.MODES:
        raise ValueError(f"mode must be one of 'full', 'valid', 'same' (got {mode!r})")


def _is_c128(x) -> bool:
    """Does the reference's complex128 upcast (utils.py:1279-1282) change x's
    values?  complex64 / float32 data upcast exactly (the complex64 path is
    then numpy's arithmetic on the same values); wider dtypes keep 128 bits."""
    if _is_dev(x):
        return x.dtype in (torch.complex128, torch.float64, torch.int64, torch.int32)
    dt = np.asarray(x).dtype
    return not (dt == np.complex64 or dt == np.float32 or dt == np.float16
                or dt == np.int8 or dt == np.uint8 or dt == np.int16 or dt == np.uint16)


def _device_c128(x, ctx):
    if _is_dev(x):
        t = x if x.is_cuda else x.to(f"cuda:{ctx.device}")
        return t.to(torch.complex128).contiguous()
    a = np.ascontiguousarray(np.asarray(x), dtype=np.complex128)
    if a.ndim != 1:
        raise ValueError("vector_amd works on 1-D signals")
    return torch.from_numpy(a).to(f"cuda:{ctx.device}")


def _correlate_dev(a, v, mode, want_array, ctx, out128=False):
    """np.correlate(a, v, mode) on the GPU; returns (c tensor or None, peak
    buffer, nout).  complex128 operands (or any input whose complex128 upcast
    is not exact) go to the library as complex128: the FFT pass runs in
    complex64, the argmax refine (refine.hip) in the operands' precision.
    out128: c is returned as complex128 with the refined outputs patched in."""
    in128 = _is_c128(a) or _is_c128(v)
    conv = _device_c128 if in128 else _device_c64
    ad, vd = conv(a, ctx), conv(v, ctx)
    ctx.sync_blas_threads()
    na, nv = int(ad.shape[0]), int(vd.shape[0])
    if na == 0:
        raise ValueError("a cannot be empty")
    if nv == 0:
        raise ValueError("v cannot be empty")
    nout = _corr_len(mode, na, nv)
    odt = torch.complex128 if out128 else torch.complex64
    c = torch.empty(nout, dtype=odt, device=ad.device) if want_array else None
    pk = _peak_buffer(ctx)
    ctx.check(ctx.lib.vsig_correlate_dev(ctx.h, _lib.DTYPES["c128" if in128 else "c64"], _ptr(ad),
                                         na, _ptr(vd), nv, _lib.MODES[mode],
                                         _lib.DTYPES["c128" if out128 else "c64"],
                                         _ptr(c) if c is not None else None, _ptr(pk)),
              "correlate")
    return c, pk, nout, (ad, vd, in128)


def refine_status(ctx=None):
    """(status, candidates) of the last correlation's argmax refine:
    0 refined, 1 skipped (more candidate outputs than a 'refine_cap' option
    set > 0; the default is no limit), 2 no refine pass ran, 3 the refine's
    watchdog fired since the last call (vsig.h vsig_refine_status; reported
    once, the refine's counters are cleared by the call)."""
    ctx = ctx or _lib.get_context()
    st, nc = C.c_int32(), C.c_int64()
    ctx.check(ctx.lib.vsig_refine_status(ctx.h, C.byref(st), C.byref(nc)), "refine_status")
    return int(st.value), int(nc.value)


def check_refine(ctx=None):
    """The exact-argmax contract after a correlation: status 3 (the refine's
    watchdog fired: a device fault) raises RefineFault; status 1 (an opt-in
    'refine_cap' exceeded) warns -- that limit is the caller's own choice.
    Device-tensor callers (Correlator, cross_correlate_signals on CUDA
    tensors) run asynchronously and call this themselves when they read the
    result (StreamChain.global_peak does)."""
    ctx = ctx or _lib.get_context()
    st, nc = refine_status(ctx)
    if st == 3:
        raise _lib.RefineFault("correlation argmax refine: watchdog fired (device fault); the "
                               "peak record is invalid (vsig_refine_status 3)")
    if st == 1:
        warnings.warn(f"correlation argmax left at fp32 accuracy: the {nc} candidate items within "
                      f"the refine band exceed the 'refine_cap' option", RuntimeWarning, stacklevel=3)


def cross_correlate_signals(signal1, signal2, mode="full"):
    """utils.py:1258-1295: ``np.correlate(signal2, signal1, mode)`` and the lag
    axis.  numpy inputs -> complex128 numpy: the FFT pass runs in complex64, the
    outputs within the refine band of the peak -- however many (a tone puts
    every full-overlap output there) -- are recomputed in numpy's own
    operation order, so find_correlation_peak over the result gives numpy's
    argmax and |c| to the bit; elsewhere complex64 accuracy.  A 'refine_cap'
    option > 0 (an explicit opt-in; default none) leaves a larger band at
    fp32 accuracy with a RuntimeWarning (refine_status)."""
    _check_mode(mode)
    ctx = _lib.get_context()
    dev = _is_dev(signal1) or _is_dev(signal2)
    out128 = (not dev) or _is_c128(signal1) or _is_c128(signal2)
    c, _, _, _ = _correlate_dev(signal2, signal1, mode, True, ctx, out128=out128)
    l1 = int(signal1.shape[0]) if _is_dev(signal1) else len(signal1)
    l2 = int(signal2.shape[0]) if _is_dev(signal2) else len(signal2)
    lags = _lags(mode, l1, l2)
    if dev:
        return c, lags
    out = c.cpu().numpy()
    check_refine(ctx)
    return out, lags


correlate = cross_correlate_signals


def peak_stats(a):
    """(argmax of |a| (first), max |a|, sum |a|, sum |a|^2, n) in double
    precision on the GPU, for numpy or CUDA arrays of complex/real dtype."""
    ctx = _lib.get_context()
    t, code = _lib.upload_native(a, ctx)
    n = int(t.numel())
    if n == 0:
        raise ValueError("attempt to get argmax of an empty sequence")
    pk = _peak_buffer(ctx)
    ctx.check(ctx.lib.vsig_peak_dev(ctx.h, _lib.DTYPES[code], _ptr(t), n, _ptr(pk)), "peak")
    mx, idx, s1, s2 = _read_peak(pk)
    return idx, mx, s1, s2, n


def find_correlation_peak(correlation, lags, threshold_ratio=0.5):
    """utils.py:1298-1342 — (lags[argmax |c|], max |c|, confidence).
    complex128 / float64 arrays (cross_correlate_signals' output): mean and std
    of |c| exactly as numpy forms them (its pairwise sums, two passes); other
    dtypes: from double sums of |c| (single pass)."""
    ctx = _lib.get_context()
    t, code = _lib.upload_native(correlation, ctx)
    n = int(t.numel())
    if n == 0:
        raise ValueError("attempt to get argmax of an empty sequence")
    pk = _peak_buffer(ctx)
    ctx.check(ctx.lib.vsig_peak_dev(ctx.h, _lib.DTYPES[code], _ptr(t), n, _ptr(pk)), "peak")
    peak, idx, s1, s2 = _read_peak(pk)
    if code in ("c128", "f64"):
        mean, std = _abs_stats(t, code, ctx)
    else:
        mean, std, _ = _fused_stats(peak, s1, s2, n)
    return lags[idx], np.float64(peak), _confidence_np(peak, mean, std, threshold_ratio)


def correlate_peak(signal1, signal2, mode="full", threshold_ratio=0.5):
    """``find_correlation_peak(*cross_correlate_signals(signal1, signal2, mode))``
    fused: the correlation is reduced inside the kernel and never stored."""
    _check_mode(mode)
    ctx = _lib.get_context()
    _, pk, nout, (ad, vd, in128) = _correlate_dev(signal2, signal1, mode, False, ctx)
    peak, idx, s1, s2 = _read_peak(pk)
    check_refine(ctx)
    mean, std, resolved = _fused_stats(peak, s1, s2, nout)
    if not resolved:
        # a (nearly) flat |c|: numpy's std is decided by rounding; every
        # output's |c| in numpy's order, then numpy's two-pass statistics
        st = torch.empty(2, dtype=torch.float64, device=ad.device)
        ctx.check(ctx.lib.vsig_correlate_stats_dev(
            ctx.h, _lib.DTYPES["c128" if in128 else "c64"], _ptr(ad), int(ad.shape[0]), _ptr(vd),
            int(vd.shape[0]), _lib.MODES[mode], _ptr(st)), "correlate stats")
        mean, std = (np.float64(x) for x in st.cpu().tolist())
    conf = _confidence_np(peak, mean, std, threshold_ratio)
    l1 = int(signal1.shape[0]) if _is_dev(signal1) else len(signal1)
    l2 = int(signal2.shape[0]) if _is_dev(signal2) else len(signal2)
    if mode == "full":
        lag = np.int64(idx - (l1 - 1))
    elif mode == "valid":
        if idx >= l2 - l1 + 1:          # lag axis np.arange(l2 - l1 + 1) (utils.py:1291)
            raise IndexError(f"index {idx} is out of bounds for axis 0 with size "
                             f"{max(0, l2 - l1 + 1)}")
        lag = np.int64(idx)
    else:
        lag = _lags(mode, l1, l2)[idx]      # raises IndexError like the reference
    return lag, np.float64(peak), conf


class Correlator:
    """Streaming sync detector: a fixed template (any length; > 8192 samples
    runs as one pass per 8192-sample chunk), correlated against long
    device-resident streams with the |c| argmax fused in the kernel and
    refined (refine.hip) -- all asynchronous on the current stream."""

    def __init__(self, template, device: int | None = None):
        t = np.ascontiguousarray(np.asarray(template).ravel(), dtype=np.complex64)
        if t.size == 0:
            raise ValueError("v cannot be empty")
        self.ctx = _lib.get_context(device)
        self.L = int(t.size)
        self.h = None
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.vsig_xcorr_create(self.ctx.h, t.ctypes.data_as(C.c_void_p),
                                                      self.L, C.byref(h)), "vsig_xcorr_create")
        self.h = h

    def __call__(self, s: torch.Tensor, mode="valid", out: torch.Tensor | None = None,
                 peak: torch.Tensor | None = None):
        """Enqueue; returns (c or None, peak buffer (device vsig_peak_t)).  The
        refine matches numpy's current OpenBLAS thread count, as the numpy
        front end does (Context.sync_blas_threads: one C call)."""
        self.ctx.bind_stream()
        self.ctx.sync_blas_threads()
        _check_dev(s, 1, torch.complex64, "correlator stream", self.ctx.device)
        if mode not in ("valid", "full"):
            raise ValueError("Correlator supports mode 'valid' and 'full'")
        ns = int(s.shape[0])
        nout = ns - self.L + 1 if mode == "valid" else ns + self.L - 1
        if nout < 1:
            raise ValueError("stream shorter than the template")
        if out is not None:
            _check_dev(out, nout, torch.complex64, "correlator output", self.ctx.device)
        if peak is None:
            peak = _peak_buffer(self.ctx)
        _check_dev(peak, 4, torch.float64, "peak record", self.ctx.device)
        self.ctx.check(self.ctx.lib.vsig_xcorr_exec_dev(
            self.h, _ptr(s), ns, _lib.MODES[mode],
            _ptr(out) if out is not None else None, _ptr(peak)), "xcorr")
        return out, peak

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.vsig_xcorr_free(self.h)
                self.h = None
        except Exception:
            pass


# ---------------------------------------------------------------------------
# template bank — K templates against one stream in one pass; the carrier
# offset search built on it
# ---------------------------------------------------------------------------
BANK_MAX_TEMPLATES = 4096      # vsig_xcorr_bank_create: K and L limits
BANK_MAX_LENGTH = 4096


def _bank_templates(templates):
    """(rows, K, L, on_device) of a (K, L) template set, checked on the host."""
    if _is_dev(templates):
        t = templates
        shape, dev = tuple(t.shape), t.is_cuda
    else:
        t = np.asarray(templates)
        shape, dev = t.shape, False
    if len(shape) != 2:
        raise ValueError(f"CorrelatorBank: templates must be a (K, L) array, got shape {tuple(shape)}")
    K, L = int(shape[0]), int(shape[1])
    if K < 1 or L < 1:
        raise ValueError(f"CorrelatorBank: empty template set {tuple(shape)}")
    if K > BANK_MAX_TEMPLATES:
        raise ValueError(f"CorrelatorBank: {K} templates, at most {BANK_MAX_TEMPLATES}")
    if L > BANK_MAX_LENGTH:
        raise NotImplementedError(f"CorrelatorBank: templates of {L} samples, at most {BANK_MAX_LENGTH}")
    return t, K, L, dev


class CorrelatorBank:
    """K templates of one length L (K, L <= 4096) correlated against one
    device-resident stream in one pass: the stream's transform runs once per
    block and its spectrum meets the K template spectra in registers
    (vsig_xcorr_bank_*).  ``templates``: a (K, L) complex array-like, or a CUDA
    complex64 tensor (used where it is).  Record k is the unrefined fp32
    result: the first maximum of the fp32 |c_k|^2, its square root, and the
    sums of |c_k| and |c_k|^2 -- no exact re-rank runs on a bank."""

    def __init__(self, templates, device: int | None = None):
        t, self.K, self.L, dev = _bank_templates(templates)
        self.h = None
        self.ctx = _lib.get_context(device)
        h = C.c_void_p()
        lib = self.ctx.lib
        if dev:
            if t.device.index != self.ctx.device:
                raise ValueError(f"templates: on {t.device}, expected cuda:{self.ctx.device}")
            t = t.to(torch.complex64).contiguous()
            self.ctx.check(lib.vsig_xcorr_bank_create_dev(self.ctx.h, _ptr(t), self.K, self.L, C.byref(h)),
                           "vsig_xcorr_bank_create_dev")
        else:
            a = t.numpy() if _is_dev(t) else t
            a = np.ascontiguousarray(a, dtype=np.complex64)
            self.ctx.check(lib.vsig_xcorr_bank_create(self.ctx.h, a.ctypes.data_as(C.c_void_p), self.K,
                                                      self.L, C.byref(h)), "vsig_xcorr_bank_create")
        self.h = h

    def out_len(self, n: int, mode="valid") -> int:
        if mode not in ("valid", "full"):
            raise ValueError("CorrelatorBank supports mode 'valid' and 'full'")
        return n - self.L + 1 if mode == "valid" else n + self.L - 1

    def plan(self, n: int, mode="valid"):
        """(M, hop, nblocks, grid) of a call on n samples (vsig_xcorr_bank_plan)."""
        self.out_len(n, mode)
        M, hop, nb, grid = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vsig_xcorr_bank_plan(self.h, int(n), _lib.MODES[mode], C.byref(M),
                                                         C.byref(hop), C.byref(nb), C.byref(grid)),
                       "vsig_xcorr_bank_plan")
        return int(M.value), int(hop.value), int(nb.value), int(grid.value)

    def __call__(self, s: torch.Tensor, mode="valid", out: torch.Tensor | None = None,
                 peaks: torch.Tensor | None = None):
        """Enqueue; returns (out or None, peaks): out a (K, nout) complex64
        device tensor, peaks a (K, 4) float64 device tensor of K vsig_peak_t
        records (read_peaks)."""
        self.ctx.bind_stream()
        _check_dev(s, 1, torch.complex64, "correlator stream", self.ctx.device)
        if s.dim() != 1:
            raise ValueError("correlator stream: expected a 1-D tensor")
        ns = int(s.shape[0])
        nout = self.out_len(ns, mode)
        if nout < 1:
            raise ValueError("stream shorter than the templates")
        if out is not None:
            _check_dev(out, self.K * nout, torch.complex64, "correlator output", self.ctx.device)
        if peaks is None:
            peaks = torch.empty((self.K, PEAK_BYTES // 8), dtype=torch.float64, device=s.device)
        _check_dev(peaks, 4 * self.K, torch.float64, "peak records", self.ctx.device)
        self.ctx.check(self.ctx.lib.vsig_xcorr_bank_exec_dev(
            self.h, _ptr(s), ns, _lib.MODES[mode], _ptr(out) if out is not None else None,
            _ptr(peaks)), "xcorr bank")
        return out, peaks

    @staticmethod
    def read_peaks(peaks: torch.Tensor):
        """Host arrays (peak[K], index[K], sum_abs[K], sum_abs2[K]) of the records."""
        h = peaks.detach().cpu().contiguous().reshape(-1, PEAK_BYTES // 8)
        raw = h.numpy()
        idx = h.view(torch.int64).numpy()[:, 1].copy()
        return raw[:, 0].copy(), idx, raw[:, 2].copy(), raw[:, 3].copy()

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.vsig_xcorr_bank_free(self.h)
                self.h = None
        except Exception:
            pass


FrequencySearch = namedtuple("FrequencySearch", ["offset_hz", "lag", "peak", "confidence", "offsets",
                                                 "lags", "peaks", "confidences"])


def _search_grid(offsets, max_offset, step, sample_rate, Lt):
    """The hypotheses in Hz, checked on the host."""
    if (offsets is None) == (max_offset is None):
        raise ValueError("frequency_search: give exactly one of offsets and max_offset")
    if offsets is not None:
        if step is not None:
            raise ValueError("frequency_search: step goes with max_offset, not with offsets")
        grid = np.array(offsets, dtype=np.float64)
        if grid.ndim != 1:
            raise ValueError("frequency_search: offsets must be a 1-D array of Hz")
    else:
        max_offset = float(max_offset)
        if not np.isfinite(max_offset) or max_offset < 0:
            raise ValueError("frequency_search: max_offset must be finite and >= 0")
        step = sample_rate / (2.0 * Lt) if step is None else float(step)
        if not np.isfinite(step) or step <= 0:
            raise ValueError("frequency_search: step must be finite and > 0")
        m = int(np.ceil(max_offset / step))
        if 2 * m + 1 > BANK_MAX_TEMPLATES:
            raise ValueError(f"frequency_search: {2 * m + 1} hypotheses, at most {BANK_MAX_TEMPLATES} "
                             "(a coarser step, or several searches)")
        grid = np.arange(-m, m + 1) * step
    if grid.size == 0:
        raise ValueError("frequency_search: empty offset grid")
    if grid.size > BANK_MAX_TEMPLATES:
        raise ValueError(f"frequency_search: {grid.size} hypotheses, at most {BANK_MAX_TEMPLATES}")
    if not np.all(np.isfinite(grid)):
        raise ValueError("frequency_search: offsets must be finite")
    return grid


def _len1d(x, what):
    shape = tuple(x.shape) if _is_dev(x) else np.shape(x)
    if len(shape) != 1:
        raise ValueError(f"{what}: vector_amd works on 1-D signals")
    return int(shape[0])


def frequency_search(vector, reference, sample_rate, offsets=None, *, max_offset=None, step=None,
                     mode="valid", threshold_ratio=0.5, max_template=4096):
    """Where ``reference`` sits in ``vector`` and at which carrier offset:
    hypothesis k is ``apply_frequency_shift(reference[:Lt], offsets[k],
    sample_rate)`` (built on the device by the same mixer), all K correlated
    against the vector in one pass (CorrelatorBank), so a packet that
    build_vector placed with ``freq_shift = f`` is found at offset ``+f``.

    Give exactly one of ``offsets`` (1-D, Hz, finite, 1 .. 4096 entries) and
    ``max_offset``; with ``max_offset`` the grid is ``np.arange(-m, m + 1) *
    step``, ``m = ceil(max_offset / step)``, and ``step`` defaults to
    ``sample_rate / (2 * Lt)`` -- a worst-case mismatch of a quarter cycle over
    the template, which keeps sinc(1/4) = 0.90 of the peak.

    Only the first ``Lt = min(len(reference), max_template)`` samples of the
    reference are correlated (``max_template`` <= 4096, the bank's limit); the
    lag is still the start of the reference.  Returns a FrequencySearch:
    the winner (first maximum of ``peaks``) as ``offset_hz, lag, peak,
    confidence`` and every hypothesis as ``offsets, lags, peaks, confidences``.
    ``lag`` is correlate_peak(reference[:Lt], vector, mode)'s; ``confidence``
    is find_correlation_peak's z-score formula on the fused fp32 sums of each
    hypothesis.  The records are the bank's unrefined fp32 results; run
    correlate_peak on the vector mixed by ``-offset_hz`` for numpy's own
    (find_packet_location_with_offset does)."""
    if mode not in ("valid", "full"):
        raise ValueError("frequency_search supports mode 'valid' and 'full'")
    sample_rate = float(sample_rate)
    if not np.isfinite(sample_rate) or sample_rate <= 0:
        raise ValueError("frequency_search: sample_rate must be finite and > 0")
    max_template = int(max_template)
    if not 1 <= max_template <= BANK_MAX_LENGTH:
        raise ValueError(f"frequency_search: max_template must be in [1, {BANK_MAX_LENGTH}]")
    nref, nvec = _len1d(reference, "reference"), _len1d(vector, "vector")
    if nref < 1:
        raise ValueError("frequency_search: empty reference")
    Lt = min(nref, max_template)
    grid = _search_grid(offsets, max_offset, step, sample_rate, Lt)
    nout = nvec - Lt + 1 if mode == "valid" else nvec + Lt - 1
    if nvec < 1 or nout < 1:
        raise ValueError("frequency_search: vector shorter than the reference")
    ctx = _lib.get_context()
    ctx.bind_stream()
    ref = _device_c64(reference, ctx)[:Lt].contiguous()
    K = int(grid.size)
    rows = torch.empty((K, Lt), dtype=torch.complex64, device=ref.device)
    for k, f in enumerate(grid):
        if f == 0:                       # apply_frequency_shift returns the signal itself
            rows[k].copy_(ref)
            continue
        w = (2j * np.pi * f).imag        # the imaginary part numpy multiplies t by
        ctx.check(ctx.lib.vsig_mix_c64_dev(ctx.h, _ptr(ref), Lt, float(w), sample_rate, 0,
                                           C.c_void_p(rows[k].data_ptr())), "mix")
    bank = CorrelatorBank(rows, ctx.device)
    _, pk = bank(_device_c64(vector, ctx), mode)
    peaks, idx, s1, s2 = bank.read_peaks(pk)
    lags = idx - (Lt - 1) if mode == "full" else idx
    confs = np.empty(K, dtype=np.float64)
    for k in range(K):
        mean, std, _ = _fused_stats(peaks[k], s1[k], s2[k], nout)
        confs[k] = _confidence_np(peaks[k], mean, std, threshold_ratio)
    best = int(np.argmax(np.where(np.isnan(peaks), -np.inf, peaks)))
    return FrequencySearch(np.float64(grid[best]), np.int64(lags[best]), np.float64(peaks[best]),
                           np.float64(confs[best]), grid, lags.astype(np.int64), peaks, confs)


# ---------------------------------------------------------------------------
# peak list — every instance, where find_correlation_peak stops at one argmax
# ---------------------------------------------------------------------------
def _check_peaks_args(threshold, min_distance, max_peaks):
    if np.isnan(threshold):
        raise ValueError("threshold must not be NaN")
    if int(min_distance) < 0:
        raise ValueError("min_distance must be >= 0")
    if int(max_peaks) < 0:
        raise ValueError("max_peaks must be >= 0")


def _peaks_dev(t, code, threshold, min_distance, relative, max_peaks, ctx):
    """vsig_peaks_dev on a contiguous CUDA tensor: (indices int64[max_peaks],
    values float64[max_peaks], info int64[4]) on the device, nothing synchronised."""
    n = int(t.numel())
    if n == 0:
        raise ValueError("attempt to get argmax of an empty sequence")
    max_peaks = int(max_peaks)
    rec = torch.empty((max_peaks, 2), dtype=torch.int64, device=t.device)
    rec[:, 0] = -1
    rec[:, 1] = 0
    info = torch.empty(4, dtype=torch.int64, device=t.device)
    ctx.check(ctx.lib.vsig_peaks_dev(ctx.h, _lib.DTYPES[code], _ptr(t), n, float(threshold),
                                     1 if relative else 0, int(min_distance),
                                     _ptr(rec) if max_peaks else None, max_peaks, _ptr(info)), "peaks")
    return rec[:, 0].contiguous(), rec[:, 1].contiguous().view(torch.float64), info


def _trim_peaks(idx, val, info, max_peaks, what):
    """Host (indices, values) of a device peak list, cut at its count."""
    count = int(info[0].item())
    if count > max_peaks:
        warnings.warn(f"{what}: {count} instances, the first {max_peaks} are returned",
                      RuntimeWarning, stacklevel=3)
    k = min(count, int(max_peaks))
    return idx[:k].cpu().numpy(), val[:k].cpu().numpy()


def find_peaks(a, threshold, min_distance=0, relative=False, max_peaks=65536):
    """The peaks of ``m = |a|`` (complex or real, numpy's abs in a's precision):
    every index i with ``m[i] >= threshold`` that is the first maximum of m
    over ``[i - min_distance, i + min_distance]`` (clipped to the array), i.e.
    ``lo + np.argmax(m[lo:hi+1]) == i`` -- in ascending order, found on the GPU
    (vsig_peaks_dev).  relative=True: the threshold is ``threshold * max(m)``.

    This is a maximum filter, not the greedy selection of
    ``scipy.signal.find_peaks(distance=)``: a peak beaten by a higher
    neighbour within min_distance is dropped even if that neighbour is itself
    dropped.  Two peaks are more than min_distance apart; min_distance=0 keeps
    every element at or above the threshold; a flat array has the one peak 0;
    relative=True with threshold 1.0 returns np.argmax's index alone.  A NaN
    magnitude counts as -1: it is never a peak, never suppresses one and
    never becomes the maximum (unlike np.argmax, which takes the first NaN;
    an array of nothing but NaN has count 0, argmax 0 and max -1).

    numpy in -> ``(indices int64[k], values float64[k])``; with more than
    max_peaks peaks a RuntimeWarning and the first max_peaks.  CUDA tensor in
    -> ``(indices, values, info)`` device tensors, nothing synchronised:
    max_peaks entries each (-1 / 0 past the count), info = int64[4] holding
    vsig_peaks_info_t (count, argmax; max and thr_used as float64 bits:
    ``info.view(torch.float64)[2:]``)."""
    _check_peaks_args(threshold, min_distance, max_peaks)
    ctx = _lib.get_context()
    if _is_dev(a) and a.dim() != 1:
        raise ValueError("vector_amd works on 1-D signals")
    t, code = _lib.upload_native(a, ctx)
    idx, val, info = _peaks_dev(t, code, threshold, min_distance, relative, max_peaks, ctx)
    if _is_dev(a):
        return idx, val, info
    return _trim_peaks(idx, val, info, int(max_peaks), "find_peaks")


def find_packet_instances(vector, packet, threshold_ratio=0.5, min_distance=None,
                          max_instances=65536):
    """Where every instance of ``packet`` starts in ``vector``:
    ``c = np.correlate(vector, packet, 'valid')`` on the GPU, stored as
    complex64 (no argmax refine runs), then ``find_peaks(c, threshold_ratio,
    min_distance, relative=True)``.  A start is the index in ``vector`` of the
    packet's first sample; min_distance defaults to ``len(packet) // 2``.

    The values are |c| at complex64 accuracy (about 1e-5 relative of numpy's
    complex128 correlation).  The threshold is relative to the stored array's
    own maximum, so the call is self-consistent and does not depend on the
    exact-argmax refine of the other correlation front ends.

    numpy in -> ``(starts int64[k], values float64[k])`` (RuntimeWarning and
    the first max_instances when there are more); CUDA tensors in -> device
    tensors of max_instances entries, -1 / 0 past the count, nothing
    synchronised.  ValueError when the vector is shorter than the packet or
    either is empty."""
    nv = int(vector.shape[0]) if _is_dev(vector) else len(vector)
    npk = int(packet.shape[0]) if _is_dev(packet) else len(packet)
    if nv == 0:
        raise ValueError("a cannot be empty")
    if npk == 0:
        raise ValueError("v cannot be empty")
    if nv < npk:
        raise ValueError(f"vector ({nv} samples) shorter than the packet ({npk})")
    d = npk // 2 if min_distance is None else int(min_distance)
    _check_peaks_args(threshold_ratio, d, max_instances)
    ctx = _lib.get_context()
    vd, pd = _device_c64(vector, ctx), _device_c64(packet, ctx)
    nout = nv - npk + 1
    c = torch.empty(nout, dtype=torch.complex64, device=vd.device)
    # the entry point refines its peak record whether or not the caller takes
    # one; the stored array is all that is used here, so the refine is off
    # for this one call
    was = C.c_int()
    ctx.check(ctx.lib.vsig_get_option(ctx.h, b"refine", C.byref(was)), "refine option")
    ctx.check(ctx.lib.vsig_set_option(ctx.h, b"refine", 0), "refine option")
    try:
        ctx.check(ctx.lib.vsig_correlate_c64_dev(ctx.h, _ptr(vd), nv, _ptr(pd), npk,
                                                 _lib.MODES["valid"], _ptr(c), None), "correlate")
    finally:
        ctx.check(ctx.lib.vsig_set_option(ctx.h, b"refine", was.value), "refine option")
    idx, val, info = _peaks_dev(c, "c64", threshold_ratio, d, True, max_instances, ctx)
    if _is_dev(vector) or _is_dev(packet):
        return idx, val
    return _trim_peaks(idx, val, info, int(max_instances), "find_packet_instances")


# ---------------------------------------------------------------------------
# run list — every burst, where threshold_stats stops at the first and last index
# ---------------------------------------------------------------------------
Runs = namedtuple("Runs", ["start", "end", "argmax", "max", "mean"])
RUN_WORDS = C.sizeof(_lib.Run) // 8            # a record as int64 words: start, end, argmax, max, sum
MAX_RETRY_RUNS = 1 << 24                       # the largest exact count find_runs re-runs for


def _check_runs_args(threshold, max_gap, min_length, max_runs):
    if np.isnan(threshold):
        raise ValueError("threshold must not be NaN")
    if int(max_gap) < 0:
        raise ValueError("max_gap must be >= 0")
    if int(min_length) < 1:
        raise ValueError("min_length must be >= 1")
    if int(max_runs) < 0:
        raise ValueError("max_runs must be >= 0")


def _runs_dev(t, code, threshold, max_gap, relative, cap, ctx):
    """vsig_runs_dev on a contiguous CUDA tensor: (records int64[cap, 5], info
    int64[5]) on the device, nothing synchronised.  A record is vsig_run_t as
    int64 words (-1 / 0 past the count), info is vsig_runs_info_t."""
    cap = int(cap)
    rec = torch.empty((cap, RUN_WORDS), dtype=torch.int64, device=t.device)
    rec[:, :3] = -1
    rec[:, 3:] = 0
    info = torch.empty(RUN_WORDS, dtype=torch.int64, device=t.device)
    ctx.check(ctx.lib.vsig_runs_dev(ctx.h, _lib.DTYPES[code], _ptr(t), int(t.numel()), float(threshold),
                                    1 if relative else 0, int(max_gap), _ptr(rec) if cap else None, cap,
                                    _ptr(info)), "runs")
    return rec, info


def _runs_host(t, code, threshold, max_gap, relative, min_length, max_runs, ctx, what):
    """The run list of a device array on the host (Runs, info as a host int64
    tensor): one more call with cap = count when the list overflowed max_runs
    and the count allows it, then the min_length mask on the device."""
    max_runs = int(max_runs)
    rec, info = _runs_dev(t, code, threshold, max_gap, relative, max_runs, ctx)
    h = info.cpu()
    count = int(h[0])
    k = min(count, max_runs)
    if count > max_runs:
        if count <= MAX_RETRY_RUNS:
            rec, _ = _runs_dev(t, code, threshold, max_gap, relative, count, ctx)
            k = count
        else:
            warnings.warn(f"{what}: {count} runs, the first {max_runs} are returned",
                          RuntimeWarning, stacklevel=3)
    rec = rec[:k]
    if int(min_length) > 1:
        rec = rec[(rec[:, 1] - rec[:, 0] + 1) >= int(min_length)]
    r = rec.cpu().numpy().reshape(-1, RUN_WORDS)
    start, end = r[:, 0].copy(), r[:, 1].copy()
    mx = np.ascontiguousarray(r[:, 3]).view(np.float64)
    mean = np.ascontiguousarray(r[:, 4]).view(np.float64) / (end - start + 1)
    return Runs(start, end, r[:, 2].copy(), mx, mean), h


def find_runs(a, threshold, max_gap=0, min_length=1, relative=False, max_runs=65536):
    """The runs of ``m = |a| >= threshold`` (complex or real, numpy's abs in
    a's precision): every maximal interval ``[start, end]`` (end inclusive)
    whose ends are at or above the threshold and that holds no stretch of more
    than max_gap consecutive elements below it -- in ascending order, found on
    the GPU (vsig_runs_dev).  relative=True: the threshold is ``threshold *
    max(m)``.  In numpy::

        idx = np.flatnonzero(m >= thr)
        brk = np.flatnonzero(np.diff(idx) > max_gap + 1)
        start = idx[np.r_[0, brk + 1]]; end = idx[np.r_[brk, idx.size - 1]]

    max_gap=0 gives the plain runs of the mask; a max_gap of len(a) or more at
    most the one run (first, last).  min_length keeps the runs with
    ``end - start + 1 >= min_length`` (applied after the kernel).

    numpy in -> ``Runs(start, end, argmax, max, mean)`` arrays trimmed to the
    count: argmax / max the first maximum of m over the run (gaps included),
    mean its average.  With more than max_runs runs (counted before
    min_length) the call is repeated once with room for all of them when there
    are at most 2**24; beyond that a RuntimeWarning and the first max_runs.
    CUDA tensor in -> ``(records, info)`` device tensors, nothing
    synchronised and nothing retried: records int64[max_runs, 5] holding
    vsig_run_t (start, end, argmax; max and sum as float64 bits; -1 / 0 past
    the count), info int64[5] holding vsig_runs_info_t; min_length must be 1."""
    _check_runs_args(threshold, max_gap, min_length, max_runs)
    dev = _is_dev(a)
    if dev and a.dim() != 1:
        raise ValueError("vector_amd works on 1-D signals")
    if (int(a.numel()) if isinstance(a, torch.Tensor) else int(np.size(a))) == 0:
        raise ValueError("find_runs of an empty array")
    if dev and int(min_length) != 1:
        raise ValueError("min_length must be 1 for a CUDA tensor (the records stay on the device)")
    ctx = _lib.get_context()
    t, code = _lib.upload_native(a, ctx)
    t = t.reshape(-1)
    if dev:
        return _runs_dev(t, code, threshold, max_gap, relative, max_runs, ctx)
    return _runs_host(t, code, threshold, max_gap, relative, min_length, max_runs, ctx, "find_runs")[0]


def find_packet_location_in_vector(vector, packet_signal, reference_segment,
                                   search_window=None, correlation_threshold=0.5):
    """utils.py:1372-1434 with both correlations reduced on the GPU."""
    if search_window is None:
        s0, s1 = 0, len(vector)
    else:
        s0, s1 = search_window
        s0, s1 = max(0, s0), min(len(vector), s1)
    vlag, _, vconf = correlate_peak(reference_segment, vector[s0:s1], "full", correlation_threshold)
    plag, _, pconf = correlate_peak(reference_segment, packet_signal, "full", correlation_threshold)
    return s0 + vlag - plag, 0, min(vconf, pconf)


def find_packet_location_with_offset(vector, packet_signal, reference_segment, sample_rate, max_offset,
                                     step=None, search_window=None, correlation_threshold=0.5):
    """find_packet_location_in_vector for a vector whose carrier is off by an
    unknown offset of at most ``max_offset`` Hz (a reference cut from another
    capture): frequency_search of the reference over the search window, then
    the window mixed by ``-offset_hz`` once (apply_frequency_shift) and handed
    to find_packet_location_in_vector -- the location and confidence are that
    function's refined, numpy-exact ones.  Returns (vector_location,
    offset_hz, confidence)."""
    from .vectors import apply_frequency_shift
    n = _len1d(vector, "vector")
    if search_window is None:
        s0, s1 = 0, n
    else:
        s0, s1 = search_window
        s0, s1 = max(0, s0), min(n, s1)
    region = vector[s0:s1]
    fs = frequency_search(region, reference_segment, sample_rate, max_offset=max_offset, step=step,
                          mode="full", threshold_ratio=correlation_threshold)
    region = apply_frequency_shift(region, -float(fs.offset_hz), sample_rate)
    loc, _, conf = find_packet_location_in_vector(region, packet_signal, reference_segment, None,
                                                  correlation_threshold)
    return s0 + loc, fs.offset_hz, conf
