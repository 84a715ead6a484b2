"""The line plots of the reference's figures on the GPU.

Every figure the reference draws is a spectrogram plus lines of two kinds:

  time-domain lines      np.abs(signal) over time
      plot_spectrogram's lower axis     utils.py:551-554
      plot_packet_with_markers          utils.py:853-856
      adjust_packet_start_gui           utils.py:939
      adjust_packet_bounds_gui          utils.py:1090
  whole-capture spectra  20 * log10(|np.fft.fft(data)|), or the magnitude itself
      vector_analyzer/spectrogram_analysis.py:9-30
      vector_analyzer/analyze_channels.py:6-25
      vector_analyzer/analyze_vectors.py:17-40   linear magnitude, band mask
      vector_analyzer/display_vectors.py:26-35   fftshifted
      vector_analyzer/mat_analyzer.py:202-215    DC removed, fftshifted, + 1e-12, minus the maximum

averaged_spectrum_trace is the spectrum line for captures of any length: a
detector (mean, max-hold, min-hold) over the frames of the block PSD
(dsp.averaged_spectrum), where capture_spectrum is one transform of the whole
capture and stops at 2^28 points.

signal_envelope and capture_spectrum produce those lines, reduced on the
device (trace.hip, vsig_trace_envelope_dev) to what an axis can show: with
max_points, a min / max envelope per pixel column instead of one value per
sample (the reference's own precedent, sig[::factor], throws samples away).
At bin == 1 the result is the reference's line itself.  Drawing stays with
the caller: ``fill_between(x, lo, hi, step="post")``, or ``plot(x, hi)`` when
bin == 1.  The phase trace np.angle(signal) (utils.py:559) is out of scope.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .dsp import _averaged_spectrum_dev, _check_detectors, _is_dev, _ptr

__all__ = ["Trace", "trace_bin", "trace_envelope", "time_axis", "spectrum_axis", "signal_envelope", "capture_spectrum",
           "averaged_spectrum_trace"]

Trace = namedtuple("Trace", "x lo hi bin argmax max")


def trace_bin(n, max_points):
    """Positions per column of a line of n points drawn with at most
    max_points columns: ceil(n / max_points); 1 for None."""
    if max_points is None:
        return 1
    max_points = int(max_points)
    if max_points < 1:
        raise ValueError("max_points must be at least 1")
    return max(1, -(-int(n) // max_points))


def _check_eps(eps):
    eps = float(eps)
    if not math.isfinite(eps) or eps < 0:
        raise ValueError(f"eps must be finite and not negative, got {eps}")
    return eps


def _one_dim(a, dev):
    if (a.dim() if dev else a.ndim) != 1:
        raise ValueError("vector_amd works on 1-D signals")


def _out_dtype(a, dev):
    """float32 for complex64 / float32 input, else float64."""
    if dev:
        return torch.float32 if a.dtype in (torch.complex64, torch.float32) else torch.float64
    return torch.float32 if a.dtype in (np.dtype(np.complex64), np.dtype(np.float32)) else torch.float64


def trace_envelope(t, *, shift=False, lo=0, hi=None, bin=1, db=False, eps=0.0, want_min=True, ctx=None):
    """vsig_trace_envelope_dev on a contiguous 1-D CUDA tensor of one of the
    four dtypes -> (env_min or None, env_max, info): the envelope tensors in
    the output dtype and a 4-element int64 tensor holding vsig_trace_info_t
    (argmin, argmax, then the bits of min and max).  Nothing synchronises."""
    n = t.numel()
    hi = n if hi is None else hi
    ctx = ctx or _lib.get_context(t.device.index)
    cols = max(0, -(-(hi - lo) // bin)) if bin >= 1 else 0
    real = torch.float32 if t.dtype in (torch.complex64, torch.float32) else torch.float64
    emax = torch.empty(cols, dtype=real, device=t.device)
    emin = torch.empty(cols, dtype=real, device=t.device) if want_min else None
    info = torch.empty(4, dtype=torch.int64, device=t.device)
    ctx.check(ctx.lib.vsig_trace_envelope_dev(
        ctx.h, _lib.DTYPES[_lib.TORCH_CODES[t.dtype]], _ptr(t), n, int(bool(shift)), lo, hi, bin,
        _lib.TRACE_DB20 if db else _lib.TRACE_ABS, float(eps), _ptr(emin) if want_min else None, _ptr(emax),
        _ptr(info)), "trace envelope")
    return emin, emax, info


def _read_info(info):
    """(argmin, argmax, min, max) of the info tensor (synchronises)."""
    h = info.cpu().numpy()
    v = h[2:].view(np.float64)
    return int(h[0]), int(h[1]), float(v[0]), float(v[1])


def _empty(dev_in, device, real, bin_):
    if dev_in:
        e = torch.empty(0, dtype=real, device=device)
    else:
        e = np.zeros(0, np.float32 if real == torch.float32 else np.float64)
    return Trace(np.zeros(0, np.float64), e, e, bin_, -1, float("nan"))


def _planes(emin, emax, dev_in):
    """(lo, hi) of a Trace: the same object when there is one plane."""
    hi = emax if dev_in else emax.cpu().numpy()
    if emin is None:
        return hi, hi
    return (emin if dev_in else emin.cpu().numpy()), hi


def signal_envelope(signal, sample_rate=None, *, start=0, stop=None, max_points=None, db=False, eps=0.0):
    """The time-domain line of the reference's figures, np.abs(signal)[start:stop]
    (with db: 20 * np.log10(that + eps)) -> Trace(x, lo, hi, bin, argmax, max).

    max_points: at most that many columns of bin = trace_bin(stop - start,
      max_points) samples each; lo / hi are the minimum / maximum of the line
      over each column (np.min / np.max: a NaN makes its column NaN).  With
      bin == 1 (max_points None or not below the length) ``lo is hi`` and it is
      the line itself.
    x: float64 numpy, the axis value of each column's first sample:
      (np.arange(n) / sample_rate)[start:stop:bin], or the sample indices when
      sample_rate is None (utils.py:551).
    argmax / max: the index in ``signal`` of the first maximum of the line over
      [start, stop) and the (mapped) value there, a Python float.
    start / stop follow slice rules.  signal: complex64 / complex128 / float32
      / float64 (others are widened to float64 / complex128); the envelope is
      float32 for the 32-bit dtypes, else float64.  numpy in -> numpy lo / hi;
      a CUDA tensor in -> tensors.  Empty input or an empty [start, stop)
      gives an empty Trace (argmax -1, max nan) and no device call."""
    dev_in = _is_dev(signal)
    if not dev_in:
        signal = np.asarray(signal)
    _one_dim(signal, dev_in)
    eps = _check_eps(eps)
    n = int(signal.shape[0])
    start, stop, _ = slice(start, stop).indices(n)
    bin_ = trace_bin(max(stop - start, 0), max_points)
    real = _out_dtype(signal, dev_in)
    if stop <= start:
        return _empty(dev_in, signal.device if dev_in else None, real, bin_)
    ctx = _lib.get_context(signal.device.index if dev_in and signal.is_cuda else None)
    t, _ = _lib.upload_native(signal[start:stop], ctx)
    emin, emax, info = trace_envelope(t, bin=bin_, db=db, eps=eps, want_min=bin_ > 1, ctx=ctx)
    _, argmax, _, mx = _read_info(info)
    x = time_axis(start, stop, bin_, sample_rate)
    lo, hi = _planes(emin, emax, dev_in)
    return Trace(x, lo, hi, bin_, start + argmax, mx)


def _freq_of(p, n, val, center_freq, shift):
    """np.fft.fftfreq(n, d)[...] + center_freq at positions p (an int or an
    int64 array) of the natural or fftshifted axis, formed as numpy forms it:
    the integer bin number times val = 1.0 / (n * d), then + center_freq."""
    if shift:
        k = p - n // 2
    elif isinstance(p, np.ndarray):
        k = np.where(p < (n + 1) // 2, p, p - n)
    else:
        k = p if p < (n + 1) // 2 else p - n
    if isinstance(k, np.ndarray):
        return k * val + center_freq
    return float(k) * val + center_freq


def time_axis(start, stop, bin_=1, sample_rate=None):
    """signal_envelope's x: (np.arange(n) / sample_rate)[start:stop:bin_], or
    the sample indices as float64 when sample_rate is None."""
    x = np.arange(start, stop, bin_)
    return x.astype(np.float64) if sample_rate is None else x / sample_rate


def spectrum_axis(n, sample_rate, center_freq=0.0, shift=True, lo=0, hi=None, bin_=1):
    """capture_spectrum's x: (np.fft.fftfreq(n, 1 / sample_rate) + center_freq,
    fftshifted with shift)[lo:hi:bin_], without forming the axis at length n."""
    hi = n if hi is None else hi
    val = 1.0 / (n * (1 / sample_rate))                  # np.fft.fftfreq's own expression
    return _freq_of(np.arange(lo, hi, bin_, dtype=np.int64), n, val, center_freq, shift)


def _band_window(n, val, center_freq, band):
    """[lo, hi) of the fftshifted positions with f_lo <= axis <= f_hi (the axis
    does not decrease with the position)."""
    f_lo, f_hi = band

    def first(pred):                  # the first position in [0, n] where pred holds (monotone)
        a, b = 0, n
        while a < b:
            m = (a + b) // 2
            if pred(_freq_of(m, n, val, center_freq, True)):
                b = m
            else:
                a = m + 1
        return a

    return first(lambda f: f >= f_lo), first(lambda f: f > f_hi)


def capture_spectrum(data, sample_rate, center_freq=0.0, *, scale="db", eps=0.0, shift=True, band=None,
                     normalize=False, remove_dc=False, max_points=None):
    """The whole-capture spectrum line of the reference's analysis scripts ->
    Trace(x, lo, hi, bin, argmax, max): one transform of the whole capture
    (vsig_dft_dev, any length, complex64 arithmetic; real input is widened to
    complex first), then the envelope kernel on the result.

    scale: "db" is 20 * np.log10(np.abs(X) + eps); "linear" is np.abs(X)
      (analyze_vectors.analyze_channel's return value).
    shift: np.fft.fftshift of the line and of the axis (display_vectors.py,
      mat_analyzer.py); False keeps the natural order of
      spectrogram_analysis.py and analyze_channels.py.
    x: float64 numpy, np.fft.fftfreq(n, 1 / sample_rate) + center_freq
      (fftshifted with shift) at each column's first position; never formed at
      length n.  spectrogram_analysis.py:13 multiplies its axis by sample_rate
      once more; that is not reproduced (it changes tick labels only).
    band: (f_lo, f_hi) keeps the positions with f_lo <= axis <= f_hi
      (analyze_vectors.py:28); needs shift=True, where they are contiguous.
      An empty band gives an empty Trace (argmax -1, max nan).
    normalize: subtracts the maximum of the whole spectrum (not only of the
      band) from lo and hi (mat_analyzer.py:215); dB only.  Trace.max is the
      normalised value.
    remove_dc: transforms data - data.mean() (mat_analyzer.py:203).  The
      de-interleave of a real I/Q array (mat_analyzer.py:206) stays with the
      caller.
    max_points: at most that many columns of bin = trace_bin(len, max_points)
      positions, lo / hi their minimum / maximum; bin == 1: ``lo is hi``, the
      line itself.
    argmax: the position (of the shifted line with shift) of the first maximum
      inside the band; max: the value there, a Python float.
    lo / hi are float64 for complex128 / float64 input -- the values of the
    complex64 transform, widened, as cross_correlate_signals does -- and
    float32 otherwise.  numpy in -> numpy out; a CUDA tensor in -> tensors.
    Empty input raises ValueError, as np.fft.fft does."""
    dev_in = _is_dev(data)
    if not dev_in:
        data = np.asarray(data)
    _one_dim(data, dev_in)
    if scale not in ("db", "linear"):
        raise ValueError(f"scale must be 'db' or 'linear', got {scale!r}")
    eps = _check_eps(eps)
    if normalize and scale != "db":
        raise ValueError("normalize applies to scale='db' only")
    if band is not None:
        if not shift:
            raise ValueError("band needs shift=True, where its positions are contiguous")
        f_lo, f_hi = (float(b) for b in band)
        if math.isnan(f_lo) or math.isnan(f_hi):
            raise ValueError("band edges must not be NaN")
        band = (f_lo, f_hi)
    n = int(data.shape[0])
    if n < 1:
        raise ValueError(f"Invalid number of FFT data points ({n}) specified.")
    sample_rate = float(sample_rate)
    if not (math.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError("sample_rate must be positive and finite")
    val = 1.0 / (n * (1 / sample_rate))                  # np.fft.fftfreq's own expression
    real = _out_dtype(data, dev_in)
    wide = real == torch.float64
    lo_p, hi_p = (0, n) if band is None else _band_window(n, val, center_freq, band)
    bin_ = trace_bin(max(hi_p - lo_p, 0), max_points)
    if hi_p <= lo_p:
        return _empty(dev_in, data.device if dev_in else None, real, bin_)

    ctx = _lib.get_context(data.device.index if dev_in and data.is_cuda else None)
    t, _ = _lib.upload_native(data, ctx)
    if remove_dc:
        t = t - t.mean()
    if not t.is_complex():
        t = t.to(torch.complex128 if t.dtype == torch.float64 else torch.complex64)
    X = torch.empty(n, dtype=torch.complex64, device=t.device)
    ctx.check(ctx.lib.vsig_dft_dev(ctx.h, _lib.DTYPES[_lib.TORCH_CODES[t.dtype]], _ptr(t), n, 1, 0, _lib.DTYPES["c64"],
                                   _ptr(X)), "dft")
    db = scale == "db"
    emin, emax, info = trace_envelope(X, shift=shift, lo=lo_p, hi=hi_p, bin=bin_, db=db, eps=eps,
                                      want_min=bin_ > 1, ctx=ctx)
    whole = None
    if normalize and band is not None:                   # the maximum of the whole spectrum
        whole = trace_envelope(X, shift=shift, bin=n, db=db, eps=eps, want_min=False, ctx=ctx)[2]
    _, argmax, _, mx = _read_info(info)
    if wide:
        emax = emax.to(torch.float64)
        emin = None if emin is None else emin.to(torch.float64)
    if normalize:                                        # in the output dtype
        top = mx if whole is None else _read_info(whole)[3]
        emax = emax - top
        emin = None if emin is None else emin - top
        mx = mx - top if wide else float(np.float32(mx) - np.float32(top))
    x = spectrum_axis(n, sample_rate, center_freq, shift, lo_p, hi_p, bin_)
    lo, hi = _planes(emin, emax, dev_in)
    return Trace(x, lo, hi, bin_, argmax, mx)


def averaged_spectrum_trace(data, sample_rate, center_freq=0.0, *, nfft=8192, window="hann", noverlap=0,
                            detector="mean", scale="db", eps=0.0, normalize=False, max_points=None):
    """The spectrum line of a capture of any length -> Trace(x, lo, hi, bin,
    argmax, max): one detector of ``averaged_spectrum(data, sample_rate,
    window, nperseg, noverlap, nfft, fftshift=True)`` -- the per-bin "mean",
    "max" (max-hold) or "min" (min-hold) power over the capture's frames --
    then the envelope kernel on that line.  The capture is read once and no
    scratch of its size is needed, unlike capture_spectrum's single transform.

    window: a name (frames of nfft samples, fewer for a shorter capture) or an
      array (its length is the frame length, at most nfft); noverlap as in
      spectrum().
    scale: "db" is 10 * np.log10(P + eps) (P is a power), mapped by
      vsig_db_dev on the envelope values: the map does not decrease, so the
      envelope of the mapped line is the mapped envelope; "linear" is P.
    normalize: subtracts the line's maximum from lo and hi; dB only.
    x: np.fft.fftshift(np.fft.fftfreq(nfft, 1 / sample_rate)) + center_freq at
      each column's first position (spectrum_axis).
    max_points: at most that many columns of bin = trace_bin(nfft, max_points)
      bins, lo / hi their minimum / maximum; bin == 1: ``lo is hi``.
    argmax: the position in the shifted line of the first maximum; max: the
      (mapped, normalised) value of its column in hi, a Python float.
    lo / hi are float64 for complex128 / float64 input, else float32; numpy in
    -> numpy out, a CUDA tensor in -> tensors.  Empty input raises ValueError."""
    dev_in = _is_dev(data)
    if not dev_in:
        data = np.asarray(data)
    _one_dim(data, dev_in)
    if scale not in ("db", "linear"):
        raise ValueError(f"scale must be 'db' or 'linear', got {scale!r}")
    eps = _check_eps(eps)
    if normalize and scale != "db":
        raise ValueError("normalize applies to scale='db' only")
    if not isinstance(detector, str):
        raise ValueError(f"detector must be one name, got {detector!r}")
    detector, = _check_detectors(detector)
    n = int(data.shape[0])
    if n < 1:
        raise ValueError("averaged_spectrum_trace needs at least one sample")
    sample_rate = float(sample_rate)
    if not (math.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError("sample_rate must be positive and finite")
    nfft = int(nfft)
    if nfft < 1:
        raise ValueError("nfft must be at least 1")
    bin_ = trace_bin(nfft, max_points)
    nperseg = nfft if isinstance(window, (str, tuple)) else None
    if dev_in and not data.is_cuda:
        data = data.to(f"cuda:{_lib.get_context().device}")
    out, nfft, _ = _averaged_spectrum_dev(data, window, nperseg, noverlap, nfft, True, (detector,), 1, None)
    line = out[("mean", "max", "min").index(detector)]
    ctx = _lib.get_context(line.device.index)
    emin, emax, info = trace_envelope(line, bin=bin_, want_min=bin_ > 1, ctx=ctx)
    if scale == "db":
        code = _lib.DTYPES[_lib.TORCH_CODES[line.dtype]]

        def db(t):
            o = torch.empty_like(t)
            ctx.check(ctx.lib.vsig_db_dev(ctx.h, code, _ptr(t), int(t.numel()), eps, _ptr(o)), "db")
            return o

        emax = db(emax)
        emin = None if emin is None else db(emin)
    _, argmax, _, _ = _read_info(info)
    if not 0 <= argmax < nfft:                           # a line of nothing but NaN has no maximum
        argmax = 0
    top = emax[argmax // bin_]
    if normalize:
        emax = emax - top
        emin = None if emin is None else emin - top
        top = emax[argmax // bin_]
    x = spectrum_axis(nfft, sample_rate, center_freq, True, 0, nfft, bin_)
    lo, hi = _planes(emin, emax, dev_in)
    return Trace(x, lo, hi, bin_, argmax, float(top))
