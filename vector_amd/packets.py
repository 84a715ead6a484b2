"""Per-burst spectra and measurements: at which frequency every packet of a
capture sits and how wide it is, in one pass over the bursts' frames.

  segment_spectra   averaged_spectrum's mean / max-hold / min-hold traces for
                    every segment of a burst list (vsig_psd_segments_run: one
                    launch over all frames of all segments)
  measure_packets   centre frequency, occupied bandwidth, peak and power of
                    every burst, from its averaged spectrum
                    (vsig_band_measure_run)

The burst list is what detect_packets / find_runs return: starts and inclusive
ends, host arrays.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .dsp import _DETECTORS, _check_detectors, _device_c64, _is_dev, _out_real_dtype, _ptr
from .windows import get_window

__all__ = ["SegmentSpectra", "PacketMeasurements", "segment_spectra", "measure_packets"]

SegmentSpectra = namedtuple("SegmentSpectra", "f mean max min nframes")
PacketMeasurements = namedtuple("PacketMeasurements",
                                "center_freq peak_freq f_lo f_hi bandwidth power nframes spectra")

BAND_DTYPE = np.dtype([("power", "f8"), ("centroid", "f8"), ("peak", "f8"), ("peak_bin", "i4"),
                       ("lo_bin", "i4"), ("hi_bin", "i4"), ("flags", "i4")])
NFFT_MIN, NFFT_MAX = 64, 8192
MAX_SEGMENTS = 1 << 24


def default_nperseg(lengths):
    """The largest power of two in [64, 1024] not above the shortest segment
    (64 if every one is shorter, or there is none)."""
    shortest = int(np.min(lengths)) if len(lengths) else 0
    p = 64
    while p * 2 <= min(shortest, 1024):
        p *= 2
    return p


def segment_frames(lengths, nperseg, hop):
    """Frames of each segment: (len - nperseg) // hop + 1, 0 below nperseg."""
    lengths = np.asarray(lengths, np.int64)
    return np.where(lengths >= nperseg, (lengths - nperseg) // hop + 1, 0).astype(np.int64)


def _check_segments(n, starts, ends):
    starts, ends = np.asarray(starts), np.asarray(ends)
    if starts.ndim != 1 or ends.ndim != 1 or starts.shape != ends.shape:
        raise ValueError("starts and ends must be 1-D arrays of one length")
    for name, a in (("starts", starts), ("ends", ends)):
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"{name} must hold integers")
    starts, ends = starts.astype(np.int64), ends.astype(np.int64)
    if starts.size > MAX_SEGMENTS:
        raise ValueError(f"more than 2**24 segments ({starts.size})")
    bad = np.flatnonzero((starts < 0) | (ends < starts) | (ends >= n))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"segment {k} [{int(starts[k])}, {int(ends[k])}] is outside the signal "
                         f"(need 0 <= start <= end < {n})")
    return starts, ends


def _plan_args(n, starts, ends, window, nperseg, noverlap, nfft):
    """Everything segment_spectra checks, with no device:
    (starts, lengths, float32 window, nperseg, hop, nfft, nframes)."""
    if n < 1:
        raise ValueError("segment_spectra of an empty signal")
    starts, ends = _check_segments(n, starts, ends)
    lengths = ends - starts + 1
    if isinstance(window, (str, tuple)):
        nperseg = default_nperseg(lengths) if nperseg is None else int(nperseg)
        if nperseg < 1:
            raise ValueError("nperseg must be >= 1")
        win = get_window(window, nperseg)
    else:
        win = np.asarray(window)
        if win.ndim != 1 or win.size < 1:
            raise ValueError("window must be 1-D")
        if nperseg is None:
            nperseg = win.shape[0]
        elif int(nperseg) != win.shape[0]:
            raise ValueError("value specified for nperseg is different from length of window")
        nperseg = int(nperseg)
    nfft = nperseg if nfft is None else int(nfft)
    if nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    if nfft < NFFT_MIN or nfft > NFFT_MAX or nfft & (nfft - 1):
        raise NotImplementedError(f"segment_spectra: nfft {nfft} is not a power of two in [64, 8192]")
    noverlap = int(noverlap)
    if noverlap < 0 or noverlap >= nperseg:
        raise ValueError("noverlap must be in [0, nperseg).")
    hop = nperseg - noverlap
    return starts, lengths, win.astype(np.float32), nperseg, hop, nfft, segment_frames(lengths, nperseg, hop)


def _signal_length(signal):
    if _is_dev(signal):
        if signal.dim() != 1:
            raise ValueError("vector_amd works on 1-D signals")
        return int(signal.shape[0])
    if signal.ndim != 1:
        raise ValueError("vector_amd works on 1-D signals")
    return signal.shape[0]


def _segments_dev(ctx, xd, n, starts, lengths, win32, nperseg, hop, nfft, fftshift, detectors):
    """(mean float64, max, min float32) device tensors (K, nfft), None where
    not asked for: one plan, one run."""
    dev = f"cuda:{ctx.device}"
    K = int(starts.size)
    table = np.ascontiguousarray(np.stack([starts, lengths], axis=1), dtype=np.int64)
    scale = float(1.0 / float(np.sum(win32, dtype=np.float64)) ** 2)
    wd = torch.from_numpy(win32).to(dev)
    mean = torch.empty((K, nfft), dtype=torch.float64, device=dev) if "mean" in detectors else None
    mx = torch.empty((K, nfft), dtype=torch.float32, device=dev) if "max" in detectors else None
    mn = torch.empty((K, nfft), dtype=torch.float32, device=dev) if "min" in detectors else None
    if K == 0:                                     # nothing to measure: empty rows
        return mean, mx, mn
    plan = _lib.P()
    ctx.check(ctx.lib.vsig_psd_segments_create(ctx.h, table.ctypes.data_as(C.POINTER(_lib.Segment)), K, n, nperseg,
                                               hop, nfft, C.byref(plan)), "segment_spectra")
    try:
        ctx.check(ctx.lib.vsig_psd_segments_run(plan, _ptr(xd), _ptr(wd), scale, 1 if fftshift else 0,
                                                *(None if t is None else _ptr(t) for t in (mean, mx, mn))),
                  "segment_spectra")
    finally:
        ctx.lib.vsig_psd_segments_free(plan)       # waits for the run: the plan owns its scratch
    return mean, mx, mn


def _spectra(signal, starts, ends, fs, window, nperseg, noverlap, nfft, detectors, fftshift, mean64):
    detectors = _check_detectors(detectors)
    dev_in = _is_dev(signal)
    if not dev_in:
        signal = np.asarray(signal)
    n = _signal_length(signal)
    starts, lengths, win32, nperseg, hop, nfft, nframes = _plan_args(n, starts, ends, window, nperseg, noverlap,
                                                                     nfft)
    if not fs > 0:
        raise ValueError("fs must be > 0")
    f = np.fft.fftfreq(nfft, 1 / fs)
    if fftshift:
        f = np.fft.fftshift(f)
    ctx = _lib.get_context()
    if dev_in:
        wide = signal.dtype in (torch.complex128, torch.float64)
    else:
        wide = _out_real_dtype(signal) == np.float64
    xd = _device_c64(signal, ctx)
    mean, mx, mn = _segments_dev(ctx, xd, n, starts, lengths, win32, nperseg, hop, nfft, fftshift, detectors)
    real = torch.float64 if wide else torch.float32
    out = [None if t is None else t.to(real) for t in (mean, mx, mn)]
    if mean64:
        out[0] = mean
    if not dev_in:
        out = [None if t is None else t.cpu().numpy() for t in out]
    return SegmentSpectra(f, *out, nframes), mean, win32, nfft, ctx


def segment_spectra(signal, starts, ends, fs=1.0, *, window="hann", nperseg=None, noverlap=0, nfft=None,
                    detectors=("mean",), fftshift=True):
    """averaged_spectrum of every segment ``signal[starts[k]:ends[k] + 1]``
    (ends inclusive, as in Packets) -> SegmentSpectra(f, mean, max, min,
    nframes): arrays of shape (K, nfft), one row per segment, all segments'
    frames in one pass.

    Segments may touch, overlap, repeat and come in any order.  A segment
    shorter than nperseg has no frame: nframes 0 and a row of NaN.
    nperseg=None takes the largest power of two in [64, 1024] that is not above
    the shortest segment (64 if every segment is shorter); nfft=None takes
    nperseg; nfft must be a power of two in [64, 8192].  noverlap defaults to 0.
    detectors: the traces to compute; the others are None.  fftshift=True (the
    default) returns the rows with the bin index ascending in frequency;
    f is the frequency of every column either way.
    complex64 / float32 input gives float32 rows (the double mean rounded
    once), inputs that promote to complex128 float64 rows.  numpy in -> numpy
    out; a CUDA tensor in -> device tensors.  nframes is a host array.
    Every argument error is raised before the device is touched."""
    return _spectra(signal, starts, ends, fs, window, nperseg, noverlap, nfft, detectors, fftshift, False)[0]


def band_to_hz(bands, nframes, nfft, sample_rate, center_freq, win32):
    """PacketMeasurements' fields from vsig_band_t records of fftshift-ed mean
    rows (a structured array of BAND_DTYPE): a dict of host arrays."""
    df = sample_rate / nfft
    ok = bands["lo_bin"] >= 0
    nan = np.float64(np.nan)
    w = win32.astype(np.float64)
    gain = float(np.sum(w)) ** 2 / (nfft * float(np.sum(w * w)))
    lo, hi, pk = (bands[k].astype(np.float64) for k in ("lo_bin", "hi_bin", "peak_bin"))
    return dict(
        center_freq=np.where(ok, center_freq + (bands["centroid"] - nfft / 2) * df, nan),
        peak_freq=np.where(ok, center_freq + (pk - nfft / 2) * df, nan),
        f_lo=np.where(ok, center_freq + (lo - nfft / 2 - 0.5) * df, nan),
        f_hi=np.where(ok, center_freq + (hi - nfft / 2 + 0.5) * df, nan),
        bandwidth=np.where(ok, (hi - lo + 1) * df, nan),
        power=bands["power"] * gain,
        nframes=np.asarray(nframes, np.int64))


def _band_measure_dev(ctx, rows, tail):
    """vsig_band_t of every row of a 2-D float64 device tensor -> a host
    structured array of BAND_DTYPE."""
    K, nbins = int(rows.shape[0]), int(rows.shape[1])
    out = torch.empty(K * BAND_DTYPE.itemsize, dtype=torch.uint8, device=rows.device)
    ctx.check(ctx.lib.vsig_band_measure_run(ctx.h, _ptr(rows), K, nbins, int(rows.stride(0)), float(tail),
                                            _ptr(out)), "measure_packets")
    return out.cpu().numpy().view(BAND_DTYPE)


def measure_packets(signal, packets, sample_rate, center_freq=0.0, *, occupied=0.99, window="hann", nperseg=None,
                    noverlap=0, nfft=None, return_spectra=False):
    """Where every burst sits in frequency -> PacketMeasurements, one entry
    per burst in every field (host arrays):

      center_freq  the power-weighted mean frequency of the burst's averaged spectrum
      peak_freq    the frequency of its strongest bin
      f_lo, f_hi   the edges of the band that holds the fraction ``occupied`` of
                   the power, (1 - occupied) / 2 left out on either side
      bandwidth    f_hi - f_lo, a whole number of bins of sample_rate / nfft
      power        the mean |x|^2 of the burst's windowed frames (Parseval, corrected
                   by the window's noise bandwidth)
      nframes      frames averaged
      spectra      with return_spectra: the SegmentSpectra measured (fftshift-ed rows,
                   f in Hz around center_freq, the mean in float64), else None

    packets: detect_packets' Packets, or a (starts, ends) pair with inclusive
    ends.  window / nperseg / noverlap / nfft are segment_spectra's.  A burst
    shorter than nperseg has no frame and NaN in every float field; one whose
    spectrum is all zero has power 0 and NaN elsewhere."""
    starts, ends = (packets.starts, packets.ends) if hasattr(packets, "starts") else packets
    occupied = float(occupied)
    if not 0.0 < occupied < 1.0:
        raise ValueError("occupied must be inside (0, 1)")
    if not sample_rate > 0:
        raise ValueError("sample_rate must be > 0")
    tail = (1.0 - occupied) / 2.0
    detectors = _DETECTORS if return_spectra else ("mean",)
    sp, mean, win32, nfft, ctx = _spectra(signal, starts, ends, sample_rate, window, nperseg, noverlap, nfft,
                                          detectors, True, True)
    if mean.shape[0]:
        bands = _band_measure_dev(ctx, mean, tail)
    else:
        bands = np.zeros(0, BAND_DTYPE)
    spectra = sp._replace(f=sp.f + center_freq) if return_spectra else None
    return PacketMeasurements(spectra=spectra, **band_to_hz(bands, sp.nframes, nfft, sample_rate, center_freq, win32))
