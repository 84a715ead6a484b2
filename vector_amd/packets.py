"""Per-burst spectra and measurements: at which frequency every packet of a
capture sits and how wide it is, in one pass over the bursts' frames.

  segment_spectra   averaged_spectrum's mean / max-hold / min-hold traces for
                    every segment of a burst list (vsig_psd_segments_run: one
                    launch over all frames of all segments)
  measure_packets   centre frequency, occupied bandwidth, peak and power of
                    every burst, from its averaged spectrum
                    (vsig_band_measure_run)

  isolate_packets   every burst taken out as a clean baseband packet: mixed
                    down by its centre and low-passed to its bandwidth, the
                    capture's own samples on both sides of the cut
                    (vsig_isolate_run: one launch over all bursts)

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

__all__ = ["SegmentSpectra", "PacketMeasurements", "segment_spectra", "measure_packets", "IsolatedPackets",
           "isolate_packets", "design_lowpass"]

SegmentSpectra = namedtuple("SegmentSpectra", "f mean max min nframes")
PacketMeasurements = namedtuple("PacketMeasurements",
                                "center_freq peak_freq f_lo f_hi bandwidth power nframes spectra")

IsolatedPackets = namedtuple("IsolatedPackets", "packets pre center_freq bandwidth cutoff")

ISOLATE_M = 1024                     # the overlap-save frame of vsig_isolate_run
ISOLATE_MAX_TAPS = 511
ISOLATE_MAX_FILTERS = 4096
HAMMING_TRANSITION = 3.3             # a Hamming design's transition width x ntaps / sample_rate
ISOLATE_SEG_DTYPE = np.dtype([("start", "i8"), ("len", "i8"), ("freq", "f8"), ("filter", "i4"), ("pad", "i4")])

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


# ---------------------------------------------------------------------------
# isolate_packets: per-burst mix-down and band filter (vsig_isolate_run)
# ---------------------------------------------------------------------------
IsolateFrames = namedtuple("IsolateFrames", "offsets hop seg x0 y0 keep")


def _check_ntaps(ntaps):
    ntaps = int(ntaps)
    if ntaps < 3 or ntaps % 2 == 0:
        raise ValueError("ntaps must be odd and >= 3")
    if ntaps > ISOLATE_MAX_TAPS:
        raise NotImplementedError(f"isolate_packets: ntaps {ntaps} is above {ISOLATE_MAX_TAPS}")
    return ntaps


def lowpass_cutoff(bandwidth, sample_rate, ntaps):
    """bandwidth / 2 + 1.65 * sample_rate / ntaps: half a Hamming design's
    transition width (3.3 / ntaps of the sample rate) above the occupied band's
    edge, so the passband edge -- not the -6 dB point -- sits on that edge."""
    return np.asarray(bandwidth, np.float64) / 2 + (HAMMING_TRANSITION / 2) * sample_rate / ntaps


def _lowpass_taps(cutoff, sample_rate, ntaps):
    """float64 Hamming windowed-sinc low-pass with its -6 dB point at cutoff,
    unit gain at 0 Hz (scipy.signal.firwin(ntaps, cutoff, fs=sample_rate));
    the unit impulse at (ntaps - 1) / 2 from cutoff >= sample_rate / 2 on."""
    d = (ntaps - 1) // 2
    if not cutoff < sample_rate / 2:
        h = np.zeros(ntaps, np.float64)
        h[d] = 1.0
        return h
    m = np.arange(ntaps, dtype=np.float64)
    c = 2.0 * cutoff / sample_rate
    h = c * np.sinc(c * (m - d)) * (0.54 - 0.46 * np.cos(2.0 * np.pi * m / (ntaps - 1)))
    return h / np.sum(h)


def design_lowpass(bandwidth, sample_rate, ntaps=255, dtype=np.float32):
    """The taps isolate_packets filters a burst of occupied ``bandwidth`` with:
    a Hamming windowed sinc of ``ntaps`` (odd) taps, cutoff lowpass_cutoff(...),
    designed in float64 and rounded once to ``dtype`` (float32: what the device
    gets).  Where the cutoff reaches sample_rate / 2 the filter is the unit
    impulse at (ntaps - 1) / 2.  Host only."""
    ntaps = _check_ntaps(ntaps)
    bandwidth, sample_rate = float(bandwidth), float(sample_rate)
    if not (sample_rate > 0 and np.isfinite(sample_rate)):
        raise ValueError("sample_rate must be finite and > 0")
    if not (bandwidth >= 0 and np.isfinite(bandwidth)):
        raise ValueError("bandwidth must be finite and >= 0")
    return _lowpass_taps(float(lowpass_cutoff(bandwidth, sample_rate, ntaps)), sample_rate, ntaps).astype(dtype)


def isolate_frames(starts, lengths, ntaps):
    """The frames vsig_isolate_create cuts the output ranges [starts[k],
    starts[k] + lengths[k]) into -> IsolateFrames(offsets, hop, seg, x0, y0,
    keep): offsets the K + 1 prefix sums of the packed output, hop = 1025 - ntaps
    outputs a frame at most; frame i belongs to segment seg[i], keeps keep[i]
    outputs at y0[i] ... of the packed output and reads the capture window
    [x0[i], x0[i] + 1024) (clipped to the capture).  Segment k's frames are
    consecutive, ceil(lengths[k] / hop) of them.  Host only."""
    ntaps = _check_ntaps(ntaps)
    starts, lengths = np.asarray(starts, np.int64), np.asarray(lengths, np.int64)
    lo = ntaps - 1
    hop, d = ISOLATE_M - lo, lo // 2
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    nf = -(-lengths // hop)
    seg = np.repeat(np.arange(starts.size, dtype=np.int64), nf)
    o = (np.arange(int(nf.sum()), dtype=np.int64) - np.repeat(np.cumsum(nf) - nf, nf)) * hop
    return IsolateFrames(offsets, hop, seg, starts[seg] + o + d - lo, offsets[seg] + o,
                         np.minimum(hop, lengths[seg] - o))


def isolate_table(lo, hi, freqs, bandwidths, sample_rate, center_freq, ntaps):
    """vsig_isolate_create's host operands for the output ranges [lo[k], hi[k])
    at absolute centres ``freqs`` with occupied ``bandwidths`` -> (table, taps,
    cutoff): a structured array of ISOLATE_SEG_DTYPE, the float32 (F, ntaps) tap
    rows -- one per distinct cutoff, the impulse among them where a cutoff
    reaches sample_rate / 2 -- and every burst's cutoff.  A burst whose centre or
    bandwidth is NaN is mixed by 0 Hz through the impulse: cutoff NaN.  Host only."""
    freqs, bandwidths = np.asarray(freqs, np.float64), np.asarray(bandwidths, np.float64)
    nan = np.isnan(freqs) | np.isnan(bandwidths)
    cutoff = np.where(nan, np.nan, lowpass_cutoff(np.where(nan, 0.0, bandwidths), sample_rate, ntaps))
    key = np.where(nan | (cutoff >= sample_rate / 2), np.inf, cutoff)
    uniq, inv = np.unique(key, return_inverse=True)
    if uniq.size > ISOLATE_MAX_FILTERS:
        raise NotImplementedError(f"isolate_packets: {uniq.size} distinct bandwidths (at most {ISOLATE_MAX_FILTERS} "
                                  "filters a call)")
    taps = np.stack([_lowpass_taps(float(fc), sample_rate, ntaps) for fc in uniq]).astype(np.float32) \
        if uniq.size else np.zeros((0, ntaps), np.float32)
    table = np.zeros(freqs.size, ISOLATE_SEG_DTYPE)
    table["start"], table["len"] = lo, np.asarray(hi, np.int64) - np.asarray(lo, np.int64)
    table["freq"] = np.where(nan, 0.0, freqs - center_freq)
    table["filter"] = inv.reshape(-1)
    return table, np.ascontiguousarray(taps), cutoff


def _per_burst(name, a, K, lo=None):
    a = np.asarray(a, np.float64)
    if a.ndim != 1 or a.size != K:
        raise ValueError(f"{name} must be 1-D with one entry per burst ({K})")
    if np.any(np.isinf(a)) or (lo is not None and np.any(a < lo)):
        raise ValueError(f"{name} must be finite" + ("" if lo is None else f" and >= {lo}") + " (NaN: the plain slice)")
    return a


def _isolate_dev(ctx, xd, n, table, taps, sample_rate):
    """The packed complex64 device output of one plan, one run."""
    plan = _lib.P()
    ctx.check(ctx.lib.vsig_isolate_create(ctx.h, table.ctypes.data_as(C.POINTER(_lib.IsolateSeg)), int(table.size), n,
                                          taps.ctypes.data_as(C.POINTER(C.c_float)), int(taps.shape[0]),
                                          int(taps.shape[1]), float(sample_rate), C.byref(plan)), "isolate_packets")
    try:
        y = torch.empty(int(table["len"].sum()), dtype=torch.complex64, device=xd.device)
        ctx.check(ctx.lib.vsig_isolate_run(plan, _ptr(xd), _ptr(y)), "isolate_packets")
    finally:
        ctx.lib.vsig_isolate_free(plan)            # waits for the run: the plan owns its tables
    return y


def isolate_packets(signal, packets, sample_rate, center_freq=0.0, *, measurements=None, freqs=None,
                    bandwidths=None, pre_samples=0, post_samples=0, ntaps=255):
    """Every burst of ``packets`` as a clean baseband packet ->
    IsolatedPackets(packets, pre, center_freq, bandwidth, cutoff).

    Burst k is ``signal[max(0, s - pre_samples):min(n, e + 1 + post_samples)]``
    (extract_packets' slice) of the capture mixed down by the burst's centre --
    apply_frequency_shift(signal, -(center_freq[k] - center_freq), sample_rate),
    phase origin at the capture's first sample -- and low-passed by
    design_lowpass(bandwidth[k], sample_rate, ntaps) with the filter's delay
    removed.  The filter runs over the capture, not the slice: a cut has no edge
    transient, zeros enter only beyond the capture's own ends, and an emitter
    on another carrier that shares the burst's time span is filtered out.  All
    bursts run in one launch (vsig_isolate_run).

      packets      1-D views into one packed buffer, one per burst
      pre          the lead-in actually applied (as extract_packets')
      center_freq  the absolute centre each burst was mixed down from
      bandwidth    the occupied bandwidth each filter was designed for
      cutoff       the filters' -6 dB points (design_lowpass); bursts of one
                   cutoff share a filter; >= sample_rate / 2: not filtered

    Centres and bandwidths are, in this order: ``freqs`` / ``bandwidths``
    (absolute Hz, one per burst), the fields of ``measurements`` (a
    PacketMeasurements of these bursts), measure_packets(signal, packets,
    sample_rate, center_freq).  A burst whose centre or bandwidth is NaN (too
    short to measure, an all-zero spectrum) is returned as the plain slice
    (mixed by 0 Hz, the impulse): its cutoff is NaN.
    packets: detect_packets' Packets, or a (starts, ends) pair with inclusive
    ends; bursts may overlap, repeat and come in any order.  complex64 only.
    numpy in -> numpy out; a CUDA tensor in -> device views.  No burst: empty
    lists, no launch.  Every argument error is raised before the device is
    touched."""
    starts, ends = (packets.starts, packets.ends) if hasattr(packets, "starts") else packets
    dev_in = _is_dev(signal)
    if not dev_in:
        signal = np.asarray(signal)
    n = _signal_length(signal)
    if signal.dtype != (torch.complex64 if dev_in else np.complex64):
        raise NotImplementedError("isolate_packets: complex64 signals only")
    if n < 1:
        raise ValueError("isolate_packets of an empty signal")
    starts, ends = _check_segments(n, starts, ends)
    K = int(starts.size)
    pre_samples, post_samples = int(pre_samples), int(post_samples)
    if pre_samples < 0 or post_samples < 0:
        raise ValueError("pre_samples and post_samples must be >= 0")
    ntaps = _check_ntaps(ntaps)
    sample_rate, center_freq = float(sample_rate), float(center_freq)
    if not (sample_rate > 0 and np.isfinite(sample_rate)):
        raise ValueError("sample_rate must be finite and > 0")
    if not np.isfinite(center_freq):
        raise ValueError("center_freq must be finite")
    if freqs is not None:
        freqs = _per_burst("freqs", freqs, K)
    if bandwidths is not None:
        bandwidths = _per_burst("bandwidths", bandwidths, K, 0)
    if measurements is not None:
        for name in ("center_freq", "bandwidth"):
            _per_burst(f"measurements.{name}", getattr(measurements, name), K)
    lo = np.maximum(0, starts - pre_samples)
    hi = np.minimum(n, ends + 1 + post_samples)
    if K == 0:
        z = np.zeros(0, np.float64)
        return IsolatedPackets([], starts - lo, z, z, z)
    if measurements is None and (freqs is None or bandwidths is None):
        measurements = measure_packets(signal, (starts, ends), sample_rate, center_freq)
    freqs = np.asarray(measurements.center_freq, np.float64) if freqs is None else freqs
    bandwidths = np.asarray(measurements.bandwidth, np.float64) if bandwidths is None else bandwidths
    table, taps, cutoff = isolate_table(lo, hi, freqs, bandwidths, sample_rate, center_freq, ntaps)
    ctx = _lib.get_context()
    y = _isolate_dev(ctx, _device_c64(signal, ctx), n, table, taps, sample_rate)
    if not dev_in:
        y = y.cpu().numpy()
    off = np.concatenate(([0], np.cumsum(table["len"])))
    return IsolatedPackets([y[int(off[k]):int(off[k + 1])] for k in range(K)], starts - lo, freqs, bandwidths, cutoff)
