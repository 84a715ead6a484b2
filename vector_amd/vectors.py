"""The data formats and element-wise steps either side of the chain
(SURVEY.md §8(f) f2-f4), with the bulk work on the GPU:

  apply_frequency_shift        utils.py:120-127            mix_c64 kernel
  transplant_packet_in_vector  utils.py:1437-1501          |x|^2 sums + scale_c64
  extract_reference_segment    utils.py:1345-1369          host (a slice)
  extract_packets              the bursts detect_packets lists, with margins
                                                           host (slices)
  measure_packet_timing        utils.py:827-846            find_packet_start
  validate_transplant_quality  utils.py:1504-1591          correlate_peak + region_power kernel
  transplant_and_validate      unified_gui.py:1087-1233    the four transplant steps in one call
  mat2wv / save_vector_wv      mat_to_wv_converter.py:7-64, utils.py:672-677
                                                           wv_quantize kernel
  load_packet / load_packet_info / save_vector
                               utils.py:48-105, 659-670    MAT v5 planes <-> complex64
                                                           (planar_to_c64 / c64_to_planar)
  vector_plan / build_vector   unified_gui.py:1692-1791, main.py:214-284
                                                           vector_build + normalize_c64
  compute_freq_ranges          utils.py:129-159            host

The MAT v5 container (128-byte header, tagged data elements) and the SMU-WV
text header are parsed / written on the host (O(1) work); sample planes move
as raw bytes and are converted on the device.  Reference semantics are kept:
the same dtypes, the same printed messages, the same error conditions.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import time
import zlib
from datetime import datetime
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .analysis import find_packet_start
from .dsp import (_device_c64, _is_dev, _ptr, correlate_peak, find_packet_instances,
                  find_packet_location_in_vector, peak_stats)

__all__ = ["apply_frequency_shift", "resample_signal", "transplant_packet_in_vector",
           "extract_reference_segment", "extract_packets", "measure_packet_timing",
           "validate_transplant_quality",
           "transplant_and_validate", "mat2wv", "save_vector_wv",
           "load_packet", "load_packet_info", "save_vector", "read_mat", "write_mat_vector",
           "VectorPlan", "vector_plan", "build_vector", "compute_freq_ranges",
           "validate_packet_timing", "verify_vector"]


def _as_out(t: torch.Tensor, like_dev: bool):
    return t if like_dev else t.cpu().numpy()


# ---------------------------------------------------------------------------
# apply_frequency_shift — utils.py:120-127
# ---------------------------------------------------------------------------
def apply_frequency_shift(signal, freq_shift, sample_rate, start_index: int = 0):
    """signal * exp(2j*pi*freq_shift*t), t = arange(n)/sample_rate, as complex64.
    The phase is formed in double precision exactly as numpy forms it
    (w = (2*pi)*f, theta = w * (i / sr)), reduced modulo 2*pi in double, and the
    rotation applied in fp32 (agrees with the reference to ~1e-7 relative).
    ``start_index`` offsets t (for time-chunk shards of one capture)."""
    if freq_shift == 0:
        return signal
    ctx = _lib.get_context()
    x = _device_c64(signal, ctx)
    n = int(x.shape[0])
    y = torch.empty_like(x)
    w = (2j * np.pi * freq_shift).imag          # the imaginary part numpy multiplies t by
    ctx.bind_stream()
    ctx.check(ctx.lib.vsig_mix_c64_dev(ctx.h, _ptr(x), n, float(w), float(sample_rate),
                                       int(start_index), _ptr(y)), "mix")
    return _as_out(y, _is_dev(signal))


# ---------------------------------------------------------------------------
# transplant_packet_in_vector — utils.py:1437-1501
# ---------------------------------------------------------------------------
def resample_signal(signal, orig_sr, target_sr):
    """utils.py:107-118: ``scipy.signal.resample(signal, int(len * ratio))`` as
    complex64 -- the spectrum of any length (Bluestein on the FFT engine,
    bigfft.hip), its bins copied into the new length with scipy's Nyquist
    rule, the inverse transform of any length.  Returns ``signal`` itself when
    the rates are equal, like the reference."""
    if orig_sr == target_sr:
        return signal
    dev = _is_dev(signal)
    n = int(signal.shape[0]) if dev else len(signal)
    num = int(n * (target_sr / orig_sr))
    if num < 1:
        raise ValueError(f"invalid number of data points ({num}) specified")
    ctx = _lib.get_context()
    if dev:
        real = not signal.is_complex()
        t = signal.to(torch.complex128 if signal.dtype in (torch.complex128, torch.float64)
                      else torch.complex64).contiguous()
    else:
        a = np.asarray(signal)
        real = not np.iscomplexobj(a)
        wide = a.dtype in (np.complex128, np.float64, np.longdouble, np.clongdouble) or \
            np.issubdtype(a.dtype, np.integer)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128 if wide else np.complex64)
                             ).to(f"cuda:{ctx.device}")
    code = "c128" if t.dtype == torch.complex128 else "c64"
    y = torch.empty(num, dtype=torch.complex64, device=t.device)
    ctx.check(ctx.lib.vsig_resample_dev(ctx.h, _lib.DTYPES[code], _ptr(t), n, num, 1 if real else 0,
                                        _ptr(y)), "resample")
    return y if dev else y.cpu().numpy()


def _mean_power(t: torch.Tensor) -> np.float32:
    """np.mean(np.abs(seg) ** 2) of a complex64 segment: sum in double on the
    GPU, rounded to the float32 numpy returns."""
    if t.numel() == 0:
        return np.float32(np.nan)
    _, _, _, s2, n = peak_stats(t)
    return np.float32(s2 / n)


def transplant_packet_in_vector(vector, packet_signal, vector_location, packet_location=0,
                                replace_length=None, normalize_power=True):
    """utils.py:1437-1501: a copy of ``vector`` with
    packet_signal[packet_location : +L] (power-normalised to the region it
    replaces when normalize_power) written at vector_location.  complex64
    vectors (the reference's load_packet dtype); numpy in -> numpy out."""
    ctx = _lib.get_context()
    dev_in = _is_dev(vector)
    if dev_in:
        if vector.dtype != torch.complex64:
            raise NotImplementedError("transplant_packet_in_vector: complex64 vectors only")
        v = vector.contiguous()
    else:
        va = np.asarray(vector)
        if va.dtype != np.complex64:
            raise NotImplementedError("transplant_packet_in_vector: complex64 vectors only")
        v = torch.from_numpy(np.ascontiguousarray(va)).to(f"cuda:{ctx.device}")
    p = _device_c64(packet_signal, ctx)
    new = v.clone()
    nv, npk = int(v.shape[0]), int(p.shape[0])
    if replace_length is None:
        replace_length = npk - packet_location
    vector_end = min(vector_location + replace_length, nv)
    actual_replace_length = vector_end - vector_location
    packet_end = min(packet_location + actual_replace_length, npk)
    actual_packet_length = packet_end - packet_location
    if 0 <= vector_location < nv and actual_packet_length > 0:
        seg = p[packet_location:packet_location + actual_packet_length]
        scale = None
        if normalize_power and actual_packet_length > 0:
            orig = v[vector_location:vector_location + actual_packet_length]
            original_power = _mean_power(orig)
            packet_power = _mean_power(seg)
            if packet_power > 0 and original_power > 0:
                scale = np.sqrt(original_power / packet_power)
                print(f"Power normalization applied: scale factor = {scale:.3f}")
            elif packet_power == 0:
                print("Warning: Packet has zero power - normalization skipped")
            elif original_power == 0:
                print("Warning: Original region has zero power - normalization skipped")
        dst = new[vector_location:vector_location + actual_packet_length]
        if not dst.is_contiguous() or not seg.is_contiguous():
            raise RuntimeError("internal: non-contiguous transplant views")
        ctx.bind_stream()
        ctx.check(ctx.lib.vsig_scale_c64_dev(ctx.h, _ptr(seg), int(actual_packet_length),
                                             float(scale) if scale is not None else 1.0, _ptr(dst)),
                  "scale")
    return _as_out(new, dev_in)


# ---------------------------------------------------------------------------
# the transplant workflow's other steps — utils.py:1345-1369, 827-846, 1504-1591
# ---------------------------------------------------------------------------
def extract_reference_segment(signal, start_sample, end_sample):
    """utils.py:1345-1369: signal[max(0, start_sample):min(len(signal),
    end_sample)] (a view; numpy arrays and device tensors alike), ValueError
    for an empty range.  Host only: no device, no library."""
    start_sample = max(0, start_sample)
    end_sample = min(len(signal), end_sample)
    if start_sample >= end_sample:
        raise ValueError("Invalid sample range: start_sample >= end_sample")
    return signal[start_sample:end_sample]


def extract_packets(signal, packets, pre_samples=0, post_samples=0):
    """The slices of ``signal`` that hold the bursts of ``packets``
    (detect_packets' result, or any sequence of inclusive ``(start, end)``
    pairs): ``[(signal[max(0, s - pre_samples):min(n, e + 1 + post_samples)],
    pre), ...]``, pre the lead-in actually applied (``pre_samples``, less
    where the signal starts first) -- the value load_packet_info /
    write_mat_vector carry beside a packet.  Views: numpy arrays and device
    tensors alike.  Host only: no device, no library.  ValueError for a
    negative margin or a burst that is not inside the signal."""
    pre_samples, post_samples = int(pre_samples), int(post_samples)
    if pre_samples < 0 or post_samples < 0:
        raise ValueError("pre_samples and post_samples must be >= 0")
    if hasattr(packets, "starts") and hasattr(packets, "ends"):
        pairs = zip(packets.starts, packets.ends)
    else:
        pairs = packets
    n = len(signal)
    out = []
    for s, e in pairs:
        s, e = int(s), int(e)
        if s < 0 or e >= n or s > e:
            raise ValueError(f"burst ({s}, {e}) is not inside the signal ({n} samples)")
        lo = max(0, s - pre_samples)
        out.append((signal[lo:min(n, e + 1 + post_samples)], s - lo))
    return out


def measure_packet_timing(signal, template=None):
    """utils.py:827-846: (pre_samples, post_samples, packet_start) around
    find_packet_start's packet_start; post_samples is 0 without a template."""
    packet_start = find_packet_start(signal, template)
    pre_samples = packet_start
    post_samples = len(signal) - packet_start - len(template) if template is not None else 0
    return pre_samples, post_samples, packet_start


def _region_c64(vector, lo, hi, ctx, what):
    """vector[lo:hi] (Python slicing) of a complex64 vector as a device tensor;
    a host vector uploads the region alone."""
    if _is_dev(vector):
        if vector.dtype != torch.complex64 or vector.dim() != 1:
            raise NotImplementedError(f"{what}: complex64 vectors only")
        t = vector[lo:hi]
        return (t if t.is_cuda else t.to(f"cuda:{ctx.device}")).contiguous()
    va = np.asarray(vector)
    if va.dtype != np.complex64 or va.ndim != 1:
        raise NotImplementedError(f"{what}: complex64 vectors only")
    return torch.from_numpy(np.ascontiguousarray(va[lo:hi])).to(f"cuda:{ctx.device}")


def _region_powers(a: torch.Tensor, b: torch.Tensor, ctx):
    """(mean |a|^2, mean |b|^2, mean |a - b|^2) of two complex64 regions as the
    float32 numpy's means return: one pass on the GPU (region.hip: numpy's
    float32 element values, summed in double), one copy of three doubles."""
    n = int(a.shape[0])
    sums = torch.empty(3, dtype=torch.float64, device=a.device)
    ctx.bind_stream()
    ctx.check(ctx.lib.vsig_region_power_dev(ctx.h, _ptr(a), _ptr(b), n, _ptr(sums)), "region power")
    return tuple(np.float32(s / n) for s in sums.cpu().tolist())


def validate_transplant_quality(original_vector, transplanted_vector, packet_signal,
                                vector_location, reference_segment, sample_rate):
    """utils.py:1504-1591: the same dict (keys, nested ``criteria``, thresholds
    0.3 / 0.01 / -30) scored on the GPU.  Both regions are
    ``vector[vector_location:transplant_end]`` as the reference slices them
    (a negative location follows Python slicing); the correlation with
    ``reference_segment`` is correlate_peak (never stored), the three mean
    powers come from one pass over both regions (vsig_region_power_dev), each
    rounded to the float32 numpy's mean returns, and the reference's
    expressions are evaluated on those scalars.  complex64 vectors, numpy
    arrays or device tensors (the same dict either way); ``packet_signal``
    counts for its length only.

    ValueError for an empty region -- the reference raises it through
    np.correlate when ``reference_segment`` is not empty and would go on to the
    mean of an empty slice (nan, with a warning) when it is; both raise here --
    and for regions of different lengths (numpy's broadcast error)."""
    ctx = _lib.get_context()
    what = "validate_transplant_quality"
    transplant_end = min(vector_location + len(packet_signal), len(transplanted_vector))
    transplant_length = transplant_end - vector_location
    lo, hi = int(vector_location), int(transplant_end)
    transplanted_region = _region_c64(transplanted_vector, lo, hi, ctx, what)
    original_region = _region_c64(original_vector, lo, hi, ctx, what)
    n = int(transplanted_region.shape[0])

    if len(reference_segment) > 0:
        _, ref_peak_val, ref_confidence = correlate_peak(reference_segment, transplanted_region)
    else:
        ref_confidence = 0.0
        ref_peak_val = 0.0
    if n == 0:
        raise ValueError(f"{what}: empty transplant region")
    if int(original_region.shape[0]) != n:
        raise ValueError(f"operands could not be broadcast together with shapes "
                         f"({int(original_region.shape[0])},) ({n},)")

    original_power, transplanted_power, noise_power = _region_powers(
        original_region, transplanted_region, ctx)
    power_ratio = transplanted_power / original_power if original_power > 0 else 0.0
    signal_power = transplanted_power
    snr_improvement = 10 * np.log10(signal_power / noise_power) if noise_power > 0 else np.inf

    time_precision_us = 1e6 / sample_rate
    confidence_threshold = 0.3
    power_ratio_threshold = 0.01
    min_snr_threshold = -30
    confidence_ok = ref_confidence > confidence_threshold
    power_ok = power_ratio > power_ratio_threshold
    snr_ok = snr_improvement > min_snr_threshold
    success = confidence_ok and power_ok and snr_ok
    return {
        'reference_correlation': ref_peak_val,
        'reference_confidence': ref_confidence,
        'power_ratio': power_ratio,
        'snr_improvement_db': snr_improvement,
        'transplant_length_samples': transplant_length,
        'transplant_length_us': transplant_length * 1e6 / sample_rate,
        'time_precision_us': time_precision_us,
        'vector_location': vector_location,
        'success': success,
        'criteria': {
            'confidence_ok': confidence_ok,
            'power_ok': power_ok,
            'snr_ok': snr_ok,
            'confidence_threshold': confidence_threshold,
            'power_ratio_threshold': power_ratio_threshold,
            'min_snr_threshold': min_snr_threshold,
        },
    }


def transplant_and_validate(vector, packet_signal, ref_start, ref_end, sample_rate,
                            search_window=None, correlation_threshold=0.5):
    """The transplant tab's sequence (unified_gui.py:1087-1233) in one call:
    extract_reference_segment(packet_signal, ref_start, ref_end),
    find_packet_location_in_vector, transplant_packet_in_vector at the location
    found (packet_location as returned, normalize_power=True) and
    validate_transplant_quality.  Returns (new_vector, location, validation),
    location = dict(vector_location, packet_location, confidence).  A device
    ``vector`` keeps everything but the scalar results on the device."""
    reference_segment = extract_reference_segment(packet_signal, ref_start, ref_end)
    vector_location, packet_location, confidence = find_packet_location_in_vector(
        vector, packet_signal, reference_segment, search_window, correlation_threshold)
    new_vector = transplant_packet_in_vector(vector, packet_signal, vector_location,
                                             packet_location, normalize_power=True)
    validation = validate_transplant_quality(vector, new_vector, packet_signal, vector_location,
                                             reference_segment, sample_rate)
    location = dict(vector_location=vector_location, packet_location=packet_location,
                    confidence=confidence)
    return new_vector, location, validation


# ---------------------------------------------------------------------------
# SMU-WV writer — vector_analyzer/mat_to_wv_converter.py:7-64
# ---------------------------------------------------------------------------
def _max_abs_f32(x: torch.Tensor) -> np.float32:
    """np.max(np.abs(x)) of complex64 x, with numpy's complex-abs formula."""
    ctx = _lib.get_context()
    n = int(x.shape[0])
    a = torch.empty(n, dtype=torch.complex64, device=x.device)
    ctx.check(ctx.lib.vsig_abs_c64_dev(ctx.h, _lib.DTYPES["c64"], _ptr(x), n, _ptr(a)), "abs")
    from .analysis import _thresh_dev
    f = torch.view_as_real(a).reshape(-1)
    _, _, _, mx = _thresh_dev(ctx, f, "f32", np.inf)
    return np.float32(mx)


def mat2wv(path_signal, sFilename, fSampleRate, bNormalize=True, var_name=None):
    """mat2wv (mat_to_wv_converter.py:7-64): quantise to interleaved int16 I/Q on
    the GPU and write the SMU-WV file (same header fields and order)."""
    ctx = _lib.get_context()
    if isinstance(path_signal, str):
        if var_name is None:
            raise ValueError("When path_signal is a filename, var_name must be specified")
        data = read_mat(path_signal)
        if var_name not in data:
            raise KeyError(var_name)
        x = _load_complex64_dev(data, var_name, ctx)
    elif _is_dev(path_signal):
        x = _device_c64(path_signal.reshape(-1), ctx)
    else:
        x = _device_c64(np.asarray(path_signal).flatten(), ctx)
    N = int(x.shape[0])
    norm = 0.0
    if bNormalize:
        print("Normalize signal")
        m = _max_abs_f32(x)
        norm = float(m)
        # peak / mean power of the normalised signal (metadata of the header)
        xs = torch.empty_like(x)
        ctx.check(ctx.lib.vsig_scale_c64_dev(ctx.h, _ptr(x), N, float(np.float32(1) / m)
                                             if m else 0.0, _ptr(xs)), "scale")
        _, peak, _, s2, _ = peak_stats(xs)
        fPeakPower = np.float32(np.float32(peak) ** 2)
        fPeakPowerdBfs = -10 * np.log10(fPeakPower)
        fMeanPower = np.float32(s2 / N)
        fRMSdBfs = -10 * np.log10(fMeanPower)
    else:
        fPeakPowerdBfs = 0.0
        fRMSdBfs = 0.0
    q = torch.empty(2 * N, dtype=torch.int16, device=x.device)
    ctx.bind_stream()
    ctx.check(ctx.lib.vsig_wv_quantize_dev(ctx.h, _ptr(x), N, float(norm), _ptr(q)), "wv")
    interleaved = q.cpu().numpy()
    total_bytes = 4 * N + 1
    with open(sFilename, "wb") as fid:
        fid.write("{TYPE: SMU-WV,0}".encode())
        fid.write("{COMMENT: Generated by mat2wv.py}".encode())
        fid.write(f"{{DATE: {datetime.now().strftime('%Y-%m-%d;%H:%M:%S')}}}".encode())
        fid.write(f"{{LEVEL OFFS: {fRMSdBfs}, {fPeakPowerdBfs}}}".encode())
        fid.write(f"{{CLOCK: {fSampleRate}}}".encode())
        fid.write(f"{{SAMPLES: {N}}}".encode())
        fid.write(f"{{WAVEFORM-{total_bytes}:#".encode())
        fid.write(interleaved.tobytes())
        fid.write(b"}")


def save_vector_wv(vector, output_path, sample_rate, normalize=False):
    """utils.py:672-677."""
    mat2wv(vector, output_path, sample_rate, bNormalize=normalize)


# ---------------------------------------------------------------------------
# MAT v5 (uncompressed and miCOMPRESSED elements) — the subset scipy.io
# loadmat / savemat produce for the reference's packets and vectors
# ---------------------------------------------------------------------------
_MI_NP = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.uint16, 5: np.int32, 6: np.uint32,
          7: np.float32, 9: np.float64, 12: np.int64, 13: np.uint64}
_MX_NP = {6: np.float64, 7: np.float32, 8: np.int8, 9: np.uint8, 10: np.int16, 11: np.uint16,
          12: np.int32, 13: np.uint32, 14: np.int64, 15: np.uint64}


def _tag(buf, off, endian):
    t, n = struct.unpack(endian + "II", buf[off:off + 8])
    if t >> 16:                                   # small data element
        return t & 0xFFFF, t >> 16, off + 4, off + 8
    return t, n, off + 8, off + 8 + ((n + 7) // 8) * 8


def _parse_matrix(buf, endian):
    """-> (name, mx_class, dims, complex, (re_type, re_bytes), (im_type, im_bytes))."""
    off = 0
    t, n, d, off = _tag(buf, off, endian)         # array flags
    flags = struct.unpack(endian + "I", buf[d:d + 4])[0]
    mx_class, is_complex = flags & 0xFF, bool(flags & 0x800)
    t, n, d, off = _tag(buf, off, endian)         # dimensions
    dims = struct.unpack(endian + f"{n // 4}i", buf[d:d + n])
    t, n, d, off = _tag(buf, off, endian)         # name
    name = bytes(buf[d:d + n]).decode("latin1")
    if mx_class not in _MX_NP:
        return name, mx_class, dims, is_complex, None, None
    t, n, d, off = _tag(buf, off, endian)
    re = (t, buf[d:d + n])
    im = None
    if is_complex:
        t, n, d, off = _tag(buf, off, endian)
        im = (t, buf[d:d + n])
    return name, mx_class, dims, is_complex, re, im


def _mat_elements(path):
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    if len(raw) < 128:
        raise ValueError(f"{path}: not a MAT-file")
    endian = "<" if bytes(raw[126:128]) == b"IM" else ">"
    if struct.unpack(endian + "H", bytes(raw[124:126]))[0] != 0x0100:
        raise NotImplementedError(f"{path}: only MAT v5 files are supported (v7.3 is HDF5)")
    header = bytes(raw[:116]).rstrip(b"\x00 ")
    off = 128
    elems = []
    mv = memoryview(raw)
    while off + 8 <= len(raw):
        t, n = struct.unpack(endian + "II", bytes(raw[off:off + 8]))
        body = mv[off + 8:off + 8 + n]
        off += 8 + ((n + 7) // 8) * 8
        if t == 15:                               # miCOMPRESSED: one zlib stream
            inner = zlib.decompress(bytes(body))
            t2, n2 = struct.unpack(endian + "II", inner[:8])
            if t2 == 14:
                elems.append(_parse_matrix(memoryview(inner)[8:8 + n2], endian))
        elif t == 14:
            elems.append(_parse_matrix(body, endian))
    return header, endian, elems


def _plane_to_np(plane, endian):
    t, b = plane
    dt = np.dtype(_MI_NP[t]).newbyteorder(endian)
    return np.frombuffer(b, dtype=dt)


def read_mat(path):
    """{name: value} for the numeric arrays of a MAT v5 file, on the host
    (scalars as Python numbers, arrays squeezed) — loadmat(squeeze_me=True)'s
    view of the reference's files.  Sample planes of complex arrays are kept as
    raw planes under key (name, 'planes') for the GPU loader."""
    header, endian, elems = _mat_elements(path)
    out = {"__header__": header, "__version__": "1.0", "__globals__": []}
    for name, mx_class, dims, is_complex, re, im in elems:
        if re is None:
            continue
        r = _plane_to_np(re, endian)
        if len(r) > 4:                            # sample planes: converted on the GPU
            out[(name, "planes")] = (re, im, endian, dims)
            arr = None
        elif is_complex:
            arr = r.astype(np.float64) + 1j * _plane_to_np(im, endian).astype(np.float64)
        else:
            arr = r.astype(_MX_NP[mx_class])
        if arr is not None:
            arr = arr.reshape(dims, order="F").squeeze()
            out[name] = arr.item() if arr.ndim == 0 else arr
        else:
            out[name] = None                      # materialised by the GPU loader
    return out


def _packet_var(data, file_path):
    if "Y" in data:
        return "Y"
    candidates = [k for k in data.keys() if isinstance(k, str) and not k.startswith("__")]
    if len(candidates) == 1:
        return candidates[0]
    keys = [k for k in data.keys() if isinstance(k, str)]
    raise ValueError(f"Ambiguous packet data in {file_path}. Available keys: {keys}")


def _load_complex64_dev(data, name, ctx):
    """GPU conversion of a variable's planes to a flat complex64 tensor."""
    planes = data.get((name, "planes"))
    dev = f"cuda:{ctx.device}"
    if planes is None:                            # real array (or scalar)
        val = np.asarray(data[name]).ravel(order="F")
        return torch.from_numpy(np.ascontiguousarray(val.astype(np.complex64))).to(dev)
    (rt, rb), im, endian, dims = planes
    n = int(np.prod(dims))
    if rt not in _MI_NP:
        raise NotImplementedError(f"MAT storage type {rt}")
    if endian != "<":
        raise NotImplementedError("big-endian MAT files")
    re_d = torch.frombuffer(bytearray(rb), dtype=torch.uint8).to(dev)
    im_d = torch.frombuffer(bytearray(im[1]), dtype=torch.uint8).to(dev) if im else None
    if im is not None and im[0] != rt:            # mixed storage types: bring imag to re's
        imv = _plane_to_np(im, endian).astype(_MI_NP[rt])
        im_d = torch.from_numpy(imv.view(np.uint8).copy()).to(dev)
    y = torch.empty(n, dtype=torch.complex64, device=dev)
    ctx.bind_stream()
    ctx.check(ctx.lib.vsig_planar_to_c64_dev(ctx.h, int(rt), _ptr(re_d),
                                             _ptr(im_d) if im_d is not None else None, n, _ptr(y)),
              "planar_to_c64")
    # MATLAB is column-major: a 1-D capture (1 x n or n x 1) is already in order;
    # a 2-D matrix is flattened in C order like packet.flatten() after loadmat
    if len(dims) == 2 and dims[0] > 1 and dims[1] > 1:
        y = y.view(dims[1], dims[0]).t().contiguous().view(-1)
    return y


def load_packet(file_path, device: bool = False):
    """utils.py:48-86: the 'Y' variable (or the only variable) as a flat
    complex64 array; device=True keeps it in HBM (torch tensor)."""
    try:
        file_size_mb = os.path.getsize(file_path) / (1024 * 1024)
        is_large_file = file_size_mb > 50
        if is_large_file:
            print(f"📁 Loading large file: {file_size_mb:.1f}MB")
        ctx = _lib.get_context()
        data = read_mat(file_path)
        name = _packet_var(data, file_path)
        packet = _load_complex64_dev(data, name, ctx)
        if packet.numel() > 20_000_000:
            duration_sec = packet.numel() / 56e6
            memory_mb = packet.numel() * 8 / (1024 * 1024)
            print(f"⚠️ Heavy packet loaded: {packet.numel():,} samples ({duration_sec:.2f}s, "
                  f"{memory_mb:.1f}MB)")
        return packet if device else packet.cpu().numpy()
    except Exception as e:
        print(f"Error loading packet from {file_path}: {e}")
        raise


def load_packet_info(file_path, device: bool = False):
    """utils.py:88-105: (packet complex64, pre_samples)."""
    ctx = _lib.get_context()
    data = read_mat(file_path)
    name = _packet_var(data, file_path)
    packet = _load_complex64_dev(data, name, ctx)
    pre = int(data.get("pre_samples", 0))
    return (packet if device else packet.cpu().numpy()), pre


def write_mat_vector(output_path, y_re: np.ndarray, y_im: np.ndarray, pre_samples: int = 0):
    """scipy.io.savemat(path, {'Y': complex64 row vector, 'pre_samples': int})
    byte layout (format 5, oned_as='row'); the header carries the write time."""
    n = len(y_re)
    if 4 * n >= 2 ** 32:
        raise ValueError("Matrix too large to save with Matlab 5 format")

    def pad8(b):
        return b + b"\x00" * ((8 - len(b) % 8) % 8)

    def el(t, payload):
        return struct.pack("<II", t, len(payload)) + pad8(payload)

    hdr = (f"MATLAB 5.0 MAT-file Platform: {os.name}, Created on: {time.asctime()}"
           ).encode().ljust(116, b"\x00")
    hdr += b"\x00" * 8 + struct.pack("<H", 0x0100) + b"IM"
    y = (el(6, struct.pack("<II", 0x0800 | 7, 0)) + el(5, struct.pack("<ii", 1, n))
         + struct.pack("<HH", 1, 1) + b"Y\x00\x00\x00"
         + el(7, y_re.astype("<f4").tobytes()) + el(7, y_im.astype("<f4").tobytes()))
    pre = (el(6, struct.pack("<II", 14, 0)) + el(5, struct.pack("<ii", 1, 1))
           + el(1, b"pre_samples") + el(12, struct.pack("<q", int(pre_samples))))
    with open(output_path, "wb") as f:
        f.write(hdr + el(14, y) + el(14, pre))


def save_vector(vector, output_path):
    """utils.py:659-670: flat complex64 'Y' + pre_samples=0, planes split on the GPU."""
    ctx = _lib.get_context()
    if _is_dev(vector):
        x = _device_c64(vector.reshape(-1), ctx)
    else:
        x = _device_c64(np.asarray(vector).flatten(), ctx)
    n = int(x.shape[0])
    re = torch.empty(n, dtype=torch.float32, device=x.device)
    im = torch.empty(n, dtype=torch.float32, device=x.device)
    ctx.bind_stream()
    ctx.check(ctx.lib.vsig_c64_to_planar_dev(ctx.h, _ptr(x), n, _ptr(re), _ptr(im)), "planes")
    write_mat_vector(output_path, re.cpu().numpy(), im.cpu().numpy(), 0)


# ---------------------------------------------------------------------------
# vector assembly — generate_vector, unified_gui.py:1692-1791 / main.py:214-284
# ---------------------------------------------------------------------------
_MARKER_STYLES = ["x", "o", "^", "s", "D", "P", "v", "1", "2", "3", "4"]
_MARKER_COLORS = [f"C{i}" for i in range(10)]


class VectorPlan(NamedTuple):
    """Where generate_vector puts every packet: places[i] = (start_offset,
    period_samples, count) of config i, the vector's length, and the markers
    (time of the instance's first payload sample, freq_shift, base name,
    marker style, marker colour) in the reference's append order."""
    places: list
    total_samples: int
    markers: list


def _mat_packet_shape(path):
    """(samples, pre_samples) of a packet file from its MAT v5 tags alone (host)."""
    data = read_mat(path)
    name = _packet_var(data, path)
    planes = data.get((name, "planes"))
    n = int(np.prod(planes[3])) if planes is not None else int(np.asarray(data[name]).size)
    return n, int(data.get("pre_samples", 0))


def _base_name(cfg, idx):
    if cfg.get("file") is not None:
        return os.path.splitext(os.path.basename(cfg["file"]))[0]
    return str(cfg.get("name", f"packet_{idx + 1}"))


def _plan(configs, lengths, pres, vector_length, sample_rate) -> VectorPlan:
    total_samples = int(vector_length * sample_rate)
    places, markers, styles = [], [], {}
    for idx, (cfg, n, pre) in enumerate(zip(configs, lengths, pres)):
        name = _base_name(cfg, idx)
        if name not in styles:
            styles[name] = (_MARKER_STYLES[len(styles) % len(_MARKER_STYLES)],
                            _MARKER_COLORS[len(styles) % len(_MARKER_COLORS)])
        style, color = styles[name]
        period_samples = int(cfg["period"] * sample_rate)
        if period_samples <= 0:
            raise ValueError(f"Invalid period for packet {idx + 1}")
        start = max(0, int(round(cfg["start_time"] * sample_rate)) - pre)
        # instances while pos + len <= total_samples (a cut-off one is not inserted)
        count = (total_samples - n - start) // period_samples + 1 if start + n <= total_samples else 0
        places.append((start, period_samples, count))
        shift = cfg.get("freq_shift", 0)
        markers.extend(((start + k * period_samples + pre) / sample_rate, shift, name, style, color)
                       for k in range(count))
    return VectorPlan(places, total_samples, markers)


def _check_vector_args(configs, vector_length):
    if not configs:
        raise ValueError("No packets configured")
    if not vector_length > 0:
        raise ValueError("Vector length must be positive")


def _resampled_len(n, cfg, sample_rate):
    sr = cfg.get("sample_rate")
    return n if sr is None or sr == sample_rate else int(n * (sample_rate / sr))


def vector_plan(configs, vector_length, sample_rate) -> VectorPlan:
    """The placement arithmetic of generate_vector (unified_gui.py:1711,
    1748-1769), on the host: total_samples = int(vector_length * sample_rate),
    period_samples = int(period * sample_rate), start_offset =
    max(0, int(round(start_time * sample_rate)) - pre_samples), instances while
    pos + len <= total_samples.  A config's packet length comes from its
    ``length`` key, its ``signal``, or its ``file``'s MAT header (with the
    file's pre_samples).  ValueError for what the GUI rejects: no configs,
    vector_length <= 0, a period below one sample."""
    configs = list(configs)
    _check_vector_args(configs, vector_length)
    lengths, pres = [], []
    for cfg in configs:
        pre = int(cfg.get("pre_samples", 0))
        if cfg.get("length") is not None:
            n = int(cfg["length"])
        elif cfg.get("signal") is not None:
            n = int(cfg["signal"].shape[0])
        else:
            n, pre = _mat_packet_shape(cfg["file"])
        lengths.append(_resampled_len(n, cfg, sample_rate))
        pres.append(pre)
    return _plan(configs, lengths, pres, vector_length, sample_rate)


def _prepare_packets(configs, sample_rate, ctx):
    """Every config's packet as generate_vector inserts it (device complex64)
    and its pre_samples: loaded (``file``) or taken (``signal``), resampled
    when its ``sample_rate`` differs (main.py:236-237), mixed by
    ``freq_shift`` once.  Shared by build_vector and verify_vector."""
    packets, pres = [], []
    for cfg in configs:
        if cfg.get("signal") is not None:
            y, pre = _device_c64(cfg["signal"], ctx), int(cfg.get("pre_samples", 0))
        else:
            y, pre = load_packet_info(cfg["file"], device=True)
        sr = cfg.get("sample_rate")
        if sr is not None and sr != sample_rate:
            y = resample_signal(y, sr, sample_rate)
        shift = cfg.get("freq_shift", 0)
        if shift != 0:
            y = apply_frequency_shift(y, shift, sample_rate)
        packets.append(y.contiguous())
        pres.append(pre)
    return packets, pres


def build_vector(configs, vector_length, sample_rate, normalize=False, device=False):
    """generate_vector (unified_gui.py:1692-1791) up to the save: every
    packet loaded (``file``: load_packet_info; ``signal``: an array or device
    tensor, with ``pre_samples``), resampled when its ``sample_rate`` differs
    (main.py:236-237), mixed by ``freq_shift`` once (the phase restarts at
    every instance) and added into a zeroed complex64 vector every ``period``
    seconds from ``start_time`` -- one vsig_vector_build_dev, numpy's adds in
    numpy's order -- then divided by its peak |v| on the device when
    ``normalize`` (left as is when the peak is 0).  Returns (vector, markers):
    a numpy array, or with device=True the tensor in HBM, ready for
    save_vector / save_vector_wv / create_spectrogram."""
    configs = list(configs)
    _check_vector_args(configs, vector_length)
    ctx = _lib.get_context()
    packets, pres = _prepare_packets(configs, sample_rate, ctx)
    plan = _plan(configs, [int(y.shape[0]) for y in packets], pres, vector_length, sample_rate)
    n = plan.total_samples
    out = torch.empty(n, dtype=torch.complex64, device=f"cuda:{ctx.device}")
    live = [(y, pl) for y, pl in zip(packets, plan.places) if y.shape[0] > 0]
    places = (_lib.PacketPlace * max(1, len(live)))()
    for p, (y, (start, period, count)) in zip(places, live):
        p.y, p.len, p.start, p.period, p.count = y.data_ptr(), int(y.shape[0]), start, period, count
    peak = torch.empty(1, dtype=torch.float32, device=out.device) if normalize and n else None
    ctx.bind_stream()
    if n:
        ctx.check(ctx.lib.vsig_vector_build_dev(ctx.h, places, len(live), _ptr(out), n,
                                                _ptr(peak) if peak is not None else None),
                  "vector_build")
    if peak is not None:
        ctx.check(ctx.lib.vsig_normalize_c64_dev(ctx.h, _ptr(out), n, _ptr(peak), _ptr(out)),
                  "normalize")
    return (out if device else out.cpu().numpy()), plan.markers


def _timing_status(overall):
    if overall > 99.5:
        return "✅ PERFECT"
    if overall > 99.0:
        return "✅ EXCELLENT"
    if overall > 95.0:
        return "⚠️ GOOD"
    if overall > 90.0:
        return "⚠️ FAIR"
    return "❌ POOR"


def validate_packet_timing(markers, configs):
    """The timing score of validate_packet_timing (unified_gui.py:1496-1690) as
    a host function on plain config dicts (the keys build_vector takes; a
    config's name is its file's base name, else ``name``, else packet_<i+1>),
    so that measured markers (verify_vector) score like planned ones
    (VectorPlan.markers).  Per named packet, marker times sorted:

      start     |first time - start_time| in ms against a tolerance of 10 ms
                (<= 2 instances) or 5 ms: 100 inside it, else
                max(0, 100 - err / tol * 50)
      period    e = |mean interval - period| / period * 100:  100 if e <= 1,
                100 - (e - 1) * 5 if e <= 5, else max(0, 80 - (e - 5) * 2)
      frequency always 100;  consistency 100, or 80 for a single instance
      packet    0.4 period + 0.3 start + 0.2 frequency + 0.1 consistency,
                + min(5, instances - 2) above 2 instances, capped at 100

    Overall is the mean over packets.  Returns
    ``(f"Timing Validation: {overall:.1f}% {status}", details)`` -- details:
    one dict per packet (packet_name, instances, start_time_error_ms,
    period_error_percent, freq_shift_mhz, explanations) -- or
    ``("No packets to validate", [])``.  Prints nothing."""
    by_name = {}
    for time_sec, shift, name, _style, _colour in markers:
        by_name.setdefault(name, []).append((time_sec, shift))
    scores, details = [], []
    for idx, cfg in enumerate(configs):
        if not cfg:
            continue
        name = _base_name(cfg, idx)
        if name not in by_name:
            continue
        found = sorted(by_name[name], key=lambda m: m[0])
        times = [m[0] for m in found]
        shifts = [m[1] for m in found]
        count = len(times)
        period_ms = cfg["period"] * 1000
        want_shift = cfg.get("freq_shift", 0)

        start_err = abs(times[0] * 1000 - cfg["start_time"] * 1000)
        tol = 10.0 * (1.0 if count <= 2 else 0.5)
        if start_err <= tol:
            start_acc, start_txt = 100.0, f"start within tolerance ({start_err:.2f} ms off)"
        else:
            start_acc = max(0, 100 - (start_err / tol * 50))
            start_txt = f"start outside tolerance ({start_err:.2f} ms off)"

        period_acc, period_err, period_txt = 100.0, 0.0, ""
        if count > 1:
            gaps = [(times[i] - times[i - 1]) * 1000 for i in range(1, count)]
            avg, std = np.mean(gaps), np.std(gaps)
            period_err = abs(avg - period_ms) / period_ms * 100
            if period_err <= 1.0:
                period_txt = f"period on target (mean {avg:.2f} ms, std {std:.2f} ms)"
            elif period_err <= 5.0:
                period_acc = 100 - (period_err - 1.0) * 5
                period_txt = f"period close (mean {avg:.2f} ms, {period_err:.1f}% off)"
            else:
                period_acc = max(0, 80 - (period_err - 5.0) * 2)
                period_txt = f"period off target (mean {avg:.2f} ms, {period_err:.1f}% off)"
        else:
            period_txt = "one instance: no period to check"

        distinct = set(shifts)
        if len(distinct) > 1:
            freq_txt = f"{len(distinct)} different frequency shifts"
        elif shifts[0] == want_shift:
            freq_txt = f"frequency shift as configured ({want_shift / 1e6:.1f} MHz)"
        else:
            freq_txt = (f"frequency shift {shifts[0] / 1e6:.1f} MHz, configured "
                        f"{want_shift / 1e6:.1f} MHz")

        if count >= 2:
            cons_acc, cons_txt = 100.0, f"{count} instances"
        else:
            cons_acc, cons_txt = 80.0, "one instance: consistency cannot be checked"

        acc = period_acc * 0.4 + start_acc * 0.3 + 100.0 * 0.2 + cons_acc * 0.1
        if count > 2:
            acc = min(100.0, acc + min(5.0, (count - 2) * 1.0))
        scores.append(acc)
        details.append({
            "packet_name": name,
            "instances": count,
            "start_time_error_ms": start_err,
            "period_error_percent": period_err if count > 1 else 0,
            "freq_shift_mhz": want_shift / 1e6,
            "explanations": {"start": start_txt, "period": period_txt, "freq": freq_txt,
                             "consistency": cons_txt},
        })
    if not scores:
        return "No packets to validate", []
    overall = sum(scores) / len(scores)
    return f"Timing Validation: {overall:.1f}% {_timing_status(overall)}", details


def verify_vector(vector, configs, vector_length, sample_rate, threshold_ratio=0.5):
    """Where every configured packet really sits in ``vector`` (a numpy array
    or a device tensor, e.g. build_vector's output or a capture), and how that
    timing scores.  Each config's packet is prepared exactly as build_vector
    inserts it (loaded, resampled, mixed), correlated over the vector and its
    instances listed (dsp.find_packet_instances at ``threshold_ratio`` of the
    strongest, min_distance = min(len(packet), period_samples) // 2).  Returns
    ``(measured_markers, validate_packet_timing(measured_markers, configs))``;
    a measured marker is ((start + pre_samples) / sample_rate, freq_shift,
    name, style, colour), the layout and order of VectorPlan.markers."""
    configs = list(configs)
    _check_vector_args(configs, vector_length)
    ctx = _lib.get_context()
    packets, pres = _prepare_packets(configs, sample_rate, ctx)
    vd = _device_c64(vector.reshape(-1) if _is_dev(vector) else np.asarray(vector).ravel(), ctx)
    markers, styles = [], {}
    for idx, (cfg, y, pre) in enumerate(zip(configs, packets, pres)):
        name = _base_name(cfg, idx)
        if name not in styles:
            styles[name] = (_MARKER_STYLES[len(styles) % len(_MARKER_STYLES)],
                            _MARKER_COLORS[len(styles) % len(_MARKER_COLORS)])
        style, color = styles[name]
        period_samples = int(cfg["period"] * sample_rate)
        if period_samples <= 0:
            raise ValueError(f"Invalid period for packet {idx + 1}")
        n = int(y.shape[0])
        if n == 0 or n > int(vd.shape[0]):
            continue
        starts, _ = find_packet_instances(vd, y, threshold_ratio, min(n, period_samples) // 2)
        starts = starts[starts >= 0].cpu().tolist()
        shift = cfg.get("freq_shift", 0)
        markers.extend(((s + pre) / sample_rate, shift, name, style, color) for s in starts)
    return markers, validate_packet_timing(markers, configs)


def compute_freq_ranges(shifts, margin=1e6):
    """utils.py:129-159: one (min - margin, max + margin) range over the
    shifts that are ints or floats (bools and anything else skipped), or None
    when there are none or every shift is zero."""
    if not shifts or all(s == 0 for s in shifts):
        return None
    numbers = [s for s in shifts if isinstance(s, (int, float)) and not isinstance(s, bool)]
    if not numbers:
        return None
    return [(min(numbers) - margin, max(numbers) + margin)]
