"""Detection / display helpers of the reference on the GPU (SURVEY.md §8(a)
rows a3, a7, a8):

  normalize_spectrogram   utils.py:356-404  (spectrogram_levels: its level selection alone)
  find_packet_start       utils.py:784-809
  detect_packet_bounds    utils.py:811-825
  detect_packets          every burst of the same smoothed energy (the run list, runs.hip)

The data-parallel work — |S| order statistics, the dB transform, the |x|^2
prefix scan and boxcar smoothing, the threshold scan, the magnitude
correlation — runs in libvsig.so (analysis.hip, psd.hip, xcorr.hip, reduce.hip).  What is left on
the host is O(1) scalar arithmetic, written so that numpy's own rules
(np.percentile 'linear' in the array's dtype, np.median, NEP 50 promotion)
give the same numbers the reference computes.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .dsp import _correlate_dev, _is_dev, _ptr, _runs_host

__all__ = ["normalize_spectrogram", "spectrogram_levels", "find_packet_start", "detect_packet_bounds",
           "order_statistics", "threshold_stats", "boxcar_energy", "detect_packets", "Packets"]

def _to_device(x, ctx, real_only=False):
    """_lib.upload_native, flattened; real_only refuses a complex array."""
    t, code = _lib.upload_native(x, ctx)
    if real_only and code in ("c64", "c128"):
        raise ValueError("expected a real array")
    return t.reshape(-1), code


def order_statistics(a, ranks):
    """k-th smallest |a| (0-based) for up to 4 ranks — MSB-first radix select
    on the GPU (real float32 / float64 data)."""
    ctx = _lib.get_context()
    t, code = _to_device(a, ctx, real_only=True)
    return _order_stats_dev(ctx, t, code, ranks)


def _order_stats_dev(ctx, t, code, ranks):
    ranks = [int(r) for r in ranks]
    out = []
    for i in range(0, len(ranks), 4):
        rk = ranks[i:i + 4]
        rarr = (C.c_int64 * len(rk))(*rk)
        vals = (C.c_double * len(rk))()
        ctx.check(ctx.lib.vsig_select_dev(ctx.h, _lib.DTYPES[code], _ptr(t), int(t.numel()), rarr,
                                          len(rk), vals), "select")
        out.extend(vals[:len(rk)])
    return out


def threshold_stats(a, thr):
    """(count, first, last, max) of |a| >= thr over a real array (first = n,
    last = -1 when nothing passes)."""
    ctx = _lib.get_context()
    t, code = _to_device(a, ctx, real_only=True)
    return _thresh_dev(ctx, t, code, thr)


def _thresh_dev(ctx, t, code, thr):
    cnt, first, last = C.c_int64(), C.c_int64(), C.c_int64()
    mx = C.c_double()
    ctx.check(ctx.lib.vsig_threshold_dev(ctx.h, _lib.DTYPES[code], _ptr(t), int(t.numel()),
                                         float(thr), C.byref(cnt), C.byref(first), C.byref(last),
                                         C.byref(mx)), "threshold")
    return cnt.value, first.value, last.value, mx.value


def boxcar_energy(signal, w):
    """np.convolve(np.abs(signal) ** 2, np.ones(w) / w, 'same') as a float64
    CUDA tensor (length max(n, w))."""
    ctx = _lib.get_context()
    t, code = _to_device(signal, ctx)
    return _boxcar_dev(ctx, t, code, w)


def _boxcar_dev(ctx, t, code, w):
    n = int(t.numel())
    if n == 0:
        raise ValueError("v cannot be empty")
    sm = torch.empty(max(n, int(w)), dtype=torch.float64, device=t.device)
    ctx.check(ctx.lib.vsig_boxcar_energy_dev(ctx.h, _lib.DTYPES[code], _ptr(t), n, int(w), _ptr(sm)),
              "boxcar")
    return sm


# ---------------------------------------------------------------------------
# numpy's order-statistic reductions restated over GPU order statistics
# ---------------------------------------------------------------------------
def _percentile(n, pct, dt, fetch):
    """np.percentile(arr, pct) (method 'linear') for an array of n elements
    of dtype dt, given fetch(ranks) -> k-th smallest values.  Mirrors numpy's
    _quantile / _get_indexes / _get_gamma / _lerp including the dtype the
    arithmetic runs in (float32 arrays interpolate in float32), and its NaN
    rule: NaN sorts last, so a NaN largest element means one is present and
    the result is NaN (the last rank rides in the same select call)."""
    dt = np.dtype(dt)
    q = np.asanyarray(np.true_divide(pct, dt.type(100)))
    if np.any(q < 0) or np.any(q > 1):
        raise ValueError("Percentiles must be in the range [0, 100]")
    virtual = np.asanyarray((n - 1) * q)
    prev = np.asanyarray(np.floor(virtual))
    nxt = prev + 1
    if virtual >= n - 1:
        prev, nxt = np.asanyarray(-1), np.asanyarray(-1)
    if virtual < 0:
        prev, nxt = np.asanyarray(0), np.asanyarray(0)
    if np.isnan(virtual):
        prev, nxt = np.asanyarray(-1), np.asanyarray(-1)
    pi, ni = int(prev) % n, int(nxt) % n
    vals = fetch(sorted({pi, ni, n - 1}))
    if np.isnan(vals[n - 1]):
        return np.asarray(np.nan, dtype=dt)[()]
    a = np.asarray(vals[pi], dtype=dt)
    b = np.asarray(vals[ni], dtype=dt)
    gamma = np.asanyarray(virtual - prev.astype(np.intp), dtype=virtual.dtype)
    diff = np.subtract(b, a)
    res = np.asanyarray(np.add(a, diff * gamma))
    np.subtract(b, diff * (1 - gamma), out=res, where=gamma >= 0.5, casting="unsafe",
                dtype=res.dtype)
    return res[()]


def _median(n, dt, fetch):
    """np.median of n elements of dtype dt from order statistics (NaN when the
    largest element is NaN, i.e. when any is)."""
    if n == 0:
        return np.dtype(dt).type(np.nan)
    k = n // 2
    v = fetch(sorted({k, n - 1} if n % 2 else {k - 1, k, n - 1}))
    if np.isnan(v[n - 1]):
        return np.dtype(dt).type(np.nan)
    if n % 2:
        return np.dtype(dt).type(v[k])
    return np.mean(np.array([v[k - 1], v[k]], dtype=dt))


# ---------------------------------------------------------------------------
# normalize_spectrogram — utils.py:356-404
# ---------------------------------------------------------------------------
def _select_levels(Sxx, low_percentile, high_percentile, max_dynamic_range):
    """The selection half of normalize_spectrogram (utils.py:363-402) for a
    non-empty Sxx: the noise floor and vmin / vmax from order statistics of |S|,
    with no dB map.  Returns (ctx, t, code, src, transposed, floor_v, db_dt,
    vmin, vmax): t the flat device array the statistics were taken over (in the
    storage order of src, which is Sxx or its transpose), db_dt the dtype numpy
    evaluates the dB map in."""
    dev_in = _is_dev(Sxx)
    ctx = _lib.get_context()
    # transposed views (spectrum() returns (nfft, frames) over frame-major
    # memory) are reduced in their storage order and returned in the same view
    src = Sxx
    transposed = False
    if dev_in and Sxx.dim() == 2 and not Sxx.is_contiguous() and Sxx.t().is_contiguous():
        src, transposed = Sxx.t(), True
    t, code = _to_device(src, ctx, real_only=True)
    dt = np.float32 if code == "f32" else np.float64
    n = int(t.numel())
    cache = {}

    def fetch(ranks, base=0):
        need = [r for r in ranks if r + base not in cache]
        if need:
            got = _order_stats_dev(ctx, t, code, [r + base for r in need])
            cache.update({r + base: v for r, v in zip(need, got)})
        return {r: cache[r + base] for r in ranks}

    # |S| > 0 count: |S| >= the smallest subnormal of the dtype
    tiny = float(np.finfo(dt).smallest_subnormal)
    npos, _, _, mx = _thresh_dev(ctx, t, code, tiny)
    # np.max is NaN exactly when an element is; they sort last and are counted
    # only then (|S| >= 0 is false for a NaN alone)
    nnan = n - _thresh_dev(ctx, t, code, 0.0)[0] if np.isnan(mx) else 0
    if npos > 0:
        nzero = n - npos - nnan
        noise_floor = _percentile(npos, 5, dt, lambda rk: fetch(rk, nzero))
    else:
        noise_floor = 1e-12
    noise_floor = max(noise_floor, 1e-12)
    # numpy's promotion of |S| + noise_floor (NEP 50: a Python float is weak)
    db_dt = np.result_type(np.empty(0, dt), noise_floor)
    floor_v = float(np.asarray(noise_floor, dtype=db_dt))

    def db_of(v):
        return 10 * np.log10(np.asarray(v, dtype=db_dt) + np.asarray(floor_v, dtype=db_dt))

    def fetch_db(ranks):
        return {r: db_of(v) for r, v in fetch(ranks).items()}

    def min_max_db():
        """np.min / np.max of the dB map (both NaN when an element is)."""
        if nnan:
            return db_of(np.nan)[()], db_of(np.nan)[()]
        return db_of(fetch([0])[0])[()], db_of(fetch([n - 1])[n - 1])[()]

    try:
        vmin = _percentile(n, low_percentile, db_dt, fetch_db)
        vmax = _percentile(n, high_percentile, db_dt, fetch_db)
    except Exception:
        vmin, vmax = min_max_db()
    if np.isnan(vmin) or np.isnan(vmax) or vmax <= vmin:
        vmin, vmax = min_max_db()
        if vmax <= vmin:
            vmax = vmin + max_dynamic_range
    actual_range = vmax - vmin
    if actual_range > max_dynamic_range:
        vmin = vmax - max_dynamic_range
    elif actual_range < 20:
        mid_point = (vmax + vmin) / 2
        vmin = mid_point - 10
        vmax = mid_point + 10
    vmin = max(vmin, -120)
    if actual_range != vmax - vmin:
        print(f"📊 Dynamic range adjusted: {actual_range:.1f}dB → {vmax - vmin:.1f}dB "
              "(optimized for resolution)")
    return ctx, t, code, src, transposed, floor_v, db_dt, vmin, vmax


def spectrogram_levels(Sxx, low_percentile=10.0, high_percentile=95.0, max_dynamic_range=25):
    """(floor, vmin, vmax) of normalize_spectrogram (utils.py:356-404) without
    its dB map: floor = max(5th percentile of the positive |S|, 1e-12), vmin /
    vmax the percentiles of 10 log10(|S| + floor) after the dynamic-range
    clamps, typed as the reference's.  An empty Sxx gives (0.0, 0, 0)."""
    size = int(Sxx.numel()) if _is_dev(Sxx) else int(np.size(Sxx))
    if size == 0:
        return 0.0, 0, 0
    _, _, _, _, _, floor_v, _, vmin, vmax = _select_levels(Sxx, low_percentile, high_percentile,
                                                          max_dynamic_range)
    return floor_v, vmin, vmax


def normalize_spectrogram(Sxx, low_percentile=10.0, high_percentile=95.0, max_dynamic_range=25):
    """utils.py:356-404: (Sxx_db, vmin, vmax) with Sxx_db = 10 log10(|S| + floor),
    floor = max(5th percentile of the positive |S|, 1e-12), vmin / vmax the
    10th / 95th percentiles of Sxx_db, then the dynamic-range clamps.

    The percentiles come from radix-select order statistics of |S| on the GPU:
    10 log10(. + floor) is non-decreasing, so the k-th smallest dB value is
    the transform of the k-th smallest |S|.  numpy in -> numpy out; a CUDA
    tensor in -> Sxx_db stays on the device."""
    dev_in = _is_dev(Sxx)
    size = int(Sxx.numel()) if dev_in else int(np.size(Sxx))
    if size == 0:
        return np.array([]), 0, 0
    shape = tuple(Sxx.shape)
    ctx, t, code, src, transposed, floor_v, db_dt, vmin, vmax = _select_levels(
        Sxx, low_percentile, high_percentile, max_dynamic_range)
    n = int(t.numel())
    out_t = torch.float32 if db_dt == np.float32 else torch.float64
    if db_dt == np.float64 and code == "f32":
        t = t.to(torch.float64)
        code = "f64"
    db = torch.empty(n, dtype=out_t, device=t.device)
    ctx.check(ctx.lib.vsig_db_dev(ctx.h, _lib.DTYPES[code], _ptr(t), n, floor_v, _ptr(db)), "db")
    if transposed:
        db = db.reshape(tuple(src.shape)).t()
    else:
        db = db.reshape(shape)
    if dev_in:
        return db, vmin, vmax
    return db.cpu().numpy(), vmin, vmax


# ---------------------------------------------------------------------------
# find_packet_start / detect_packet_bounds — utils.py:784-825
# ---------------------------------------------------------------------------
def _energy_threshold(ctx, sm, m, threshold_ratio):
    """(noise, thr): noise = median(sm[:m]), thr = noise + r (max - noise)."""
    head = sm[:m]
    cache = {}

    def fetch(ranks):
        need = [r for r in ranks if r not in cache]
        if need:
            cache.update(zip(need, _order_stats_dev(ctx, head, "f64", need)))
        return {r: cache[r] for r in ranks}

    noise = _median(m, np.float64, fetch)
    _, _, _, max_en = _thresh_dev(ctx, sm, "f64", np.inf)
    return noise, noise + threshold_ratio * (np.float64(max_en) - noise)


def _threshold_first_last(ctx, sm, m, threshold_ratio):
    """First / last index of sm >= _energy_threshold's thr (a NaN thr or
    count 0 -> None)."""
    _, threshold = _energy_threshold(ctx, sm, m, threshold_ratio)
    if np.isnan(threshold):
        return None
    cnt, first, last, _ = _thresh_dev(ctx, sm, "f64", float(threshold))
    if cnt == 0:
        return None
    return first, last


def find_packet_start(signal, template=None, threshold_ratio=0.2, window_size=None):
    """utils.py:784-809.  Template branch: argmax of
    np.correlate(|signal|, |template|, 'valid') (overlap-save correlator on the
    magnitudes, argmax fused); energy branch: boxcar-smoothed |x|^2 (prefix
    scan), median of the first 10 % (radix select), first index above
    noise + r (max - noise)."""
    ctx = _lib.get_context()
    if template is not None:
        s, scode = _to_device(signal, ctx)
        tm, tcode = _to_device(template, ctx)
        if s.numel() == 0 or tm.numel() == 0:
            raise ValueError("v cannot be empty" if tm.numel() == 0 else "a cannot be empty")
        # np.abs keeps the input's precision: complex64 / float32 magnitudes are
        # float32 (exact in complex64), wider ones float64 (complex128 operands
        # of the correlation, so the argmax refine sees numpy's values)
        wide = scode in ("c128", "f64") or tcode in ("c128", "f64")
        odt = torch.complex128 if wide else torch.complex64
        absfn = ctx.lib.vsig_abs_c128_dev if wide else ctx.lib.vsig_abs_c64_dev
        sa = torch.empty(int(s.numel()), dtype=odt, device=s.device)
        ta = torch.empty(int(tm.numel()), dtype=odt, device=s.device)
        ctx.check(absfn(ctx.h, _lib.DTYPES[scode], _ptr(s), int(s.numel()), _ptr(sa)), "abs")
        ctx.check(absfn(ctx.h, _lib.DTYPES[tcode], _ptr(tm), int(tm.numel()), _ptr(ta)), "abs")
        _, pk, _, _ = _correlate_dev(sa, ta, "valid", False, ctx)
        return int(pk.cpu().view(torch.int64)[1].item())
    t, code = _to_device(signal, ctx)
    n = int(t.numel())
    if window_size is None:
        window_size = max(1, int(0.02 * n))
    w = max(1, window_size)
    sm = _boxcar_dev(ctx, t, code, w)
    r = _threshold_first_last(ctx, sm, int(sm.numel()) // 10, threshold_ratio)
    return int(r[0]) if r is not None else 0


def detect_packet_bounds(signal, sample_rate, threshold_ratio=0.2):
    """utils.py:811-825: (start, end) of the smoothed-energy burst (1 us
    boxcar), (0, len(signal)) when nothing passes the threshold."""
    ctx = _lib.get_context()
    t, code = _to_device(signal, ctx)
    n = int(t.numel())
    w = max(1, int(sample_rate // 1_000_000))
    sm = _boxcar_dev(ctx, t, code, w)
    r = _threshold_first_last(ctx, sm, max(1, int(sm.numel()) // 10), threshold_ratio)
    if r is None:
        return 0, n
    return np.int64(r[0]), np.int64(r[1])


# ---------------------------------------------------------------------------
# detect_packets — every burst of a capture, where detect_packet_bounds
# returns the first and last sample above its threshold
# ---------------------------------------------------------------------------
class Packets(NamedTuple):
    """detect_packets' result: one entry per burst in starts / ends (inclusive)
    / peak_index / peak / mean_power, and the scalars the rule used."""
    starts: np.ndarray        # int64: first sample of the smoothed energy at or above the threshold
    ends: np.ndarray          # int64: last one (inclusive)
    peak_index: np.ndarray    # int64: first maximum of the smoothed energy inside the burst
    peak: np.ndarray          # float64: that maximum
    mean_power: np.ndarray    # float64: mean smoothed energy over [start, end]
    noise: float              # median of the first tenth of the smoothed energy (nan with ``threshold``)
    threshold: float          # the level applied
    window: int               # boxcar length, samples


def detect_packets(signal, sample_rate, threshold_ratio=0.2, max_gap=None, min_length=None,
                   threshold=None, max_packets=65536):
    """Where every burst of ``signal`` begins and ends, without a template:
    the runs (find_runs' definition, vsig_runs_dev) of detect_packet_bounds'
    own smoothed energy ``sm = np.convolve(np.abs(x) ** 2, np.ones(w) / w,
    'same')``, ``w = max(1, int(sample_rate // 1e6))``, at or above its own
    threshold ``noise + threshold_ratio * (max(sm) - noise)``, noise the median
    of sm's first tenth.  ``threshold`` replaces that rule by an absolute
    level on sm.

    max_gap and min_length default to w: a dropout shorter than the smoother
    cannot separate two packets and a burst shorter than it is not resolved.
    With min_length=1 and any max_gap, ``(starts[0], ends[-1])`` is
    detect_packet_bounds' pair.  Nothing above the threshold, or a NaN
    threshold, gives an empty list (not detect_packet_bounds' (0, n)).

    Returns ``Packets`` with host arrays (numpy or CUDA tensor in).  More than
    max_packets bursts (counted before min_length): one more call with room
    for all when there are at most 2**24, else a RuntimeWarning and the first
    max_packets."""
    w = max(1, int(sample_rate // 1_000_000))
    max_gap = w if max_gap is None else int(max_gap)
    min_length = w if min_length is None else int(min_length)
    if max_gap < 0:
        raise ValueError("max_gap must be >= 0")
    if min_length < 1:
        raise ValueError("min_length must be >= 1")
    if int(max_packets) < 0:
        raise ValueError("max_packets must be >= 0")
    if (int(signal.numel()) if isinstance(signal, torch.Tensor) else int(np.size(signal))) == 0:
        raise ValueError("detect_packets of an empty signal")
    ctx = _lib.get_context()
    t, code = _to_device(signal, ctx)
    sm = _boxcar_dev(ctx, t, code, w)
    if threshold is None:
        noise, thr = _energy_threshold(ctx, sm, max(1, int(sm.numel()) // 10), threshold_ratio)
    else:
        noise, thr = np.float64(np.nan), np.float64(threshold)
    if np.isnan(thr):
        e = np.zeros(0, np.int64)
        f = np.zeros(0, np.float64)
        return Packets(e, e.copy(), e.copy(), f, f.copy(), float(noise), float(thr), w)
    r, _ = _runs_host(sm, "f64", float(thr), max_gap, False, min_length, max_packets, ctx, "detect_packets")
    return Packets(r.start, r.end, r.argmax, r.max, r.mean, float(noise), float(thr), w)
