"""numpy restatement of the line traces (vector_amd/csrc/trace.hip,
vsig_trace_envelope_dev in include/vsig.h), shared by test_traces_cpu.py and
test_gpu_traces.py.

  line        s[p] = |a[(p + rot) % n]| in the array's precision (np.abs)
  envelope    np.min / np.max of s over columns of `bin` positions from lo
              (NaN propagates), then the map applied to the 2 * cols results
  db20        20 * np.log10(E + eps) in E's dtype
  info        first argmin / argmax of s over [lo, hi) and the mapped values
  freq_axis   np.fft.fftfreq(n, 1 / sample_rate) + center_freq, fftshifted or not
  spectrum_line   the reference's spectrum sites on a given transform
"""
import numpy as np

ABS, DB20 = 0, 1


def line(a, shift=False):
    m = np.abs(a)
    return np.fft.fftshift(m) if shift else m


def db20(E, eps=0.0):
    dt = E.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20 * np.log10(E + dt(eps))


def columns(s, lo, hi, bin_):
    """[(first, last + 1)] of the columns of [lo, hi)."""
    return [(p, min(p + bin_, hi)) for p in range(lo, hi, bin_)]


def envelope_of(s, lo=0, hi=None, bin_=1):
    """(E_min, E_max) of the line s over [lo, hi) in columns of bin_."""
    hi = len(s) if hi is None else hi
    w = s[lo:hi]
    cols = -(-len(w) // bin_)
    whole = (len(w) // bin_) * bin_
    emin, emax = np.empty(cols, s.dtype), np.empty(cols, s.dtype)
    with np.errstate(invalid="ignore"):
        if whole:
            body = w[:whole].reshape(-1, bin_)
            emin[:whole // bin_], emax[:whole // bin_] = body.min(axis=1), body.max(axis=1)
        if whole < len(w):
            emin[-1], emax[-1] = np.min(w[whole:]), np.max(w[whole:])
    return emin, emax


def restate(a, shift=False, lo=0, hi=None, bin_=1, kind=ABS, eps=0.0):
    """(E_min, E_max, info) with info = (argmin, argmax, min, max)."""
    s = line(a, shift)
    hi = len(s) if hi is None else hi
    emin, emax = envelope_of(s, lo, hi, bin_)
    amin, amax = lo + int(np.argmin(s[lo:hi])), lo + int(np.argmax(s[lo:hi]))
    ext = np.array([s[amin], s[amax]])
    if kind == DB20:
        emin, emax, ext = db20(emin, eps), db20(emax, eps), db20(ext, eps)
    return emin, emax, (amin, amax, float(ext[0]), float(ext[1]))


def freq_axis(n, sample_rate, center_freq=0.0, shift=True):
    f = np.fft.fftfreq(n, 1 / sample_rate) + center_freq
    return np.fft.fftshift(f) if shift else f


def spectrum_line(X, scale="db", eps=0.0, shift=True, normalize=False):
    """The spectrum sites' line on the transform X: np.abs, fftshift, 20 *
    np.log10(. + eps), minus the maximum (mat_analyzer.py:212-215)."""
    m = line(X, shift)
    if scale == "db":
        m = db20(m, eps)
        if normalize:
            m = m - np.max(m)
    return m


def ulps(got, want):
    """|got - want| in spacings of want, 0 where both are the same infinity or
    both NaN."""
    got, want = np.asarray(got), np.asarray(want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want))
    return np.where(same, 0.0, d)
