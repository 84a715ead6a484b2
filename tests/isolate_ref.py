"""The definition of vsig_isolate_run / isolate_packets in numpy float64, from
the oracle's pieces, and a restatement of the frame planner.

    u = ref.apply_frequency_shift(x.astype(complex128), -f, sr)
    z = np.convolve(np.r_[u, zeros(d)], h.astype(float64))[d:d+n][lo:hi]

isolate_full is that, literally.  isolate computes the same numbers from the
samples the outputs depend on alone, x[lo - d : hi + d): the mixer is
elementwise and the convolution's terms are the same in the same order, so the
two agree bit for bit (tests/test_isolate_cpu.py pins it) and a short segment of
a long capture costs its own length.
"""
import numpy as np

from oracle import ref

M = 1024                                   # the overlap-save frame


def isolate_full(x, lo, hi, f, h, sr):
    x = np.asarray(x)
    n, d = len(x), (len(h) - 1) // 2
    u = ref.apply_frequency_shift(x.astype(np.complex128), -f, sr)
    return np.convolve(np.r_[u, np.zeros(d)], np.asarray(h).astype(np.float64))[d:d + n][lo:hi].astype(np.complex128)


def isolate(x, lo, hi, f, h, sr):
    """z_s[j], j < hi - lo, complex128."""
    x = np.asarray(x)
    n, T = len(x), len(h)
    d = (T - 1) // 2
    a, b = max(0, lo - d), min(n, hi + d)
    u = x[a:b].astype(np.complex128)
    if f != 0:                                           # apply_frequency_shift(., -f, sr) on the indices a .. b
        t = np.arange(a, b) / sr
        u = (u * np.exp(2j * np.pi * -f * t)).astype(np.complex64)
    u = np.r_[np.zeros(a - (lo - d)), u, np.zeros(hi + d - b)]
    return np.convolve(u, np.asarray(h).astype(np.float64))[T - 1:T - 1 + hi - lo].astype(np.complex128)


def frames(starts, lengths, ntaps):
    """The planner, restated: [(segment, x0, y0, keep)] and the offsets."""
    hop, d = M - (ntaps - 1), (ntaps - 1) // 2
    out, offsets = [], [0]
    for s, (st, ln) in enumerate(zip(starts, lengths)):
        for o in range(0, ln, hop):
            out.append((s, st + o + d - (ntaps - 1), offsets[s] + o, min(hop, ln - o)))
        offsets.append(offsets[s] + ln)
    return out, offsets


def rel_err(got, want):
    """max |got - want| / max |want| (tests/test_gpu_mixfir.py::_close)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    return float(np.abs(got.astype(np.complex128) - want).max() / np.abs(want).max())
