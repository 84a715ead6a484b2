"""The run list's reference (vsig_runs_dev, vector_amd.find_runs /
detect_packets), in numpy: the runs of m >= thr with dropouts of up to max_gap
elements bridged, and the same definition as the per-index rule the kernels
evaluate."""
import math

import numpy as np


def runs_ref(m, thr, max_gap):
    """(start, end) int64 arrays, end inclusive."""
    idx = np.flatnonzero(np.asarray(m) >= thr)
    if idx.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    brk = np.flatnonzero(np.diff(idx) > max_gap + 1)
    start = idx[np.r_[0, brk + 1]]
    end = idx[np.r_[brk, idx.size - 1]]
    return start.astype(np.int64), end.astype(np.int64)


def runs_by_rule(mask, max_gap):
    """The per-index rule, element by element: a masked i is a start iff the
    previous masked index p (or -inf) has i - p > max_gap + 1, an end iff the
    next masked index q (or +inf) has q - i > max_gap + 1."""
    n = len(mask)
    starts, ends = [], []
    for i in range(n):
        if not mask[i]:
            continue
        p = next((j for j in range(i - 1, -1, -1) if mask[j]), -math.inf)
        q = next((j for j in range(i + 1, n) if mask[j]), math.inf)
        if i - p > max_gap + 1:
            starts.append(i)
        if q - i > max_gap + 1:
            ends.append(i)
    return np.asarray(starts, np.int64), np.asarray(ends, np.int64)


def run_stats(m, start, end):
    """(argmax, max, fsum) of float64 m over each [start, end]."""
    am = np.asarray([s + int(np.argmax(m[s:e + 1])) for s, e in zip(start, end)], np.int64)
    mx = np.asarray([m[i] for i in am], np.float64)
    sums = np.asarray([math.fsum(m[s:e + 1]) for s, e in zip(start, end)], np.float64)
    return am, mx, sums
