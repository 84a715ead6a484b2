"""numpy / scipy restatement of the peak list (vector_amd/csrc/peaks.hip), shared
by the GPU and CPU tests: with m = np.abs(a) widened to float64, the candidates
are the elements at or above the threshold that equal
scipy.ndimage.maximum_filter1d over the +-d window; a candidate i is an
instance iff lo + np.argmax(m[lo:hi+1]) == i."""
import numpy as np
from scipy.ndimage import maximum_filter1d


def ref_peaks(m, thr, d):
    """(indices, values) of the instances of m (float64) by the definition."""
    n = len(m)
    w = min(int(d), n)
    mx = maximum_filter1d(m, 2 * w + 1, mode="constant", cval=-np.inf)
    cand = np.flatnonzero((m == mx) & (m >= thr))
    # a candidate equals its window's maximum, so it is the FIRST maximum iff
    # no equal element lies within d to its left: the previous index holding
    # the same value, from a stable sort
    order = np.argsort(m, kind="stable")
    prev = np.full(n, -1, np.int64)
    same = m[order[1:]] == m[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    keep = cand[(prev[cand] < 0) | (cand - prev[cand] > d)]
    if len(cand) * (2 * w + 1) <= 2e7:           # the literal rule where it is affordable
        lit = [i for i in cand
               if max(0, i - d) + np.argmax(m[max(0, i - d):min(n - 1, i + d) + 1]) == i]
        assert np.array_equal(keep, np.asarray(lit, np.int64))
    return keep.astype(np.int64), m[keep]
