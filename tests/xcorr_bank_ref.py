"""Plain numpy definition of the template bank and the frequency search built
on it (the reference of tests/test_xcorr_bank_cpu.py and
tests/test_gpu_xcorr_bank.py): hypothesis k is np.correlate of the stream with
template k in complex128; the search mixes one reference at K offsets with the
reference's own apply_frequency_shift and takes the first maximum."""
import numpy as np

from oracle import ref

SIGMA = 0.1          # noise per component of planted()


def bank_ref(s, templates, mode):
    """[np.correlate(s, t_k, mode) for k] in complex128, as a (K, nout) array."""
    s = np.asarray(s).astype(np.complex128)
    return np.stack([np.correlate(s, np.asarray(t).astype(np.complex128), mode) for t in templates])


def records_ref(c):
    """(index, peak, sum_abs, sum_abs2) per row of a bank_ref result."""
    a = np.abs(c)
    idx = a.argmax(axis=1)
    return idx, a[np.arange(len(a)), idx], a.sum(axis=1), (a * a).sum(axis=1)


def default_step(sample_rate, Lt):
    """A quarter cycle of mismatch over the template at worst: sinc(1/4) = 0.90."""
    return sample_rate / (2.0 * Lt)


def offset_grid(max_offset, step):
    m = int(np.ceil(max_offset / step))
    return np.arange(-m, m + 1) * step


def hypotheses(reference, offsets, sample_rate, max_template=4096):
    """The K templates of a search: reference[:Lt] mixed by each offset."""
    t = np.asarray(reference)[:max_template].astype(np.complex64)
    return np.stack([np.asarray(ref.apply_frequency_shift(t, f, sample_rate)).astype(np.complex64)
                     for f in offsets])


def frequency_search_ref(vector, reference, sample_rate, offsets, mode="valid", max_template=4096):
    """(offset_hz, lag, peak, lags[K], peaks[K]): the winner is the first
    maximum of the per-hypothesis peaks; lag as find_correlation_peak's lag axis
    (valid: the index; full: index - (Lt - 1))."""
    offsets = np.asarray(offsets, dtype=np.float64)
    T = hypotheses(reference, offsets, sample_rate, max_template)
    idx, peaks, _, _ = records_ref(bank_ref(vector, T, mode))
    lags = idx - (T.shape[1] - 1) if mode == "full" else idx
    k = int(np.argmax(peaks))
    return offsets[k], int(lags[k]), peaks[k], lags, peaks


def planted(L, n, offsets, k0, pos, seed, sample_rate=56e6):
    """(stream, reference): complex noise of sigma SIGMA per component, plus
    oracle.ref.qpsk_preamble(L, seed=L) mixed by offsets[k0] added at pos."""
    rng = np.random.default_rng(seed)
    s = (SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    p = ref.qpsk_preamble(L, seed=L)
    s[pos:pos + L] += np.asarray(ref.apply_frequency_shift(p, offsets[k0], sample_rate)).astype(np.complex64)
    return s, p
