"""CPU checks of the line traces: the numpy restatement (tests/trace_ref.py)
against numpy's own expressions at the reference's plot sites, the x axes of
signal_envelope / capture_spectrum, trace_bin, and every argument error, which
is raised before any device work (none of this needs a GPU)."""
import numpy as np
import pytest

import trace_ref as tr
from oracle import ref

LENGTHS = (1, 2, 7, 1000, 65_537)


def spectrum(n):
    """A float32-precision transform of synth_iq."""
    return np.fft.fft(ref.synth_iq(n, seed=n)).astype(np.complex64)


# ---------------------------------------------------------------------------
# the restatement against the sites' expressions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4097, 8192, 65_537])
def test_restatement_is_the_sites_line(n):
    """bin = 1: the line of every spectrum site; bin > 1: np.min / np.max of
    that line per column -- also for the dB lines, where the restatement maps
    the envelope and numpy maps every element ("map, then min / max" equals
    "min / max, then map" bit for bit: + eps and log10 are monotone)."""
    X = spectrum(n)
    with np.errstate(divide="ignore"):
        sites = {
            ("db", 0.0, False, False): 20 * np.log10(np.abs(X)),                        # spectrogram_analysis.py
            ("linear", 0.0, True, False): np.fft.fftshift(np.abs(X)),                   # analyze_vectors.py
            ("db", 0.0, True, False): 20 * np.log10(np.fft.fftshift(np.abs(X))),        # display_vectors.py
            ("db", 1e-12, True, False): 20 * np.log10(np.abs(np.fft.fftshift(X)) + np.float32(1e-12)),
        }
    m = sites[("db", 1e-12, True, False)]
    sites[("db", 1e-12, True, True)] = m - np.max(m)                                    # mat_analyzer.py
    for (scale, eps, shift, normalize), want in sites.items():
        assert want.dtype == np.float32
        got = tr.spectrum_line(X, scale, eps, shift, normalize)
        assert np.array_equal(got, want)
        kind = tr.DB20 if scale == "db" else tr.ABS
        for bin_ in (1, 7, 300):
            emin, emax, info = tr.restate(X, shift, 0, n, bin_, kind, eps)
            line = m if normalize else want                 # the envelope is taken before the subtraction
            for c, (a, b) in enumerate(tr.columns(line, 0, n, bin_)):
                assert emin[c] == np.min(line[a:b]) and emax[c] == np.max(line[a:b])
            if bin_ == 1:
                assert np.array_equal(emin, line) and np.array_equal(emax, line)
            assert info[1] == np.argmax(line) and info[3] == np.max(line)
            assert info[0] == np.argmin(line) and info[2] == np.min(line)


def test_restatement_band_and_window():
    """analyze_vectors.py:28: the masked line is a window of the shifted one."""
    n, sr, fc = 1000, 56e6, 5.2e9
    X = spectrum(n)
    f = np.fft.fftshift(np.fft.fftfreq(n, 1 / sr)) + fc
    mask = (f >= fc - 7e6) & (f <= fc + 3e6)
    want = np.fft.fftshift(np.abs(X))[mask]
    lo, hi = int(np.argmax(mask)), int(n - np.argmax(mask[::-1]))
    assert np.array_equal(tr.restate(X, True, lo, hi, 1)[1], want)
    emin, emax, info = tr.restate(X, True, lo, hi, 7)
    assert len(emax) == -(-(hi - lo) // 7)
    assert emax[-1] == want[(len(want) - 1) // 7 * 7:].max() and emin[0] == want[:7].min()
    assert info[1] == lo + np.argmax(want)


def test_restatement_time_line_and_nan():
    x = ref.synth_iq(1000, seed=3)
    assert np.array_equal(tr.restate(x, False, 100, 900, 1)[1], np.abs(x)[100:900])
    x[250] = np.nan
    emin, emax, _ = tr.restate(x, False, 0, 1000, 100)
    assert np.isnan(emin[2]) and np.isnan(emax[2])
    assert not np.isnan(np.delete(emax, 2)).any() and not np.isnan(np.delete(emin, 2)).any()


def test_fftshift_is_a_rotation_by_half_rounded_up():
    for n in LENGTHS:
        m = np.arange(n)
        assert np.array_equal(np.fft.fftshift(m), m[(np.arange(n) + (n + 1) // 2) % n])


# ---------------------------------------------------------------------------
# the axes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bin_", [1, 7])
@pytest.mark.parametrize("n", LENGTHS)
def test_axes_equal_numpys(n, bin_):
    from vector_amd import traces
    for sr, fc in ((56e6, 0.0), (61.44e6, 5.23e9), (3, 0.1)):
        for shift in (True, False):
            want = tr.freq_axis(n, sr, fc, shift)
            got = traces.spectrum_axis(n, sr, fc, shift, 0, n, bin_)
            assert got.dtype == np.float64 and np.array_equal(got, want[::bin_])
            lo, hi = n // 3, n - n // 5
            assert np.array_equal(traces.spectrum_axis(n, sr, fc, shift, lo, hi, bin_), want[lo:hi:bin_])
        t = np.arange(n) / sr
        lo, hi = n // 4, n - n // 7
        got = traces.time_axis(lo, hi, bin_, sr)
        assert got.dtype == np.float64 and np.array_equal(got, t[lo:hi:bin_])
    got = traces.time_axis(0, n, bin_, None)
    assert got.dtype == np.float64 and np.array_equal(got, np.arange(n)[::bin_])


def test_band_window_is_the_mask():
    from vector_amd import traces
    for n in (1, 2, 7, 1000):
        for sr, fc in ((56e6, 5.2e9), (1.0, 0.0)):
            val = 1.0 / (n * (1 / sr))
            f = tr.freq_axis(n, sr, fc, True)
            for band in ((fc - sr / 7, fc + sr / 9), (f[0], f[-1]), (f[n // 2], f[n // 2]),
                         (fc + sr, fc + 2 * sr), (fc + 1.0, fc - 1.0), (-np.inf, np.inf)):
                lo, hi = traces._band_window(n, val, fc, band)
                mask = (f >= band[0]) & (f <= band[1])
                assert max(hi - lo, 0) == mask.sum()
                if mask.any():
                    assert mask[lo:hi].all()


def test_trace_bin():
    from vector_amd import trace_bin
    assert trace_bin(1000, None) == 1
    assert trace_bin(1000, 2000) == 1 and trace_bin(1000, 1000) == 1
    assert trace_bin(1000, 999) == 2 and trace_bin(1000, 3) == 334 and trace_bin(1000, 1) == 1000
    assert trace_bin(0, 5) == 1
    assert trace_bin(1 << 28, 2048) == 1 << 17
    for bad in (0, -3):
        with pytest.raises(ValueError):
            trace_bin(1000, bad)


# ---------------------------------------------------------------------------
# argument errors: raised before any device work
# ---------------------------------------------------------------------------
def test_argument_errors_need_no_device(monkeypatch):
    import vector_amd as va
    from vector_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(_lib, "get_context", no_device)
    x = ref.synth_iq(64, seed=1)
    for kw in (dict(max_points=0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            va.signal_envelope(x, 56e6, **kw)
        with pytest.raises(ValueError):
            va.capture_spectrum(x, 56e6, **kw)
    with pytest.raises(ValueError):
        va.signal_envelope(x.reshape(8, 8))
    with pytest.raises(ValueError):
        va.capture_spectrum(x.reshape(8, 8), 56e6)
    with pytest.raises(ValueError):
        va.capture_spectrum(x, 56e6, scale="power")
    with pytest.raises(ValueError):
        va.capture_spectrum(x, 56e6, scale="linear", normalize=True)
    with pytest.raises(ValueError):
        va.capture_spectrum(x, 56e6, shift=False, band=(-1e6, 1e6))
    with pytest.raises(ValueError):
        va.capture_spectrum(x[:0], 56e6)
    with pytest.raises(ValueError):
        np.fft.fft(x[:0])                                   # the behaviour it mirrors


def test_empty_traces_need_no_device(monkeypatch):
    import vector_amd as va
    from vector_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("device work for an empty trace")
    monkeypatch.setattr(_lib, "get_context", no_device)
    x = ref.synth_iq(64, seed=1)
    for t in (va.signal_envelope(x[:0], 56e6), va.signal_envelope(x, 56e6, start=40, stop=40),
              va.signal_envelope(x, start=50, stop=10, max_points=4),
              va.capture_spectrum(x, 56e6, band=(60e6, 70e6)), va.capture_spectrum(x, 56e6, band=(1e6, -1e6))):
        assert isinstance(t, va.Trace)
        assert t.x.dtype == np.float64 and len(t.x) == 0
        assert t.lo.dtype == np.float32 and len(t.lo) == 0 and t.lo is t.hi
        assert t.argmax == -1 and np.isnan(t.max)
    assert va.signal_envelope(x.astype(np.complex128)[:0]).lo.dtype == np.float64
