"""CPU-only checks of the spectrum traces: the numpy helper the GPU tests
compare with is scipy's Welch mean and numpy's max / min of the stored
spectrogram, and averaged_spectrum's argument errors come before any device
call."""
import numpy as np
import pytest

import accuracy_ref as acc
import spectrum_traces_ref as st
from oracle import ref


@pytest.mark.parametrize("nperseg,noverlap,nfft", [(256, 0, 256), (200, 150, 256), (1000, 0, 1000)])
def test_helper_is_welch_mean_and_numpy_extrema(nperseg, noverlap, nfft):
    x = ref.synth_iq(9 * nperseg + 17, seed=nfft + nperseg)
    got = st.traces(x, "hann", nperseg, noverlap, nfft, np.complex128)
    f, want = st.welch_mean(x, 2.5e6, "hann", nperseg, noverlap, nfft)
    assert np.array_equal(f, np.fft.fftfreq(nfft, 1 / 2.5e6))
    assert got["mean"].dtype == np.float64
    assert np.abs(got["mean"] - want).max() <= 1e-12 * np.abs(want).max()
    S = acc.spectrum(x, "hann", nperseg, noverlap, nfft, np.complex128)
    assert S.shape[1] == (len(x) - nperseg) // (nperseg - noverlap) + 1 > 3
    assert np.array_equal(got["max"], np.max(S, axis=1)) and np.array_equal(got["min"], np.min(S, axis=1))
    assert np.all(got["min"] <= got["mean"]) and np.all(got["mean"] <= got["max"])


def test_helper_nan_and_inputs():
    S = np.array([[1.0, np.nan, 3.0], [1.0, 2.0, 4.0]], np.float32)
    r = st.reduce_frames(S)
    assert np.isnan(r["mean"][0]) and np.isnan(r["max"][0]) and np.isnan(r["min"][0])
    assert (r["mean"][1], r["max"][1], r["min"][1]) == (7.0 / 3.0, 4.0, 1.0)
    x, p2 = st.constant_frames(64, 7, seed=1)
    assert x.dtype == np.complex64 and len(x) == 7 * 64 and np.all(p2 > 0)
    a = x[::64].astype(np.complex128)
    assert np.array_equal(a.real ** 2 + a.imag ** 2, p2) and np.all(x.reshape(7, 64) == x[::64, None])
    t = st.tiled(x, 3, seed=2)
    assert t.dtype == np.complex64 and len(t) == 3 * len(x)
    g = np.random.default_rng(2).integers(-3, 4, 3)
    for r in range(3):
        assert np.array_equal(t[r * len(x):(r + 1) * len(x)], x * np.float32(2.0 ** int(g[r])))


def test_argument_errors_need_no_device():
    """spectrum()'s ValueErrors and the detector check, all raised before the
    library or a device is asked for (this machine may have neither)."""
    import vector_amd as va
    x = np.zeros(1000, np.complex64)
    with pytest.raises(ValueError, match="nfft must be greater than or equal to nperseg"):
        va.averaged_spectrum(x, nperseg=256, nfft=128)
    with pytest.raises(ValueError, match="noverlap must be less than nperseg"):
        va.averaged_spectrum(x, nperseg=256, noverlap=256)
    with pytest.raises(ValueError, match="window is longer than input signal"):
        va.averaged_spectrum(x, window=np.ones(2000))
    with pytest.raises(ValueError, match="1-D"):
        va.averaged_spectrum(np.zeros((4, 256), np.complex64), nperseg=256)
    with pytest.raises(ValueError, match="unknown detector"):
        va.averaged_spectrum(x, nperseg=256, detectors=("mean", "median"))
    with pytest.raises(ValueError, match="no detector"):
        va.averaged_spectrum(x, nperseg=256, detectors=())
    e = va.averaged_spectrum(np.zeros(0, np.complex64), detectors=("max",))
    assert isinstance(e, va.SpectrumTraces) and e.nframes == 0 and e.max.size == 0 and e.mean is None
    for bad in (dict(detector="median"), dict(scale="power"), dict(eps=-1.0), dict(normalize=True, scale="linear"),
                dict(max_points=0)):
        with pytest.raises(ValueError):
            va.averaged_spectrum_trace(x, 1e6, **bad)
    with pytest.raises(ValueError):
        va.averaged_spectrum_trace(np.zeros(0, np.complex64), 1e6)
    with pytest.raises(ValueError):
        va.averaged_spectrum_trace(x, 0.0)
