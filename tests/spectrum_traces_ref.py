"""numpy / scipy statements of the spectrum traces (averaged_spectrum), shared
by test_spectrum_traces_cpu.py and test_gpu_spectrum_traces.py.

  reduce_frames   the three detectors of a stored (nfft, nframes) spectrogram:
                  the mean summed in double, np.max, np.min (a NaN stays)
  traces          the same of accuracy_ref.spectrum in a chosen precision
  welch_mean      scipy.signal.welch(..., average='mean') with the arguments the
                  reference gives scipy.signal.spectrogram and the float32 window
  constant_frames frame m is the constant p_m + 1j q_m, small integers: the one
                  non-zero bin of every frame is exact in fp32
  tiled           a vetted 3-frame input repeated under exact power-of-two gains
  bound           the detectors' error bound from the project's own constants
"""
import numpy as np
import scipy.signal

import accuracy_ref as acc

DETECTORS = ("mean", "max", "min")


def reduce_frames(S):
    """{detector: array[nfft]} of S[nfft, nframes]."""
    S = np.asarray(S)
    return {"mean": S.mean(axis=1, dtype=np.float64), "max": S.max(axis=1), "min": S.min(axis=1)}


def traces(x, window, nperseg, noverlap, nfft, dtype=np.complex128, fftshift=False):
    return reduce_frames(acc.spectrum(x, window, nperseg, noverlap, nfft, dtype, fftshift=fftshift))


def welch_mean(x, fs, window, nperseg, noverlap, nfft):
    w = acc.window32(window, nperseg).astype(np.float64)
    f, p = scipy.signal.welch(np.asarray(x).astype(np.complex128), fs, w, nperseg, noverlap, nfft,
                              detrend=False, return_onesided=False, scaling="spectrum", average="mean")
    return f, p


def constant_frames(nfft, nframes, seed):
    """(x, |a_m|^2): nframes frames of nfft samples, frame m the constant a_m =
    p_m + 1j q_m with p, q integers in [-7, 7], not both 0."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-7, 8, nframes)
    q = rng.integers(-7, 8, nframes)
    p[(p == 0) & (q == 0)] = 3
    a = (p + 1j * q).astype(np.complex64)
    return np.repeat(a, nfft), (p * p + q * q).astype(np.float64)


def tiled(x, reps, seed):
    """x repeated reps times, repetition r times 2 ** g_r, g_r in [-3, 3]
    (exact in fp32: the references' errors scale with the gain)."""
    g = np.random.default_rng(seed).integers(-3, 4, reps)
    return np.concatenate([x * np.float32(2.0 ** int(k)) for k in g]).astype(np.complex64)


def bound(K, S32, S64, want):
    """max |y_d - d(S64)| allowed: max, min and mean are 1-Lipschitz in the sup
    norm, so a detector of a spectrogram within K max|S32 - S64| of S64 is
    within that of the detector of S64; plus one float32 rounding of the
    result."""
    return K * float(np.abs(S32.astype(np.float64) - S64).max()) + 2.0 ** -23 * float(np.abs(want).max())
