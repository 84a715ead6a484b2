"""The accuracy references and the fp32 engine model of tests/accuracy_ref.py,
without a GPU.  test_gpu_accuracy.py's bounds (K_EXACT, K_ANCHOR times the
complex64 scipy reference's own error) are derived from what is pinned here:

* the model with twiddles rounded once from double stays within 2 x scipy's
  complex64 error, with every twiddle component off by a uniform +-10 ulp (the
  documented worst case of the anchor chains) within 8 x;
* each bound is live: the +-10 ulp model fails the exact-class bound, the
  +-30 ulp model the anchor-class bound, with the model standing in for a
  kernel;
* the references compute what the oracle computes, and the fp32 ones stay
  complex64.
"""
import functools

import numpy as np
import pytest
import scipy.signal

import accuracy_ref as acc
from oracle import ref

SIZES = (64, 1024, 8192, 16384)


@functools.lru_cache(maxsize=None)
def _errors(n, ulp):
    """(rel_rms, max_norm) of scipy's complex64 transform and of the model."""
    x = acc.noise(n, seed=n)
    r = np.fft.fft(x.astype(np.complex128))
    s = acc.dft(x)
    y = acc.model_fft(x, ulp=ulp, seed=n)
    out = (acc.rel_rms(s, r), acc.max_norm(s, r)), (acc.rel_rms(y, r), acc.max_norm(y, r))
    print(f"n={n} ulp={ulp} scipy rms {out[0][0]:.3g} max {out[0][1]:.3g}  "
          f"model rms {out[1][0]:.3g} max {out[1][1]:.3g}  ratios "
          f"{out[1][0] / out[0][0]:.2f} {out[1][1] / out[0][1]:.2f}")
    return out


@pytest.mark.parametrize("n", SIZES)
def test_model_is_a_dft(n):
    x = acc.noise(n, seed=7)
    r = np.fft.fft(x.astype(np.complex128))
    assert acc.max_norm(acc.model_fft(x), r) < 1e-6
    assert acc.model_fft(x).dtype == np.complex64


@pytest.mark.parametrize("n", sorted(acc.PLAN_RADICES))
def test_model_plans_multiply_out(n):
    assert int(np.prod(acc.PLAN_RADICES[n])) == n
    x = acc.noise(n, seed=n)
    assert acc.max_norm(acc.model_fft(x), np.fft.fft(x.astype(np.complex128))) < 1e-6


@pytest.mark.parametrize("n", SIZES)
def test_scipy_complex64_error(n):
    """The floor the bounds scale: about 1e-7 (8e-8 at 64 .. 1.4e-7 at 16384)."""
    (rms, mx), _ = _errors(n, 0)
    assert 5e-8 < rms < 2e-7 and 5e-8 < mx < 3e-7


@pytest.mark.parametrize("n", SIZES)
def test_exact_twiddle_class(n):
    (srms, smax), (rms, mx) = _errors(n, 0)
    assert rms <= 2 * srms and mx <= 2 * smax


@pytest.mark.parametrize("n", SIZES)
def test_anchor_twiddle_class(n):
    (srms, smax), (rms, mx) = _errors(n, 10)
    assert rms <= 8 * srms and mx <= 8 * smax


@pytest.mark.parametrize("n", SIZES)
def test_bounds_are_live(n):
    """The model standing in for a kernel: one class worse fails each K."""
    (srms, smax), (rms10, max10) = _errors(n, 10)
    assert rms10 > acc.K_EXACT * srms and max10 > acc.K_EXACT * smax
    _, (rms30, max30) = _errors(n, 30)
    assert rms30 > acc.K_ANCHOR * srms and max30 > acc.K_ANCHOR * smax


@pytest.mark.parametrize("n", [64, 1024, 2048])
def test_two_level_twiddles_are_exact_class(n):
    """TwLds: one fp32 product of two rounded table entries per twiddle."""
    x = acc.noise(n, seed=n)
    r = np.fft.fft(x.astype(np.complex128))
    s, y = acc.dft(x), acc.model_fft(x, two_level=True)
    assert acc.rel_rms(y, r) <= 2 * acc.rel_rms(s, r) and acc.max_norm(y, r) <= 2 * acc.max_norm(s, r)


@pytest.mark.parametrize("case", sorted(acc.SPECTRUM_SEEDS))
def test_spectrum_inputs_meet_the_derivation(case):
    """On every spectrum input of the GPU test the model of the case's class
    stays within the multiple of scipy's error its K was derived from: rel_rms,
    max-norm and the worst frame."""
    nfft, nperseg, noverlap = case
    _, ulp, limit = acc.spectrum_class(nfft)
    x = acc.spectrum_input(nfft, nperseg, noverlap)
    assert len(x) == nperseg + 2 * (nperseg - noverlap)
    got = acc.spectrum_premise(x, nperseg, noverlap, nfft, ulp)
    print(case, "model multiples (rms, max, frame): %.2f %.2f %.2f" % got)
    assert max(got) <= limit


def test_metrics():
    r = np.array([3.0, 4.0j])
    y = r + np.array([0.0, 0.5])
    assert acc.rel_rms(y, r) == pytest.approx(0.1)
    assert acc.max_norm(y, r) == pytest.approx(0.125)
    assert acc.rel_rms(r.astype(np.complex64), r) == 0.0


@pytest.mark.parametrize("window", ["hann", "blackmanharris"])
@pytest.mark.parametrize("n", [64, 7168, 8192])
def test_window_is_the_library_window(window, n):
    """The kernels get vector_amd.windows' samples rounded to float32: the
    references must multiply by the same values."""
    from vector_amd.windows import get_window
    np.testing.assert_array_equal(acc.window32(window, n), get_window(window, n).astype(np.float32))


@pytest.mark.parametrize("nperseg,noverlap,nfft,shift", [(256, 0, 256, False), (200, 72, 256, False),
                                                         (256, 128, 256, True)])
def test_spectrum_references(nperseg, noverlap, nfft, shift):
    x = ref.synth_iq(3 * nfft + 11, seed=5)
    _, _, R = ref.spectrum(x.astype(np.complex128), 1.0, "hann", nperseg, noverlap, nfft)
    if shift:
        R = np.fft.fftshift(R, axes=0)
    r64 = acc.spectrum(x, "hann", nperseg, noverlap, nfft, np.complex128, fftshift=shift)
    r32 = acc.spectrum(x, "hann", nperseg, noverlap, nfft, fftshift=shift)
    assert r64.shape == R.shape and r32.dtype == np.float32
    # scipy's float64 window against its float32 rounding: 2^-24 per sample
    assert acc.max_norm(r64, R) < 3e-7
    assert 1e-8 < acc.rel_rms(r32, r64) < 5e-7


@pytest.mark.parametrize("decim", [1, 3])
def test_fir_references(decim):
    x = ref.synth_iq(3000, seed=6)
    taps = scipy.signal.firwin(255, 0.2)
    want = ref.fir_filter(x.astype(np.complex128), taps.astype(np.float32).astype(np.float64), decim)
    r64 = acc.fir(x, taps, decim, np.complex128)
    assert acc.max_norm(r64, want) < 1e-13
    assert acc.max_norm(acc.fir_direct(x, taps, decim), want) < 1e-15
    r32 = acc.fir(x, taps, decim)
    assert r32.dtype == np.complex64 and 1e-8 < acc.rel_rms(r32, r64) < 5e-7


def test_correlate_references():
    s = ref.synth_iq(5000, seed=8)
    t = ref.qpsk_preamble(700)
    want = np.correlate(s.astype(np.complex128), t.astype(np.complex128), "valid")
    r64 = acc.correlate_valid(s, t, np.complex128)
    assert r64.shape == want.shape and acc.max_norm(r64, want) < 1e-13
    r32 = acc.correlate_valid(s, t)
    assert r32.dtype == np.complex64 and 1e-8 < acc.rel_rms(r32, r64) < 5e-7


@pytest.mark.parametrize("C,P,cut", [(64, 4, 0), (128, 16, 1)])
def test_pfb_references(C, P, cut):
    proto = scipy.signal.firwin(P * C, 1.0 / C).astype(np.float32)
    x = ref.synth_iq((20 + P - 1) * C - cut, seed=9)
    want = ref.pfb_channelize(x, proto, C)                 # complex128, stored as complex64
    r64 = acc.pfb(x, proto, C, np.complex128)
    assert r64.shape == want.shape == (C, 20 - cut)
    assert acc.max_norm(r64, want) < 2e-7
    r32 = acc.pfb(x, proto, C)
    assert r32.dtype == np.complex64 and 1e-8 < acc.rel_rms(r32, r64) < 5e-7


@pytest.mark.parametrize("n", [1000, 12_289])
def test_dft_references(n):
    x = ref.synth_iq(n, seed=n)
    for inv in (False, True):
        r64 = acc.dft(x, inv, np.complex128)
        want = (np.fft.ifft if inv else np.fft.fft)(x.astype(np.complex128))
        assert acc.max_norm(r64, want) < 1e-13
        r32 = acc.dft(x, inv)
        assert r32.dtype == np.complex64 and 1e-8 < acc.rel_rms(r32, r64) < 5e-7
