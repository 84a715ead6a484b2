"""The fp32 accuracy floor of test_gpu_accuracy.py on the engine's other routes:
transforms of any length (vsig_dft_dev: the direct sum up to 512 points, the
four-step transform of a power of two above 16384, chirp-z for everything else
that is no power of two), long and odd spectrum frames, resample_signal,
filter_channel on both of its routes, the two NCO mixers at sample offsets past
2^31 and 2^32, filters over 8192 taps and np.correlate's 'full' / 'same' modes.

The rule is the same: with r128 the complex128 reference and r32 the same
operation on the same rounded operands in complex64 scipy (accuracy_ref.py),

    rel_rms(gpu, r128) <= K * rel_rms(r32, r128)
    max_norm(gpu, r128) <= K * max_norm(r32, r128)

over the case and for each frame where there are frames; K_EXACT = 3 for all of
bigfft.hip (tables rounded once from double, one extra fp32 product in the
four-step twiddle), K_ANCHOR = 8 for the FIR and correlator kernels.  Every
figure is printed as an ``ACC`` line (pytest -s) before it is asserted.
"""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import accuracy_ref as acc
from accuracy_ref import K_ANCHOR, K_EXACT
from oracle import ref

pytestmark = pytest.mark.gpu

_floor, _say = acc.floor, acc.say


# ---------------------------------------------------------------------------
# 1. vsig_dft_dev
# ---------------------------------------------------------------------------
def _dft(gpu, x, inverse=False, batch=1, c128=False):
    from vector_amd import _lib
    ctx = gpu.get_context()
    dt, code = (np.complex128, _lib.DTYPES["c128"]) if c128 else (np.complex64, _lib.DTYPES["c64"])
    t = torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    y = torch.empty_like(t)
    ctx.check(ctx.lib.vsig_dft_dev(ctx.h, code, gpu.dsp._ptr(t), t.numel() // batch, batch,
                                   1 if inverse else 0, code, gpu.dsp._ptr(y)), "dft")
    return y.cpu().numpy()


DFT_SIZES = [
    1, 2, 64, 128,                  # below the smallest plan: the direct sum in double
    255, 257,                       # either side of 256 (a plan): the direct sum
    511, 513,                       # the last direct sum, the first chirp-z (in LDS, M = 2048)
    16383,                          # chirp-z at M = 32768: the first four-step size (N1 = 64, N2 = 512)
    1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 20,   # one four-step transform, row plans 512 .. 16384
    1 << 21,                        # N1 = 128
    20_000, (1 << 17) + 1,          # four-step chirp-z, M = 65536 / 2^19
]
# chirp-z lengths bounded against the chirp-z composite in complex64 scipy
# (acc.chirpz at the route's own M) instead of pocketfft's one mixed-radix
# transform of that length: three transforms and two chirp products against one.
# 3000 = 2^3 3 5^3 (batched case): pocketfft's max-norm error there is 3.5e-8,
# a quarter of its rel_rms; every other smooth length held against plain scipy.
DFT_COMPOSITE = {3000}


def _pow2(n):
    return n & (n - 1) == 0


@functools.lru_cache(maxsize=4)
def _dft_refs(n, inverse):
    x = ref.synth_iq(n, seed=n)
    return x, acc.dft(x, inverse), acc.dft(x, inverse, np.complex128)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", DFT_SIZES)
def test_dft_route_floor(gpu, n, inverse):
    """Measured on an MI355X (ratio = e_gpu / e_ref, m_ratio the max-norm's):
    one four-step transform at 2^15 .. 2^21: ratio 0.95 .. 1.09, m_ratio
    0.64 .. 2.45 (as a chirp-z before: 1.85 .. 2.31 and 2.22 .. 6.87);
    chirp-z at 16383, 20 000, 2^17 + 1: ratio 0.92 .. 1.72, m_ratio
    1.27 .. 2.13; the direct sum in double at 64, 128, 255, 257: ratio
    0.12 .. 0.46, m_ratio 0.32 .. 0.90.

    Those four ran as chirp-z too (M = 256 .. 1024) until this test: 257
    points forward then sat at m_gpu 2.19e-7 against m_ref 6.21e-8, 3.53 x
    (rel_rms 1.05 x; 64 points at 2.40 x) -- the figure the chirp-z gives with
    the engine's exact-twiddle CPU model as its 1024-point transform
    (test_accuracy_cpu.test_chirpz_model_at_257_points): the engine's error in
    a dominant bin, taken three times.  dft_any now sums every length up to 512
    points that has no plan directly in double (bf_direct_kernel)."""
    x, r32, r64 = _dft_refs(n, inverse)
    y = _dft(gpu, x, inverse)
    assert y.dtype == np.complex64
    case = f"dft n={n} inverse={int(inverse)}"
    if n <= 2:                       # scipy's complex64 error is 0: so must the kernel's be
        _say(case, e_ref=acc.rel_rms(r32, r64), e_gpu=acc.rel_rms(y, r64))
        np.testing.assert_array_equal(y, r64.astype(np.complex64))
        return
    if not _pow2(n):                 # the composite's figures beside scipy's, whichever bounds
        rc = acc.chirpz(x, acc.chirpz_size(n), inverse)
        _say(case + " chirpz-composite", e_ref=acc.rel_rms(rc, r64), m_ref=acc.max_norm(rc, r64))
        if n in DFT_COMPOSITE:
            r32 = rc
    _floor(case, y, r32, r64, K_EXACT)


@pytest.mark.parametrize("n", [1 << 15, 3000])
def test_dft_batched_floor(gpu, n):
    """Three frames, each bounded on its own (a wrong second frame cannot hide)."""
    b = 3
    x = ref.synth_iq(n * b, seed=n + b).reshape(b, n)
    r32 = np.stack([acc.dft(f) for f in x])
    r64 = np.stack([acc.dft(f, False, np.complex128) for f in x])
    y = _dft(gpu, x.ravel(), batch=b).reshape(b, n)
    if not _pow2(n):
        rc = np.stack([acc.chirpz(f, acc.chirpz_size(n)) for f in x])
        for f in range(b):
            _say(f"dft-batched n={n} frame={f} scipy", e_ref=acc.rel_rms(r32[f], r64[f]),
                 m_ref=acc.max_norm(r32[f], r64[f]))
        if n in DFT_COMPOSITE:
            r32 = rc
    for f in range(b):
        _floor(f"dft-batched n={n} frame={f}", y[f], r32[f], r64[f], K_EXACT)


def test_dft_complex128_io(gpu):
    """complex128 in and out (converted at the loads and stores): the same
    transform, the same bound."""
    n = 1 << 15
    x, r32, r64 = _dft_refs(n, False)
    y = _dft(gpu, x.astype(np.complex128), c128=True)
    assert y.dtype == np.complex128
    _floor(f"dft-c128 n={n}", y, r32, r64, K_EXACT)
    yi = _dft(gpu, x.astype(np.complex128), inverse=True, c128=True)
    _floor(f"dft-c128 n={n} inverse=1", yi, acc.dft(x, True), acc.dft(x, True, np.complex128), K_EXACT)


def _impulse(n, j):
    x = np.zeros(n, np.complex64)
    x[j] = 1
    return x


@pytest.mark.parametrize("n", [1 << 15, 1 << 16])
def test_impulse_dft_fourstep(gpu, n):
    """Every bin has modulus 1: element-wise, K 2^-24 sqrt(log2 n)."""
    bound = K_EXACT * 2.0 ** -24 * np.sqrt(np.log2(n))
    k = np.arange(n)
    worst = {}
    for j in (0, 1, n // 2 - 1, n - 1):
        want = np.exp(-2j * np.pi * ((j * k) % n) / n)
        worst[f"j{j}"] = np.abs(_dft(gpu, _impulse(n, j)).astype(np.complex128) - want).max()
    _say(f"impulse-dft n={n}", bound=bound, **worst)
    assert max(worst.values()) <= bound, worst


# ---------------------------------------------------------------------------
# 3. long and odd spectrum frames
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _long_spectrum_refs(nfft, nperseg, noverlap, stride, shift):
    x = acc.route_spectrum_input(nfft, nperseg, noverlap, stride)
    xs = x[::stride]
    r32 = acc.spectrum(xs, "hann", nperseg, noverlap, nfft, fftshift=shift)
    r64 = acc.spectrum(xs, "hann", nperseg, noverlap, nfft, np.complex128, fftshift=shift)
    assert r32.shape == (nfft, 3)
    return x, r32, r64


@pytest.mark.parametrize("nfft,nperseg,hop,shift", [
    (32768, 32768, 32768, False),
    (65536, 40_000, 10_000, False),     # zero fill and overlap
    (32768, 32768, 32768, True),        # fftshift in the row pass's store
])
def test_spectrum_long_frames_floor(gpu, nfft, nperseg, hop, shift):
    """One four-step transform per frame (bf_col -> bf_row MODE 2), 3 frames."""
    x, r32, r64 = _long_spectrum_refs(nfft, nperseg, nperseg - hop, 1, shift)
    _, _, S = gpu.spectrum(x, 1.0, "hann", nperseg, nperseg - hop, nfft, fftshift=shift)
    assert S.dtype == np.float32 and S.shape == r64.shape
    _floor(f"spectrum nfft={nfft} nperseg={nperseg} hop={hop} shift={int(shift)}", S, r32, r64,
           K_EXACT, frame_axis=1)


@pytest.mark.parametrize("nfft,nperseg,shift", [
    (1000, 1000, False),                # chirp-z in LDS, M = 2048
    (12_000, 9000, False),              # M = 32768: four-step chirp-z, zero fill
    (1000, 1000, True),                 # odd / even placement of nout / 2
    (1001, 1001, True),
])
def test_spectrum_any_nfft_floor(gpu, nfft, nperseg, shift):
    """Bluestein per frame on noise (the CPU model of the plans does not cover
    a chirp-z, so no seed is chosen by it), 3 frames.  Held against plain scipy
    (ratio 1.9 .. 2.1, m_ratio 1.3 .. 2.2); no composite reference needed."""
    x = acc.noise(3 * nperseg, seed=nfft + nperseg)
    r32 = acc.spectrum(x, "hann", nperseg, 0, nfft, fftshift=shift)
    r64 = acc.spectrum(x, "hann", nperseg, 0, nfft, np.complex128, fftshift=shift)
    case = f"spectrum nfft={nfft} nperseg={nperseg} shift={int(shift)}"
    _, _, S = gpu.spectrum(x, 1.0, "hann", nperseg, 0, nfft, fftshift=shift)
    assert S.dtype == np.float32 and S.shape == r64.shape == (nfft, 3)
    _floor(case, S, r32, r64, K_EXACT, frame_axis=1)


@pytest.mark.parametrize("stride", [2, 3])
@pytest.mark.parametrize("nfft", [8192, 32768])
def test_spectrum_stride_floor(gpu, nfft, stride):
    """vsig_psd_c64_dev's element stride (create_spectrogram's sig[::factor] on
    a device tensor): the reference is taken on x[::stride]."""
    x, r32, r64 = _long_spectrum_refs(nfft, nfft, 0, stride, False)
    xd = torch.from_numpy(x).cuda()
    _, _, S = gpu.spectrum(xd, 1.0, "hann", nfft, 0, nfft, _stride=stride, _nsamples=len(x[::stride]))
    S = S.cpu().numpy()
    assert S.shape == r64.shape
    _floor(f"spectrum nfft={nfft} stride={stride}", S, r32, r64, acc.route_spectrum_class(nfft)[0],
           frame_axis=1)


def _tones(nfft, second=0.0):
    """exp(2 pi i k1 n / nfft), k1 = nfft / 8, 3 frames; plus `second` times a
    tone at k2 = 3 nfft / 8."""
    n = np.arange(3 * nfft)
    k1, k2 = nfft // 8, 3 * nfft // 8
    x = np.exp(2j * np.pi * ((k1 * n) % nfft) / nfft)
    if second:
        x = x + second * np.exp(2j * np.pi * ((k2 * n) % nfft) / nfft)
    return x.astype(np.complex64), k1, k2


def _tone_floor_db(P, k1, nfft):
    """(median, maximum) power in dB relative to the peak bin over the bins
    more than 4 away from the tone, all frames."""
    d = (np.arange(nfft) - k1 + nfft // 2) % nfft - nfft // 2
    rel = P[np.abs(d) > 4].astype(np.float64) / P[k1].astype(np.float64)[None, :]
    with np.errstate(divide="ignore"):
        return 10 * np.log10(np.median(rel)), 10 * np.log10(rel.max())


def test_tone_floor_long_frame(gpu):
    """test_gpu_accuracy.test_tone_floor at nfft = 32768: the four-step
    transform's noise at most 20 dB above the complex64 reference's."""
    nfft = 32768
    x, k1, _ = _tones(nfft)
    r32 = acc.spectrum(x, "blackmanharris", nfft, 0, nfft)
    _, _, S = gpu.spectrum(x, 1.0, "blackmanharris", nfft, 0, nfft)
    assert np.all(S.argmax(axis=0) == k1)
    med_ref, max_ref = _tone_floor_db(r32, k1, nfft)
    med_gpu, max_gpu = _tone_floor_db(S, k1, nfft)
    _say(f"tone nfft={nfft}", med_ref_db=med_ref, med_gpu_db=med_gpu, max_ref_db=max_ref,
         max_gpu_db=max_gpu)
    assert med_gpu <= med_ref + 20 and max_gpu <= max_ref + 20


def test_two_tones_long_frame(gpu):
    """A line 80 dB under the carrier reads within 0.05 dB of its complex128 value."""
    nfft = 32768
    x, k1, k2 = _tones(nfft, second=1e-4)
    r64 = acc.spectrum(x, "blackmanharris", nfft, 0, nfft, np.complex128)
    _, _, S = gpu.spectrum(x, 1.0, "blackmanharris", nfft, 0, nfft)
    want = 10 * np.log10(r64[k2] / r64[k1])
    got = 10 * np.log10(S[k2].astype(np.float64) / S[k1].astype(np.float64))
    dev = np.abs(got - want).max()
    _say(f"two-tones nfft={nfft}", want_db=want[0], dev_db=dev)
    assert np.all(np.abs(want + 80) < 0.01)
    assert dev <= 0.05


# ---------------------------------------------------------------------------
# 4. resample_signal and filter_channel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,num", [
    (4096, 2048),           # two plans of their own
    (5000, 2500),           # chirp-z in LDS, both ways
    (5000, 14_000),         # in LDS forward, four-step chirp-z (M = 32768) back
    (65_536, 32_768),       # two four-step transforms
    (50_000, 35_714),       # four-step chirp-z, both ways
])
def test_resample_floor(gpu, n, num):
    """Every case held against plain scipy (ratio 0.96 .. 2.3, m_ratio
    0.84 .. 2.7 with both transforms as chirp-z); no composite reference needed."""
    x = ref.synth_iq(n, seed=n + num)
    a, b = float(n), float(num)
    assert int(n * (b / a)) == num
    r32, r64 = acc.resample(x, num), acc.resample(x, num, np.complex128)
    case = f"resample {n}->{num}"
    y = gpu.resample_signal(x, a, b)
    assert y.dtype == np.complex64 and y.shape == (num,)
    _floor(case, y, r32, r64, K_EXACT)


def test_resample_real_input_floor(gpu):
    n, num = 4096, 10_240
    x = np.cos(0.01 * np.arange(n)).astype(np.float32)
    r32 = acc.resample(x, num, real_input=True)
    r64 = acc.resample(x, num, np.complex128, real_input=True)
    y = gpu.resample_signal(x, 10.0, 25.0)
    assert y.shape == (num,) and np.all(y.imag == 0)
    case = f"resample-real {n}->{num}"
    _floor(case, y, r32, r64, K_EXACT)


def _kept_bins(n, cf, sr, bw):
    """nk of vsig_filter_channel_dev: the kept non-negative bins k < n / 2 of
    the reference's axis fftfreq(n, 1 / sr) * sr + CENTER_FREQ."""
    return int(acc.channel_mask(n, cf, sr, bw)[:n // 2].sum())


# The FFT route is taken for nk * n > 2^32.  The reference's axis has its extra
# * sr, so bin k sits at CENTER + k sr^2 / n: at sr = 56e6 the spacing is 2.4e10
# Hz and a 60 MHz band keeps bin 0 alone (nk * n = n: the direct route).  Every
# non-negative bin is kept only while (n / 2) sr^2 / n <= bw / 2, i.e.
# sr <= sqrt(60e6) = 7746: at sr = 5600, nk = n / 2 = 65 536 and
# nk * n = 8.6e9 > 2^32.  Both rates are run; the test states which route each
# takes from nk * n.
@pytest.mark.parametrize("sr", [56e6, 5600.0])
@pytest.mark.parametrize("n", [131_072, 131_070])
def test_filter_channel_wide_band_floor(gpu, n, sr):
    cf, bw = 5230e6, 60e6
    x = ref.synth_iq(n, seed=n)
    nk = _kept_bins(n, cf, sr, bw)
    fft_route = nk * n > 1 << 32
    assert fft_route == (sr == 5600.0) and nk == (n // 2 if fft_route else 1)
    r32 = acc.filter_channel(x, cf, sr, bw)
    r64 = acc.filter_channel(x, cf, sr, bw, np.complex128)
    y = gpu.filter_channel(x, cf, sr, bw)
    assert y.dtype == np.float64 and y.shape == (n,)
    _floor(f"filter_channel n={n} sr={sr:g} nk*n={nk * n:.3g} route={'fft' if fft_route else 'direct'}",
           y, r32, r64, K_EXACT)


def test_filter_channel_direct_route(gpu):
    """sr = 4000: bins 800 Hz apart, 1251 kept, nk * n = 2.5e7 <= 2^32: sums in
    double.  Two correct summation orders in double differ by a small multiple
    of d, the error of
    numpy's double FFT route against the np.longdouble sum (at 512 of the
    20 000 output samples, 2.56 %): 8 d, the headroom of K_ANCHOR."""
    p = acc.CHANNEL_DIRECT
    x, idx, L, d = acc.channel_direct_refs()
    assert _kept_bins(p["n"], p["cf"], p["sr"], p["bw"]) * p["n"] == 1251 * 20_000 <= 1 << 32
    y = gpu.filter_channel(x, p["cf"], p["sr"], p["bw"])
    e = float(np.abs(y[idx].astype(np.longdouble) - L).max() / np.abs(L).max())
    _say("filter_channel direct n=20000", d=d, e_gpu=e, ratio=e / d)
    assert e <= 8 * d


@pytest.mark.parametrize("n,sr", [(20_000, 800.0), (131_072, 5600.0)])
def test_filter_channel_empty_band(gpu, n, sr):
    """A band that keeps no bin gives exact zeros (whatever the band's width
    would have chosen as the route)."""
    x = ref.synth_iq(n, seed=n + 1)
    for cf, bw in ((5230e6 - 5e6, 2e6), (5230e6 + 0.5 * sr * sr / n, 0.1 * sr * sr / n)):
        assert _kept_bins(n, cf, sr, bw) == 0
        y = gpu.filter_channel(x, cf, sr, bw)
        assert y.shape == (n,) and not np.any(y)
        assert not np.any(ref.filter_channel(x, cf, sr, bw))


# ---------------------------------------------------------------------------
# 5. the mixers at large sample offsets
# ---------------------------------------------------------------------------
MIX_OFFSETS = [0, (1 << 31) - 2048, (1 << 32) - 2048, (1 << 34) + 12_345]
MIX_TONES = [(1.5e6, 56e6), (-13.37e6, 56e6), (0.31, 1.0)]


def _theta_max(n, f, sr, i0):
    return float(np.abs(acc.mix_phase(n, f, sr, i0)).max())


@pytest.mark.parametrize("f,sr", MIX_TONES)
@pytest.mark.parametrize("i0", MIX_OFFSETS)
def test_mix_at_offset(gpu, i0, f, sr):
    """vsig_mix_c64_dev through apply_frequency_shift(start_index=i0): two full
    4096-sample tiles and the bounds-checked tail; numpy's own operation order,
    so the per-sample bound does not depend on i0."""
    n = 2 * 4096 + 5
    x = ref.synth_iq(n, seed=7)
    r = acc.mix(x, f, sr, i0, np.complex128)
    y = gpu.apply_frequency_shift(x, f, sr, start_index=i0)
    assert y.dtype == np.complex64 and y.shape == (n,)
    e = float((np.abs(y.astype(np.complex128) - r) / np.abs(x.astype(np.complex128))).max())
    _say(f"mix i0={i0} f={f:g} sr={sr:g}", e_gpu=e, bound=1e-6)
    assert e <= 1e-6


FUSED_N, FUSED_TAPS = 3 * 1024 + 77, 255


def _fused(gpu, taps, decim, xk, h, f, sr, i0):
    """FirFilter(taps, decim) over [h history samples | chunk], xk[0] at global
    sample i0."""
    flt = gpu.FirFilter(taps, decim)
    assert flt.block == 1024            # the fused kernel, not mix-then-filter
    return flt(torch.from_numpy(xk).cuda(), nhist=h, freq_shift=f, sample_rate=sr, i0=i0).cpu().numpy()


@pytest.mark.parametrize("f,sr", MIX_TONES)
@pytest.mark.parametrize("i0", MIX_OFFSETS)
def test_fused_mixer_phase(gpu, i0, f, sr):
    """The fused loads' rotation alone: an identity filter (taps = [1]) returns
    x[k] e^{j theta(i0 + k)}.  Against numpy's phase order, per sample:
    1e-6 + 4 spacings of theta (the kernel forms (w / sr) * gi, ~2 ulp of theta
    from numpy's w * (gi / sr); accuracy_ref.mix_rot_model pins that on the CPU)."""
    n = FUSED_N
    # the identity still runs through the overlap-save transforms, whose error
    # scales with the block and not with the sample: a unit-modulus input
    x = np.exp(2j * np.pi * ((3 * np.arange(n)) % 64) / 64).astype(np.complex64)
    r = acc.mix(x, f, sr, i0, np.complex128)
    y = _fused(gpu, np.ones(1, np.float32), 1, x, 0, f, sr, i0)
    bound = 1e-6 + 4 * np.spacing(_theta_max(n, f, sr, i0))
    e = float((np.abs(y.astype(np.complex128) - r) / np.abs(x.astype(np.complex128))).max())
    _say(f"fused-mixer-phase i0={i0} f={f:g} sr={sr:g}", e_gpu=e, bound=bound)
    assert e <= bound


def _fused_order(n, f, sr, i0):
    """Where 4 spacings of theta exceed the fp32 floor of this case (K_ANCHOR
    times the reference's own rel_rms of 3e-7: the offsets 2^32 - 2048 and
    2^34 + 12 345 at |f| = 13.37e6 or sr = 1), the filtered case feeds its
    references the kernel's documented phase order (w / sr) * gi, so that it
    measures the transform; test_fused_mixer_phase bounds the order itself."""
    return "fused" if 4 * np.spacing(_theta_max(n, f, sr, i0)) > K_ANCHOR * 3e-7 else "numpy"


@functools.lru_cache(maxsize=None)
def _fused_refs(h, f, sr, i0):
    n = FUSED_N
    xk = ref.synth_iq(h + n, seed=13 + h)
    taps = scipy.signal.firwin(FUSED_TAPS, 0.2)
    order = _fused_order(h + n, f, sr, i0)
    r32 = acc.fir(acc.mix(xk, f, sr, i0, np.complex64, order), taps)[h:]
    r64 = acc.fir(acc.mix(xk, f, sr, i0, np.complex128, order), taps, 1, np.complex128)[h:]
    return xk, taps, order, r32, r64


@pytest.mark.parametrize("f,sr", MIX_TONES)
@pytest.mark.parametrize("i0", MIX_OFFSETS)
@pytest.mark.parametrize("h", [0, 254])
@pytest.mark.parametrize("decim", [1, 2, 3, 4])
def test_fused_mixed_filter_floor(gpu, decim, h, i0, f, sr):
    """vsig_fir_exec_mix_dev, 255 taps, every decimation's kernel, with and
    without real history samples: the filtered output to the FIR bound against
    the composite reference that mixes in complex64 too."""
    xk, taps, order, r32, r64 = _fused_refs(h, f, sr, i0)
    y = _fused(gpu, taps, decim, xk, h, f, sr, i0)
    _floor(f"fused-mix-fir D={decim} h={h} i0={i0} f={f:g} sr={sr:g} order={order}", y, r32[::decim],
           r64[::decim], K_ANCHOR)


@pytest.mark.parametrize("decim", [1, 4])
def test_fused_chunk_continuity_past_2_32(gpu, decim):
    """Two adjacent chunks at i0 and i0 + n (the second with the first's last
    254 samples as history) equal one call over 2n samples."""
    n, h, i0 = 3 * 1024 + 76, 254, (1 << 32) - 2048          # n a multiple of 4: chunks on the output grid
    f, sr = -13.37e6, 56e6                                   # sample 2^32 falls in the first chunk
    x = ref.synth_iq(2 * n, seed=17)
    taps = scipy.signal.firwin(FUSED_TAPS, 0.2)
    whole = _fused(gpu, taps, decim, x, 0, f, sr, i0)
    a = _fused(gpu, taps, decim, x[:n], 0, f, sr, i0)
    b = _fused(gpu, taps, decim, x[n - h:], h, f, sr, i0 + n - h)
    got = np.concatenate([a, b])
    assert got.shape == whole.shape
    e = float(np.abs(got.astype(np.complex128) - whole).max())
    _say(f"fused-chunks D={decim} i0={i0}", e_abs=e, bound=2e-6)
    assert e <= 2e-6


# ---------------------------------------------------------------------------
# 6. filters over 8192 taps, np.correlate's other modes
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_fir_refs(ntaps, nhist):
    n = 30_000
    rng = np.random.default_rng(ntaps + nhist)
    x = ref.synth_iq(nhist + n, seed=ntaps + nhist)
    taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    return x, taps, acc.fir(x, taps)[nhist:], acc.fir(x, taps, 1, np.complex128)[nhist:]


@pytest.mark.parametrize("decim", [1, 4])
@pytest.mark.parametrize("ntaps,nhist", [(9000, 0), (20_000, 0), (9000, 3000), (20_000, 19_999)])
def test_long_taps_floor(gpu, ntaps, nhist, decim):
    """8192-tap parts summed by fir_part_accum (2 parts / 3 parts), and their
    time-chunk form with history."""
    x, taps, r32, r64 = _long_fir_refs(ntaps, nhist)
    y = gpu.FirFilter(taps, decim)(torch.from_numpy(x).cuda(), nhist=nhist).cpu().numpy()
    _floor(f"long-fir ntaps={ntaps} nhist={nhist} D={decim} parts={-(-ntaps // 8192)}", y,
           r32[::decim], r64[::decim], K_ANCHOR)


@functools.lru_cache(maxsize=None)
def _corr_operands(l1, l2):
    return ref.synth_iq(l1, seed=l1), ref.synth_iq(l2, seed=l2 + 1)


@pytest.mark.parametrize("mode", ["full", "same"])
@pytest.mark.parametrize("l1,l2", [(1500, 3 * 8192 + 77), (20_000, 61_234), (61_234, 20_000)])
def test_correlate_modes_floor(gpu, l1, l2, mode):
    """cross_correlate_signals(s1, s2, mode) = np.correlate(s2, s1, mode); the
    long pairs run as chunk passes accumulated in c, in both argument orders."""
    s1, s2 = _corr_operands(l1, l2)
    r32, r64 = acc.correlate(s2, s1, mode), acc.correlate(s2, s1, mode, np.complex128)
    c, lags = gpu.cross_correlate_signals(s1, s2, mode)
    assert c.shape == r64.shape
    _floor(f"correlate l1={l1} l2={l2} mode={mode}", c, r32, r64, K_ANCHOR)
