"""fp32 and fp64 references of the FFT paths and an fp32 model of the engine,
shared by test_accuracy_cpu.py and test_gpu_accuracy.py (numpy / scipy only).

Every operation below exists once, with a ``dtype`` argument:

  dtype=np.complex128  the high-precision reference r (error ~1e-16);
  dtype=np.complex64   the same mathematical operation in single precision with
                       ``scipy.fft`` (pocketfft keeps complex64), asserted to
                       stay complex64.  Its error against r, e_ref, is what a
                       correct fp32 implementation costs on that input.

A kernel is then bounded by ``e_gpu <= K * e_ref`` (rel_rms and max_norm), K
from the class of its twiddles (fft_engine.hpp):

  K_EXACT  = 3  twiddles rounded once from double (TwTable, TwRegs, TwLds with
                its one extra product, the PFB's table, bigfft's tables): the
                model below lands at 1.2-1.5 x scipy, times 2;
  K_ANCHOR = 8  twiddles rebuilt by a chain of products (TwAnchors, TwAnchorsX,
                the ratio-form butterflies), documented worst case 10 ulp: the
                model at +-10 ulp lands at 4.5-6.3 x scipy, plus a quarter.

test_accuracy_cpu.py pins both model classes, and that the next class up
fails each bound, without a GPU.

Operands that the kernels receive rounded (the float32 window, the complex64
taps, the float32 prototype) enter both references with those rounded values:
the references differ in arithmetic only, never in input.

  window32        periodic window as float32 (scipy.signal.get_window)
  spectrum        |fft(frame * window32)|^2 * scale, (nfft, nframes)
  fir             one whole-length FFT convolution, np.convolve(x, h)[:n][::D]
  fir_direct      the same as a direct complex128 sum (np.convolve)
  correlate_valid one whole-length FFT correlation, np.correlate(s, t, 'valid')
  pfb             pre-sum in the real dtype, then fft along the channel axis
  dft             fft / ifft
  model_fft       fp32 Stockham mixed-radix transform with the engine's radices,
                  butterflies and inter-pass products rounded to fp32, the
                  inter-pass twiddles off by uniform +-ulp spacings (or formed
                  as TwLds forms them)
  spectrum_input  the seeded input of a spectrum case (SPECTRUM_SEEDS)
"""
import numpy as np
import scipy.fft
import scipy.signal

K_EXACT = 3.0
K_ANCHOR = 8.0

# radices per pass of the engine's plans (fft_engine.hpp: Plan64 ... Plan16384)
PLAN_RADICES = {64: (8, 8), 128: (8, 16), 256: (16, 16), 512: (8, 8, 8), 1024: (32, 32),
                2048: (8, 32, 8), 4096: (16, 16, 16), 8192: (16, 32, 16), 16384: (16, 4, 16, 16)}


def _c128(a):
    return np.asarray(a).astype(np.complex128)


def rel_rms(y, r):
    """||y - r||_2 / ||r||_2 in float64 / complex128."""
    y, r = _c128(y), _c128(r)
    assert y.shape == r.shape, (y.shape, r.shape)
    return float(np.linalg.norm((y - r).ravel()) / np.linalg.norm(r.ravel()))


def max_norm(y, r):
    """max |y - r| / max |r| (the suite's 1e-5 metric)."""
    y, r = _c128(y), _c128(r)
    assert y.shape == r.shape, (y.shape, r.shape)
    return float(np.abs(y - r).max() / np.abs(r).max())


def _real_of(dtype):
    return np.float32 if np.dtype(dtype) == np.complex64 else np.float64


def _kept(a, dtype):
    assert a.dtype == np.dtype(dtype), f"{a.dtype}: the reference left {np.dtype(dtype)}"
    return a


def window32(window, nperseg):
    """The float32 window the kernels multiply by: a name (periodic, as
    scipy.signal.spectrogram builds it) or an array."""
    if isinstance(window, (str, tuple)):
        return scipy.signal.get_window(window, nperseg).astype(np.float32)
    w = np.asarray(window).astype(np.float32)
    assert w.shape == (nperseg,)
    return w


def spectrum(x, window, nperseg, noverlap, nfft, dtype=np.complex64, fftshift=False, transform=None):
    """scipy.signal.spectrogram(..., detrend=False, return_onesided=False,
    scaling='spectrum') of a 1-D complex64 signal: (nfft, nframes) of the real
    dtype, scale = 1 / sum(window32)^2.  transform: a stand-in for scipy.fft.fft
    of one zero-padded frame (the model)."""
    x = np.asarray(x)
    real = _real_of(dtype)
    w = window32(window, nperseg)
    scale = 1.0 / float(np.sum(w, dtype=np.float64)) ** 2
    hop = nperseg - noverlap
    nframes = (len(x) - nperseg) // hop + 1
    frames = np.lib.stride_tricks.sliding_window_view(x, nperseg)[::hop][:nframes]
    frames = frames.astype(dtype) * w.astype(real)[None, :]
    if transform is None:
        X = scipy.fft.fft(frames, n=nfft, axis=1)
    else:
        pad = np.zeros((nframes, nfft), dtype)
        pad[:, :nperseg] = frames
        X = np.stack([transform(f) for f in pad])
    X = _kept(X, dtype)
    P = (X.real * X.real + X.imag * X.imag) * real(scale)
    assert P.dtype == real
    if fftshift:
        P = np.fft.fftshift(P, axes=1)
    return P.T


def fir(x, taps, decim=1, dtype=np.complex64):
    """np.convolve(x, taps)[:len(x)][::decim] by one FFT of the whole length."""
    x = np.asarray(x)
    h = np.asarray(taps).astype(np.complex64)
    n = len(x)
    L = scipy.fft.next_fast_len(n + len(h) - 1)
    X = scipy.fft.fft(x.astype(dtype), L)
    H = scipy.fft.fft(h.astype(dtype), L)
    return _kept(scipy.fft.ifft(X * H), dtype)[:n][::decim]


def fir_direct(x, taps, decim=1):
    """The complex128 direct sum."""
    h = np.asarray(taps).astype(np.complex64)
    return np.convolve(_c128(x), _c128(h))[:len(x)][::decim]


def correlate_valid(stream, template, dtype=np.complex64):
    """np.correlate(stream, template, 'valid'): c[k] = sum_m s[k + m] conj(t[m]),
    by one FFT of the whole length."""
    s, t = np.asarray(stream), np.asarray(template)
    L = scipy.fft.next_fast_len(len(s))
    S = scipy.fft.fft(s.astype(dtype), L)
    T = scipy.fft.fft(t.astype(dtype), L)
    return _kept(scipy.fft.ifft(S * np.conj(T)), dtype)[:len(s) - len(t) + 1]


def pfb(x, proto, nchan, dtype=np.complex64):
    """oracle.ref.pfb_channelize's definition: z_m[p] = sum_q h[qC + p] x[(m + q)C + p]
    accumulated over q in the real dtype, Y[:, m] = fft(z_m).  (C, M)."""
    real = _real_of(dtype)
    C = int(nchan)
    h = np.asarray(proto).astype(np.float32).astype(real)
    P = len(h) // C
    assert P * C == len(h)
    M = (len(x) - P * C) // C + 1
    rows = np.asarray(x)[:(M + P - 1) * C].astype(dtype).reshape(M + P - 1, C)
    z = np.zeros((M, C), dtype)
    for q in range(P):
        z += h[q * C:(q + 1) * C][None, :] * rows[q:q + M]
    return _kept(scipy.fft.fft(_kept(z, dtype), axis=1), dtype).T


def dft(x, inverse=False, dtype=np.complex64):
    f = scipy.fft.ifft if inverse else scipy.fft.fft
    return _kept(f(np.asarray(x).astype(dtype)), dtype)


# ---------------------------------------------------------------------------
# the fp32 model of the engine
# ---------------------------------------------------------------------------
def _dft_reg(a):
    """Natural-order DFT along axis 0 (a power of two <= 64) by radix-2 steps in
    complex64: every sum and product rounds to fp32, the constants are the
    fp32-rounded exact values (fft_engine.hpp: kCos64 / kSin64)."""
    R = a.shape[0]
    if R == 1:
        return a
    ev, od = _dft_reg(a[0::2]), _dft_reg(a[1::2])
    w = np.exp(-2j * np.pi * np.arange(R // 2) / R).astype(np.complex64)
    t = od * w.reshape((-1,) + (1,) * (a.ndim - 1))
    return np.concatenate([ev + t, ev - t])


def _perturbed(w, ulp, rng):
    """complex64 twiddles with each component moved by uniform(-ulp, ulp)
    spacings of its fp32 value."""
    w = w.astype(np.complex64)
    if not ulp:
        return w

    def comp(c):
        d = rng.uniform(-ulp, ulp, c.shape) * np.spacing(np.abs(c)).astype(np.float64)
        return (c.astype(np.float64) + d).astype(np.float32)
    return (comp(w.real) + 1j * comp(w.imag)).astype(np.complex64)


def model_fft(x, radices=None, ulp=0.0, seed=0, two_level=False):
    """The engine's Stockham transform (fft_engine.hpp's index convention) in
    complex64.  ulp = 0: twiddles rounded once from double (the exact class);
    ulp = 10: the documented worst case of the anchor chains.  two_level: TwLds,
    W_N^m = A[m >> S] * B[m & (2^S - 1)] as an fp32 product of two rounded
    tables, S = ceil(log2(N) / 2)."""
    a = np.asarray(x).astype(np.complex64)
    N = len(a)
    radices = PLAN_RADICES[N] if radices is None else tuple(radices)
    assert int(np.prod(radices)) == N
    rng = np.random.default_rng(seed)
    S = (int(np.log2(N)) + 1) // 2
    hi = np.exp(-2j * np.pi * (np.arange(N >> S) << S) / N).astype(np.complex64)
    lo = np.exp(-2j * np.pi * np.arange(1 << S) / N).astype(np.complex64)
    Ns = 1
    for p, R in enumerate(radices):
        j = np.arange(N // R)
        k = j % Ns
        v = a.reshape(R, N // R)                       # v[r, j] = a[j + r N/R]
        if p > 0:
            r = np.arange(R)[:, None]
            if two_level:
                m = r * k[None, :] * (N // (Ns * R))
                tw = hi[m >> S] * lo[m & ((1 << S) - 1)]
            else:
                tw = _perturbed(np.exp(-2j * np.pi * (r * k[None, :]) / (Ns * R)), ulp, rng)
            tw[0] = 1                                  # r = 0 is not multiplied
            v = v * tw
        v = _dft_reg(v)
        assert v.dtype == np.complex64
        out = np.empty(N, np.complex64)
        base = (j // Ns) * Ns * R + k
        out[base[None, :] + np.arange(R)[:, None] * Ns] = v
        a = out
        Ns *= R
    return a


def noise(n, seed):
    """CN(0, 1) as complex64."""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)


# ---------------------------------------------------------------------------
# inputs of the spectrum cases
# ---------------------------------------------------------------------------
# K is twice (exact) / a quarter above (anchor) the model's worst multiple of
# scipy's error on noise.  oracle.ref.synth_iq adds three tones, which put a
# Hann frame's power -- and so both rel_rms and the max-norm of a power
# spectrum -- in about nine bins; on so few bins scipy's own error varies
# several-fold between seeds, and with it the model's multiple (1024 points,
# exact twiddles, 30 seeds: 0.6 .. 4.1).  A seed on which the model itself sits
# above the multiple K was derived from says nothing about a kernel, so each
# case takes the first seed, counting up from nfft + nperseg + noverlap, on
# which the model of its class stays within that multiple for all three
# figures the GPU test bounds (spectrum_premise).  Only the references and the
# model choose the seed; test_accuracy_cpu.py checks the table.
MODEL_EXACT, MODEL_ANCHOR = 1.5, 6.3
SPECTRUM_SEEDS = {                      # (nfft, nperseg, noverlap): seed   seeds tried
    (64, 64, 0): 128,                   # 1
    (128, 128, 0): 256,                 # 1
    (256, 256, 0): 512,                 # 1
    (512, 512, 0): 1025,                # 2
    (1024, 1024, 0): 2059,              # 12
    (2048, 2048, 0): 4096,              # 1
    (4096, 4096, 0): 8192,              # 1
    (8192, 8192, 0): 16386,             # 3
    (16384, 16384, 0): 32768,           # 1
    (8192, 7168, 0): 15360,             # 1
    (8192, 8192, 4096): 20480,          # 1
}


def spectrum_class(nfft):
    """(K, model ulp, the model's multiple K derives from) of a spectrum plan:
    psd_pair_kernel (>= 4096 points) takes anchors, psd_split_kernel TwLds."""
    return (K_ANCHOR, 10, MODEL_ANCHOR) if nfft >= 4096 else (K_EXACT, 0, MODEL_EXACT)


def spectrum_input(nfft, nperseg, noverlap, seed=None):
    """3 frames of synth_iq under the case's seed."""
    from oracle import ref
    seed = SPECTRUM_SEEDS[nfft, nperseg, noverlap] if seed is None else seed
    return ref.synth_iq(nperseg + 2 * (nperseg - noverlap), seed=seed)


def spectrum_premise(x, nperseg, noverlap, nfft, ulp):
    """The model's rel_rms, max-norm and worst per-frame rel_rms as multiples of
    the complex64 reference's (per frame: of its whole-case rel_rms)."""
    r64 = spectrum(x, "hann", nperseg, noverlap, nfft, np.complex128)
    r32 = spectrum(x, "hann", nperseg, noverlap, nfft)
    y = spectrum(x, "hann", nperseg, noverlap, nfft, transform=lambda f: model_fft(f, ulp=ulp))
    e_ref = rel_rms(r32, r64)
    frame = max(rel_rms(y[:, f], r64[:, f]) for f in range(y.shape[1]))
    return rel_rms(y, r64) / e_ref, max_norm(y, r64) / max_norm(r32, r64), frame / e_ref
