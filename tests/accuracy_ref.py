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

and for the routes of test_gpu_accuracy_routes.py:

  resample        scipy.signal.resample's spectrum copy around scipy.fft
  filter_channel  oracle.ref.filter_channel around scipy.fft
  filter_channel_exact  the same masked inverse sum evaluated directly in
                  np.longdouble at chosen output samples
  chirpz          the three-transform chirp-z composite of an M-point engine
  mix             apply_frequency_shift at a global sample offset (numpy's phase
                  order, or the fused FIR loads' own)
  mix_rot_model   numpy model of the fused mixer's rotation (vsig_kernels.h)
  correlate       np.correlate(a, v, mode) by one FFT of the whole length
  model_fourstep  the fp32 model of bigfft.hip's two-pass transform
  floor / say     the bound itself and its ``ACC`` line
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


# ---------------------------------------------------------------------------
# the bound (shared by test_gpu_accuracy.py and test_gpu_accuracy_routes.py)
# ---------------------------------------------------------------------------
def say(case, **figs):
    print("ACC " + case + " " + " ".join(f"{k}={v:.4g}" for k, v in figs.items()))


def floor(case, y, r32, r64, K, frame_axis=None):
    """The bound: rel_rms over the case and of each frame, max-norm over the
    case, each within K times the complex64 reference's own."""
    e_ref, e_gpu = rel_rms(r32, r64), rel_rms(y, r64)
    m_ref, m_gpu = max_norm(r32, r64), max_norm(y, r64)
    figs = dict(e_ref=e_ref, e_gpu=e_gpu, ratio=e_gpu / e_ref, m_ref=m_ref, m_gpu=m_gpu,
                m_ratio=m_gpu / m_ref)
    e_frame = 0.0
    if frame_axis is not None:
        e_frame = max(rel_rms(np.take(y, f, axis=frame_axis), np.take(r64, f, axis=frame_axis))
                      for f in range(y.shape[frame_axis]))
        figs["frame_ratio"] = e_frame / e_ref
    say(case, **figs)
    assert e_gpu <= K * e_ref, (case, figs)
    assert m_gpu <= K * m_ref, (case, figs)
    assert e_frame <= K * e_ref, (case, figs)


# ---------------------------------------------------------------------------
# the two-pass (four-step) transform of bigfft.hip
# ---------------------------------------------------------------------------
def bigfft_split(M):
    """(N1, N2) of bigfft.hip's bigfft_split."""
    if M <= 16384:
        return 1, M
    n2 = min(max(M // 64, 512), 16384)
    return M // n2, n2


def model_fourstep(x):
    """bf_col_kernel then bf_row_kernel in complex64: FFT_N1 down the columns of
    x[n1 N2 + n2], times W_M^(n2 k1) formed as tw_big forms it (an fp32 product
    of two tables rounded from double, S = ceil(log2 M / 2)), FFT_N2 along the
    rows, X[k1 + N1 k2]."""
    a = np.asarray(x).astype(np.complex64)
    M = len(a)
    N1, N2 = bigfft_split(M)
    if N1 == 1:
        return model_fft(a)
    S = (int(np.log2(M)) + 1) // 2
    hi = np.exp(-2j * np.pi * (np.arange(M >> S) << S) / M).astype(np.complex64)
    lo = np.exp(-2j * np.pi * np.arange(1 << S) / M).astype(np.complex64)
    A = a.reshape(N1, N2)
    cols = np.stack([model_fft(A[:, n2]) for n2 in range(N2)], axis=1)       # [k1, n2]
    m = np.arange(N1)[:, None] * np.arange(N2)[None, :]
    cols = cols * (hi[m >> S] * lo[m & ((1 << S) - 1)])
    assert cols.dtype == np.complex64
    rows = np.stack([model_fft(cols[k1]) for k1 in range(N1)])               # [k1, k2]
    return np.ascontiguousarray(rows.T).reshape(M)                            # k1 + N1 k2


# seeds of the long / strided spectrum cases, chosen as SPECTRUM_SEEDS' are: the
# first seed, counting up from nfft + nperseg + noverlap + stride, on which the
# model of the case's route (model_fourstep above 16384 points: exact class;
# the +-10 ulp model at 8192) stays within the multiple its K derives from.
ROUTE_SPECTRUM_SEEDS = {                # (nfft, nperseg, noverlap, stride): seed   seeds tried
    (32768, 32768, 0, 1): 65537,        # 1
    (65536, 40000, 30000, 1): 135569,   # 33 (zero-filled, overlapping frames: the model's worst
                                        #     frame sat at 1.6 .. 5.3 x on the seeds before)
    (8192, 8192, 0, 2): 16386,          # 1
    (8192, 8192, 0, 3): 16387,          # 1
    (32768, 32768, 0, 2): 65539,        # 2
    (32768, 32768, 0, 3): 65540,        # 2
}


def route_spectrum_class(nfft):
    """(K, transform of one padded frame, the model's multiple) of a spectrum
    case of test_gpu_accuracy_routes.py."""
    if nfft > 16384:
        return K_EXACT, model_fourstep, MODEL_EXACT
    K, ulp, limit = spectrum_class(nfft)
    return K, (lambda f: model_fft(f, ulp=ulp)), limit


def route_spectrum_input(nfft, nperseg, noverlap, stride=1, seed=None):
    """3 frames of synth_iq (taken every `stride` samples) under the case's seed."""
    from oracle import ref
    seed = ROUTE_SPECTRUM_SEEDS[nfft, nperseg, noverlap, stride] if seed is None else seed
    return ref.synth_iq(stride * (nperseg + 2 * (nperseg - noverlap)), seed=seed)


def route_spectrum_premise(x, nperseg, noverlap, nfft, stride=1):
    """spectrum_premise with the route's model, on x[::stride]."""
    xs = np.asarray(x)[::stride]
    model = route_spectrum_class(nfft)[1]
    r64 = spectrum(xs, "hann", nperseg, noverlap, nfft, np.complex128)
    r32 = spectrum(xs, "hann", nperseg, noverlap, nfft)
    y = spectrum(xs, "hann", nperseg, noverlap, nfft, transform=model)
    e_ref = rel_rms(r32, r64)
    frame = max(rel_rms(y[:, f], r64[:, f]) for f in range(y.shape[1]))
    return rel_rms(y, r64) / e_ref, max_norm(y, r64) / max_norm(r32, r64), frame / e_ref


# ---------------------------------------------------------------------------
# resample_signal, filter_channel, chirp-z
# ---------------------------------------------------------------------------
def resample(x, num, dtype=np.complex64, real_input=False):
    """scipy.signal.resample(x, num) (scipy 1.15.3, domain='time', no window)
    restated around scipy.fft with the dtype kept, as oracle.ref.resample_signal
    restates it: the complex path, the imaginary part zeroed for real input."""
    x = np.asarray(x)
    real = _real_of(dtype)
    Nx, num = len(x), int(num)
    X = _kept(scipy.fft.fft(x.astype(dtype)), dtype)
    Y = np.zeros(num, dtype)
    N = min(num, Nx)
    nyq = N // 2 + 1
    Y[:nyq] = X[:nyq]
    if N > 2:
        Y[nyq - N:] = X[nyq - N:]
    if N % 2 == 0:
        if num < Nx:
            Y[-N // 2] += X[-N // 2]
        elif Nx < num:
            Y[N // 2] *= real(0.5)
            Y[num - N // 2] = Y[N // 2]
    y = _kept(scipy.fft.ifft(Y), dtype) * real(float(num) / float(Nx))
    if real_input:
        y = y.real.astype(dtype)
    return _kept(y, dtype)


CENTER_FREQ = 5230e6


def channel_mask(n, center_freq, sample_rate, bandwidth):
    """oracle.ref.filter_channel's brick-wall mask over the n bins (its axis
    with the extra * sample_rate)."""
    freqs = np.fft.fftfreq(n, 1 / sample_rate) * sample_rate + CENTER_FREQ
    return (freqs >= center_freq - bandwidth / 2) & (freqs <= center_freq + bandwidth / 2)


def filter_channel(x, center_freq, sample_rate, bandwidth, dtype=np.complex64):
    """oracle.ref.filter_channel around scipy.fft with the dtype kept: the real
    dtype's array of len(x)."""
    x = np.asarray(x)
    n = len(x)
    freqs = np.fft.fftfreq(n, 1 / sample_rate) * sample_rate + CENTER_FREQ
    X = _kept(scipy.fft.fft(x.astype(dtype)), dtype)
    mask = channel_mask(n, center_freq, sample_rate, bandwidth)
    F = np.zeros(n, dtype)
    F[mask] = X[mask]
    neg = np.fft.fftshift(freqs) < CENTER_FREQ
    pos = np.fft.fftshift(freqs) >= CENTER_FREQ
    Fs = np.fft.fftshift(F)
    Fs[neg] = np.conj(np.flip(Fs[pos]))
    y = _kept(scipy.fft.ifft(np.fft.ifftshift(Fs)), dtype).real
    assert y.dtype == _real_of(dtype)
    return y


def _ld_table(n):
    """exp(-2 pi i r / n), r < n, as np.longdouble (cos, sin)."""
    ld = np.longdouble
    a = (2 * (4 * np.arctan(ld(1)))) * np.arange(n, dtype=ld) / ld(n)
    return np.cos(a), -np.sin(a)


def filter_channel_exact(x, center_freq, sample_rate, bandwidth, samples):
    """The channel filter's masked inverse sum evaluated directly in
    np.longdouble at the output indices `samples` (even n):
        X[k] = sum_m x[m] e^{-2 pi i k m / n}         for the kept bins k < n/2,
        y[m] = Re sum_k (X[k] e^{2 pi i k m / n} + conj X[k] e^{2 pi i (n-1-k) m / n}) / n
    (the mirror of bin k lands on bin n - 1 - k).  Phases from k m mod n."""
    ld = np.longdouble
    x = np.asarray(x)
    n = len(x)
    keep = np.flatnonzero(channel_mask(n, center_freq, sample_rate, bandwidth)[:n // 2])
    samples = np.asarray(samples, np.int64)
    if len(keep) == 0:
        return np.zeros(len(samples), ld)
    tc, ts = _ld_table(n)                       # e^{-i a}: (cos a, -sin a)
    xr, xi = x.real.astype(ld), x.imag.astype(ld)
    m = np.arange(n, dtype=np.int64)
    Xr, Xi = np.empty(len(keep), ld), np.empty(len(keep), ld)
    for j0 in range(0, len(keep), 64):
        r = (keep[j0:j0 + 64, None] * m[None, :]) % n
        c, s = tc[r], ts[r]
        Xr[j0:j0 + 64] = (xr * c - xi * s).sum(axis=1)
        Xi[j0:j0 + 64] = (xr * s + xi * c).sum(axis=1)
    y = np.empty(len(samples), ld)
    for i0 in range(0, len(samples), 64):
        mm = samples[i0:i0 + 64, None]
        r1 = (keep[None, :] * mm) % n
        r2 = ((n - 1 - keep)[None, :] * mm) % n
        # e^{+i a} = (tc, -ts)
        t = Xr * tc[r1] + Xi * ts[r1] + Xr * tc[r2] - Xi * ts[r2]
        y[i0:i0 + 64] = t.sum(axis=1) / ld(n)
    return y


CHANNEL_DIRECT = dict(n=20_000, cf=5230e6 + 100.0, sr=4000.0, bw=2e6)
_channel_direct = []


def channel_direct_refs():
    """The direct-route case of filter_channel (bins 800 Hz apart on the
    reference's axis: 1251 kept bins of 20 000 samples): x, the 512 output samples checked (2.56 % of the length: evenly
    spread, plus both ends' neighbours), the np.longdouble evaluation L there,
    and d = max_norm of numpy's own double-precision FFT route
    (oracle.ref.filter_channel) against L.  Computed once."""
    from oracle import ref
    if not _channel_direct:
        p = CHANNEL_DIRECT
        x = ref.synth_iq(p["n"], seed=46)
        idx = np.unique(np.concatenate([np.linspace(0, p["n"] - 1, 510).astype(np.int64), [1, p["n"] - 2]]))
        L = filter_channel_exact(x, p["cf"], p["sr"], p["bw"], idx)
        # complex128 in: numpy's FFT runs in the precision of its input
        want = ref.filter_channel(x.astype(np.complex128), p["cf"], p["sr"], p["bw"])[idx]
        d = float(np.abs(want.astype(np.longdouble) - L).max() / np.abs(L).max())
        _channel_direct.append((x, idx, L, d))
    return _channel_direct[0]


def chirpz(x, M, inverse=False, dtype=np.complex64, transform=None):
    """The DFT of len(x) points as bigfft.hip's Bluestein route forms it, with
    scipy.fft as the M-point engine: a = x c zero-padded, X = c IFFT_M(FFT_M(a)
    FFT_M(b)), c[n] = exp(-i pi n^2 / N) from n^2 mod 2N, rounded to the dtype.
    A composite reference for a composite route.  transform: a stand-in for
    the forward M-point transform (the engine's model; complex64, the inverse by
    conj and B = FFT_M(b / M) as the kernels form them)."""
    x = np.asarray(x).astype(dtype)
    N = len(x)
    assert M >= 2 * N - 1
    k = np.arange(N, dtype=np.int64)
    c = np.exp(-1j * np.pi * ((k * k) % (2 * N)) / N).astype(dtype)
    if inverse:
        x = np.conj(x)
    a = np.zeros(M, dtype)
    a[:N] = x * c
    b = np.zeros(M, dtype)
    b[:N] = np.conj(c)
    b[M - N + 1:] = np.conj(c[1:][::-1])
    if transform is None:
        A = _kept(scipy.fft.fft(a), dtype)
        B = _kept(scipy.fft.fft(b), dtype)
        conv = _kept(scipy.fft.ifft(A * B), dtype)
    else:
        B = transform(b * _real_of(dtype)(1.0 / M))
        conv = _kept(np.conj(transform(np.conj(transform(a) * B))), dtype)
    y = (c * conv[:N]).astype(dtype)
    if inverse:
        y = np.conj(y) * _real_of(dtype)(1.0 / N)
    return _kept(y, dtype)


def chirpz_size(N):
    """M of dft_any's Bluestein plan: the power of two >= max(256, 2N - 1)."""
    M = 256
    while M < 2 * N - 1:
        M *= 2
    return M


# ---------------------------------------------------------------------------
# the mixers
# ---------------------------------------------------------------------------
def mix_phase(n, f, sr, i0, order="numpy"):
    """theta of apply_frequency_shift at global samples i0 .. i0 + n - 1 in
    float64.  order="numpy": w = 2 pi f, t = (i0 + arange(n)) / sr, w * t (the
    standalone mixer's order); order="fused": (w / sr) * gi, the fused FIR
    loads' order (vsig_kernels.h: mix_rot_fast)."""
    w = 2 * np.pi * f
    gi = (int(i0) + np.arange(n, dtype=np.int64)).astype(np.float64)
    assert int(i0) + n < 2 ** 53
    if order == "numpy":
        return w * (gi / sr)
    assert order == "fused"
    return (w / sr) * gi


def mix(x, f, sr, i0=0, dtype=np.complex64, order="numpy"):
    """x * exp(1j * theta) in complex128, rounded to complex64 for dtype
    complex64 (oracle.ref.apply_frequency_shift with a sample offset)."""
    x = np.asarray(x)
    y = x.astype(np.complex128) * np.exp(1j * mix_phase(len(x), f, sr, i0, order))
    return _kept(y.astype(dtype), dtype)


def mix_rot_model(n, f, sr, i0):
    """numpy model of mix_rot_fast / cis_rev (vsig_kernels.h): the phase in
    revolutions ((w / sr) / 2 pi) * gi in float64, reduced to a quarter turn and
    |g| <= 1/8 turn in float64, fp32 Taylor polynomials of degree 9 / 10."""
    f32 = np.float32
    wsr = (2 * np.pi * f) / sr
    gi = (int(i0) + np.arange(n, dtype=np.int64)).astype(np.float64)
    rev = (wsr * 1.59154943091895345608e-01) * gi
    fr = rev - np.rint(rev)
    q = np.rint(4.0 * fr)
    x = (fr - 0.25 * q).astype(f32) * f32(6.283185307179586)
    x2 = x * x
    sn = x * ((((x2 * f32(2.7557319e-6) + f32(-1.9841270e-4)) * x2 + f32(8.3333333e-3)) * x2
               + f32(-1.6666667e-1)) * x2 + f32(1.0))
    cs = ((((x2 * f32(-2.7557319e-7) + f32(2.4801587e-5)) * x2 + f32(-1.3888889e-3)) * x2
           + f32(4.1666667e-2)) * x2 + f32(-0.5)) * x2 + f32(1.0)
    assert sn.dtype == cs.dtype == np.float32
    qi = q.astype(np.int64) & 3
    c = np.choose(qi, [cs, -sn, -cs, sn])
    s = np.choose(qi, [sn, cs, -sn, -cs])
    return (c + 1j * s).astype(np.complex64)


# ---------------------------------------------------------------------------
# np.correlate in every mode
# ---------------------------------------------------------------------------
def correlate(a, v, mode="full", dtype=np.complex64):
    """np.correlate(a, v, mode): c[l] = sum_n a[n + l] conj(v[n]) over the lags
    -(len(v) - 1) .. len(a) - 1 ('full'), by one FFT of the whole length; 'same'
    and 'valid' are numpy's slices of it."""
    a, v = np.asarray(a), np.asarray(v)
    na, nv = len(a), len(v)
    L = scipy.fft.next_fast_len(na + nv - 1)
    A = scipy.fft.fft(a.astype(dtype), L)
    V = scipy.fft.fft(v.astype(dtype), L)
    c = _kept(scipy.fft.ifft(A * np.conj(V)), dtype)
    full = np.concatenate([c[L - (nv - 1):], c[:na]]) if nv > 1 else c[:na]
    lo, hi = min(na, nv), max(na, nv)
    if mode == "full":
        return full
    if mode == "valid":
        return full[lo - 1:hi]
    assert mode == "same"
    start = (lo - 1) // 2 if na >= nv else lo - 1 - (lo - 1) // 2
    return full[start:start + hi]
