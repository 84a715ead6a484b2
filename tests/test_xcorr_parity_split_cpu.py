"""The parity split of the M = 16384 correlator (xcorr.hip, xcorr_half_kernel
with PS) as a numpy model: the M-point frame is split by sample parity, so
both radix-2 steps land on the frequency side and fold into the template
product.

  E, O = FFT_H(x[0::2]), FFT_H(x[1::2])                       (H = M / 2)
  X[k] = E[k] + w^k O[k],  X[k + H] = E[k] - w^k O[k]         (w = exp(-2 pi i / M))
  Z = conj(X) P;  r = FFT_M(Z) taken as low / high halves:
  r[2 m] = FFT_H(Z[k] + Z[k + H]),  r[2 m + 1] = FFT_H((Z[k] - Z[k + H]) w^k)
  =>  U = conj(E) S + conj(O) D,   V = conj(E) D W_H^k + conj(O) S
      S = P[k] + P[k + H],   D = (P[k] - P[k + H]) conj(w^k)
  c[2 m] = conj(FFT_H(U))[m],   c[2 m + 1] = conj(FFT_H(V))[m]

This pins the (S, D) table's definition and the output map (thread column m,
key 2 rank + parity) against np.fft's circular correlation in complex128."""
import numpy as np
import pytest


def parity_tables(P):
    """(S, D) from the M-point template spectrum P (natural order)."""
    M = len(P)
    H = M // 2
    k = np.arange(H)
    S = P[:H] + P[H:]
    D = (P[:H] - P[H:]) * np.exp(2j * np.pi * k / M)
    return S, D


def parity_correlate(x, S, D):
    """The circular correlation of one M-sample frame x with the template
    behind (S, D), outputs de-interleaved from the two H-point transforms."""
    H = len(S)
    E = np.fft.fft(x[0::2])
    O = np.fft.fft(x[1::2])
    k = np.arange(H)
    U = np.conj(E) * S + np.conj(O) * D
    V = np.conj(E) * D * np.exp(-2j * np.pi * k / H) + np.conj(O) * S
    c = np.empty(2 * H, np.complex128)
    c[0::2] = np.conj(np.fft.fft(U))
    c[1::2] = np.conj(np.fft.fft(V))
    return c


def circular_correlate(x, p):
    """c[n] = sum_j x[(n + j) mod M] conj(p[j]) by np.fft in complex128."""
    M = len(x)
    pp = np.zeros(M, np.complex128)
    pp[: len(p)] = p
    return np.fft.ifft(np.fft.fft(x) * np.conj(np.fft.fft(pp)))


@pytest.mark.parametrize("M,L", [(64, 17), (64, 32), (16384, 4096), (16384, 8192)])
def test_parity_split_matches_circular_correlation(M, L):
    rng = np.random.default_rng(M + L)
    x = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    p = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    pp = np.zeros(M, np.complex128)
    pp[:L] = p
    P = np.fft.fft(pp) / M                       # the library's spectrum carries the 1 / M
    S, D = parity_tables(P)
    got = parity_correlate(x, S, D)
    want = circular_correlate(x, p)
    # complex128 transforms of M points: a few 1e-16 log2(M) of the largest output
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the overlap-save outputs proper (no wrap-around) are np.correlate's
    direct = np.correlate(x, p, "valid")
    assert np.abs(got[: M - L + 1] - direct).max() <= 1e-12 * np.abs(direct).max()


def test_parity_tables_definition():
    """S and D against their defining sums at single bins (M = 64)."""
    M, H = 64, 32
    rng = np.random.default_rng(3)
    P = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    S, D = parity_tables(P)
    for k in (0, 1, 7, 16, 31):
        assert S[k] == P[k] + P[k + H]
        w_k = np.exp(-2j * np.pi * k / M)
        assert abs(D[k] - (P[k] - P[k + H]) * np.conj(w_k)) <= 1e-15 * abs(P[k] - P[k + H])
    # D's twiddle cancels the one of X[k] = E + w^k O in the even outputs and
    # leaves W_H^k = w^(2 k) in the odd ones
    k = np.arange(H)
    assert np.allclose(D * np.exp(-2j * np.pi * k / H), (P[:H] - P[H:]) * np.exp(-2j * np.pi * k / M),
                       rtol=1e-14, atol=0)


def test_parity_output_map_is_monotone_bijection():
    """Thread column m (< 256) of a block holds the outputs 2 (m + 256 rank) +
    parity; its 6-bit key 2 rank + parity (< 64) rises with the output index,
    and (m, key) <-> index covers [0, 16384) once.  Interior blocks at hop
    12288 keep the keys below 48: ranks below 24 of both parities."""
    kstep, E = 256, 32
    seen = np.zeros(2 * kstep * E, bool)
    for m in range(kstep):
        key = np.arange(2 * E)
        idx = 2 * (m + kstep * (key >> 1)) + (key & 1)
        assert (np.diff(idx) > 0).all()
        assert not seen[idx].any()
        seen[idx] = True
        assert (idx[key < 48] < 12288).all() and (idx[key >= 48] >= 12288).all()
    assert seen.all()
