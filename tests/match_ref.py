"""float64 definition of the all-pairs burst similarity (vsig_match_run,
packet_similarity), and the inputs its tests share.  Host only.

  E_k       = sum_j |p_k[j]|^2
  c_ab[l]   = sum_j p_a[j + l] conj(p_b[j]),  l in [-(L_b - 1), L_a - 1]
            = np.correlate(p_a, p_b, 'full')[l + L_b - 1]
  peak[a,b] = max_l |c_ab[l]|,  lag[a,b] = the smallest l attaining it
  rho[a,b]  = peak / sqrt(E_a E_b)
For a < b as written; (b, a) is the mirror (same peak, lag negated); the
diagonal is E_a with lag 0.  A non-finite energy: peak NaN, lag 0; a zero one:
peak 0, lag 0, rho 0."""
from collections import namedtuple

import numpy as np

MatchRef = namedtuple("MatchRef", "peak lag energy rho margin")


def pair(pa, pb):
    """(peak, lag, margin) of one ordered pair: margin = (largest |c| - second
    largest) / largest (inf for a single lag, 0 for an all-zero c)."""
    pa, pb = np.asarray(pa, np.complex128), np.asarray(pb, np.complex128)
    if pa.size * pb.size > 1 << 18:                 # the same sums by float64 FFTs (error ~1e-13 of the peak)
        import scipy.signal
        mag = np.abs(scipy.signal.correlate(pa, pb, "full", method="fft"))
    else:
        mag = np.abs(np.correlate(pa, pb, "full"))
    i = int(np.argmax(mag))                         # the first maximum: the smallest lag
    if mag.size == 1:
        margin = np.inf
    elif mag[i] == 0:
        margin = 0.0
    else:
        margin = float((mag[i] - np.partition(mag, -2)[-2]) / mag[i])
    return float(mag[i]), i - (pb.size - 1), margin


def match(packets):
    K = len(packets)
    p = [np.asarray(x, np.complex128) for x in packets]
    with np.errstate(all="ignore"):
        energy = np.array([np.sum(x.real ** 2 + x.imag ** 2) for x in p])
    peak = np.zeros((K, K))
    lag = np.zeros((K, K), np.int64)
    margin = np.full((K, K), np.inf)
    for a in range(K):
        peak[a, a] = energy[a] if np.isfinite(energy[a]) else np.nan
        for b in range(a + 1, K):
            if not (np.isfinite(energy[a]) and np.isfinite(energy[b])):
                peak[a, b], lag[a, b], margin[a, b] = np.nan, 0, 0.0
            elif energy[a] == 0 or energy[b] == 0:
                peak[a, b], lag[a, b], margin[a, b] = 0.0, 0, 0.0
            else:
                peak[a, b], lag[a, b], margin[a, b] = pair(p[a], p[b])
            peak[b, a], lag[b, a], margin[b, a] = peak[a, b], -lag[a, b], margin[a, b]
    with np.errstate(all="ignore"):
        rho = peak / (np.sqrt(energy[:, None]) * np.sqrt(energy[None, :]))
    fin = np.isfinite(energy)
    rho[((energy[:, None] == 0) | (energy[None, :] == 0)) & fin[:, None] & fin[None, :]] = 0.0
    return MatchRef(peak, lag, energy, rho, margin)


def brute(pa, pb):
    """The definition as a double loop (small packets): (peak, lag)."""
    pa, pb = np.asarray(pa, np.complex128), np.asarray(pb, np.complex128)
    best, at = -1.0, 0
    for l in range(-(pb.size - 1), pa.size):
        s = 0j
        for j in range(pb.size):
            if 0 <= j + l < pa.size:
                s += pa[j + l] * np.conj(pb[j])
        if abs(s) > best:
            best, at = abs(s), l
    return best, at


def emitters(lmax, seed=0):
    """The 15 packets of the GPU tests and the emitter of each (-1: none):
    three emitters of random-phase unit-modulus samples of lengths lmax,
    lmax - 1, lmax / 2 + 1, four instances each (amplitude 0.5 .. 3.5, a
    random constant phase, noise 0.05; instance 1 cut 3 samples late, instance
    2 ended 5 samples early), then a length-1 packet, a length-2 packet and a
    noise packet."""
    rng = np.random.default_rng(1000 + seed + lmax)
    packets, who = [], []
    for e, L in enumerate((lmax, lmax - 1, lmax // 2 + 1)):
        base = np.exp(2j * np.pi * rng.random(L))
        for i, amp in enumerate((0.5, 1.5, 2.5, 3.5)):
            p = amp * np.exp(2j * np.pi * rng.random()) * base
            p = p + 0.05 * (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * np.sqrt(0.5)
            if i == 1:
                p = p[3:]
            if i == 2:
                p = p[:-5]
            packets.append(p.astype(np.complex64))
            who.append(e)
    packets.append(np.array([0.7 - 0.2j], np.complex64))
    packets.append(np.array([0.3 + 0.1j, -0.4 + 0.9j], np.complex64))
    packets.append(((rng.standard_normal(lmax // 3) + 1j * rng.standard_normal(lmax // 3)) * np.sqrt(0.5))
                   .astype(np.complex64))
    who += [-1, -1, -1]
    order = rng.permutation(len(packets))           # emitters interleaved
    return [packets[i] for i in order], np.array([who[i] for i in order])
