"""The float64 definition of combine_packets (vsig_combine_*), in numpy: the
yardstick of tests/test_combine_cpu.py and tests/test_gpu_combine.py, and the
planted scene both use.

K packets p_k, G groups, group[k] in [-1, G), lag[k] = d_k (the representative's
sample j lines up with p_k[j + d_k]), rep[g] a member of g with d = 0.  All
ranges half open.  See include/vsig.h for the same text."""
from collections import namedtuple

import numpy as np
import scipy.optimize

Records = namedtuple("Records", "a freq m rho Ep Ev res n used")
Combined = namedtuple("Combined", "y gain first second snr y_first")

_FIELDS = (("a", np.complex128), ("freq", np.float64), ("m", np.float64), ("rho", np.float64), ("Ep", np.float64),
           ("Ev", np.float64), ("res", np.float64), ("n", np.int64), ("used", bool))


def overlap(Lg, Lk, d):
    """(lo, n) of a member of Lk samples at lag d in a frame of Lg."""
    lo, hi = max(0, -int(d)), min(int(Lg), int(Lk) - int(d))
    return (lo, hi - lo) if hi > lo else (0, 0)


def estimate_one(p, v, d, f0, min_rho):
    """One member against the reference v: the nine record fields, in order."""
    lo, n = overlap(v.size, p.size, d)
    if n == 0:
        return 0j, f0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, False
    h, m = n // 2, lo + (n - 1) / 2
    x = p[lo + d:lo + d + n].astype(np.complex128)
    r = v[lo:lo + n].astype(np.complex128)
    with np.errstate(all="ignore"):
        rot = np.exp(-2j * np.pi * f0 * (np.arange(lo, lo + n) - m)) if f0 != 0 else 1.0
        z = x * rot * np.conj(r)
        A1, A2 = z[:h].sum(), z[h:].sum()
        xp, rp = x.real ** 2 + x.imag ** 2, r.real ** 2 + r.imag ** 2
        Ep1, Ep2, Ev1, Ev2 = xp[:h].sum(), xp[h:].sum(), rp[:h].sum(), rp[h:].sum()
        Ep, Ev = Ep1 + Ep2, Ev1 + Ev2
        fin = bool(np.isfinite([A1.real, A1.imag, A2.real, A2.imag, Ep, Ev]).all())
        phi = float(np.angle(A2 * np.conj(A1))) if A1 != 0 and A2 != 0 else 0.0
        B = A1 * np.exp(0.5j * phi) + A2 * np.exp(-0.5j * phi)
        rho = np.abs(B) / np.sqrt(Ep * Ev)
        res = Ep - ((abs(A1) ** 2 / Ev1 if Ev1 > 0 else 0.0) + (abs(A2) ** 2 / Ev2 if Ev2 > 0 else 0.0))
        used = bool(fin and Ev > 0 and rho >= min_rho)
    if not used:
        return 0j, f0, m, (0.0 if fin else np.nan), Ep, Ev, res, n, False
    return B / Ev, f0 + phi / (np.pi * n), m, rho, Ep, Ev, res, n, True


def estimate(packets, group, lag, rep, ref=None, f0=None, min_rho=0.0):
    """Every packet's record.  ref: None (the representatives, whose own records
    are a = 1, freq = 0, rho = 1, res = 0 by definition) or the list of the G
    outputs; f0: None (0) or K priors."""
    K = len(packets)
    out = {name: np.zeros(K, dt) for name, dt in _FIELDS}
    for k in range(K):
        fk = 0.0 if f0 is None else float(f0[k])
        g = int(group[k])
        if g < 0:
            out["freq"][k] = fk
            continue
        v = packets[int(rep[g])] if ref is None else ref[g]
        rec = estimate_one(packets[k], np.asarray(v), int(lag[k]), fk, min_rho)
        if ref is None and int(rep[g]) == k:
            rec = (1.0 + 0j, 0.0, rec[2], 1.0, rec[4], rec[5], 0.0, rec[7], True)
        for (name, _), val in zip(_FIELDS, rec):
            out[name][k] = val
    return Records(**out)


def combine_sum(packets, group, lag, rep, rec):
    """The G outputs (complex128) of the records."""
    ys = []
    for g, r in enumerate(rep):
        Lg = packets[int(r)].size
        num, den = np.zeros(Lg, np.complex128), np.zeros(Lg)
        for k in np.flatnonzero(np.asarray(group) == g):
            if not rec.used[k]:
                continue
            d, Lk = int(lag[k]), packets[k].size
            lo, n = overlap(Lg, Lk, d)
            if n == 0:
                continue
            j = np.arange(lo, lo + n)
            t = packets[k][lo + d:lo + d + n].astype(np.complex128)
            with np.errstate(all="ignore"):
                if rec.freq[k] != 0:
                    t = t * np.exp(-2j * np.pi * rec.freq[k] * (j - rec.m[k]))
                if rec.a[k] != 1:
                    t = t * np.conj(rec.a[k])
                num[j] += t
            den[j] += abs(rec.a[k]) ** 2
        with np.errstate(all="ignore"):
            ys.append(np.where(den > 0, num / np.where(den > 0, den, 1.0), 0))
    return ys


def gain_of(group, G, rec):
    """gain_g = the sum of |a_k|^2 over the used members of g."""
    group = np.asarray(group)
    return np.array([np.sum(np.abs(rec.a[(group == g) & rec.used]) ** 2) for g in range(G)])


def snr_of(group, first, second):
    """snr_k = (Ep - res) / res (1 - share_k) of the second pass, share_k =
    |a_k|^2 / gain_g of the first (0 for a member it did not use); inf where
    res <= 0; NaN for a packet in no group, without overlap or with a
    non-finite sum."""
    group = np.asarray(group)
    K = group.size
    gain = gain_of(group, int(group.max()) + 1 if K else 0, first)
    snr = np.full(K, np.nan)
    for k in range(K):
        if group[k] < 0 or second.n[k] == 0 or not np.isfinite([second.Ep[k], second.res[k]]).all():
            continue
        share = abs(first.a[k]) ** 2 / gain[group[k]] if first.used[k] and gain[group[k]] > 0 else 0.0
        res = second.res[k]
        snr[k] = np.inf if res <= 0 else (second.Ep[k] - res) / res * (1 - share)
    return snr


def combine(packets, group, lag, rep, min_rho=0.0, refine=False):
    """The whole path: estimate against the representatives, sum, estimate
    against the sum with the first frequencies as priors, the per-instance SNR;
    refine: the sum once more with the second records."""
    first = estimate(packets, group, lag, rep, None, None, min_rho)
    y1 = combine_sum(packets, group, lag, rep, first)
    second = estimate(packets, group, lag, rep, y1, first.freq, min_rho)
    y = combine_sum(packets, group, lag, rep, second) if refine else y1
    return Combined(y, gain_of(group, len(rep), first), first, second, snr_of(group, first, second), y1)


# ---------------------------------------------------------------------------
# the planted scene
# ---------------------------------------------------------------------------
SCENE_L, SCENE_M, SCENE_SIGMA, SCENE_PAD = 3000, 8, 0.3, 7
SCENE_SEEDS = (101, 102, 103)
# the worst factor between the corrected snr_k and the planted amp^2 / sigma^2 over
# SCENE_SEEDS, measured on this reference (test_combine_cpu.py records the three
# figures); the bar is 1.25 times it, the estimate being itself noisy at sigma = 0.3
SNR_FACTOR_MEASURED = 1.041
SNR_FACTOR_BAR = SNR_FACTOR_MEASURED * 1.25
Scene = namedtuple("Scene", "packets group lag rep clean amp phase freq cut sigma")


def planted_scene(seed, sigma=SCENE_SIGMA):
    """One emitter of SCENE_L unit-modulus random-phase samples in SCENE_M
    instances: gains 0.5 - 2.0, random phases, frequency offsets |f| L <= 0.3,
    cuts of +-7 samples (cut > 0: the burst starts that many samples before the
    packet), ends up to 5 samples early, complex noise of variance sigma^2.
    The representative is the instance with the most energy; the lags are the
    planted ones."""
    rng = np.random.default_rng(seed)
    L, M, pad = SCENE_L, SCENE_M, SCENE_PAD
    clean = np.exp(2j * np.pi * rng.random(L))
    amp = rng.uniform(0.5, 2.0, M)
    phase = rng.uniform(0, 2 * np.pi, M)
    freq = rng.uniform(-0.3, 0.3, M) / L
    cut = rng.integers(-pad, pad + 1, M)
    early = rng.integers(0, 6, M)
    t = np.arange(L)
    packets = []
    for i in range(M):
        full = np.zeros(L + 2 * pad, np.complex128)
        full[pad:pad + L] = amp[i] * np.exp(1j * phase[i]) * np.exp(2j * np.pi * freq[i] * t) * clean
        full += sigma * (rng.standard_normal(full.size) + 1j * rng.standard_normal(full.size)) * np.sqrt(0.5)
        packets.append(full[pad - cut[i]:pad + L - early[i]].astype(np.complex64))
    energy = np.array([np.sum(np.abs(p.astype(np.complex128)) ** 2) for p in packets])
    r = int(np.argmax(energy))
    return Scene(packets, np.zeros(M, np.int32), (cut - cut[r]).astype(np.int64), np.array([r], np.int32), clean,
                 amp, phase, freq, cut, sigma)


def noise_to_signal(x, clean, start):
    """Error power over signal power of x against the clean packet (whose
    sample 0 sits at x[start]) after fitting one complex gain and a linear
    phase by least squares."""
    lo, hi = max(0, start), min(x.size, start + clean.size)
    xs, s = np.asarray(x[lo:hi], np.complex128), clean[lo - start:hi - start]
    w, t = xs * np.conj(s), np.arange(hi - lo)
    fit = scipy.optimize.minimize_scalar(lambda f: -abs(np.sum(w * np.exp(-2j * np.pi * f * t))),
                                         bounds=(-0.6 / s.size, 0.6 / s.size), method="bounded",   # one lobe
                                         options={"xatol": 1e-12})
    rot = np.exp(2j * np.pi * fit.x * t)
    c = np.sum(w * np.conj(rot)) / np.sum(np.abs(s) ** 2)
    model = c * rot * s
    return np.sum(np.abs(xs - model) ** 2) / np.sum(np.abs(model) ** 2)


def scene_figures(scene, y, gain, freq, snr):
    """(measured gain / gain_g, max |freq_k - planted| L, the worst factor
    between snr_k and its planted amp^2 / sigma^2) of one combined scene."""
    r = int(scene.rep[0])
    measured = noise_to_signal(scene.packets[r], scene.clean, scene.cut[r]) / noise_to_signal(y, scene.clean, scene.cut[r])
    ferr = np.max(np.abs(np.asarray(freq) - (scene.freq - scene.freq[r]))) * SCENE_L
    ratio = np.asarray(snr) / (scene.amp ** 2 / scene.sigma ** 2)
    return measured / gain, ferr, float(np.max(np.maximum(ratio, 1 / ratio)))
