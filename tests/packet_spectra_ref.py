"""numpy / scipy statements of the per-burst spectra and measurements
(segment_spectra, measure_packets), shared by test_packet_spectra_cpu.py and
test_gpu_packet_spectra.py.

  nframes          frames of each segment (0 below nperseg)
  segment_traces   spectrum_traces_ref.traces of every slice, one row a segment,
                   a NaN row where a segment has no frame
  band             vsig_band_t of one row with np.cumsum's sequential sums
  band_margin      how far, relative to the total, the nearest cumulative sum
                   lies from either target (the premise of exact indices)
  to_hz            PacketMeasurements' fields from a band record
  band rows        flat noise, a band on a -60 dB floor, a single bin, two tones
"""
import numpy as np

import spectrum_traces_ref as st

# no np.cumsum value may lie this close (relative to the total) to a target:
# the kernel's fixed-order sums are within nbins * 2^-52 (1.8e-12 at 8192 bins)
PREMISE = 1e-9


def nframes(lengths, nperseg, hop):
    return np.array([(n - nperseg) // hop + 1 if n >= nperseg else 0 for n in lengths], np.int64)


def segment_traces(x, starts, ends, window, nperseg, noverlap, nfft, dtype=np.complex128, fftshift=False):
    """{detector: (K, nfft)} of the slices x[start:end + 1] (ends inclusive)."""
    rows = {d: [] for d in st.DETECTORS}
    for s, e in zip(starts, ends):
        seg = x[s:e + 1]
        if len(seg) < nperseg:
            for d in st.DETECTORS:
                rows[d].append(np.full(nfft, np.nan))
            continue
        r = st.traces(seg, window, nperseg, noverlap, nfft, dtype, fftshift)
        for d in st.DETECTORS:
            rows[d].append(r[d])
    return {d: np.array(v).reshape(len(starts), nfft) for d, v in rows.items()}


def band(row, tail):
    """dict(power, centroid, peak, peak_bin, lo_bin, hi_bin) of one row, in
    double, sequentially."""
    m = np.asarray(row, np.float64)
    c = np.cumsum(m)
    total = c[-1]
    if np.isnan(m).any() or not total > 0:
        return dict(power=total, centroid=np.nan, peak=np.nan, peak_bin=-1, lo_bin=-1, hi_bin=-1)
    k = np.arange(m.size, dtype=np.float64)
    wsum = np.cumsum(k * m)[-1]
    pk = int(np.argmax(m))
    return dict(power=total, centroid=wsum / total, peak=m[pk], peak_bin=pk,
                lo_bin=int(np.flatnonzero(c >= tail * total)[0]),
                hi_bin=int(np.flatnonzero(c >= (1.0 - tail) * total)[0]))


def band_margin(row, tail):
    """min |c[k] - target| / total over both targets and every k."""
    c = np.cumsum(np.asarray(row, np.float64))
    total = c[-1]
    return min(np.abs(c - tail * total).min(), np.abs(c - (1.0 - tail) * total).min()) / total


def to_hz(b, nfft, sample_rate, center_freq, window32):
    """The table of the front end's fields, from one band() record."""
    df = sample_rate / nfft
    w = window32.astype(np.float64)
    power = b["power"] * (w.sum() ** 2 / (nfft * (w * w).sum()))
    if b["lo_bin"] < 0:
        nan = np.nan
        return dict(center_freq=nan, peak_freq=nan, f_lo=nan, f_hi=nan, bandwidth=nan, power=power)
    return dict(center_freq=center_freq + (b["centroid"] - nfft / 2) * df,
                peak_freq=center_freq + (b["peak_bin"] - nfft / 2) * df,
                f_lo=center_freq + (b["lo_bin"] - nfft / 2 - 0.5) * df,
                f_hi=center_freq + (b["hi_bin"] - nfft / 2 + 0.5) * df,
                bandwidth=(b["hi_bin"] - b["lo_bin"] + 1) * df,
                power=power)


# ---------------------------------------------------------------------------
# rows of the band measurement tests
# ---------------------------------------------------------------------------
ROW_KINDS = ("flat", "band", "single", "tones")


def band_row(kind, nbins, seed):
    """A non-negative float64 row of unit scale."""
    rng = np.random.default_rng(seed)
    if kind == "flat":                       # the periodogram of noise: exponential around 1
        return rng.exponential(1.0, nbins)
    if kind == "band":                       # a band of a third of the bins on a -60 dB floor
        m = rng.exponential(1e-6, nbins)
        a = int(rng.integers(nbins // 8, nbins // 2))
        m[a:a + nbins // 3] += rng.exponential(1.0, nbins // 3)
        return m
    if kind == "single":
        m = np.zeros(nbins)
        m[int(rng.integers(0, nbins))] = 1.0 + rng.random()
        return m
    if kind == "tones":                      # two tones 60 dB apart over a weak floor
        m = rng.exponential(1e-12, nbins)
        a, b = rng.choice(nbins, 2, replace=False)
        m[a] += 1.0 + rng.random()
        m[b] += 1e-6 * (1.0 + rng.random())
        return m
    raise ValueError(kind)


def vetted_row(kind, nbins, tails, gain, first_seed):
    """The first seed, counting up, whose row (times the exact power-of-two
    gain) keeps every np.cumsum value at least PREMISE * total from both
    targets of every tail: only the reference chooses.  -> (row, seed)."""
    for seed in range(first_seed, first_seed + 64):
        m = band_row(kind, nbins, seed) * gain
        if all(band_margin(m, t) > PREMISE for t in tails):
            return m, seed
    raise AssertionError(f"no seed in [{first_seed}, {first_seed + 64}) meets the premise for {kind} {nbins}")
