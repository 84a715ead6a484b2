"""numpy restatement of the display image (vector_amd/csrc/display.hip), shared by
test_display_cpu.py and test_gpu_display.py, and the loader of
tests/golden/display.npz.

  pooled_abs   |S|, the (2, 1) median filter as the maximum of rows i-1 and i
               (row 0 with itself), then the peak-hold block maximum; NaN
               propagates
  db_map       10 log10(P + floor) in P's dtype, as oracle.ref forms it
  rows_of      matplotlib's Normalize + Colormap lookup (table row 0..258)
  image        table[rows], flipped last
  interval     the ordinal table position of a dB map moved by -/+ ulps
"""
import functools
import os

import numpy as np

from oracle import ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "display.npz")
UNDER, OVER, BAD = 256, 257, 258
FLOOR, VMIN, VMAX = 1e-7, -60.0, -35.0      # the levels of the GPU tests' synthetic maps


def centred(nf, nt, dt):
    """Sxx whose dB values sit at the centres of bins k[i, j], a pattern that
    tells neighbours, rows, columns and 64-cell tiles apart."""
    i, j = np.meshgrid(np.arange(nf), np.arange(nt), indexing="ij")
    k = (i * 7 + j * 13 + (i // 64) * 3 + (j // 64) * 5 + (i // 16) + (j // 256) * 11) % 256
    S = 10 ** ((VMIN + (k + 0.5) / 256 * (VMAX - VMIN)) / 10) - FLOOR
    assert S.min() > 0
    return S.astype(dt)


def noise_floor(S):
    """normalize_spectrogram's floor (utils.py:365-366)."""
    a = np.abs(S)
    nf = np.percentile(a[a > 0], 5) if np.any(a > 0) else 1e-12
    return max(nf, 1e-12)


def median_rows(db):
    """ndimage.median_filter(db, size=(2, 1)): the upper of rows i-1 and i."""
    return np.maximum(db, np.vstack([db[:1], db[:-1]]))


def pooled_abs(S, median=False, pool=(1, 1)):
    a = np.abs(S)
    if median:
        a = median_rows(a)
    pf, pt = pool
    nf, nt = a.shape
    rows, cols = -(-nf // pf), -(-nt // pt)
    pad = np.zeros((rows * pf, cols * pt), a.dtype)          # |S| >= 0: zeros never win
    pad[:nf, :nt] = a
    return pad.reshape(rows, pf, cols, pt).max(axis=(1, 3))   # np.max keeps NaN


def db_map(P, floor):
    dt = P.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10 * np.log10(P + dt(floor))


def ordinals(m, vmin, vmax):
    """Position along the table: -1 under, 0..255, 256 over; BAD for NaN."""
    dt = m.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        xa = (m - dt(vmin)) / (dt(vmax) - dt(vmin)) * dt(256)
        o = np.where(xa == 256, 255, np.trunc(np.clip(xa, -1, 257)))
        o = np.where(xa < 0, -1, np.where(xa > 256, 256, o))
    return np.where(np.isnan(xa), BAD, o).astype(np.int64)


def rows_from_ordinals(o):
    return np.where(o == -1, UNDER, np.where(o == 256, OVER, o))


def rows_of(m, vmin, vmax):
    return rows_from_ordinals(ordinals(m, vmin, vmax))


def image(m, vmin, vmax, lut, flip=False):
    img = lut[rows_of(m, vmin, vmax)]
    return img[::-1] if flip else img


def restate(S, floor, vmin, vmax, lut, median=False, flip=False, pool=(1, 1)):
    return image(db_map(pooled_abs(S, median, pool), floor), vmin, vmax, lut, flip)


def interval(m, vmin, vmax, ulps=8):
    """(o_lo, o_hi): ordinals of the dB map moved down and up by ulps spacings."""
    sp = np.spacing(np.abs(m))
    with np.errstate(invalid="ignore"):
        return ordinals(m - ulps * sp, vmin, vmax), ordinals(m + ulps * sp, vmin, vmax)


def within_interval(img, o_lo, o_hi, lut):
    """Per pixel: img equals the table row of some ordinal in [o_lo, o_hi]."""
    ok = np.zeros(o_lo.shape, bool)
    bad = o_lo == BAD
    span = int(np.max(np.where(bad, 0, o_hi - o_lo), initial=0))
    for d in range(span + 1):
        o = np.where(bad, BAD, np.minimum(o_lo + d, o_hi))
        ok |= np.all(img == lut[rows_from_ordinals(o)], axis=-1)
    return ok


@functools.lru_cache(maxsize=None)
def golden_cases():
    """{case: dict(f, t, Sxx, rgba, vmin, vmax, lut, kind, options)} with Sxx
    recomputed from the stored signal by the oracle's create_spectrogram."""
    z = np.load(GOLDEN)
    sr = float(z["sample_rate"])
    spec = {k: ref.create_spectrogram(z[k], sr) for k in ("sig_abc", "sig_d", "sig_f")}
    out = {}
    for c in (str(s) for s in z["cases"]):
        if c == "e":
            f, t, Sxx = z["e_f"], z["e_t"], z["e_sxx"]
        else:
            f, t, Sxx = spec["sig_abc" if c in "abc" else f"sig_{c}"]
        lut = z[f"{c}_lut"]
        d = dict(f=f, t=t, Sxx=Sxx, lut=lut, rgba=lut[z[f"{c}_index"]], vmin=z[f"{c}_vmin"][()],
                 vmax=z[f"{c}_vmax"][()], kind="gui" if c == "f" else "plot")
        if d["kind"] == "plot":
            d["enhance_contrast"] = bool(z[f"{c}_enhance_contrast"])
            d["high_detail_mode"] = bool(z[f"{c}_high_detail_mode"])
        out[c] = d
    return out


def golden_percentiles(d):
    """normalize_spectrogram's arguments at the case's call site."""
    if d["kind"] == "plot" and d["enhance_contrast"]:
        return dict(low_percentile=5, high_percentile=95, max_dynamic_range=25)
    return {}
