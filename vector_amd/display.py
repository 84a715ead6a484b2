"""The display tail of the reference on the GPU: a spectrogram to RGBA pixels.

The reference turns Sxx into pixels in three places, all of them
normalize_spectrogram -> (median filter) -> Normalize(vmin, vmax) -> the colour
map's 256-entry table:

  plot_spectrogram             utils.py:429-449, 491-499   5 / 95, median (2, 1), turbo / inferno
  adjust_packet_bounds_gui     utils.py:1017-1022, 1062    10 / 95, viridis, rows flipped
  spectrogram_analysis.py      :56-62                      10 / 95, viridis

spectrogram_image does that in one kernel (display.hip): it reads Sxx once
and writes finished pixels, optionally peak-hold pooled to screen size; no dB
map is written and nothing crosses to the host.  Drawing (figures, axes,
markers, text) stays with the caller: hand ``rgba`` and ``extent`` to imshow.

The colour tables (_colormaps.py, written by tools/make_colormaps.py) are
matplotlib's own bytes; matplotlib is not needed at run time.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .analysis import spectrogram_levels
from .dsp import _is_dev, _ptr

__all__ = ["SpectrogramImage", "spectrogram_levels", "spectrogram_image", "plot_spectrogram_image",
           "colormap_table", "pool_factors", "image_extent"]

SpectrogramImage = namedtuple("SpectrogramImage", "rgba vmin vmax pool")

_TABLES = None
_dev_tables = {}            # (device, name) -> (259, 4) uint8 tensor


def colormap_table(cmap) -> np.ndarray:
    """The (259, 4) uint8 table of a colour map: rows 0..255, then under, over,
    bad (matplotlib's lookup-table order).  cmap: "turbo", "inferno",
    "viridis", or a (256, 4) / (259, 4) uint8 array; a 256-row table gets
    under = row 0, over = row 255, bad = zeros."""
    global _TABLES
    if isinstance(cmap, str):
        if _TABLES is None:
            from ._colormaps import HEX
            _TABLES = {k: np.frombuffer(bytes.fromhex("".join(v)), np.uint8).reshape(259, 4)
                       for k, v in HEX.items()}
        if cmap not in _TABLES:
            raise ValueError(f"unknown colour map {cmap!r}: expected one of {sorted(_TABLES)} or a table")
        return _TABLES[cmap]
    a = cmap.cpu().numpy() if _is_dev(cmap) else np.asarray(cmap)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != 4 or a.shape[0] not in (256, 259):
        raise ValueError("a colour table is a (256, 4) or (259, 4) uint8 array")
    if a.shape[0] == 256:
        a = np.vstack([a, a[:1], a[255:], np.zeros((1, 4), np.uint8)])
    return np.ascontiguousarray(a)


def _device_table(cmap, device):
    if isinstance(cmap, str):
        key = (device, cmap)
        if key not in _dev_tables:
            _dev_tables[key] = torch.from_numpy(colormap_table(cmap).copy()).to(f"cuda:{device}")
        return _dev_tables[key]
    return torch.from_numpy(colormap_table(cmap).copy()).to(f"cuda:{device}")


def pool_factors(shape, max_size):
    """(pf, pt) for an (n_freq, n_time) spectrogram shown in at most max_size =
    (max_rows, max_cols) pixels: ceil(n / max) per axis; (1, 1) for None."""
    if max_size is None:
        return 1, 1
    max_rows, max_cols = (int(m) for m in max_size)
    if max_rows < 1 or max_cols < 1:
        raise ValueError("max_size must be at least (1, 1)")
    return max(1, -(-int(shape[0]) // max_rows)), max(1, -(-int(shape[1]) // max_cols))


def _check_levels(levels):
    floor, vmin, vmax = levels
    if not (math.isfinite(float(vmin)) and math.isfinite(float(vmax))) or not float(vmax) > float(vmin):
        raise ValueError(f"levels need finite vmin < vmax, got vmin={vmin}, vmax={vmax}")
    return float(floor), vmin, vmax


def _layout(t: torch.Tensor):
    """(tensor, freq_fast, ld) of a 2-D (n_freq, n_time) device tensor whose
    fast axis has unit stride: rendered where it lies.  Anything else (a
    stepped slice) is gathered first."""
    nf, nt = t.shape
    sf, st = t.stride()
    if (st == 1 or nt == 1) and (nf == 1 or sf >= nt):
        return t, 0, (sf if nf > 1 else nt)
    if (sf == 1 or nf == 1) and (nt == 1 or st >= nf):
        return t, 1, (st if nt > 1 else nf)
    return t.contiguous(), 0, nt


def spectrogram_image(Sxx, *, low_percentile=10.0, high_percentile=95.0, max_dynamic_range=25,
                      median_filter=False, cmap="viridis", flip_freq=False, max_size=None, levels=None):
    """Sxx (n_freq, n_time), real float32 / float64 -> SpectrogramImage(rgba,
    vmin, vmax, pool): the (rows, cols, 4) uint8 image the reference's plot
    sites draw, rows ascending in frequency (descending with flip_freq).

    levels: (floor, vmin, vmax) to use as they are -- a fixed colour scale
      across redraws and zooms; None selects them as normalize_spectrogram
      does (spectrogram_levels, with the three percentile arguments).
    median_filter: ndimage.median_filter(Sxx_db, size=(2, 1)) before the
      colour map (plot_spectrogram), which is the maximum of rows i-1 and i.
    max_size: (max_rows, max_cols) peak-hold pools blocks of pool = (pf, pt)
      cells into one pixel (pool_factors); peak-hold pooling has no reference
      counterpart (the reference hands every cell to matplotlib).
    cmap: see colormap_table.

    numpy in -> numpy out; a CUDA tensor in -> a CUDA tensor out, nothing
    synchronises when levels are given.  Contiguous arrays, transposed views
    (what spectrum / create_spectrogram return) and unit-stride slices of
    either are rendered where they lie; selecting levels of a sliced view
    gathers it for the order statistics.  A NaN cell makes its pixel the bad
    colour."""
    dev_in = _is_dev(Sxx)
    if not dev_in:
        Sxx = np.asarray(Sxx)
    if (Sxx.is_complex() if dev_in else np.iscomplexobj(Sxx)):
        raise ValueError("expected a real array")
    table = colormap_table(cmap)                     # argument errors before any device work
    if levels is not None:
        levels = _check_levels(levels)
    if (Sxx.numel() if dev_in else Sxx.size) == 0:
        pool_factors((0, 0), max_size)
        empty = torch.empty((0, 0, 4), dtype=torch.uint8, device=Sxx.device) if dev_in \
            else np.zeros((0, 0, 4), np.uint8)
        return SpectrogramImage(empty, 0, 0, (1, 1))
    if (Sxx.dim() if dev_in else Sxx.ndim) != 2:
        raise ValueError("expected a 2-D (n_freq, n_time) array")
    pool = pool_factors(Sxx.shape, max_size)
    ctx = _lib.get_context(Sxx.device.index if dev_in and Sxx.is_cuda else None)
    if dev_in:
        t = Sxx if Sxx.is_cuda else Sxx.to(f"cuda:{ctx.device}")
    else:
        try:
            t = torch.from_numpy(Sxx)
        except (ValueError, TypeError):              # negative strides, read-only odd layouts
            t = torch.from_numpy(np.ascontiguousarray(Sxx))
        t = t.to(f"cuda:{ctx.device}")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if levels is None:
        levels = _check_levels(spectrogram_levels(t, low_percentile, high_percentile, max_dynamic_range))
    floor, vmin, vmax = levels
    t, freq_fast, ld = _layout(t)
    n_freq, n_time = (int(s) for s in t.shape)
    rows, cols = -(-n_freq // pool[0]), -(-n_time // pool[1])
    lut = _device_table(cmap if isinstance(cmap, str) else table, t.device.index)
    rgba = torch.empty((rows, cols, 4), dtype=torch.uint8, device=t.device)
    code = "f32" if t.dtype == torch.float32 else "f64"
    ctx.check(ctx.lib.vsig_spectrogram_image_dev(
        ctx.h, _lib.DTYPES[code], _ptr(t), n_freq, n_time, freq_fast, int(ld), floor, float(vmin),
        float(vmax), int(bool(median_filter)), int(bool(flip_freq)), pool[0], pool[1], _ptr(lut),
        _ptr(rgba)), "spectrogram image")
    return SpectrogramImage(rgba if dev_in else rgba.cpu().numpy(), vmin, vmax, pool)


def _axis(a):
    return a.detach().cpu().numpy() if _is_dev(a) else np.asarray(a)


def image_extent(f, t, pool=(1, 1)):
    """imshow(origin="lower") extent of an image of Sxx over the bin centres f
    (Hz) and t (s), pooled by (pf, pt): (t0 - dt/2, t1 + dt/2, (f0 - df/2) / 1e6,
    (f1 + df/2) / 1e6) with t0, t1 / f0, f1 the centres of the first and last
    pixel and dt, df the bin steps times the pool factors (a pixel of a last,
    partial block is drawn as wide as the others).  An axis of one bin has
    step 1."""
    f, t = _axis(f), _axis(t)
    pf, pt = pool

    def edges(a, p):
        n = len(a)
        step = float(a[1] - a[0]) if n > 1 else 1.0
        lo = float(a[0]) - step / 2
        return lo, lo + -(-n // p) * p * step

    t_lo, t_hi = edges(t, pt)
    f_lo, f_hi = edges(f, pf)
    return t_lo, t_hi, f_lo / 1e6, f_hi / 1e6


def plot_spectrogram_image(f, t, Sxx, enhance_contrast=True, high_detail_mode=True, max_size=None):
    """plot_spectrogram's data path (utils.py:429-449, 491-499) -> (rgba,
    extent, vmin, vmax): percentiles 5 / 95 with enhance_contrast (else the
    defaults), the median filter always, turbo with high_detail_mode (else
    inferno; its gouraud shading is not reproduced).  A single time bin is
    drawn as two identical columns over t -+ 0.5 us (utils.py:443-448).
    ``imshow(rgba, origin="lower", extent=extent, aspect="auto",
    interpolation="none")`` shows what pcolormesh(shading="nearest") does."""
    kw = dict(low_percentile=5, high_percentile=95, max_dynamic_range=25) if enhance_contrast else {}
    img = spectrogram_image(Sxx, median_filter=True, cmap="turbo" if high_detail_mode else "inferno",
                            max_size=max_size, **kw)
    rgba, t = img.rgba, _axis(t)
    if len(t) == 1 and rgba.shape[1] == 1:
        dt = 1e-6
        t = np.array([t[0] - dt / 2, t[0] + dt / 2])
        rgba = torch.cat([rgba, rgba], dim=1) if _is_dev(rgba) else np.hstack([rgba, rgba])
    return rgba, image_extent(f, t, img.pool), img.vmin, img.vmax
