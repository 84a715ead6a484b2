"""Generate tests/golden/display.npz from the REFERENCE itself.

Like make_golden_transplant.py, it needs a checkout of the reference named by
VECTOR_REFERENCE and imports its ``utils`` module (CPU only, matplotlib on the
Agg backend):

    VECTOR_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python tests/golden/make_golden_display.py

The reference's images are recorded where it hands them to matplotlib:
``utils.plot_spectrogram(f, t, Sxx)`` leaves a figure behind whose QuadMesh
(``fig.axes[0].collections[0]``) holds the plotted array, the norm's vmin /
vmax and the colour map; ``to_rgba(array, bytes=True)`` is the image.  Only
data is stored -- input signals and images, no dB maps:

  a   plot_spectrogram on a seeded 20 000-sample burst-in-noise capture at
      56 MHz (create_spectrogram gives Sxx 512 x 353)
  b   the same with enhance_contrast=False
  c   the same with high_detail_mode=False
  d   the first 4096 samples of the reference's data/packet_2_chirp.mat
      through load_packet and create_spectrogram (the whole file's image alone
      would be several MB)
  e   a one-time-bin Sxx (64 x 1): two identical columns
  f   adjust_packet_bounds_gui's image (utils.py:1017-1022, 1062) of a seeded
      6000-sample capture: normalize_spectrogram, rows flipped, viridis
      through pcolormesh(shading='nearest', vmin=, vmax=)

Per case: ``<case>_index``, ``<case>_vmin``, ``<case>_vmax``, ``<case>_lut``
(the colour map's 259-row byte table, (lut * 255).astype(uint8)) and the
options; inputs ``sig_abc``, ``sig_d``, ``sig_f`` (complex64), ``e_sxx``,
``e_f``, ``e_t``.  The image is ``lut[index]``: each pixel is stored as the
table row (0..255) that holds its four bytes, and the script checks that
``lut[index]`` gives to_rgba's bytes back exactly before it writes.  Stored as
RGBA the three 512 x 353 images of noise alone deflate to 0.85 MB and the
fixture would pass the 1 MiB a committed file may have; as rows it is 0.8 MB.

The script refuses to write a fixture whose levels sit on a branch boundary
of normalize_spectrogram's clamps: the percentile range within 1e-3 dB of 25
or 20, or vmin within 1e-3 dB of -120.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import matplotlib
import numpy as np
import scipy

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["VECTOR_REFERENCE"]
sys.path.insert(0, REF)

import utils as refutils  # noqa: E402  (the reference)

SR = 56e6


def quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def capture(rng, n, at, length, f0):
    """Complex noise of sigma 0.05 with a tone burst of amplitude 1 at f0."""
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x = (0.05 * np.sqrt(0.5) * w).astype(np.complex64)
    x[at:at + length] += np.exp(2j * np.pi * f0 / SR * np.arange(length)).astype(np.complex64)
    return x


def lut_bytes(cmap):
    if not cmap._isinit:
        cmap._init()
    return (cmap._lut * 255).astype(np.uint8)


def mesh_image(mesh):
    """(rgba, vmin, vmax, lut) of a QuadMesh as matplotlib will draw it."""
    arr = mesh.get_array()
    rgba = np.asarray(mesh.to_rgba(arr, bytes=True))
    return rgba, mesh.norm.vmin, mesh.norm.vmax, lut_bytes(mesh.cmap)


def to_index(rgba, lut):
    """uint8 table rows with lut[rows] == rgba (first matching row of 0..255)."""
    w = np.array([1, 1 << 8, 1 << 16, 1 << 24], np.uint32)
    key, rows = rgba.reshape(-1, 4).astype(np.uint32) @ w, lut[:256].astype(np.uint32) @ w
    order = np.argsort(rows, kind="stable")
    pos = np.minimum(np.searchsorted(rows[order], key), 255)
    index = order[pos].astype(np.uint8).reshape(rgba.shape[:-1])
    assert np.array_equal(lut[index], rgba), "a pixel is not a row of the table"
    return index


def check_levels(case, Sxx, low, high):
    a = np.abs(Sxx)
    nf = max(np.percentile(a[a > 0], 5) if np.any(a > 0) else 1e-12, 1e-12)
    db = 10 * np.log10(a + nf)
    lo, hi = np.percentile(db, low), np.percentile(db, high)
    rng = float(hi - lo)
    assert hi > lo, case
    assert abs(rng - 25) > 1e-3 and abs(rng - 20) > 1e-3, (case, rng)
    vmin = hi - 25 if rng > 25 else ((hi + lo) / 2 - 10 if rng < 20 else lo)
    assert vmin > -120 + 1e-3, (case, vmin)


def record_plot(out, case, f, t, Sxx, **kw):
    plt.close("all")
    quiet(refutils.plot_spectrogram, f, t, Sxx, **kw)
    fig = plt.figure(plt.get_fignums()[-1])
    rgba, vmin, vmax, lut = mesh_image(fig.axes[0].collections[0])
    plt.close("all")
    cols = 2 if len(t) == 1 else len(t)
    rgba = rgba.reshape(len(f), cols, 4)
    enhance = kw.get("enhance_contrast", True)
    check_levels(case, Sxx, 5 if enhance else 10.0, 95)
    out[f"{case}_index"] = to_index(rgba, lut)
    out[f"{case}_vmin"] = np.asarray(vmin)
    out[f"{case}_vmax"] = np.asarray(vmax)
    out[f"{case}_lut"] = lut
    out[f"{case}_enhance_contrast"] = np.asarray(enhance)
    out[f"{case}_high_detail_mode"] = np.asarray(kw.get("high_detail_mode", True))
    print(case, rgba.shape, repr(vmin), repr(vmax))


def main():
    rng = np.random.default_rng(20251020)
    out = {"sample_rate": np.float64(SR)}

    sig = capture(rng, 20_000, 6000, 5000, 4e6)
    f, t, Sxx = quiet(refutils.create_spectrogram, sig, SR)
    assert Sxx.shape == (512, 353) and Sxx.dtype == np.float32, (Sxx.shape, Sxx.dtype)
    out["sig_abc"] = sig
    record_plot(out, "a", f, t, Sxx)
    record_plot(out, "b", f, t, Sxx, enhance_contrast=False)
    record_plot(out, "c", f, t, Sxx, high_detail_mode=False)

    y = quiet(refutils.load_packet, os.path.join(REF, "data", "packet_2_chirp.mat"))
    sig_d = np.asarray(y[:4096], np.complex64)
    f, t, Sxx = quiet(refutils.create_spectrogram, sig_d, SR)
    out["sig_d"] = sig_d
    record_plot(out, "d", f, t, Sxx)

    e_sxx = (rng.exponential(size=(64, 1)) ** 2 * 1e-4).astype(np.float32)
    e_f = (np.arange(64) - 32) * (SR / 64)
    e_t = np.array([2.5e-6])
    out["e_sxx"], out["e_f"], out["e_t"] = e_sxx, e_f, e_t
    record_plot(out, "e", e_f, e_t, e_sxx)
    assert np.array_equal(out["e_index"][:, 0], out["e_index"][:, 1])

    # adjust_packet_bounds_gui, utils.py:1016-1022 and :1062
    sig_f = capture(rng, 6000, 1500, 2000, -9e6)
    f, t, Sxx = quiet(refutils.create_spectrogram, sig_f, SR, max_samples=2_000_000, time_resolution_us=1,
                      adaptive_resolution=True)
    Sxx_db, vmin, vmax = quiet(refutils.normalize_spectrogram, Sxx)
    assert f[0] < f[-1]
    f = f[::-1]
    Sxx_db = Sxx_db[::-1, :]
    fig, ax1 = plt.subplots()
    pcm = ax1.pcolormesh(t * 1000, f / 1e6, Sxx_db, shading="nearest", cmap="viridis", vmin=vmin, vmax=vmax)
    rgba, nvmin, nvmax, lut = mesh_image(pcm)
    plt.close("all")
    assert nvmin == vmin and nvmax == vmax
    check_levels("f", Sxx, 10.0, 95)
    out["sig_f"] = sig_f
    out["f_index"] = to_index(rgba.reshape(Sxx_db.shape + (4,)), lut)
    out["f_vmin"], out["f_vmax"], out["f_lut"] = np.asarray(vmin), np.asarray(vmax), lut
    print("f", out["f_index"].shape, repr(vmin), repr(vmax))

    out["cases"] = np.array(["a", "b", "c", "d", "e", "f"])
    out["meta_numpy"] = np.array(np.__version__)
    out["meta_scipy"] = np.array(scipy.__version__)
    out["meta_matplotlib"] = np.array(matplotlib.__version__)
    out["meta_reference"] = np.array("ramiyako/vector@2025-07-18 utils.py")
    path = os.path.join(HERE, "display.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < 1 << 20, "fixture over 1 MiB"


if __name__ == "__main__":
    main()
