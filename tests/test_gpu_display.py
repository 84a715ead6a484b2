"""GPU tests of the display image: display.hip's spectrogram_image kernel through
vsig_spectrogram_image_dev and vector_amd.spectrogram_image /
plot_spectrogram_image, against the numpy restatement (tests/display_ref.py)
and the reference's recorded images (tests/golden/display.npz).

1. Geometry, exact: every cell's dB sits at a bin centre (half a bin, 0.05 dB,
   from the nearest edge: thousands of float32 ulps), so the image must equal
   the restatement byte for byte whatever the last bits of the logarithm.
2. Special values: zero, above vmax, inf, NaN (alone, pooled, under the
   median), all-zero input.
3. Noise-like data and the goldens, by the interval rule: the device's float32
   dB map agrees with numpy's to a few ulp (the dB-map test of
   test_gpu_analysis.py allows 8), so a pixel within 8 ulp of a bin edge may
   land one row off.  The host dB map moved by -8 / +8 np.spacing gives
   o_lo <= o_hi per pixel; every GPU pixel must be the table row of some
   position in [o_lo, o_hi], hence exact where the two agree, and the pixels
   where they differ must be under 1 % of the image.
4. Determinism, tensor in / tensor out, levels reuse across a zoom, max_size
   shapes, the one-bin rule and extent, every refused argument.

Tile sizes below are display.hip's: 64 x 64 cells (frequency x time) for
frame-major input, 16 x 256 for C-contiguous input.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import display_ref as dr
from oracle import ref

pytestmark = pytest.mark.gpu

from display_ref import FLOOR, VMAX, VMIN, centred

LAYOUTS = ["time_fast", "freq_fast"]


def turbo(va):
    return va.colormap_table("turbo")


def on_device(S, layout):
    """(n_freq, n_time) device view of S over C-contiguous or frame-major memory."""
    if layout == "time_fast":
        return torch.from_numpy(S).to("cuda:0")
    return torch.from_numpy(np.ascontiguousarray(S.T)).to("cuda:0").t()


def render(va, T, **kw):
    kw.setdefault("levels", (FLOOR, VMIN, VMAX))
    kw.setdefault("cmap", "turbo")
    return va.spectrogram_image(T, **kw).rgba.cpu().numpy()


def expected(va, S, median=False, flip=False, pool=(1, 1)):
    return dr.restate(S, FLOOR, VMIN, VMAX, turbo(va), median, flip, pool)


def size_for(shape, pool):
    """max_size that gives these pool factors (for factors pool_factors can give)."""
    return tuple(-(-n // p) for n, p in zip(shape, pool))


def render_dev(va, T, median, flip, pool):
    """The entry point itself, with pool factors max_size cannot ask for."""
    from vector_amd.display import _layout
    t, freq_fast, ld = _layout(T)
    nf, nt = t.shape
    rows, cols = -(-nf // pool[0]), -(-nt // pool[1])
    lut = torch.from_numpy(turbo(va).copy()).to(t.device)
    out = torch.empty((rows, cols, 4), dtype=torch.uint8, device=t.device)
    ctx = va.get_context()
    code = va._lib.DTYPES["f32" if t.dtype == torch.float32 else "f64"]
    ctx.check(ctx.lib.vsig_spectrogram_image_dev(
        ctx.h, code, C.c_void_p(t.data_ptr()), nf, nt, freq_fast, ld, FLOOR, VMIN, VMAX, int(median),
        int(flip), pool[0], pool[1], C.c_void_p(lut.data_ptr()), C.c_void_p(out.data_ptr())), "image")
    return out.cpu().numpy()


def check_exact(va, S, T, median=False, flip=False, pool=(1, 1)):
    ms = size_for(S.shape, pool)
    if va.pool_factors(S.shape, ms) == pool:
        got = render(va, T, median_filter=median, flip_freq=flip, max_size=ms)
    else:
        got = render_dev(va, T, median, flip, pool)
    want = expected(va, S, median, flip, pool)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (S.shape, S.dtype, median, flip, pool,
                                       np.argwhere(np.any(got != want, axis=-1))[:5])


# ---------------------------------------------------------------- 1. geometry
SHAPES = [(1, 1), (1, 7), (2, 1), (3, 5),
          (64, 64), (65, 64), (63, 64), (64, 65), (64, 63),          # the frame-major tile
          (16, 256), (17, 256), (15, 256), (16, 257), (16, 255),     # the C-contiguous tile
          (257, 130), (512, 353), (2048, 1200)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_geometry_exact(gpu, shape, layout):
    nf, nt = shape
    S32 = centred(nf, nt, np.float32)
    T32 = on_device(S32, layout)
    # one option away from the default at a time, then together
    for opt in [dict(), dict(median=True), dict(flip=True), dict(pool=(2, 3)), dict(pool=(7, 5)),
                dict(pool=(nf + 5, 2)), dict(pool=(3, nt + 9)),
                dict(median=True, flip=True, pool=(2, 3)), dict(median=True, pool=(7, 5))]:
        check_exact(gpu, S32, T32, **opt)
    S64 = centred(nf, nt, np.float64)
    T64 = on_device(S64, layout)
    for opt in [dict(), dict(median=True, flip=True, pool=(2, 3)), dict(pool=(7, 5))]:
        check_exact(gpu, S64, T64, **opt)


VIEWS = [(slice(1, None), slice(None)), (slice(None), slice(3, -2)), (slice(5, 70), slice(9, 200)),
         (slice(None), slice(4, 99)), (slice(8, 70), slice(None)), (slice(8, 71), slice(4, 103))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_geometry_views(gpu, layout, dt):
    """Slices are rendered where they lie: unaligned bases, ld above the
    extent, 16-byte rows with a ragged end, the median's halo taken inside the
    view (row 0 of a slice reflects onto itself, not onto memory below it)."""
    for nf, nt in [(96, 232), (77, 231)]:                 # even and odd fast extents
        S = centred(nf, nt, dt)
        T = on_device(S, layout)
        for v in VIEWS:
            Sv, Tv = S[v], T[v]
            assert Tv.data_ptr() == T.data_ptr() + T.element_size() * (
                (v[0].start or 0) * T.stride(0) + (v[1].start or 0) * T.stride(1))
            for opt in [dict(), dict(median=True), dict(median=True, flip=True, pool=(2, 3))]:
                check_exact(gpu, Sv, Tv, **opt)


def test_stepped_slice_and_numpy_input(gpu):
    S = centred(70, 90, np.float32)
    T = on_device(S, "time_fast")
    check_exact(gpu, S[::2, ::3], T[::2, ::3], median=True)      # gathered first
    got = gpu.spectrogram_image(S.T[3:, 1:].T, levels=(FLOOR, VMIN, VMAX), cmap="turbo", median_filter=True)
    assert isinstance(got.rgba, np.ndarray)
    assert np.array_equal(got.rgba, expected(gpu, S[1:, 3:], median=True))


# ---------------------------------------------------------------- 2. special values
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_special_values(gpu, layout, dt):
    lut = turbo(gpu)
    S = centred(40, 50, dt)
    S[3, 4] = 0                      # 10 log10(floor) = -70 dB: under
    S[5, 6] = 1.0                    # 0 dB: over
    S[7, 8] = np.inf
    S[20, 30] = np.nan
    S[9, 9] = -S[9, 9]               # |S|
    T = on_device(S, layout)
    img = render(gpu, T)
    assert np.array_equal(img, expected(gpu, S))
    assert np.array_equal(img[3, 4], lut[dr.UNDER]) and np.array_equal(img[3, 4], lut[0])
    assert np.array_equal(img[5, 6], lut[dr.OVER]) and np.array_equal(img[7, 8], lut[dr.OVER])
    assert np.array_equal(img[20, 30], lut[dr.BAD]) and not img[20, 30].any()
    assert np.all(np.any(img[19] != lut[dr.BAD], axis=-1))
    # the median filter: the NaN takes its upper neighbour with it
    img = render(gpu, T, median_filter=True)
    assert np.array_equal(img, expected(gpu, S, median=True))
    assert not img[20, 30].any() and not img[21, 30].any() and img[19, 30].any() and img[22, 30].any()
    # pooled: the NaN makes its whole pixel bad, and only that one
    img = render(gpu, T, max_size=size_for(S.shape, (4, 5)))
    assert np.array_equal(img, expected(gpu, S, pool=(4, 5)))
    bad = ~np.any(img != lut[dr.BAD], axis=-1)
    assert bad.sum() == 1 and bad[5, 6]


def test_all_zero_is_uniform(gpu):
    Z = np.zeros((33, 70), np.float32)
    img = gpu.spectrogram_image(Z, cmap="viridis")
    assert np.all(img.rgba == gpu.colormap_table("viridis")[0])
    rdb, rvmin, rvmax = ref.normalize_spectrogram(Z)
    assert (img.vmin, img.vmax) == (rvmin, rvmax)


def test_custom_table(gpu):
    S = centred(20, 30, np.float32)
    tab = (np.arange(1024) * 7 % 256).astype(np.uint8).reshape(256, 4)
    img = render(gpu, on_device(S, "time_fast"), cmap=tab)
    assert np.array_equal(img, dr.restate(S, FLOOR, VMIN, VMAX, gpu.colormap_table(tab)))


# ---------------------------------------------------------------- 3. the interval rule
def check_interval(S, img, floor, vmin, vmax, lut, median, flip=False, pool=(1, 1)):
    m = dr.db_map(dr.pooled_abs(S, median, pool), floor)
    if flip:
        m = m[::-1]
    o_lo, o_hi = dr.interval(m, vmin, vmax)
    assert np.all(o_lo <= o_hi)
    share = np.mean(o_lo != o_hi)
    print(f"pixels within 8 ulp of a bin edge: {100 * share:.3f} %")
    assert share < 0.01
    ok = dr.within_interval(img, o_lo, o_hi, lut)
    assert ok.all(), (np.argwhere(~ok)[:5], (~ok).sum())
    return share


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(2025)
    S32 = (rng.exponential(size=(300, 517)) ** 3 * 1e-6).astype(np.float32)
    S32[:, ::17] = 0
    S64 = rng.exponential(size=(130, 211)) ** 2 * 1e-3
    return [S32, S64]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_noise_interval(gpu, noise, layout):
    for S in noise:
        for kw, median, pool in [(dict(), False, (1, 1)),
                                 (dict(low_percentile=5, high_percentile=95, median_filter=True), True, (1, 1)),
                                 (dict(max_size=(100, 100)), False, gpu.pool_factors(S.shape, (100, 100)))]:
            got = gpu.spectrogram_image(on_device(S, layout), cmap="turbo", **kw)
            pct = {k: v for k, v in kw.items() if k.endswith("percentile")}
            _, rvmin, rvmax = ref.normalize_spectrogram(S, **pct)
            assert got.vmin == rvmin and got.vmax == rvmax and type(got.vmin) is type(rvmin)
            assert got.pool == pool
            floor = gpu.spectrogram_levels(S, **pct)[0]
            assert floor == float(dr.noise_floor(S))
            check_interval(S, got.rgba.cpu().numpy(), floor, got.vmin, got.vmax, turbo(gpu), median, pool=pool)


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_golden_interval(gpu, case):
    d = dr.golden_cases()[case]
    S = d["Sxx"]
    if d["kind"] == "plot":
        rgba, extent, vmin, vmax = gpu.plot_spectrogram_image(
            d["f"], d["t"], S, enhance_contrast=d["enhance_contrast"], high_detail_mode=d["high_detail_mode"])
    else:
        img = gpu.spectrogram_image(S, cmap="viridis", flip_freq=True)
        rgba, vmin, vmax = img.rgba, img.vmin, img.vmax
    assert rgba.shape == d["rgba"].shape
    assert abs(float(vmin) - float(d["vmin"])) <= 1e-5 and abs(float(vmax) - float(d["vmax"])) <= 1e-5
    one_bin = d["kind"] == "plot" and len(d["t"]) == 1
    if one_bin:
        assert np.array_equal(rgba[:, 0], rgba[:, 1])
        rgba, want = rgba[:, :1], d["rgba"][:, :1]
    else:
        want = d["rgba"]
    floor = float(dr.noise_floor(S))
    check_interval(S, rgba, floor, vmin, vmax, d["lut"], d["kind"] == "plot", flip=d["kind"] == "gui")
    differ = np.mean(np.any(rgba != want, axis=-1))
    print(f"pixels that differ from the reference's image: {100 * differ:.3f} %")
    assert differ < 0.01
    if vmin == d["vmin"] and vmax == d["vmax"]:
        # the reference's own image obeys the same rule
        check_interval(S, want, floor, vmin, vmax, d["lut"], d["kind"] == "plot", flip=d["kind"] == "gui")


# ---------------------------------------------------------------- 4. other behaviour
def test_deterministic(gpu, noise):
    T = on_device(noise[0], "freq_fast")
    kw = dict(median_filter=True, max_size=(64, 100), levels=(1e-9, -80.0, -50.0))
    a = gpu.spectrogram_image(T, **kw).rgba
    b = gpu.spectrogram_image(T, **kw).rgba
    assert torch.equal(a, b)


def test_tensor_in_tensor_out_and_max_size(gpu):
    S = centred(130, 517, np.float32)
    T = on_device(S, "freq_fast")
    img = gpu.spectrogram_image(T, levels=(FLOOR, VMIN, VMAX))
    assert isinstance(img.rgba, torch.Tensor) and img.rgba.device == T.device
    assert img.rgba.dtype == torch.uint8 and img.rgba.is_contiguous() and tuple(img.rgba.shape) == (130, 517, 4)
    assert img.pool == (1, 1) and (img.vmin, img.vmax) == (VMIN, VMAX)
    for ms, pool, shape in [((65, 100), (2, 6), (65, 87)), ((130, 517), (1, 1), (130, 517)),
                            ((1000, 1000), (1, 1), (130, 517)), ((1, 1), (130, 517), (1, 1)),
                            ((64, 516), (3, 2), (44, 259))]:
        img = gpu.spectrogram_image(T, levels=(FLOOR, VMIN, VMAX), max_size=ms)
        assert img.pool == pool and tuple(img.rgba.shape) == shape + (4,)
    e = gpu.spectrogram_image(torch.empty((0, 7), device="cuda:0"))
    assert isinstance(e.rgba, torch.Tensor) and tuple(e.rgba.shape) == (0, 0, 4) and (e.vmin, e.vmax) == (0, 0)


def test_levels_reuse_across_zoom(gpu, noise):
    S = noise[0]
    T = on_device(S, "freq_fast")
    full = gpu.spectrogram_image(T, cmap="inferno")
    levels = (gpu.spectrogram_levels(T)[0], full.vmin, full.vmax)
    zoom = gpu.spectrogram_image(T[40:200, 100:400], cmap="inferno", levels=levels)
    assert (zoom.vmin, zoom.vmax) == (full.vmin, full.vmax)
    assert torch.equal(zoom.rgba, full.rgba[40:200, 100:400])


def test_plot_image_one_bin_and_extent(gpu):
    S = centred(64, 1, np.float32)
    f = (np.arange(64) - 32) * 1e6
    t = np.array([2.5e-6])
    rgba, extent, vmin, vmax = gpu.plot_spectrogram_image(f, t, S)
    assert rgba.shape == (64, 2, 4) and np.array_equal(rgba[:, 0], rgba[:, 1])
    np.testing.assert_allclose(extent, (1.5e-6, 3.5e-6, -32.5, 31.5), rtol=0, atol=1e-12)
    _, rvmin, rvmax = ref.normalize_spectrogram(S, 5, 95, 25)
    assert (vmin, vmax) == (rvmin, rvmax)
    S = centred(64, 40, np.float32)
    t = np.arange(40) * 1e-6
    rgba, extent, _, _ = gpu.plot_spectrogram_image(f, t, torch.from_numpy(S).to("cuda:0"), max_size=(16, 10))
    assert isinstance(rgba, torch.Tensor) and tuple(rgba.shape) == (16, 10, 4)
    np.testing.assert_allclose(extent, (-0.5e-6, 39.5e-6, -32.5, 31.5), rtol=0, atol=1e-12)
    lo = gpu.plot_spectrogram_image(f, t, S, high_detail_mode=False)[0]
    hi = gpu.plot_spectrogram_image(f, t, S)[0]
    assert lo.shape == hi.shape == (64, 40, 4) and not np.array_equal(lo, hi)


def image_dev(va, T, n_freq, n_time, freq_fast, ld, levels=(FLOOR, VMIN, VMAX), pool=(1, 1), dtype=None,
              sxx="T", lut="L", out="O"):
    ctx = va.get_context()
    L = torch.from_numpy(va.colormap_table("turbo").copy()).to("cuda:0")
    O = torch.zeros(max(1, n_freq * n_time) * 4 + 8, dtype=torch.uint8, device="cuda:0")
    p = {"T": T, "L": L, "O": O}
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    dtype = va._lib.DTYPES["f32"] if dtype is None else dtype
    return ctx.lib.vsig_spectrogram_image_dev(
        ctx.h, dtype, ptr(p.get(sxx)), n_freq, n_time, freq_fast, ld, *levels, 0, 0, pool[0], pool[1],
        ptr(p.get(lut)), ptr(p.get(out))), O


def test_refused_arguments(gpu):
    S = centred(8, 12, np.float32)
    T = torch.from_numpy(S).to("cuda:0")
    ok, O = image_dev(gpu, T, 8, 12, 0, 12)
    assert ok == 0
    torch.cuda.synchronize()
    assert np.array_equal(O[:8 * 12 * 4].cpu().numpy().reshape(8, 12, 4), expected(gpu, S))
    inv = -1
    for kw in [dict(sxx=None), dict(lut=None), dict(out=None)]:
        assert image_dev(gpu, T, 8, 12, 0, 12, **kw)[0] == inv
    assert image_dev(gpu, T, 0, 12, 0, 12)[0] == inv
    assert image_dev(gpu, T, 8, 0, 0, 12)[0] == inv
    assert image_dev(gpu, T, 8, 12, 0, 12, pool=(0, 1))[0] == inv
    assert image_dev(gpu, T, 8, 12, 0, 12, pool=(1, 0))[0] == inv
    assert image_dev(gpu, T, 8, 12, 0, 11)[0] == inv                  # ld below the fast extent
    assert image_dev(gpu, T, 12, 8, 1, 11)[0] == inv
    for dtype in (gpu._lib.DTYPES["c64"], gpu._lib.DTYPES["c128"], 7):
        assert image_dev(gpu, T, 8, 12, 0, 12, dtype=dtype)[0] == inv
    for levels in [(FLOOR, -35.0, -35.0), (FLOOR, -35.0, -60.0), (FLOOR, float("nan"), -35.0),
                   (FLOOR, -60.0, float("inf")), (FLOOR, float("-inf"), -35.0)]:
        assert image_dev(gpu, T, 8, 12, 0, 12, levels=levels)[0] == inv
    assert image_dev(gpu, T, 8, 12, 0, 12)[0] == 0                   # the context still works
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="expected a real array"):
        gpu.spectrogram_image(T.to(torch.complex64))
    for levels in [(FLOOR, -35.0, -35.0), (FLOOR, -35.0, -60.0), (FLOOR, float("nan"), -35.0),
                   (FLOOR, -60.0, float("inf"))]:
        with pytest.raises(ValueError):
            gpu.spectrogram_image(T, levels=levels)
    with pytest.raises(ValueError):
        gpu.spectrogram_image(T[0])
    torch.cuda.synchronize()


def test_normalize_spectrogram_unchanged(gpu, noise, capsys):
    for S in noise:
        db, vmin, vmax = gpu.normalize_spectrogram(S)
        rdb, rvmin, rvmax = ref.normalize_spectrogram(S)
        assert db.dtype == rdb.dtype and db.shape == rdb.shape
        assert vmin == rvmin and vmax == rvmax and type(vmin) is type(rvmin)
        assert np.all(np.abs(db - rdb) <= 8 * np.spacing(np.abs(rdb)) + 1e-30)
        floor, lvmin, lvmax = gpu.spectrogram_levels(S)
        assert (lvmin, lvmax) == (vmin, vmax) and isinstance(floor, float)
    assert "Dynamic range adjusted" in capsys.readouterr().out
