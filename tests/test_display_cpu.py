"""Display image, the parts that need no device: the numpy restatement
(tests/display_ref.py) reproduces the reference's recorded images
(tests/golden/display.npz, written by make_golden_display.py from the
reference's plot_spectrogram / adjust_packet_bounds_gui through matplotlib)
byte for byte; the committed colour tables are matplotlib's; pool and extent
arithmetic; argument checks that run before any device work."""
import numpy as np
import pytest

import display_ref as dr
from oracle import ref

CASES = ["a", "b", "c", "d", "e", "f"]


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden(case):
    d = dr.golden_cases()[case]
    db, vmin, vmax = ref.normalize_spectrogram(d["Sxx"], **dr.golden_percentiles(d))
    assert vmin == d["vmin"] and vmax == d["vmax"]
    if d["kind"] == "plot":                       # utils.py:438, 443-448
        m = dr.median_rows(db)
        if len(d["t"]) == 1:
            m = np.hstack([m, m])
        img = dr.image(m, vmin, vmax, d["lut"])
    else:                                         # utils.py:1017-1022, 1062
        img = dr.image(db, vmin, vmax, d["lut"], flip=True)
    assert img.dtype == np.uint8 and img.shape == d["rgba"].shape
    assert np.array_equal(img, d["rgba"])
    # the kernel's order (maximum of |S| first, one logarithm a pixel) gives the same bytes
    S = d["Sxx"]
    img2 = dr.restate(S, dr.noise_floor(S), vmin, vmax, d["lut"], median=d["kind"] == "plot",
                      flip=d["kind"] == "gui")
    if len(d["t"]) == 1:
        img2 = np.hstack([img2, img2])
    assert np.array_equal(img2, d["rgba"])


def test_golden_shapes_and_maps():
    g = dr.golden_cases()
    assert g["a"]["Sxx"].shape == (512, 353) and g["a"]["Sxx"].dtype == np.float32
    assert g["e"]["rgba"].shape == (64, 2, 4)
    assert not np.array_equal(g["a"]["rgba"], g["b"]["rgba"])
    assert not np.array_equal(g["a"]["lut"], g["c"]["lut"])


def test_committed_tables_match_goldens():
    import vector_amd as va
    g = dr.golden_cases()
    for case, name in [("a", "turbo"), ("c", "inferno"), ("f", "viridis")]:
        t = va.colormap_table(name)
        assert t.shape == (259, 4) and t.dtype == np.uint8
        assert np.array_equal(t, g[case]["lut"])
        assert np.array_equal(t[256], t[0]) and np.array_equal(t[257], t[255])
        assert not t[258].any()
    assert len({tuple(r) for r in va.colormap_table("turbo")[:256]}) == 256


def test_committed_tables_match_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    import vector_amd as va
    for name in ("turbo", "inferno", "viridis"):
        cm = matplotlib.colormaps[name]
        x = np.linspace(0, 1, 256, endpoint=False) + 0.5 / 256
        assert np.array_equal(va.colormap_table(name)[:256], cm(x, bytes=True))
        ends = cm(np.array([-1.0, 2.0, np.nan]), bytes=True)
        assert np.array_equal(va.colormap_table(name)[256:], ends)


def test_custom_tables():
    import vector_amd as va
    t256 = (np.arange(1024) % 251).astype(np.uint8).reshape(256, 4)
    t = va.colormap_table(t256)
    assert t.shape == (259, 4)
    assert np.array_equal(t[:256], t256) and np.array_equal(t[256], t256[0])
    assert np.array_equal(t[257], t256[255]) and not t[258].any()
    t259 = (np.arange(1036) % 253).astype(np.uint8).reshape(259, 4)
    assert np.array_equal(va.colormap_table(t259), t259)
    for bad in (t256.astype(np.int32), t256[:, :3], t256[:100], "jet"):
        with pytest.raises(ValueError):
            va.colormap_table(bad)


def test_pool_factors():
    import vector_amd as va
    assert va.pool_factors((2048, 18707), None) == (1, 1)
    assert va.pool_factors((2048, 18707), (1024, 2048)) == (2, 10)
    assert va.pool_factors((512, 353), (1024, 2048)) == (1, 1)
    assert va.pool_factors((513, 353), (512, 353)) == (2, 1)
    assert va.pool_factors((5, 7), (1, 1)) == (5, 7)
    with pytest.raises(ValueError):
        va.pool_factors((5, 7), (0, 4))


def test_image_extent():
    import vector_amd as va
    f = (np.arange(8) - 4) * 1e6
    t = 1e-6 + np.arange(10) * 2e-6
    e = va.image_extent(f, t)
    np.testing.assert_allclose(e, (0.0, 20e-6, -4.5, 3.5), rtol=0, atol=1e-12)
    # pooled 3 x 4: 3 rows of 3 MHz, 3 columns of 8 us; the last blocks are partial
    e = va.image_extent(f, t, (3, 4))
    np.testing.assert_allclose(e, (0.0, 24e-6, -4.5, 4.5), rtol=0, atol=1e-12)
    rows, cols = -(-8 // 3), -(-10 // 4)
    dt, df = 4 * 2e-6, 3 * 1e6
    t0, t1 = e[0] + dt / 2, e[0] + dt / 2 + (cols - 1) * dt      # pixel centres
    f0, f1 = -4.5e6 + df / 2, -4.5e6 + df / 2 + (rows - 1) * df
    np.testing.assert_allclose(e, (t0 - dt / 2, t1 + dt / 2, (f0 - df / 2) / 1e6, (f1 + df / 2) / 1e6),
                               rtol=0, atol=1e-12)


def test_public_names_and_host_side_checks():
    import vector_amd as va
    for name in ("spectrogram_image", "spectrogram_levels", "plot_spectrogram_image", "SpectrogramImage"):
        assert hasattr(va, name), name
    assert va.SpectrogramImage._fields == ("rgba", "vmin", "vmax", "pool")
    S = np.ones((4, 5), np.float32)
    with pytest.raises(ValueError, match="expected a real array"):
        va.spectrogram_image(S.astype(np.complex64))
    with pytest.raises(ValueError):
        va.spectrogram_image(S, cmap="jet")
    for levels in [(1e-9, -30.0, -30.0), (1e-9, -30.0, -40.0), (1e-9, float("nan"), 0.0),
                   (1e-9, -30.0, float("inf"))]:
        with pytest.raises(ValueError):
            va.spectrogram_image(S, levels=levels)
    with pytest.raises(ValueError):
        va.spectrogram_image(S, max_size=(0, 1))
    img = va.spectrogram_image(np.zeros((0, 5), np.float32))
    assert img.rgba.shape == (0, 0, 4) and img.rgba.dtype == np.uint8 and (img.vmin, img.vmax) == (0, 0)
    assert va.spectrogram_levels(np.zeros((0, 5), np.float32)) == (0.0, 0, 0)


def test_library_declares_the_entry_point():
    import vector_amd as va
    lib = va.load_library()
    assert lib.vsig_spectrogram_image_dev.argtypes is not None
