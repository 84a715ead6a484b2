"""CPU checks of the per-burst spectra and measurements: the numpy / scipy
statements the GPU tests compare against, the host-side rules of
segment_spectra / measure_packets, and the argument checks that come before
any device is needed."""
import ctypes as C

import numpy as np
import pytest

import accuracy_ref as acc
import packet_spectra_ref as ps
import spectrum_traces_ref as st
from vector_amd import _lib, packets


# ---------------------------------------------------------------------------
# the reference statements
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nperseg,noverlap,nfft", [(64, 0, 64), (100, 30, 128), (256, 128, 256)])
def test_segment_traces_mean_is_welch_of_the_slice(nperseg, noverlap, nfft):
    x = acc.noise(5000, seed=nfft)
    starts = np.array([0, 777, 777, 2000, 4000])
    ends = np.array([999, 1500, 1500, 2000 + nperseg - 1, 4999])
    got = ps.segment_traces(x, starts, ends, "hann", nperseg, noverlap, nfft)
    for k, (s, e) in enumerate(zip(starts, ends)):
        _, want = st.welch_mean(x[s:e + 1], 1.0, "hann", nperseg, noverlap, nfft)
        np.testing.assert_allclose(got["mean"][k], want, rtol=1e-10, atol=0)
        assert np.all(got["min"][k] <= got["mean"][k]) and np.all(got["mean"][k] <= got["max"][k])
    assert np.array_equal(got["mean"][1], got["mean"][2])
    assert np.array_equal(got["max"][3], got["min"][3])            # one frame


def test_segment_traces_short_segment_is_nan():
    x = acc.noise(1000, seed=1)
    got = ps.segment_traces(x, [0, 10], [62, 200], "hann", 64, 0, 64)
    for d in st.DETECTORS:
        assert np.all(np.isnan(got[d][0])) and np.all(np.isfinite(got[d][1]))


def test_nframes_rule():
    lengths = [0, 1, 63, 64, 65, 127, 128, 1000]
    assert list(ps.nframes(lengths, 64, 64)) == [0, 0, 0, 1, 1, 1, 2, 15]
    assert list(ps.nframes(lengths, 64, 16)) == [0, 0, 0, 1, 1, 4, 5, 59]
    for hop in (64, 16, 1):
        assert np.array_equal(packets.segment_frames(lengths, 64, hop), ps.nframes(lengths, 64, hop))


def test_default_nperseg_rule():
    for shortest, want in ((1, 64), (63, 64), (64, 64), (127, 64), (128, 128), (1000, 512), (1024, 1024),
                           (1 << 20, 1024)):
        assert packets.default_nperseg(np.array([shortest, shortest + 5000])) == want, shortest
    assert packets.default_nperseg(np.zeros(0, np.int64)) == 64
    starts, lengths, win, nperseg, hop, nfft, nf = packets._plan_args(
        10000, [0, 3000], [299, 9999], "hann", None, 0, None)
    assert (nperseg, hop, nfft) == (256, 256, 256) and win.dtype == np.float32 and list(nf) == [1, 27]
    assert list(lengths) == [300, 7000]


# ---------------------------------------------------------------------------
# the band reference on hand-made rows
# ---------------------------------------------------------------------------
def test_band_single_bin():
    m = np.zeros(100)
    m[37] = 2.5
    for tail in (1e-4, 0.005, 0.25):
        b = ps.band(m, tail)
        assert b == dict(power=2.5, centroid=37.0, peak=2.5, peak_bin=37, lo_bin=37, hi_bin=37)


def test_band_flat_row():
    nbins = 64
    b = ps.band(np.ones(nbins), 0.125)
    assert b["power"] == nbins and b["centroid"] == (nbins - 1) / 2 and b["peak_bin"] == 0 and b["peak"] == 1.0
    assert (b["lo_bin"], b["hi_bin"]) == (7, 55)                    # c[7] = 8 = 64 / 8; c[55] = 56
    assert b["lo_bin"] + b["hi_bin"] == nbins - 2                   # symmetric up to the inclusive sum


def test_band_zero_and_nan_rows():
    z = ps.band(np.zeros(16), 0.005)
    assert z["power"] == 0.0 and np.isnan(z["centroid"]) and np.isnan(z["peak"])
    assert (z["peak_bin"], z["lo_bin"], z["hi_bin"]) == (-1, -1, -1)
    m = np.ones(16)
    m[3] = np.nan
    n = ps.band(m, 0.005)
    assert np.isnan(n["power"]) and np.isnan(n["centroid"]) and (n["peak_bin"], n["lo_bin"], n["hi_bin"]) == (-1,) * 3


def test_vetted_rows_meet_the_premise():
    tails = (1e-4, 0.005, 0.05, 0.25)
    for kind in ps.ROW_KINDS:
        for nbins in (64, 100, 1000):
            m, seed = ps.vetted_row(kind, nbins, tails, 2.0 ** -40, nbins)
            assert all(ps.band_margin(m, t) > ps.PREMISE for t in tails)
            m2, seed2 = ps.vetted_row(kind, nbins, tails, 2.0 ** 40, nbins)
            assert seed2 == seed and np.array_equal(m2, m * 2.0 ** 80)       # the gain is exact


# ---------------------------------------------------------------------------
# Hz conversions
# ---------------------------------------------------------------------------
def test_band_to_hz_matches_the_table():
    nfft, sr, cf = 256, 20e6, 2.4e9
    win = acc.window32("hann", 200)
    recs = np.zeros(3, packets.BAND_DTYPE)
    rows = [np.random.default_rng(5).exponential(1.0, nfft), np.zeros(nfft)]
    bands = [ps.band(r, 0.005) for r in rows] + [dict(power=np.nan, centroid=np.nan, peak=np.nan, peak_bin=-1,
                                                      lo_bin=-1, hi_bin=-1)]
    for rec, b in zip(recs, bands):
        for k, v in b.items():
            rec[k] = v
    got = packets.band_to_hz(recs, [4, 2, 0], nfft, sr, cf, win)
    for i, b in enumerate(bands):
        want = ps.to_hz(b, nfft, sr, cf, win)
        for k, v in want.items():
            assert np.array_equal(got[k][i], v, equal_nan=True), (i, k)
    assert got["nframes"].dtype == np.int64 and list(got["nframes"]) == [4, 2, 0]
    assert got["power"][1] == 0.0 and np.isnan(got["bandwidth"][1]) and np.isnan(got["power"][2])
    df = sr / nfft
    assert got["bandwidth"][0] == pytest.approx(got["f_hi"][0] - got["f_lo"][0], rel=1e-12)
    assert round(got["bandwidth"][0] / df) == bands[0]["hi_bin"] - bands[0]["lo_bin"] + 1


def test_power_is_mean_square_for_a_boxcar():
    nfft = 128
    x = acc.noise(4 * nfft, seed=3).astype(np.complex128)
    tr = ps.segment_traces(x, [0], [len(x) - 1], "boxcar", nfft, 0, nfft, fftshift=True)
    b = ps.band(tr["mean"][0], 0.005)
    p = ps.to_hz(b, nfft, 1.0, 0.0, np.ones(nfft, np.float32))["power"]
    assert p == pytest.approx(np.mean(np.abs(x) ** 2), rel=1e-12)


# ---------------------------------------------------------------------------
# argument errors: Python, with no device
# ---------------------------------------------------------------------------
def test_python_argument_errors_come_before_the_device():
    x = np.ones(4096, np.complex64)
    s, e = [0, 1000], [511, 3000]
    ss = packets.segment_spectra
    for kw, exc, match in (
            (dict(starts=[0, 1], ends=[5]), ValueError, "one length"),
            (dict(starts=[[0]], ends=[[5]]), ValueError, "1-D"),
            (dict(starts=[0.5], ends=[5.0]), ValueError, "integers"),
            (dict(starts=[-1], ends=[5]), ValueError, "segment 0"),
            (dict(starts=[0, 7], ends=[5, 6]), ValueError, "segment 1"),
            (dict(starts=[0, 10], ends=[5, 4096]), ValueError, "segment 1"),
            (dict(nperseg=0), ValueError, "nperseg"),
            (dict(nperseg=128, nfft=64), ValueError, "nfft"),
            (dict(nperseg=100, nfft=100), NotImplementedError, "power of two"),
            (dict(nperseg=32, nfft=32), NotImplementedError, "power of two"),
            (dict(nperseg=64, nfft=16384), NotImplementedError, "power of two"),
            (dict(nperseg=64, noverlap=64), ValueError, "noverlap"),
            (dict(nperseg=64, noverlap=-1), ValueError, "noverlap"),
            (dict(window=np.ones(64), nperseg=32), ValueError, "length of window"),
            (dict(window=np.ones((2, 64))), ValueError, "1-D"),
            (dict(detectors=("median",)), ValueError, "detector"),
            (dict(detectors=()), ValueError, "no detector")):
        args = dict(starts=s, ends=e)
        args.update(kw)
        with pytest.raises(exc, match=match):
            ss(x, args.pop("starts"), args.pop("ends"), **args)
    with pytest.raises(ValueError, match="1-D"):
        ss(np.ones((2, 64), np.complex64), s, e)
    for fs in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="fs must"):
            ss(x, s, e, fs)
    with pytest.raises(ValueError, match="empty"):
        ss(np.ones(0, np.complex64), [], [])
    mp = packets.measure_packets
    for occ in (0.0, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="occupied"):
            mp(x, (s, e), 1e6, occupied=occ)
    with pytest.raises(ValueError, match="sample_rate"):
        mp(x, (s, e), 0.0)
    with pytest.raises(ValueError, match="segment 1"):
        mp(x, ([0, 7], [5, 6]), 1e6)


def test_valid_call_needs_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    import vector_amd as va
    x = np.ones(4096, np.complex64)
    with pytest.raises(va.VsigUnavailable):
        va.segment_spectra(x, [0], [511])
    with pytest.raises(va.VsigUnavailable):
        va.measure_packets(x, ([0], [511]), 1e6)


# ---------------------------------------------------------------------------
# the C entry points
# ---------------------------------------------------------------------------
def test_abi_names_and_struct_sizes():
    for name in ("vsig_psd_segments_create", "vsig_psd_segments_free", "vsig_psd_segments_info",
                 "vsig_psd_segments_run", "vsig_band_measure_run"):
        assert name in _lib.SIGNATURES and not name.endswith("_dev")
    assert C.sizeof(_lib.Segment) == 16 and C.sizeof(_lib.Band) == 40
    assert packets.BAND_DTYPE.itemsize == 40
    assert [packets.BAND_DTYPE.fields[n][1] for n in packets.BAND_DTYPE.names] == \
        [getattr(_lib.Band, n).offset for n, _ in _lib.Band._fields_]


def test_bad_arguments_are_refused_before_a_context_is_needed():
    """Every refusal comes before the first HIP call: with no context (and, on
    a box without a device, none to be had) each call returns VSIG_E_INVALID
    and leaves `out` alone."""
    lib = _lib.load_library()
    seg = (_lib.Segment * 2)(_lib.Segment(0, 100), _lib.Segment(50, 200))
    bad = (_lib.Segment * 2)(_lib.Segment(0, 100), _lib.Segment(200, 57))
    neg = (_lib.Segment * 1)(_lib.Segment(-1, 10))
    negl = (_lib.Segment * 1)(_lib.Segment(5, -1))
    for args in (
            (None, seg, 2, 256, 64, 64, 64),                    # the null context alone
            (None, seg, -1, 256, 64, 64, 64),                   # nseg < 0
            (None, seg, (1 << 24) + 1, 256, 64, 64, 64),        # nseg > 2^24
            (None, seg, 2, 0, 64, 64, 64),                      # n < 1
            (None, seg, 2, (1 << 40) + 1, 64, 64, 64),          # n > 2^40
            (None, bad, 2, 256, 64, 64, 64),                    # segment 1 ends at 257 > n
            (None, neg, 1, 256, 64, 64, 64),                    # start < 0
            (None, negl, 1, 256, 64, 64, 64),                   # len < 0
            (None, seg, 2, 256, 64, 0, 64),                     # hop < 1
            (None, seg, 2, 256, 0, 64, 64),                     # nperseg < 1
            (None, seg, 2, 256, 128, 64, 64),                   # nfft < nperseg
            (None, None, 2, 256, 64, 64, 64)):                  # NULL table
        out = C.c_void_p(0x1234)
        assert lib.vsig_psd_segments_create(*args, C.byref(out)) == -1, args
        assert out.value == 0x1234
    assert lib.vsig_psd_segments_create(None, seg, 2, 256, 64, 64, 64, None) == -1     # NULL out
    x = np.zeros(64, np.complex64)
    w = np.ones(64, np.float32)
    m = np.zeros(64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert lib.vsig_psd_segments_run(None, p(x), p(w), 1.0, 0, p(m), None, None) == -1  # NULL plan
    assert lib.vsig_psd_segments_info(None, None, None, None, None) == -1
    lib.vsig_psd_segments_free(None)                                                    # a no-op
    rows = np.ones((2, 64))
    rec = (_lib.Band * 2)()
    rp = C.cast(rec, C.c_void_p)
    before = bytes(rec)
    for args in (
            (None, p(rows), 2, 64, 64, 0.005, rp),              # the null context alone
            (None, p(rows), -1, 64, 64, 0.005, rp),             # nrows < 0
            (None, p(rows), 2, 0, 64, 0.005, rp),               # nbins < 1
            (None, p(rows), 2, 64, 63, 0.005, rp),              # ld < nbins
            (None, p(rows), 2, 64, 64, 0.0, rp),                # tail outside (0, 0.5)
            (None, p(rows), 2, 64, 64, 0.5, rp),
            (None, p(rows), 2, 64, 64, float("nan"), rp),
            (None, None, 2, 64, 64, 0.005, rp),                 # NULL rows
            (None, p(rows), 2, 64, 64, 0.005, None)):           # NULL out
        assert lib.vsig_band_measure_run(*args) == -1, args
    assert bytes(rec) == before
