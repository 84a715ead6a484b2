"""isolate_packets' host side, no device: the tap design against
scipy.signal.firwin, the frame planner against its restatement, the burst table,
the argument errors (all before the device is touched) and the export."""
import numpy as np
import pytest
import scipy.signal

import isolate_ref as iso
from vector_amd import _lib, packets as pk

SR = 56e6


# ---------------------------------------------------------------------------
# taps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 63, 255])
def test_design_lowpass_is_firwin(T):
    """float64, before the rounding to float32; 1e-12 absolute on taps that sum to 1."""
    seen = 0
    for bw in (0.0, SR / 500, SR / 50, 2e6, SR / 8, SR / 3):
        fc = bw / 2 + 1.65 * SR / T
        assert pk.lowpass_cutoff(bw, SR, T) == pytest.approx(fc, rel=1e-15)
        h = pk.design_lowpass(bw, SR, T, dtype=np.float64)
        assert h.dtype == np.float64 and h.shape == (T,)
        if fc >= SR / 2:
            continue
        seen += 1
        want = scipy.signal.firwin(T, fc, fs=SR)
        assert np.abs(h - want).max() <= 1e-12
        h32 = pk.design_lowpass(bw, SR, T)        # rounded once
        assert h32.dtype == np.float32 and np.abs(h32.astype(np.float64) - want).max() <= 2.0 ** -24 * want.max()
    if T == 3:                                    # 1.65 sr / 3 is past sr / 2: every design above is the impulse
        assert seen == 0
        for fc in (SR / 10, SR / 4, 0.49 * SR):
            assert np.abs(pk._lowpass_taps(fc, SR, T) - scipy.signal.firwin(T, fc, fs=SR)).max() <= 1e-12
    else:
        assert seen == 6


@pytest.mark.parametrize("T", [3, 63, 255, 511])
def test_design_lowpass_impulse_from_nyquist_on(T):
    d = (T - 1) // 2
    edge = 2 * (SR / 2 - 1.65 * SR / T)           # the bandwidth whose cutoff is sr / 2
    for bw in (max(edge, 0.0) * (1 + 1e-12) + 1e-3, SR, 10 * SR):
        h = pk.design_lowpass(bw, SR, T)
        assert h[d] == 1.0 and np.count_nonzero(h) == 1
    if edge > 0:
        h = pk.design_lowpass(edge * (1 - 1e-9), SR, T, dtype=np.float64)
        assert np.count_nonzero(h) > 1 and abs(h.sum() - 1) < 1e-12


def test_design_lowpass_errors():
    for bad in (2, 4, 1, 0, -3, 254):
        with pytest.raises(ValueError):
            pk.design_lowpass(1e6, SR, bad)
    with pytest.raises(NotImplementedError):
        pk.design_lowpass(1e6, SR, 513)
    for bw, sr in ((-1.0, SR), (np.nan, SR), (np.inf, SR), (1e6, 0.0), (1e6, -1.0), (1e6, np.inf)):
        with pytest.raises(ValueError):
            pk.design_lowpass(bw, sr, 255)


# ---------------------------------------------------------------------------
# planner
# ---------------------------------------------------------------------------
def _segments(hop, n):
    lens = [1, 2, hop - 1, hop, hop + 1, 2 * hop - 1, 2 * hop, 2 * hop + 1, 3 * hop + 1]
    rng = np.random.default_rng(hop)
    starts = [int(rng.integers(0, n - ln + 1)) for ln in lens]
    starts[0], starts[3] = 0, n - lens[3]
    starts += [starts[4], starts[5] + 7]           # one repeated, one overlapping
    lens += [lens[4], lens[5]]
    order = rng.permutation(len(lens))              # unordered
    return [starts[i] for i in order], [lens[i] for i in order]


@pytest.mark.parametrize("T", [3, 63, 255, 511])
def test_planner_matches_its_restatement(T):
    n = 10_007
    hop = 1025 - T
    starts, lens = _segments(hop, n)
    fr = pk.isolate_frames(starts, lens, T)
    want, offsets = iso.frames(starts, lens, T)
    assert fr.hop == hop
    assert fr.offsets.tolist() == offsets == np.concatenate(([0], np.cumsum(lens))).tolist()
    assert list(zip(fr.seg.tolist(), fr.x0.tolist(), fr.y0.tolist(), fr.keep.tolist())) == want
    assert fr.keep.min() >= 1 and fr.keep.max() <= hop
    # every output index of every segment is owned by exactly one frame, in place
    owner = np.zeros(offsets[-1], np.int64)
    d = (T - 1) // 2
    for s, x0, y0, keep in want:
        owner[y0:y0 + keep] += 1
        assert offsets[s] <= y0 and y0 + keep <= offsets[s + 1]
        # output j of the frame is capture index x0 + (T - 1) + j - d: the segment's own
        assert x0 + (T - 1) - d - starts[s] == y0 - offsets[s]
    assert np.all(owner == 1)
    assert len(want) == sum(-(-ln // hop) for ln in lens)


def test_planner_empty_and_limits():
    fr = pk.isolate_frames([], [], 255)
    assert fr.offsets.tolist() == [0] and fr.seg.size == 0
    with pytest.raises(ValueError):
        pk.isolate_frames([0], [5], 254)
    with pytest.raises(NotImplementedError):
        pk.isolate_frames([0], [5], 513)


def test_reference_window_form_is_the_full_form():
    """isolate_ref.isolate (the samples the outputs depend on) against the
    literal definition over the whole capture."""
    rng = np.random.default_rng(7)
    n = 3000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    for T in (3, 63, 255):
        h = rng.standard_normal(T).astype(np.float32)
        for lo, hi in ((0, 1), (0, 700), (1234, 1235), (500, 2100), (n - 40, n), (0, n)):
            for f in (0.0, 0.31, -7e6):
                a = iso.isolate(x, lo, hi, f, h, SR if abs(f) > 1 else 1.0)
                b = iso.isolate_full(x, lo, hi, f, h, SR if abs(f) > 1 else 1.0)
                assert a.dtype == b.dtype == np.complex128 and a.shape == (hi - lo,)
                assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max()


# ---------------------------------------------------------------------------
# burst table
# ---------------------------------------------------------------------------
def test_table_shares_filters_and_handles_nan():
    T = 255
    lo, hi = [0, 10, 20, 30, 40], [5, 500, 21, 4000, 90]
    freqs = [8e6, -6e6, np.nan, 1e6, 2e6]
    bws = [2e6, 2e6, 1e6, SR, np.nan]
    table, taps, cutoff = pk.isolate_table(lo, hi, freqs, bws, SR, 1e6, T)
    assert table.dtype == pk.ISOLATE_SEG_DTYPE and table.dtype.itemsize == 32
    assert table["start"].tolist() == lo and table["len"].tolist() == [5, 490, 1, 3970, 50]
    assert table["freq"].tolist() == [7e6, -7e6, 0.0, 0.0, 0.0]
    assert taps.shape == (2, T) and taps.dtype == np.float32
    f = table["filter"]
    assert f[0] == f[1] and f[2] == f[3] == f[4] != f[0]
    assert np.array_equal(taps[f[0]], pk.design_lowpass(2e6, SR, T))
    imp = np.zeros(T, np.float32)
    imp[127] = 1
    assert np.array_equal(taps[f[2]], imp)
    assert cutoff[0] == cutoff[1] == 1e6 + 1.65 * SR / T and cutoff[3] >= SR / 2
    assert np.isnan(cutoff[2]) and np.isnan(cutoff[4])
    import ctypes
    assert ctypes.sizeof(_lib.IsolateSeg) == 32


# ---------------------------------------------------------------------------
# errors: all raised with no device (on a machine without one they must come
# before VsigUnavailable)
# ---------------------------------------------------------------------------
X = np.zeros(1000, np.complex64)
OK = dict(freqs=[1e6], bandwidths=[1e6])


@pytest.mark.parametrize("args,kw,exc", [
    ((X.astype(np.complex128), ([10], [20]), SR), OK, NotImplementedError),
    ((X.real, ([10], [20]), SR), OK, NotImplementedError),
    ((X.reshape(10, 100), ([10], [20]), SR), OK, ValueError),
    ((X[:0], ([], []), SR), {}, ValueError),
    ((X, ([10], [1000]), SR), OK, ValueError),
    ((X, ([-1], [20]), SR), OK, ValueError),
    ((X, ([30], [20]), SR), OK, ValueError),
    ((X, ([10.5], [20.0]), SR), OK, ValueError),
    ((X, ([10, 11], [20]), SR), OK, ValueError),
    ((X, ([10], [20]), 0.0), OK, ValueError),
    ((X, ([10], [20]), np.inf), OK, ValueError),
    ((X, ([10], [20]), SR, np.nan), OK, ValueError),
    ((X, ([10], [20]), SR), dict(OK, ntaps=254), ValueError),
    ((X, ([10], [20]), SR), dict(OK, ntaps=1), ValueError),
    ((X, ([10], [20]), SR), dict(OK, ntaps=513), NotImplementedError),
    ((X, ([10], [20]), SR), dict(OK, pre_samples=-1), ValueError),
    ((X, ([10], [20]), SR), dict(OK, post_samples=-1), ValueError),
    ((X, ([10], [20]), SR), dict(freqs=[1e6, 2e6], bandwidths=[1e6]), ValueError),
    ((X, ([10], [20]), SR), dict(freqs=[1e6], bandwidths=[[1e6]]), ValueError),
    ((X, ([10], [20]), SR), dict(freqs=[np.inf], bandwidths=[1e6]), ValueError),
    ((X, ([10], [20]), SR), dict(freqs=[1e6], bandwidths=[-1.0]), ValueError),
    ((X, ([10], [20]), SR), dict(measurements=pk.PacketMeasurements(
        np.zeros(2), None, None, None, np.zeros(2), None, None, None)), ValueError),
])
def test_argument_errors_need_no_device(args, kw, exc):
    with pytest.raises(exc) as e:
        pk.isolate_packets(*args, **kw)
    assert not isinstance(e.value, _lib.VsigUnavailable)


def test_no_burst_needs_no_device():
    out = pk.isolate_packets(X, (np.zeros(0, np.int64), np.zeros(0, np.int64)), SR)
    assert out.packets == [] and all(len(a) == 0 for a in out[1:])


def test_valid_call_reaches_the_device():
    import torch
    if torch.cuda.is_available():
        assert pk.isolate_packets(X, ([10], [20]), SR, **OK).packets[0].shape == (11,)
    else:
        with pytest.raises(_lib.VsigUnavailable):
            pk.isolate_packets(X, ([10], [20]), SR, **OK)


def test_exported():
    import vector_amd
    assert vector_amd.isolate_packets is pk.isolate_packets
    assert vector_amd.design_lowpass is pk.design_lowpass
    assert vector_amd.IsolatedPackets is pk.IsolatedPackets
    for name in ("vsig_isolate_create", "vsig_isolate_free", "vsig_isolate_info", "vsig_isolate_offsets",
                 "vsig_isolate_run"):
        assert name in _lib.SIGNATURES
