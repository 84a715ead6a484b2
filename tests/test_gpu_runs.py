"""GPU checks of the run list (runs.hip behind vsig_runs_dev / vsig_runs and
vector_amd.find_runs / detect_packets / extract_packets).

The reference is tests/runs_ref.py: with m = np.abs(a) in the array's precision
(widened to float64), the runs of m >= thr with dropouts of up to max_gap
elements bridged.  The kernels form the same m and only compare, so starts,
ends, argmax and max are compared with np.array_equal; a run's sum is a sum of
non-negative doubles in some fixed order, held to twice the first-order bound
len * 2^-53 * sum of any such order against math.fsum."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import golden
from runs_ref import run_stats, runs_ref
from vector_amd import _lib

pytestmark = pytest.mark.gpu


SENT = -0x0123456789ABCDEF          # fills output buffers before a call
GUARD = 4                            # records after out[cap) that must stay SENT
NP_CODE = {np.dtype(np.complex128): "c128", np.dtype(np.complex64): "c64",
           np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}


def mags(a):
    return np.abs(a).astype(np.float64)


def dev_runs(va, t, code, thr, relative, gap, cap, null_out=False):
    """vsig_runs_dev on a device tensor: (rc, records dict, info dict, raw record
    buffer, raw info buffer)."""
    ctx = va.get_context()
    rec = torch.full((cap + GUARD, 5), SENT, dtype=torch.int64, device="cuda")
    info = torch.full((5,), SENT, dtype=torch.int64, device="cuda")
    rc = ctx.lib.vsig_runs_dev(ctx.h, _lib.DTYPES[code], C.c_void_p(t.data_ptr()), t.numel(), float(thr),
                               int(relative), int(gap), None if null_out else C.c_void_p(rec.data_ptr()),
                               cap, C.c_void_p(info.data_ptr()))
    torch.cuda.synchronize()
    r, i = rec.cpu(), info.cpu()
    f = i.view(torch.float64)
    inf = dict(count=int(i[0]), covered=int(i[1]), argmax=int(i[2]), max=float(f[3]), thr_used=float(f[4]))
    k = max(0, min(inf["count"], cap)) if rc == 0 else 0
    rf = r[:k].contiguous().view(torch.float64).numpy()
    rn = r[:k].numpy()
    got = dict(start=rn[:, 0], end=rn[:, 1], argmax=rn[:, 2], max=rf[:, 3], sum=rf[:, 4])
    return rc, got, inf, r, i


def check(va, a, thr, gap, relative=False, cap=None):
    """One call against the reference: records, info record, guard band.
    Returns the reference (start, end)."""
    m = mags(a)
    mxv = m.max()
    thr_used = thr * mxv if relative else thr
    ws, we = runs_ref(m, thr_used, gap)
    cap = len(ws) + 3 if cap is None else cap
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(a).cuda()
    rc, got, inf, rec, _ = dev_runs(va, t, NP_CODE[a.dtype], thr, relative, gap, cap)
    assert rc == 0
    assert inf == dict(count=len(ws), covered=int(np.count_nonzero(m >= thr_used)), argmax=int(np.argmax(m)),
                       max=mxv, thr_used=thr_used)
    k = min(len(ws), cap)
    assert np.array_equal(got["start"], ws[:k]) and np.array_equal(got["end"], we[:k])
    wa, wm, wsum = run_stats(m, ws[:k], we[:k])
    assert np.array_equal(got["argmax"], wa) and np.array_equal(got["max"], wm)
    length = we[:k] - ws[:k] + 1
    bound = 2 * length * 2.0 ** -53 * wsum
    err = np.abs(got["sum"] - wsum)
    TALLY["calls"] += 1
    TALLY["runs"] += k
    if k:
        TALLY["sum_err_over_bound"] = max(TALLY["sum_err_over_bound"], float((err / bound).max()))
    assert (err <= bound).all()
    assert (rec[k:] == SENT).all()
    return ws, we


TALLY = dict(calls=0, runs=0, sum_err_over_bound=0.0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\nrun list: {TALLY['calls']} calls and {TALLY['runs']} runs compared with the reference, "
          f"largest |sum - fsum| / bound {TALLY['sum_err_over_bound']:.3g}")


@pytest.fixture(scope="module")
def T(gpu):
    return gpu.load_library().vsig_runs_tile()


@pytest.fixture(scope="module")
def noise(T):
    rng = np.random.default_rng(2025)
    n = 40 * T + 17
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _sizes(T):
    return [1, T - 1, T, T + 1, 3 * T + 5, 40 * T + 17]          # the last: more than one group of tiles


def _gaps(T, n):
    return [0, 1, T - 1, T, 5 * T, n]


@pytest.mark.parametrize("ni", range(6))
def test_parity_over_sizes_and_gaps(gpu, T, noise, ni):
    n = _sizes(T)[ni]
    a = np.ascontiguousarray(noise[:n])
    m = mags(a)
    # empty, sparse, about half and full masks
    thrs = [2.0 * m.max(), float(np.quantile(m, 0.995)), float(np.quantile(m, 0.5)), float(m.min())]
    for gap in _gaps(T, n):
        for thr in thrs:
            ws, we = check(gpu, a, thr, gap)
            if gap >= n:
                assert len(ws) <= 1
        check(gpu, a, float(np.quantile(m, 0.5)) / m.max(), gap, relative=True)
    # a sparser mask at the large size, so that whole tiles are empty
    if n > 4 * T:
        b = a.copy()
        b[:] *= np.float32(0.01)
        b[5 * T + 3:5 * T + 40] = 3.0
        b[17 * T - 2:17 * T + 2] = 2.0
        b[38 * T:] = 2.5
        for gap in _gaps(T, n):
            ws, we = check(gpu, b, 1.0, gap)
            assert ws[0] == 5 * T + 3 and we[-1] == n - 1


TILE_GRID = 4096                     # kTileGrid in runs.hip: the blocks of the tile pass


@pytest.fixture(scope="module")
def three_tiles_a_block(T):
    """2 * TILE_GRID + 2 tiles of low noise: tile 2 * TILE_GRID is block 0's third,
    the one-element tile after it block 1's third (the element-wise path)."""
    n = (2 * TILE_GRID + 1) * T + 1
    return np.random.default_rng(32).random(n, dtype=np.float32) * np.float32(0.1)


@pytest.mark.parametrize("variant", ["third_tile", "last_element", "equal_in_one_block"])
def test_a_block_that_owns_three_tiles(gpu, T, three_tiles_a_block, variant):
    """A block's slot rows are used a second time and its maximum accumulates
    over three tiles: the info record and the list against the reference."""
    a = three_tiles_a_block.copy()
    n = len(a)
    a[3 * T + 11:3 * T + 14] = 2.0
    a[5000 * T + 7] = 3.0
    if variant == "third_tile":
        want = 2 * TILE_GRID * T + 100
        a[want] = 5.0
    elif variant == "last_element":
        want = n - 1
        a[want] = 5.0
    else:                                # tiles 7 and 7 + TILE_GRID are one block's: the lower index wins
        want = 7 * T + 5
        a[want] = a[(7 + TILE_GRID) * T + 9] = 5.0
    assert int(np.argmax(a)) == want
    ws, _ = check(gpu, a, 1.0, 2)
    assert len(ws) == (4 if variant == "equal_in_one_block" else 3)


def test_first_start_and_last_end_do_not_depend_on_the_gap(gpu, T, noise):
    a = np.ascontiguousarray(noise[:3 * T + 5])
    m = mags(a)
    thr = float(np.quantile(m, 0.9))
    idx = np.flatnonzero(m >= thr)
    for gap in (0, 3, T, 10 ** 9):
        ws, we = check(gpu, a, thr, gap)
        assert ws[0] == idx[0] and we[-1] == idx[-1]
    # vsig_threshold_dev's pair and count
    cnt, first, last, _ = gpu.threshold_stats(m, thr)
    ws, we = check(gpu, m, thr, len(m))
    assert (cnt, first, last) == (len(idx), ws[0], we[0]) and len(ws) == 1


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64, np.float32])
def test_dtypes(gpu, T, dtype):
    rng = np.random.default_rng(7)
    n = 3 * T + 5
    a = rng.standard_normal(n)
    if np.issubdtype(dtype, np.complexfloating):
        a = a + 1j * rng.standard_normal(n)
    a = a.astype(dtype)
    m = mags(a)
    for gap in (0, 5, T):
        check(gpu, a, float(np.quantile(m, 0.7)), gap)
        check(gpu, a, 0.25, gap, relative=True)


def test_unaligned_view(gpu, T, noise):
    """A view one complex64 (8 bytes) into a buffer: the element-wise tile pass."""
    buf = torch.from_numpy(noise[:3 * T + 6]).cuda()
    v = buf[1:]
    assert v.data_ptr() % 16 == 8
    a = noise[1:3 * T + 6]
    m = mags(a)
    thr = float(np.quantile(m, 0.8))
    ws, we = runs_ref(m, thr, 2)
    rc, got, inf, _, _ = dev_runs(gpu, v, "c64", thr, 0, 2, len(ws) + 3)
    assert rc == 0 and inf["count"] == len(ws) and inf["argmax"] == int(np.argmax(m))
    assert np.array_equal(got["start"], ws) and np.array_equal(got["end"], we)
    wa, wm, _ = run_stats(m, ws, we)
    assert np.array_equal(got["argmax"], wa) and np.array_equal(got["max"], wm)
    # a relative threshold: the mixed tiles are read a second time, element by element too
    thr_used = 0.3 * m.max()
    ws, we = runs_ref(m, thr_used, 0)
    rc, got, inf, _, _ = dev_runs(gpu, v, "c64", 0.3, 1, 0, len(ws) + 3)
    assert rc == 0 and inf["count"] == len(ws) and inf["thr_used"] == thr_used
    assert np.array_equal(got["start"], ws) and np.array_equal(got["end"], we)


def test_edges(gpu, T):
    n = 4 * T
    z = np.zeros(n, np.float64)
    # runs at the array's two ends
    m = z.copy()
    m[0:5] = 1.0
    m[n - 3:] = 2.0
    for gap in (0, 7, T):
        ws, we = check(gpu, m, 1.0, gap)
        assert (list(ws), list(we)) == ([0, n - 3], [4, n - 1])
    assert [list(x) for x in check(gpu, m, 1.0, n)] == [[0], [n - 1]]
    # one masked element on either side of a tile edge
    for pos in (T - 1, T, 0, n - 1):
        m = z.copy()
        m[pos] = 3.0
        for gap in (0, 1, T - 1, T, 10 ** 6):
            assert [list(x) for x in check(gpu, m, 1.0, gap)] == [[pos], [pos]]
    # a run crossing a tile edge
    m = z.copy()
    m[T - 10:T + 10] = 1.0
    m[T + 4] = 1.5
    for gap in (0, 3, T):
        assert [list(x) for x in check(gpu, m, 1.0, gap)] == [[T - 10], [T + 9]]
    # a gap of exactly max_gap merges, of max_gap + 1 splits, across a tile edge
    for g in (1, 5, T - 1, T, 2 * T + 1):
        m = z.copy()
        i, j = T - 3, T - 3 + g + 1                       # g unmasked elements between them
        m[i] = m[j] = 4.0
        assert [list(x) for x in check(gpu, m, 1.0, g)] == [[i], [j]]
        assert [list(x) for x in check(gpu, m, 1.0, g - 1)] == [[i, j], [i, j]]


def test_whole_tiles_inside_a_run(gpu, T):
    """Tiles that are masked throughout come from the table: a run over
    several of them, its maximum in an interior tile (the first of two equal
    ones), and the same run with a dropout bridged."""
    n = 8 * T
    m = np.full(n, 0.25, np.float64)
    rng = np.random.default_rng(1)
    m[T - 7:5 * T + 9] = 1.0 + rng.random(4 * T + 16)
    m[3 * T + 11] = 7.0
    ws, we = check(gpu, m, 1.0, 0)
    assert (list(ws), list(we)) == ([T - 7], [5 * T + 8])
    m[2 * T + 5] = 7.0
    check(gpu, m, 1.0, 0)
    m[6 * T + 1] = 9.0                                     # a second run; T - 8 elements between
    ws, we = check(gpu, m, 1.0, 5)
    assert len(ws) == 2
    ws, we = check(gpu, m, 1.0, T)
    assert (list(ws), list(we)) == ([T - 7], [6 * T + 1])
    # a run over more than a whole group of tiles (its statistics read group
    # records, tile records and the two end tiles), absolute and relative
    n = 70 * T
    m = 0.25 * rng.random(n)
    m[3 * T + 5:68 * T + 10] = 1.0 + rng.random(65 * T + 5)
    m[5] = 1.5
    for k, pos in enumerate((40 * T + 3, 10 * T + 1, 66 * T + 2, 3 * T + 5)):
        m[pos] = 5.0 + k                                   # a new maximum each time
        for a in (m, m.astype(np.float32)):
            ws, we = check(gpu, a, 1.0, 0)
            assert (list(ws), list(we)) == ([5, 3 * T + 5], [5, 68 * T + 9])
            check(gpu, a, 1.0 / float(mags(a).max()) * (1 - 1e-6), 3 * T, relative=True)
    # all equal values, relative threshold 1.0: one run over everything
    flat = np.full(3 * T + 5, 2.5, np.float32)
    for gap in (0, T):
        assert [list(x) for x in check(gpu, flat, 1.0, gap, relative=True)] == [[0], [3 * T + 4]]
    assert [len(x) for x in check(gpu, flat, 3.0, 0)] == [0, 0]


def test_alternating_mask(gpu, T):
    n = 8 * T
    m = np.tile(np.array([1.0, 0.0], np.float32), n // 2)
    ws, we = check(gpu, m, 0.5, 0)
    assert len(ws) == n // 2 and np.array_equal(ws, we)
    assert [list(x) for x in check(gpu, m, 0.5, 1)] == [[0], [n - 2]]
    ws, _ = check(gpu, m[1:].copy(), 0.5, 0, cap=100)
    assert ws[0] == 1 and len(ws) == n // 2 - 1


def test_more_runs_than_find_runs_retries_for(gpu):
    """2^24 + 1 runs: one more than the repeat with cap = count is made for."""
    count = (1 << 24) + 1
    m = np.zeros(2 * count, np.float32)
    m[0::2] = 1.0
    with pytest.warns(RuntimeWarning, match=f"{count} runs, the first 7"):
        r = gpu.find_runs(m, 0.5, max_runs=7)
    assert np.array_equal(r.start, 2 * np.arange(7)) and np.array_equal(r.end, r.start)
    assert np.array_equal(r.max, np.ones(7)) and np.array_equal(r.mean, np.ones(7))


def test_cap_guard_and_determinism(gpu, T, noise):
    a = np.ascontiguousarray(noise[:3 * T + 5])
    m = mags(a)
    thr = float(np.quantile(m, 0.5))
    t = torch.from_numpy(a).cuda()
    for gap in (0, 2):
        ws, we = runs_ref(m, thr, gap)
        cap = 100
        assert len(ws) > cap
        check(gpu, a, thr, gap, cap=cap)
        rc, _, inf, rec, info = dev_runs(gpu, t, "c64", thr, 0, gap, cap)
        assert rc == 0 and inf["count"] == len(ws)
        assert (rec[cap:] == SENT).all()                            # the guard band
        rc2, _, _, rec2, info2 = dev_runs(gpu, t, "c64", thr, 0, gap, cap)
        assert rc2 == 0 and torch.equal(rec, rec2) and torch.equal(info, info2)
        # count only
        rc, got, inf, rec, _ = dev_runs(gpu, t, "c64", thr, 0, gap, 0, null_out=True)
        assert rc == 0 and inf["count"] == len(ws) and len(got["start"]) == 0 and (rec == SENT).all()


def test_invalid_arguments_leave_buffers_alone(gpu, noise):
    t = torch.from_numpy(noise[:5000]).cuda()
    ctx = gpu.get_context()
    c64 = _lib.DTYPES["c64"]
    good = dict(dtype=c64, a=t.data_ptr(), n=t.numel(), thr=0.5, rel=0, gap=3, out=1, cap=16, info=1)
    bad = [dict(n=0), dict(n=-5), dict(n=(1 << 40) + 1), dict(cap=-1), dict(gap=-1), dict(info=0), dict(out=0),
           dict(a=0), dict(dtype=4), dict(dtype=-1), dict(thr=float("nan"))]
    for kw in bad:
        g = dict(good, **kw)
        rec = torch.full((16 + GUARD, 5), SENT, dtype=torch.int64, device="cuda")
        info = torch.full((5,), SENT, dtype=torch.int64, device="cuda")
        rc = ctx.lib.vsig_runs_dev(ctx.h, g["dtype"], C.c_void_p(g["a"]) if g["a"] else None, g["n"],
                                   g["thr"], g["rel"], g["gap"],
                                   C.c_void_p(rec.data_ptr()) if g["out"] else None, g["cap"],
                                   C.c_void_p(info.data_ptr()) if g["info"] else None)
        torch.cuda.synchronize()
        assert rc == -1, kw
        assert (rec == SENT).all() and (info == SENT).all(), kw


def test_host_entry_and_find_runs(gpu, T, noise):
    a = np.ascontiguousarray(noise[:3 * T + 5])
    m = mags(a)
    thr = float(np.quantile(m, 0.9))
    ws, we = runs_ref(m, thr, 2)
    wa, wm, wsum = run_stats(m, ws, we)
    ctx = gpu.get_context()
    out = np.zeros(len(ws) + 2, dtype=[("start", "<i8"), ("end", "<i8"), ("argmax", "<i8"), ("max", "<f8"),
                                       ("sum", "<f8")])
    out["start"] = SENT
    inf = _lib.RunsInfo()
    ctx.check(ctx.lib.vsig_runs(ctx.h, _lib.DTYPES["c64"], a.ctypes.data_as(C.c_void_p), len(a), thr, 0, 2,
                                out.ctypes.data_as(C.c_void_p), len(out), C.byref(inf)), "runs")
    assert inf.count == len(ws) and inf.covered == np.count_nonzero(m >= thr)
    assert inf.argmax == int(np.argmax(m)) and inf.max == m.max() and inf.thr_used == thr
    k = len(ws)
    assert np.array_equal(out["start"][:k], ws) and np.array_equal(out["end"][:k], we)
    assert np.array_equal(out["argmax"][:k], wa) and np.array_equal(out["max"][:k], wm)
    assert (out["start"][k:] == SENT).all()
    # the Python front end: numpy in, trimmed named result out
    r = gpu.find_runs(a, thr, 2)
    assert r._fields == ("start", "end", "argmax", "max", "mean")
    assert r.start.dtype == np.int64 and r.max.dtype == np.float64
    assert np.array_equal(r.start, ws) and np.array_equal(r.end, we)
    assert np.array_equal(r.argmax, wa) and np.array_equal(r.max, wm)
    np.testing.assert_allclose(r.mean, wsum / (we - ws + 1), rtol=1e-12)
    rr = gpu.find_runs(a, thr / m.max(), 2, relative=True)
    ws2, we2 = runs_ref(m, thr / m.max() * m.max(), 2)
    assert np.array_equal(rr.start, ws2) and np.array_equal(rr.end, we2)
    # more runs than max_runs: the call is repeated with room for all of them
    assert len(ws) > 10
    r = gpu.find_runs(a, thr, 2, max_runs=10)
    assert np.array_equal(r.start, ws) and np.array_equal(r.end, we) and np.array_equal(r.argmax, wa)
    r = gpu.find_runs(a, thr, 2, max_runs=0)
    assert np.array_equal(r.start, ws)
    # min_length: a mask on the records, after the count
    for min_length in (2, 3, 10 ** 6):
        keep = we - ws + 1 >= min_length
        for max_runs in (65536, 10):
            r = gpu.find_runs(a, thr, 2, min_length=min_length, max_runs=max_runs)
            assert np.array_equal(r.start, ws[keep]) and np.array_equal(r.end, we[keep])
            assert np.array_equal(r.max, wm[keep])
    # device in: the padded record tensor and the info record, nothing trimmed
    rec, info = gpu.find_runs(torch.from_numpy(a).cuda(), thr, 2, max_runs=len(ws) + 4)
    assert rec.is_cuda and info.is_cuda and tuple(rec.shape) == (len(ws) + 4, 5)
    assert int(info[0]) == len(ws) and float(info.view(torch.float64)[4]) == thr
    rc = rec.cpu().numpy()
    assert np.array_equal(rc[:, 0], np.r_[ws, [-1] * 4]) and np.array_equal(rc[:, 1], np.r_[we, [-1] * 4])
    assert np.array_equal(rc[:, 3].copy().view(np.float64), np.r_[wm, [0.0] * 4])
    with pytest.raises(ValueError, match="min_length"):
        gpu.find_runs(torch.from_numpy(a).cuda(), thr, 2, min_length=2)
    with pytest.raises(ValueError, match="1-D"):
        gpu.find_runs(torch.from_numpy(a).cuda().reshape(-1, 1), thr)


def test_dev_call_captures_into_a_graph(gpu, T, noise):
    """vsig_runs_dev neither synchronises nor allocates once warm: captured
    after one call, the replay's bytes equal the eager call's."""
    a_np = np.ascontiguousarray(noise[:3 * T + 5])
    call = lambda ctx, a, rec, info: ctx.lib.vsig_runs_dev(   # noqa: E731
        ctx.h, _lib.DTYPES["c64"], C.c_void_p(a.data_ptr()), a.numel(), 0.5, 1, 3,
        C.c_void_p(rec.data_ptr()), 4096, C.c_void_p(info.data_ptr()))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.from_numpy(a_np).cuda()
        rec = torch.full((4096, 5), SENT, dtype=torch.int64, device="cuda")
        info = torch.zeros(5, dtype=torch.int64, device="cuda")

        def step():
            ctx = gpu.get_context()
            ctx.check(call(ctx, a, rec, info), "runs")
        step()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        new = np.roll(a_np, 777) * np.float32(0.5)
        a.copy_(torch.from_numpy(new))
        rec.fill_(SENT)
        graph.replay()
        st.synchronize()
        rec_g, info_g = rec.clone(), info.clone()
        rec.fill_(SENT)
        info.zero_()
        step()
        st.synchronize()
        assert torch.equal(rec_g, rec) and torch.equal(info_g, info)
        m = mags(new)
        ws, we = runs_ref(m, 0.5 * m.max(), 3)
        r = rec_g.cpu().numpy()
        assert int(info_g[0]) == len(ws) and 0 < len(ws) < 4096
        assert np.array_equal(r[:len(ws), 0], ws) and np.array_equal(r[:len(ws), 1], we)
        assert (r[len(ws):] == SENT).all()


# ---------------------------------------------------------------------------
# detect_packets / extract_packets
# ---------------------------------------------------------------------------
SR = 56e6
CAPTURE = dict(n=60_000, starts=(3_100, 14_000, 27_500, 44_000), lens=(900, 4_000, 2_300, 1_500))


@pytest.fixture(scope="module")
def capture():
    """A seeded capture with four tone bursts, numpy's smoothed energy and
    threshold (detect_packet_bounds' rule), and the guard the exact comparison
    rests on: no numpy sm value within 1e-9 max(sm) of the threshold (the GPU's
    sm is within 1e-12 max(sm) of numpy's)."""
    rng = np.random.default_rng(42)
    n = CAPTURE["n"]
    x = (0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    for s, ln in zip(CAPTURE["starts"], CAPTURE["lens"]):
        x[s:s + ln] += (0.3 * np.exp(2j * np.pi * 0.031 * np.arange(ln))).astype(np.complex64)
    w = max(1, int(SR // 1e6))
    sm = np.convolve(np.abs(x) ** 2, np.ones(w) / w, "same")
    noise = np.median(sm[:max(1, len(sm) // 10)])
    thr = noise + 0.2 * (sm.max() - noise)
    assert np.count_nonzero(np.abs(sm - thr) <= 1e-9 * sm.max()) == 0
    return dict(x=x, w=w, sm=sm, noise=noise, thr=thr)


def test_detect_packets_on_the_golden_burst(gpu):
    g = golden("packet.npz")
    p = gpu.detect_packets(g["burst_x"], SR, min_length=1)
    assert len(p.starts) >= 1 and (int(p.starts[0]), int(p.ends[-1])) == tuple(g["burst_bounds"])
    assert p.window == 56


def test_detect_packets_lists_every_burst(gpu, capture):
    x, w, sm, thr = capture["x"], capture["w"], capture["sm"], capture["thr"]
    for kw, gap, min_length in ((dict(), w, w), (dict(max_gap=0), 0, w), (dict(max_gap=0, min_length=1), 0, 1)):
        ws, we = runs_ref(sm, thr, gap)
        keep = we - ws + 1 >= min_length
        ws, we = ws[keep], we[keep]
        p = gpu.detect_packets(x, SR, **kw)
        assert len(ws) == 4
        assert np.array_equal(p.starts, ws) and np.array_equal(p.ends, we)
        wa, wm, wsum = run_stats(sm, ws, we)
        # the GPU's sm differs from numpy's in the last bits, so its argmax may be
        # another sample of (nearly) the same height inside the burst
        assert ((p.peak_index >= ws) & (p.peak_index <= we)).all()
        np.testing.assert_allclose(sm[p.peak_index], wm, rtol=1e-9)
        np.testing.assert_allclose(p.peak, wm, rtol=1e-9)
        np.testing.assert_allclose(p.mean_power, wsum / (we - ws + 1), rtol=1e-9)
        assert p.window == w
        assert p.threshold == pytest.approx(thr, rel=1e-9) and p.noise == pytest.approx(capture["noise"], rel=1e-9)
    # every burst lies around its planted place
    for s, e, s0, ln in zip(p.starts, p.ends, CAPTURE["starts"], CAPTURE["lens"]):
        assert abs(s - s0) <= w and abs(e - (s0 + ln - 1)) <= w
    # the invariant against detect_packet_bounds, whatever the gap
    b = tuple(int(v) for v in gpu.detect_packet_bounds(x, SR))
    for gap in (0, w, 10 ** 6):
        p = gpu.detect_packets(x, SR, max_gap=gap, min_length=1)
        assert (int(p.starts[0]), int(p.ends[-1])) == b
    assert len(p.starts) == 1
    # a device tensor in gives the same list
    pd = gpu.detect_packets(torch.from_numpy(x).cuda(), SR)
    assert np.array_equal(pd.starts, ws) and np.array_equal(pd.ends, we)
    # an absolute level on sm; nothing above it, or a NaN one: an empty list
    pa = gpu.detect_packets(x, SR, threshold=float(thr))
    assert np.array_equal(pa.starts, ws) and np.array_equal(pa.ends, we) and math.isnan(pa.noise)
    for level in (10.0, float("nan")):
        pe = gpu.detect_packets(x, SR, threshold=level)
        assert len(pe.starts) == len(pe.ends) == len(pe.peak) == 0


def test_extract_packets(gpu, capture):
    x = capture["x"]
    p = gpu.detect_packets(x, SR)
    pre, post = 3_200, 100                                   # the first burst starts before pre samples
    for sig in (x, torch.from_numpy(x).cuda()):
        got = gpu.extract_packets(sig, p, pre_samples=pre, post_samples=post)
        assert len(got) == 4
        for (seg, applied), s, e in zip(got, p.starts, p.ends):
            lo = max(0, int(s) - pre)
            assert applied == int(s) - lo
            want = x[lo:min(len(x), int(e) + 1 + post)]
            if isinstance(seg, torch.Tensor):
                assert seg.is_cuda and seg.data_ptr() == sig.data_ptr() + 8 * lo      # a view
                seg = seg.cpu().numpy()
            assert np.array_equal(seg, want)
        assert got[0][1] == int(p.starts[0]) < pre and got[1][1] == pre
