"""GPU checks of the peak list (peaks.hip behind vsig_peaks_dev / vsig_peaks and
vector_amd.find_peaks / find_packet_instances / verify_vector).

The reference is numpy / scipy, restated below: with m = np.abs(a) in the
array's precision (widened to float64), the candidates are the elements at or
above the threshold that equal scipy.ndimage.maximum_filter1d over the +-d
window; a candidate i is an instance iff lo + np.argmax(m[lo:hi+1]) == i.  The
kernel forms the same m and only compares, so every comparison of indices and
values with that reference is np.array_equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from peaks_ref import ref_peaks
from vector_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -0x0123456789ABCDEF          # fills output buffers before a call
GUARD = 8                            # records after out[cap) that must stay SENT
NP_CODE = {np.dtype(np.complex128): "c128", np.dtype(np.complex64): "c64",
           np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}


def mags(a):
    return np.abs(a).astype(np.float64)


def dev_peaks(va, t, code, thr, relative, d, cap, null_out=False):
    """vsig_peaks_dev on a device tensor: (rc, indices, values, info dict, raw
    record buffer, raw info buffer)."""
    ctx = va.get_context()
    rec = torch.full((cap + GUARD, 2), SENT, dtype=torch.int64, device="cuda")
    info = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    rc = ctx.lib.vsig_peaks_dev(ctx.h, _lib.DTYPES[code], C.c_void_p(t.data_ptr()), t.numel(), float(thr),
                                int(relative), int(d),
                                None if null_out else C.c_void_p(rec.data_ptr()), cap,
                                C.c_void_p(info.data_ptr()))
    torch.cuda.synchronize()
    r, i = rec.cpu(), info.cpu()
    inf = dict(count=int(i[0]), argmax=int(i[1]), max=float(i.view(torch.float64)[2]),
               thr_used=float(i.view(torch.float64)[3]))
    k = max(0, min(inf["count"], cap)) if rc == 0 else 0
    return rc, r[:k, 0].numpy(), r[:k, 1].contiguous().view(torch.float64).numpy(), inf, r, i


def check(va, a, thr, d, relative=False, cap=None):
    """One call against the reference: records, info record, guard band."""
    m = mags(a)
    mxv = m.max()
    thr_used = thr * mxv if relative else thr
    wi, wv = ref_peaks(m, thr_used, d)
    cap = len(wi) + 3 if cap is None else cap
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(a).cuda()
    rc, gi, gv, inf, rec, _ = dev_peaks(va, t, NP_CODE[a.dtype], thr, relative, d, cap)
    assert rc == 0
    assert inf == dict(count=len(wi), argmax=int(np.argmax(m)), max=mxv, thr_used=thr_used)
    k = min(len(wi), cap)
    assert np.array_equal(gi, wi[:k]) and np.array_equal(gv, wv[:k])
    assert (rec[k:] == SENT).all()
    return wi


@pytest.fixture(scope="module")
def T(gpu):
    return gpu.load_library().vsig_peaks_tile()


@pytest.fixture(scope="module")
def noise(T):
    rng = np.random.default_rng(2024)
    n = 3 * T + 5
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _sizes(T):
    return [1, 2, T - 1, T, T + 1, 3 * T + 5]


def _dists(T, n):
    return [0, 1, 7, T - 1, T, T + 1, 3 * T, n, 10 ** 6]


@pytest.mark.parametrize("ni", range(6))
def test_parity_over_sizes_and_distances(gpu, T, noise, ni):
    n = _sizes(T)[ni]
    a = np.ascontiguousarray(noise[:n])
    m = mags(a)
    for d in _dists(T, n):
        for q in (0.0, 0.5, 0.99):
            thr = float(np.quantile(m, q))
            check(gpu, a, thr, d)
        check(gpu, a, float(np.quantile(m, 0.5)) / m.max(), d, relative=True)
        check(gpu, a, 0.0, d, relative=True)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64, np.float32])
def test_dtypes(gpu, T, dtype):
    rng = np.random.default_rng(7)
    n = 3 * T + 5
    a = rng.standard_normal(n)
    if np.issubdtype(dtype, np.complexfloating):
        a = a + 1j * rng.standard_normal(n)
    a = a.astype(dtype)
    m = mags(a)
    for d in (7, T + 1):
        check(gpu, a, float(np.quantile(m, 0.9)), d)
        check(gpu, a, 0.25, d, relative=True)


def test_unaligned_view(gpu, T, noise):
    """A view one complex64 (8 bytes) into a buffer: the element-wise tile pass."""
    buf = torch.from_numpy(noise).cuda()
    v = buf[1:]
    assert v.data_ptr() % 16 == 8
    a = noise[1:]
    m = mags(a)
    wi, wv = ref_peaks(m, float(np.quantile(m, 0.9)), 7)
    rc, gi, gv, inf, _, _ = dev_peaks(gpu, v, "c64", float(np.quantile(m, 0.9)), 0, 7, len(wi) + 3)
    assert rc == 0 and inf["count"] == len(wi) and inf["argmax"] == int(np.argmax(m))
    assert np.array_equal(gi, wi) and np.array_equal(gv, wv)


def test_ties_and_density(gpu, T):
    n = 3 * T + 5
    flat = np.full(n, 2.5, np.float32)
    up = np.arange(1, n + 1, dtype=np.float64)
    for d in (1, 7, T - 1, T, 3 * T, 10 ** 6):
        assert np.array_equal(check(gpu, flat, 0.5, d, relative=True), [0])
        assert np.array_equal(check(gpu, up, 0.0, d), [n - 1])
        assert np.array_equal(check(gpu, up[::-1].copy(), 0.0, d), [0])
    assert len(check(gpu, flat, 0.5, 0, relative=True)) == n          # d = 0: compaction
    rng = np.random.default_rng(11)
    quant = rng.integers(0, 4, n).astype(np.float32)
    for d in (1, 3, 50, 5000):
        for thr in (0.0, 1.0, 3.0):
            check(gpu, quant, thr, d)
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    for d in (0, 5, 10 ** 6):
        assert np.array_equal(check(gpu, a, 1.0, d, relative=True), [np.argmax(np.abs(a))])


def test_peaks_at_tile_edges(gpu, T):
    n = 4 * T
    for pos in (T, 2 * T - 1, 0, n - 1):                 # a tile's first / last element
        for d in (3, T - 1, T, 2 * T + 1):
            a = np.ones(n, np.float32)
            a[pos] = 9.0
            assert np.array_equal(check(gpu, a, 5.0, d), [pos])
    for d in (5, T - 1, T, T + 1, 2 * T):
        a = np.zeros(n, np.float64)
        a[T - 3] = a[T - 3 + d] = 4.0                    # equal peaks d apart: the first only
        assert np.array_equal(check(gpu, a, 1.0, d), [T - 3])
        a = np.zeros(n, np.float64)
        a[T - 3] = a[T - 3 + d + 1] = 4.0                # d + 1 apart: both
        assert np.array_equal(check(gpu, a, 1.0, d), [T - 3, T - 2 + d])


TILE_GRID = 4096                     # kTileGrid in peaks.hip: the blocks of the tile pass


@pytest.fixture(scope="module")
def three_tiles_a_block(T):
    """2 * TILE_GRID + 2 tiles of low noise: tile 2 * TILE_GRID is block 0's third,
    the one-element tile after it block 1's third (the element-wise path)."""
    n = (2 * TILE_GRID + 1) * T + 1
    return np.random.default_rng(31).random(n, dtype=np.float32) * np.float32(0.1)


@pytest.mark.parametrize("variant", ["third_tile", "last_element", "equal_in_one_block"])
def test_a_block_that_owns_three_tiles(gpu, T, three_tiles_a_block, variant):
    """A block's slot rows are used a second time and its maximum accumulates
    over three tiles: the info record and the list against the reference."""
    a = three_tiles_a_block.copy()
    n = len(a)
    a[3 * T + 11] = 2.0
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
    wi = check(gpu, a, 1.0, 100)
    assert len(wi) == (4 if variant == "equal_in_one_block" else 3)


def test_worst_cases_finish(gpu):
    """Every element above the threshold with a window of millions: the dense
    case (noise, threshold 0) and the flat one.  A scan that costs n * d
    compares cannot finish these inside a test's time."""
    n = 1 << 22
    rng = np.random.default_rng(5)
    dense = np.abs(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    wi = check(gpu, dense, 0.0, 1 << 20, cap=64)
    assert 1 <= len(wi) <= 4
    flat = np.full(n, 0.75, np.float32)
    assert np.array_equal(check(gpu, flat, 0.5, 1 << 21, relative=True, cap=64), [0])


def test_cap_guard_and_determinism(gpu, T, noise):
    a = noise
    m = mags(a)
    thr = float(np.quantile(m, 0.5))
    t = torch.from_numpy(a).cuda()
    for d in (0, 2):
        wi, wv = ref_peaks(m, thr, d)
        cap = 100
        assert len(wi) > cap
        rc, gi, gv, inf, rec, info = dev_peaks(gpu, t, "c64", thr, 0, d, cap)
        assert rc == 0 and inf["count"] == len(wi)
        assert np.array_equal(gi, wi[:cap]) and np.array_equal(gv, wv[:cap])
        assert (rec[cap:] == SENT).all()                            # the guard band
        rc2, _, _, _, rec2, info2 = dev_peaks(gpu, t, "c64", thr, 0, d, cap)
        assert rc2 == 0 and torch.equal(rec, rec2) and torch.equal(info, info2)
        # count only
        rc, gi, _, inf, rec, _ = dev_peaks(gpu, t, "c64", thr, 0, d, 0, null_out=True)
        assert rc == 0 and inf["count"] == len(wi) and len(gi) == 0 and (rec == SENT).all()


def test_invalid_arguments_leave_buffers_alone(gpu, noise):
    t = torch.from_numpy(noise).cuda()
    ctx = gpu.get_context()
    c64 = _lib.DTYPES["c64"]
    good = dict(dtype=c64, a=t.data_ptr(), n=t.numel(), thr=0.5, rel=0, d=3, out=1, cap=16, info=1)
    bad = [dict(n=0), dict(n=-5), dict(cap=-1), dict(d=-1), dict(info=0), dict(out=0), dict(a=0),
           dict(dtype=4), dict(dtype=-1), dict(thr=float("nan"))]
    for kw in bad:
        g = dict(good, **kw)
        rec = torch.full((16 + GUARD, 2), SENT, dtype=torch.int64, device="cuda")
        info = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
        rc = ctx.lib.vsig_peaks_dev(ctx.h, g["dtype"], C.c_void_p(g["a"]) if g["a"] else None, g["n"],
                                    g["thr"], g["rel"], g["d"],
                                    C.c_void_p(rec.data_ptr()) if g["out"] else None, g["cap"],
                                    C.c_void_p(info.data_ptr()) if g["info"] else None)
        torch.cuda.synchronize()
        assert rc == -1, kw
        assert (rec == SENT).all() and (info == SENT).all(), kw
    # the host-pointer form validates the same way
    inf = _lib.PeaksInfo(count=-7)
    rc = ctx.lib.vsig_peaks(ctx.h, c64, noise.ctypes.data_as(C.c_void_p), len(noise), 0.5, 0, 3, None, 4,
                            C.byref(inf))
    assert rc == -1 and inf.count == -7


def test_host_entry_and_find_peaks(gpu, T, noise):
    m = mags(noise)
    thr = float(np.quantile(m, 0.9))
    wi, wv = ref_peaks(m, thr, 7)
    ctx = gpu.get_context()
    out = np.zeros(len(wi) + 2, dtype=[("index", "<i8"), ("value", "<f8")])
    out["index"] = SENT
    inf = _lib.PeaksInfo()
    ctx.check(ctx.lib.vsig_peaks(ctx.h, _lib.DTYPES["c64"], noise.ctypes.data_as(C.c_void_p), len(noise),
                                 thr, 0, 7, out.ctypes.data_as(C.c_void_p), len(out), C.byref(inf)), "peaks")
    assert inf.count == len(wi) and inf.argmax == int(np.argmax(m)) and inf.max == m.max()
    assert np.array_equal(out["index"][:len(wi)], wi) and np.array_equal(out["value"][:len(wi)], wv)
    assert (out["index"][len(wi):] == SENT).all()
    # the Python front end: numpy in, trimmed numpy out
    gi, gv = gpu.find_peaks(noise, thr, 7)
    assert gi.dtype == np.int64 and gv.dtype == np.float64
    assert np.array_equal(gi, wi) and np.array_equal(gv, wv)
    ri, rv = gpu.find_peaks(noise, thr / m.max(), 7, relative=True)
    wi2, wv2 = ref_peaks(m, thr / m.max() * m.max(), 7)
    assert np.array_equal(ri, wi2) and np.array_equal(rv, wv2)
    with pytest.warns(RuntimeWarning, match="the first 5"):
        gi, gv = gpu.find_peaks(noise, thr, 7, max_peaks=5)
    assert np.array_equal(gi, wi[:5]) and np.array_equal(gv, wv[:5])
    # device in: padded device tensors and the info record, nothing trimmed
    di, dv, info = gpu.find_peaks(torch.from_numpy(noise).cuda(), thr, 7, max_peaks=len(wi) + 4)
    assert di.is_cuda and dv.is_cuda and info.is_cuda
    assert int(info[0]) == len(wi) and float(info.view(torch.float64)[3]) == thr
    assert np.array_equal(di.cpu().numpy(), np.r_[wi, [-1] * 4])
    assert np.array_equal(dv.cpu().numpy(), np.r_[wv, [0.0] * 4])
    # a host tensor is uploaded, never handed to the kernels as it is
    hi, _, hinfo = gpu.find_peaks(torch.from_numpy(noise), thr, 7, max_peaks=len(wi))
    assert hi.is_cuda and int(hinfo[0]) == len(wi) and np.array_equal(hi.cpu().numpy(), wi)


def test_dev_call_captures_into_a_graph(gpu, T, noise):
    """vsig_peaks_dev neither synchronises nor allocates once warm: captured
    after one call, it replays on new array contents."""
    ctx_args = lambda ctx, a, rec, info: ctx.lib.vsig_peaks_dev(   # noqa: E731
        ctx.h, _lib.DTYPES["c64"], C.c_void_p(a.data_ptr()), a.numel(), 0.5, 1, T + 3,
        C.c_void_p(rec.data_ptr()), 64, C.c_void_p(info.data_ptr()))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.from_numpy(noise).cuda()
        rec = torch.full((64, 2), SENT, dtype=torch.int64, device="cuda")
        info = torch.zeros(4, dtype=torch.int64, device="cuda")

        def step():
            ctx = gpu.get_context()
            ctx.check(ctx_args(ctx, a, rec, info), "peaks")
        step()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        new = np.roll(noise, 777) * np.float32(0.5)
        a.copy_(torch.from_numpy(new))
        rec.fill_(SENT)
        graph.replay()
        st.synchronize()
        m = mags(new)
        wi, wv = ref_peaks(m, 0.5 * m.max(), T + 3)
        assert int(info[0]) == len(wi) and int(info[1]) == int(np.argmax(m))
        r = rec.cpu()
        assert np.array_equal(r[:len(wi), 0].numpy(), wi)
        assert np.array_equal(r[:len(wi), 1].contiguous().view(torch.float64).numpy(), wv)
        assert (r[len(wi):] == SENT).all()


# ---------------------------------------------------------------------------
# end to end: packet instances in a vector
# ---------------------------------------------------------------------------
E2E = dict(n=60000, lens=(1500, 900), scales=(1.0, 0.6), starts=(137, 2500), periods=(7000, 4100))


def _iq(rng, n, scale):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)


@pytest.fixture(scope="module")
def e2e():
    rng = np.random.default_rng(31)
    pk = [_iq(rng, n, s) for n, s in zip(E2E["lens"], E2E["scales"])]
    v = _iq(rng, E2E["n"], 0.05)
    plan = []
    for p, s, per in zip(pk, E2E["starts"], E2E["periods"]):
        st = np.arange(s, E2E["n"] - len(p) + 1, per)
        for a in st:
            v[a:a + len(p)] += p
        plan.append(st)
    v = (v / np.abs(v).max()).astype(np.complex64)
    want = [np.abs(np.correlate(v.astype(np.complex128), p.astype(np.complex128), "valid")) for p in pk]
    return dict(v=v, pk=pk, plan=plan, want=want)


def test_find_packet_instances_end_to_end(gpu, e2e):
    assert [len(s) for s in e2e["plan"]] == [9, 14]
    vd = torch.from_numpy(e2e["v"]).cuda()
    for p, plan, want in zip(e2e["pk"], e2e["plan"], e2e["want"]):
        # the reference alone meets the condition, with a margin fp32 cannot close
        ri, _ = ref_peaks(want, 0.5 * want.max(), len(p) // 2)
        assert np.array_equal(ri, plan)
        starts, vals = gpu.find_packet_instances(e2e["v"], p)
        assert np.array_equal(starts, plan)
        rel = np.abs(vals - want[plan]) / want[plan]
        print("find_packet_instances: max relative |c| error", rel.max())
        assert rel.max() <= 1e-5
        ds, dv = gpu.find_packet_instances(vd, torch.from_numpy(p).cuda(), max_instances=32)
        assert ds.is_cuda and dv.is_cuda and ds.numel() == 32
        ds, dv = ds.cpu().numpy(), dv.cpu().numpy()
        assert np.array_equal(ds[:len(plan)], plan) and (ds[len(plan):] == -1).all()
        assert np.array_equal(dv[:len(plan)], vals) and (dv[len(plan):] == 0).all()
    with pytest.raises(ValueError):
        gpu.find_packet_instances(e2e["v"][:100], e2e["pk"][0])


def test_verify_vector_on_build_vector_output(gpu, e2e):
    sr = 1e6
    configs = [dict(name="alpha", signal=e2e["pk"][0], period=7000 / sr, start_time=137 / sr,
                    freq_shift=2.5e5),
               dict(name="beta", signal=e2e["pk"][1], period=4100 / sr, start_time=2500 / sr,
                    pre_samples=13)]
    length = 60000 / sr
    plan = gpu.vector_plan(configs, length, sr)
    assert [c for _, _, c in plan.places] == [9, 14]
    for device in (False, True):
        vec, markers = gpu.build_vector(configs, length, sr, normalize=True, device=device)
        assert markers == plan.markers
        measured, (text, details) = gpu.verify_vector(vec, configs, length, sr)
        assert measured == plan.markers
        assert (text, details) == gpu.validate_packet_timing(plan.markers, configs)
        assert text == "Timing Validation: 100.0% ✅ PERFECT"
    # the second packet's period misreported by 3 %
    wrong = [configs[0], dict(configs[1], period=configs[1]["period"] * 1.03)]
    measured, (text, details) = gpu.verify_vector(vec, wrong, length, sr)
    assert measured == plan.markers
    times = [m[0] for m in plan.markers if m[2] == "beta"]
    avg = np.mean([(b - a) * 1000 for a, b in zip(times, times[1:])])
    want_ms = wrong[1]["period"] * 1000
    err = abs(avg - want_ms) / want_ms * 100
    assert 2.9 < err < 2.95
    # 14 instances: the +5 bonus caps the packet at 100 again, as the formula says
    beta = min(100.0, (100 - (err - 1.0) * 5) * 0.4 + 30 + 20 + 10 + 5.0)
    assert beta == 100.0
    assert details[1]["period_error_percent"] == pytest.approx(err, rel=1e-12)
    assert details[0]["period_error_percent"] < 1e-9
    assert text.startswith(f"Timing Validation: {(100.0 + beta) / 2:.1f}% ")
    # the first 7500 samples hold one alpha and two beta instances (no bonus):
    # alpha 98 (single instance), beta 100, or 60 + 0.4 * (100 - (err - 1) * 5)
    head = vec[:7500]
    measured, (text, details) = gpu.verify_vector(head, configs, 7500 / sr, sr)
    assert [m[2] for m in measured] == ["alpha", "beta", "beta"]
    assert text == "Timing Validation: 99.0% ⚠️ GOOD"       # (98 + 100) / 2 is not above 99.0
    measured, (text, details) = gpu.verify_vector(head, wrong, 7500 / sr, sr)
    err2 = details[1]["period_error_percent"]
    assert err2 == pytest.approx(abs(4.1 - want_ms) / want_ms * 100, rel=1e-9)
    beta = 60 + 0.4 * (100 - (err2 - 1.0) * 5)
    assert text == f"Timing Validation: {(98.0 + beta) / 2:.1f}% ⚠️ GOOD"


def test_build_vector_unchanged_by_the_shared_helper(gpu, e2e):
    """build_vector still adds the prepared packets in numpy's order."""
    sr = 1e6
    configs = [dict(name="alpha", signal=e2e["pk"][0], period=7000 / sr, start_time=137 / sr),
               dict(name="beta", signal=e2e["pk"][1], period=4100 / sr, start_time=2500 / sr)]
    vec, _ = gpu.build_vector(configs, 60000 / sr, sr)
    want = np.zeros(60000, np.complex64)
    for p, st in zip(e2e["pk"], e2e["plan"]):
        for a in st:
            want[a:a + len(p)] += p
    assert np.array_equal(vec, want)
