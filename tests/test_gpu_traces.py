"""GPU tests of the line traces: trace.hip through vsig_trace_envelope_dev and
vector_amd.signal_envelope / capture_spectrum, against the numpy restatement
(tests/trace_ref.py) and numpy's own site expressions.

1. VSIG_TRACE_ABS is exact (np.array_equal): magnitudes are numpy's to the
   bit and min / max / first extremum do not round.
2. VSIG_TRACE_DB20 equals the device's own dB map (vsig_db_dev, doubled:
   20 x = 2 (10 x) exactly) of the ABS envelope, and is within 8 ulp of
   numpy's 20 * np.log10(E + eps), the allowance test_gpu_analysis.py gives
   the dB map.
3. capture_spectrum with scale="linear" against the complex128 transform,
   bounded by the transform's own pinned floor (test_dft_floor): abs and
   min / max are 1-Lipschitz, so
     max |env - env(|r64|)| <= K_EXACT max |r32 - r64| + 2^-23 max |r64|.

Sizes are the kernels': kTraceTile = 2048 positions (bin <= 2048: a block owns
whole columns in LDS; above: chunks of whole tiles and a merge), a run of the
array is read in 16-byte units, 4 x 256 of them per trip.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import accuracy_ref as acc
import trace_ref as tr
from accuracy_ref import K_EXACT
from oracle import ref

pytestmark = pytest.mark.gpu

TILE = 2048
DTYPES = {"c128": np.complex128, "c64": np.complex64, "f64": np.float64, "f32": np.float32}
LENGTHS = (1, 2, 63, 64, 65, 1000, 4097, 65_537, (1 << 20) + 7)
INVALID = -1


@functools.lru_cache(maxsize=None)
def array(code, n):
    """n + 1 seeded values of the dtype (so that a[1:] is an array of n)."""
    dt = DTYPES[code]
    if code.startswith("c"):
        return ref.synth_iq(n + 1, seed=n).astype(dt)
    return np.random.default_rng(n).standard_normal(n + 1).astype(dt)


def run(gpu, t, **kw):
    """trace_envelope on a device tensor -> numpy (E_min or None, E_max, info)."""
    from vector_amd import traces
    emin, emax, info = traces.trace_envelope(t, **kw)
    return (None if emin is None else emin.cpu().numpy()), emax.cpu().numpy(), traces._read_info(info)


def check_abs(gpu, a, t, shift, lo, hi, bin_):
    emin, emax, info = run(gpu, t, shift=shift, lo=lo, hi=hi, bin=bin_)
    wmin, wmax, winfo = tr.restate(a, shift, lo, hi, bin_)
    case = f"n={len(a)} shift={shift} lo={lo} hi={hi} bin={bin_}"
    assert emax.dtype == wmax.dtype and emax.shape == wmax.shape, case
    assert np.array_equal(emax, wmax), case
    assert np.array_equal(emin, wmin), case
    assert info == winfo, case


# ---------------------------------------------------------------------------
# VSIG_TRACE_ABS, exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("code", list(DTYPES))
def test_abs_envelope_is_exact(gpu, code, n):
    """Whole window and a window whose ends are no multiples of bin (a partial
    last column); both orders (odd n, columns across the wrap point); a base
    pointer one element into the array (the 16-byte units start elsewhere)."""
    full = array(code, n)
    dev = torch.from_numpy(full).cuda()
    bins = sorted({1, 3, 64, 1000, n, n + 5})
    for off in (0, 1):
        a, t = full[off:off + n], dev[off:off + n]
        for shift in (False, True):
            for bin_ in bins:
                check_abs(gpu, a, t, shift, 0, n, bin_)
            if n >= 63:
                lo, hi = n // 5 + 1, n - n // 7 - 2
                for bin_ in (3, 64, 1000):
                    check_abs(gpu, a, t, shift, lo, hi, bin_)


@pytest.mark.parametrize("code", ["c64", "f64"])
def test_tile_boundary_and_columns_over_several_blocks(gpu, code):
    """bin on each side of the tile (the last LDS column, the first chunked
    one), columns of many one-tile chunks, a window that starts off a tile."""
    n = (1 << 20) + 7
    a = array(code, n)[:n]
    t = torch.from_numpy(a).cuda()
    for shift in (False, True):
        for bin_ in (TILE - 1, TILE, TILE + 1, 3 * TILE, 300_001):
            check_abs(gpu, a, t, shift, 0, n, bin_)
        check_abs(gpu, a, t, shift, 4099, n - 3001, TILE + 1)
        check_abs(gpu, a, t, shift, 4099, n - 3001, 100_003)


def test_chunks_of_several_tiles(gpu):
    """One column of 2^24 + 3 positions: more tiles than chunks are aimed at,
    so a chunk is two tiles."""
    n = (1 << 24) + 3
    a = np.random.default_rng(24).standard_normal(n).astype(np.float32)
    t = torch.from_numpy(a).cuda()
    for shift in (False, True):
        check_abs(gpu, a, t, shift, 0, n, n)
    check_abs(gpu, a, t, True, 5, n - 9, (n - 14) // 2 + 1)


def test_first_of_repeated_extrema(gpu):
    """Equal maxima (and minima) in several lanes, waves, blocks and on both
    sides of the wrap point: info holds the first position."""
    n = 70_001
    base = ref.synth_iq(n, seed=7)
    spots = [5, 64, 300, 2047, 2050, 40_000, n - 2]
    for shift in (False, True):
        rot = (n + 1) // 2 if shift else 0
        a = base.copy()
        src = [(p + rot) % n for p in spots]
        a[src] = np.complex64(30 + 40j)                   # |.| = 50, above the rest
        a[[(p + 1 + rot) % n for p in spots]] = 0        # minima next to them
        t = torch.from_numpy(a).cuda()
        for bin_ in (1, 64, 5000, n):
            _, emax, info = run(gpu, t, shift=shift, bin=bin_)
            assert info == tr.restate(a, shift, 0, n, bin_)[2]
            assert info[0] == spots[0] + 1 and info[1] == spots[0] and info[2] == 0.0 and info[3] == 50.0
        lo = spots[2] + 1
        _, _, info = run(gpu, t, shift=shift, lo=lo, bin=64)
        assert (info[0], info[1]) == (spots[2] + 1, spots[3])


# ---------------------------------------------------------------------------
# VSIG_TRACE_DB20
# ---------------------------------------------------------------------------
def device_db(gpu, E, eps):
    """2 * vsig_db_dev(E, eps): 20 log10(E + eps) by the library's dB map."""
    ctx = gpu.get_context()
    t = torch.from_numpy(E).cuda()
    out = torch.empty_like(t)
    code = "f32" if E.dtype == np.float32 else "f64"
    ctx.check(ctx.lib.vsig_db_dev(ctx.h, gpu._lib.DTYPES[code], C.c_void_p(t.data_ptr()), t.numel(), eps,
                                  C.c_void_p(out.data_ptr())), "db")
    return (out * 2).cpu().numpy()


@pytest.mark.parametrize("code", list(DTYPES))
def test_db20_is_the_mapped_envelope(gpu, code):
    n = 65_537
    a = array(code, n)[:n]
    t = torch.from_numpy(a).cuda()
    worst = 0.0
    for shift, bin_, eps in ((True, 1, 0.0), (False, 64, 1e-12), (True, 3000, 1e-3), (False, n, 0.0)):
        amin, amax, ainfo = run(gpu, t, shift=shift, bin=bin_)
        dmin, dmax, dinfo = run(gpu, t, shift=shift, bin=bin_, db=True, eps=eps)
        assert dmax.dtype == amax.dtype
        assert np.array_equal(dmax, device_db(gpu, amax, eps))
        assert np.array_equal(dmin, device_db(gpu, amin, eps))
        assert dinfo[:2] == ainfo[:2]
        assert dinfo[2:] == tuple(float(v) for v in device_db(gpu, np.array(ainfo[2:], amax.dtype), eps))
        for got, E in ((dmin, amin), (dmax, amax)):
            u = tr.ulps(got, tr.db20(E, eps)).max()
            worst = max(worst, u)
            assert u <= 8, (shift, bin_, eps, u)
    print(f"ACC trace db20 {code}: worst {worst:.2f} ulp of numpy's 20 log10(E + eps)")


def test_db20_of_zero_is_minus_inf(gpu):
    a = ref.synth_iq(5000, seed=5)
    a[100:164] = 0
    a[4000] = 0
    t = torch.from_numpy(a).cuda()
    for bin_ in (1, 64):
        emin, emax, info = run(gpu, t, bin=bin_, db=True, eps=0.0)
        wmin, wmax, winfo = tr.restate(a, False, 0, len(a), bin_, tr.DB20, 0.0)
        assert np.array_equal(np.isneginf(emin), np.isneginf(wmin)) and np.isneginf(wmin).sum() >= 2
        assert np.array_equal(np.isneginf(emax), np.isneginf(wmax))
        assert np.isneginf(emax).sum() == (64 if bin_ == 1 else 0) + (bin_ == 1)
        assert tr.ulps(emax, wmax).max() <= 8 and tr.ulps(emin, wmin).max() <= 8
        assert info[0] == 100 and info[2] == -np.inf and info[1] == winfo[1]
    emin, _, _ = run(gpu, t, bin=64, db=True, eps=1e-6)        # eps lifts the floor
    assert np.isfinite(emin).all()


# ---------------------------------------------------------------------------
# NaN, refused arguments, determinism, capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code", ["c64", "f64"])
def test_one_nan_makes_its_column_nan(gpu, code):
    n = 20_000
    for bin_, at in ((1, 777), (64, 6500), (1000, 12_345), (TILE + 1, 9000), (n, 3)):
        for shift in (False, True):
            a = array(code, n)[:n].copy()
            a[at] = np.nan
            emin, emax, _ = run(gpu, torch.from_numpy(a).cuda(), shift=shift, bin=bin_)
            p = (at - ((n + 1) // 2 if shift else 0)) % n
            want = np.zeros(len(emax), bool)
            want[p // bin_] = True
            assert np.array_equal(np.isnan(emax), want) and np.array_equal(np.isnan(emin), want)
            wmin, wmax, _ = tr.restate(a, shift, 0, n, bin_)
            assert np.array_equal(emax, wmax, equal_nan=True) and np.array_equal(emin, wmin, equal_nan=True)


def envelope_dev(gpu, t, n, shift=0, lo=0, hi=None, bin_=1, kind=0, eps=0.0, dtype=None, a="T", emin="L",
                 emax="H", info="I"):
    ctx = gpu.get_context()
    hi = n if hi is None else hi
    bufs = {"T": t, "L": torch.zeros(64, dtype=torch.float32, device="cuda"),
            "H": torch.zeros(64, dtype=torch.float32, device="cuda"),
            "I": torch.zeros(4, dtype=torch.int64, device="cuda")}
    ptr = lambda k: C.c_void_p(bufs[k].data_ptr()) if k in bufs else None   # noqa: E731
    dtype = gpu._lib.DTYPES["c64"] if dtype is None else dtype
    rc = ctx.lib.vsig_trace_envelope_dev(ctx.h, dtype, ptr(a), n, shift, lo, hi, bin_, kind, eps, ptr(emin),
                                         ptr(emax), ptr(info))
    return rc, bufs


def test_refused_arguments(gpu):
    a = ref.synth_iq(64, seed=2)
    t = torch.from_numpy(a).cuda()
    rc, bufs = envelope_dev(gpu, t, 64)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(bufs["H"].cpu().numpy(), np.abs(a))
    assert envelope_dev(gpu, t, 64, emin=None, info=None)[0] == 0          # both may be NULL
    for kw in [dict(a=None), dict(emax=None), dict(lo=-1), dict(hi=65), dict(lo=10, hi=10), dict(lo=11, hi=10),
               dict(bin_=0), dict(bin_=-4), dict(dtype=4), dict(dtype=-1), dict(kind=2), dict(kind=-1),
               dict(eps=-1e-30), dict(eps=float("inf")), dict(eps=float("nan"))]:
        assert envelope_dev(gpu, t, 64, **kw)[0] == INVALID, kw
    assert envelope_dev(gpu, t, 0, hi=0)[0] == INVALID
    assert envelope_dev(gpu, t, -5, hi=1)[0] == INVALID
    assert envelope_dev(gpu, t, (1 << 40) + 1, hi=64)[0] == INVALID
    rc, bufs = envelope_dev(gpu, t, 64, shift=1, bin_=8)                   # the context still works
    assert rc == 0
    torch.cuda.synchronize()
    wmin, wmax, winfo = tr.restate(a, True, 0, 64, 8)
    assert np.array_equal(bufs["H"].cpu().numpy()[:8], wmax) and np.array_equal(bufs["L"].cpu().numpy()[:8], wmin)
    assert (bufs["H"][8:] == 0).all() and (bufs["L"][8:] == 0).all()       # nothing past cols
    # the Python layer's own refusals, with a device present
    with pytest.raises(ValueError):
        gpu.signal_envelope(t, max_points=0)
    with pytest.raises(ValueError):
        gpu.capture_spectrum(t, 56e6, shift=False, band=(0.0, 1.0))
    with pytest.raises(ValueError):
        gpu.capture_spectrum(t[:0], 56e6)
    torch.cuda.synchronize()


def test_two_runs_give_the_same_bytes(gpu):
    n = (1 << 20) + 7
    t = torch.from_numpy(array("c64", n)[:n]).cuda()
    from vector_amd import traces
    for bin_ in (1, 700, 70_001):
        outs = []
        for _ in range(2):
            emin, emax, info = traces.trace_envelope(t, shift=True, lo=3, hi=n - 5, bin=bin_, db=True, eps=1e-12)
            outs.append((emin.cpu().numpy().tobytes(), emax.cpu().numpy().tobytes(), info.cpu().numpy().tobytes()))
        assert outs[0] == outs[1]


def test_dev_call_captures_into_a_graph(gpu):
    """Warm, the call neither allocates nor synchronises: one capture on a
    single stream, replayed on new array contents (both kernel layouts)."""
    n = 70_001
    a = ref.synth_iq(n, seed=11)
    for bin_ in (64, 9000):
        cols = -(-n // bin_)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            t = torch.from_numpy(a).cuda()
            emin = torch.zeros(cols, dtype=torch.float32, device="cuda")
            emax = torch.zeros(cols, dtype=torch.float32, device="cuda")
            info = torch.zeros(4, dtype=torch.int64, device="cuda")

            def step():
                ctx = gpu.get_context()
                ctx.check(ctx.lib.vsig_trace_envelope_dev(
                    ctx.h, gpu._lib.DTYPES["c64"], C.c_void_p(t.data_ptr()), n, 1, 0, n, bin_, 0, 0.0,
                    C.c_void_p(emin.data_ptr()), C.c_void_p(emax.data_ptr()), C.c_void_p(info.data_ptr())), "trace")
            step()
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                step()
            new = np.roll(a, 12_345) * np.float32(0.25)
            t.copy_(torch.from_numpy(new))
            emin.zero_()
            emax.zero_()
            graph.replay()
            st.synchronize()
            from vector_amd import traces
            wmin, wmax, winfo = tr.restate(new, True, 0, n, bin_)
            assert np.array_equal(emax.cpu().numpy(), wmax) and np.array_equal(emin.cpu().numpy(), wmin)
            assert traces._read_info(info) == winfo


# ---------------------------------------------------------------------------
# signal_envelope
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code", list(DTYPES))
def test_signal_envelope(gpu, code):
    n, sr = 10_007, 56e6
    a = array(code, n)[:n]
    line = np.abs(a)
    t_axis = np.arange(n) / sr
    # numpy in, the whole line
    tr0 = gpu.signal_envelope(a, sr)
    assert isinstance(tr0, gpu.Trace) and tr0.bin == 1 and tr0.lo is tr0.hi
    assert isinstance(tr0.hi, np.ndarray) and tr0.hi.dtype == line.dtype and np.array_equal(tr0.hi, line)
    assert tr0.x.dtype == np.float64 and np.array_equal(tr0.x, t_axis)
    assert tr0.argmax == np.argmax(line) and tr0.max == line.max() and isinstance(tr0.max, float)
    # a slice, pooled, tensor in; a stepped view is gathered
    start, stop = 1003, 9001
    for src, sl in ((torch.from_numpy(a).cuda(), slice(None)),
                    (torch.from_numpy(np.repeat(a, 2)).cuda()[::2], slice(None))):
        e = gpu.signal_envelope(src, sr, start=start, stop=stop, max_points=100)
        assert e.bin == 80 and isinstance(e.hi, torch.Tensor) and e.hi.is_cuda and e.lo is not e.hi
        wmin, wmax = tr.envelope_of(line, start, stop, 80)
        assert np.array_equal(e.lo.cpu().numpy(), wmin) and np.array_equal(e.hi.cpu().numpy(), wmax)
        assert np.array_equal(e.x, t_axis[start:stop:80]) and len(e.x) == 100
        assert e.argmax == start + np.argmax(line[start:stop]) and e.max == line[start:stop].max()
    # slice rules and sample indices
    e = gpu.signal_envelope(a, start=-500, max_points=7)
    assert e.bin == 72 and np.array_equal(e.x, np.arange(n - 500, n, 72).astype(np.float64))
    assert np.array_equal(e.hi, tr.envelope_of(line, n - 500, n, 72)[1])
    # dB: 20 * np.log10(np.abs(signal) + eps) within 8 ulp
    with np.errstate(divide="ignore"):
        want = 20 * np.log10(line[start:stop] + line.dtype.type(1e-9))
    d = gpu.signal_envelope(a, sr, start=start, stop=stop, db=True, eps=1e-9)
    assert d.hi.dtype == want.dtype and tr.ulps(d.hi, want).max() <= 8
    assert d.argmax == start + np.argmax(want) and abs(d.max - want.max()) <= 8 * np.spacing(abs(want.max()))
    d = gpu.signal_envelope(a, sr, start=start, stop=stop, db=True, eps=1e-9, max_points=50)
    wmin, wmax = tr.envelope_of(want, 0, stop - start, d.bin)
    assert tr.ulps(d.hi, wmax).max() <= 8 and tr.ulps(d.lo, wmin).max() <= 8


# ---------------------------------------------------------------------------
# capture_spectrum
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spectrum_refs(n):
    x = ref.synth_iq(n, seed=n)
    return x, acc.dft(x), acc.dft(x, False, np.complex128)


@pytest.mark.parametrize("n", [1000, 8192, 65_537, 1 << 18])
def test_capture_spectrum_accuracy(gpu, n, monkeypatch):
    """The direct sum, the in-LDS plan, Bluestein and the four-step transform.
    ceil(n / max_points) is not 300 for any max_points at every length, so the
    bin width capture_spectrum derives from max_points is set directly."""
    from vector_amd import traces
    x, r32, r64 = spectrum_refs(n)
    m64 = np.abs(r64)
    bound = K_EXACT * np.max(np.abs(r32 - r64)) + 2.0 ** -23 * m64.max()
    for bin_ in (1, 300):
        for shift in (True, False):
            monkeypatch.setattr(traces, "trace_bin", lambda count, max_points, b=bin_: b)
            t = gpu.capture_spectrum(x, 56e6, scale="linear", shift=shift)
            assert t.bin == bin_ and t.hi.dtype == np.float32 and (t.lo is t.hi) == (bin_ == 1)
            wmin, wmax = tr.envelope_of(tr.line(r64, shift), 0, n, bin_)
            err = max(np.max(np.abs(t.hi - wmax)), np.max(np.abs(t.lo - wmin)))
            print(f"ACC capture_spectrum n={n} bin={bin_} shift={int(shift)}: max err {err:.3e} "
                  f"bound {bound:.3e} ratio {err / bound:.3f}")
            assert err <= bound
            assert np.array_equal(t.x, tr.freq_axis(n, 56e6, 0.0, shift)[::bin_])


def linear_line(gpu, x, shift=True, **kw):
    """The GPU's own |X| line, the input of the restatement below."""
    return gpu.capture_spectrum(x, 56e6, scale="linear", shift=shift, **kw).hi


def test_capture_spectrum_scales_band_and_normalize(gpu):
    n, sr, fc = 12_289, 56e6, 5.23e9
    x = ref.synth_iq(n, seed=9)
    lin = linear_line(gpu, x)
    assert lin.dtype == np.float32
    f = tr.freq_axis(n, sr, fc, True)
    # dB of the same transform: the device's map of the linear line
    for shift in (True, False):
        d = gpu.capture_spectrum(x, sr, fc, eps=1e-12, shift=shift)
        lin_s = lin if shift else np.fft.ifftshift(lin)
        assert np.array_equal(d.hi, device_db(gpu, lin_s, 1e-12)) and d.lo is d.hi
        assert tr.ulps(d.hi, tr.db20(lin_s, 1e-12)).max() <= 8
        assert np.array_equal(d.x, tr.freq_axis(n, sr, fc, shift))
        assert d.argmax == np.argmax(lin_s) and d.max == float(d.hi.max())
    # the band of analyze_vectors.py:28, pooled
    band = (fc - 9e6, fc + 4.5e6)
    mask = (f >= band[0]) & (f <= band[1])
    b = gpu.capture_spectrum(x, sr, fc, scale="linear", band=band)
    assert np.array_equal(b.hi, lin[mask]) and np.array_equal(b.x, f[mask])
    lo = int(np.argmax(mask))
    assert b.argmax == lo + np.argmax(lin[mask]) and b.max == float(lin[mask].max())
    bp = gpu.capture_spectrum(x, sr, fc, scale="linear", band=band, max_points=50)
    wmin, wmax = tr.envelope_of(lin, lo, lo + mask.sum(), bp.bin)
    assert bp.bin == -(-mask.sum() // 50) and np.array_equal(bp.hi, wmax) and np.array_equal(bp.lo, wmin)
    assert np.array_equal(bp.x, f[mask][::bp.bin])
    # normalize: minus the maximum of the whole spectrum (mat_analyzer.py:215), in float32
    whole = device_db(gpu, lin, 1e-12)
    nz = gpu.capture_spectrum(x, sr, fc, eps=1e-12, normalize=True)
    assert nz.hi.dtype == np.float32 and np.array_equal(nz.hi, whole - whole.max()) and nz.max == 0.0
    nb = gpu.capture_spectrum(x, sr, fc, eps=1e-12, normalize=True, band=(fc + 10e6, fc + 20e6), max_points=20)
    m2 = (f >= fc + 10e6) & (f <= fc + 20e6)
    lo2 = int(np.argmax(m2))
    wmin, wmax = tr.envelope_of(whole, lo2, lo2 + m2.sum(), nb.bin)
    assert np.array_equal(nb.hi, wmax - whole.max()) and np.array_equal(nb.lo, wmin - whole.max())
    assert nb.max == float(wmax.max() - whole.max()) and nb.max < 0
    # an empty band
    e = gpu.capture_spectrum(x, sr, fc, band=(fc + 40e6, fc + 50e6))
    assert len(e.x) == 0 and len(e.hi) == 0 and e.argmax == -1


def test_capture_spectrum_dtypes_and_remove_dc(gpu):
    n, sr = 8192, 56e6
    x = ref.synth_iq(n, seed=13) + np.complex64(3 - 2j)
    lin = linear_line(gpu, x)
    # complex128 in: the complex64 transform's values, widened
    w = gpu.capture_spectrum(x.astype(np.complex128), sr, scale="linear")
    assert w.hi.dtype == np.float64 and np.array_equal(w.hi, lin.astype(np.float64))
    wn = gpu.capture_spectrum(x.astype(np.complex128), sr, eps=1e-12, normalize=True, max_points=64)
    assert wn.hi.dtype == np.float64 and wn.lo.dtype == np.float64 and wn.hi.max() == 0.0 == wn.max
    # tensor in, tensors out
    td = gpu.capture_spectrum(torch.from_numpy(x).cuda(), sr, scale="linear", max_points=100)
    assert td.hi.is_cuda and td.lo.is_cuda and td.hi.dtype == torch.float32 and isinstance(td.x, np.ndarray)
    wmin, wmax = tr.envelope_of(lin, 0, n, td.bin)
    assert np.array_equal(td.hi.cpu().numpy(), wmax) and np.array_equal(td.lo.cpu().numpy(), wmin)
    # real input is widened to complex
    r = np.random.default_rng(5).standard_normal(n)
    for dt, out in ((np.float32, np.float32), (np.float64, np.float64)):
        g = gpu.capture_spectrum(r.astype(dt), sr, scale="linear", shift=False)
        want = np.abs(np.fft.fft(r.astype(dt).astype(np.float64)))
        assert g.hi.dtype == out and np.max(np.abs(g.hi - want)) <= 1e-5 * want.max()
    # remove_dc changes bin 0 alone beyond rounding (mat_analyzer.py:203)
    dc = gpu.capture_spectrum(x, sr, scale="linear", shift=False, remove_dc=True).hi
    raw = np.fft.ifftshift(lin)
    r64 = np.abs(np.fft.fft(x.astype(np.complex128)))
    assert raw[0] > 0.9 * n * abs(3 - 2j) and dc[0] < 1e-3 * raw[0]
    assert np.max(np.abs(dc[1:] - raw[1:])) <= 2 * K_EXACT * 2.0 ** -23 * r64.max()
