"""Every device entry point's reads and writes are confined to its operands.

Each case puts every device pointer of one call into a guard arena
(tests/guard_arena.py) and runs it under the three guard fills: writes stay
inside the documented output, inputs are never written, the elements the
contract calls unused (holes) and everything outside the operands never reach
an output, and the zero-fill result passes the entry point's existing parity
bound against a float64 / complex128 numpy reference.  The tolerance of each
family is the one of its parity test, named where it is applied.

Block sizes come from the library's queries (vsig_fir_block,
vsig_xcorr_bank_plan, vsig_psd_traces_plan, vsig_pfb_plan, vsig_peaks_tile,
vsig_runs_tile).  One geometry has no query: the single-template correlator's
block, which _xc_plan restates from the rule in api_xcorr.hip (the block is
fixed by the template length; the hop is even at 16384 points).

Every entry point is held to the bit-identical read bound.  The detector
self-tests at the end show the harness failing, on one entry point per
family, when the library is told one element more than the harness.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.signal

import display_ref as dr
import guard_arena as ga
import special_values as sv
import trace_ref as tr
from guard_arena import Case, GuardViolation, In, Out
from oracle import ref
from peaks_ref import ref_peaks
from runs_ref import run_stats, runs_ref
from vector_amd import _lib

gpu_test = pytest.mark.gpu
P = C.c_void_p
DT = {"c128": np.complex128, "c64": np.complex64, "f64": np.float64, "f32": np.float32}
CODE = _lib.DTYPES
SKEW2 = [(0, 0), (1, 0), (0, 1), (1, 1)]          # (input, output) skew in elements

# entry point -> the tests that cover it (filled by @covers)
TABLE = {}
EXEMPT = {
    "vsig_copy_dev": "a hipMemcpyAsync of the caller's byte count: no kernel, no bounds logic of ours",
    "vsig_xcorr_bank_create_dev": "exercised inside every vsig_xcorr_bank_exec_dev case, its template rows in an arena",
}
EXEC_ENTRIES = ["vsig_fir_exec_dev", "vsig_fir_exec_hist_dev", "vsig_fir_exec_mix_dev", "vsig_xcorr_exec_dev",
                "vsig_xcorr_bank_exec_dev"]


def covers(*entries):
    def deco(fn):
        for e in entries:
            TABLE.setdefault(e, []).append(fn.__name__)
        return gpu_test(fn)
    return deco


def iq(n, seed, dt=np.complex64, scale=1.0):
    rng = np.random.default_rng([seed, n])
    x = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        x = x + 1j * rng.standard_normal(n)
    return (x * scale).astype(dt)


def normwise(y, r, tol, what=""):
    """max |y - r| <= tol max |r| (tests/test_gpu_parity.py assert_normwise)."""
    y, r = np.asarray(y), np.asarray(r)
    assert y.shape == r.shape, (what, y.shape, r.shape)
    err = np.abs(y.astype(np.complex128) - r.astype(np.complex128)).max() / max(np.abs(r).max(), 1e-30)
    assert err <= tol, f"{what} error {err:.3e} > {tol}"


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    ok = sv.same_bits(got, want) if got.dtype.kind in "fc" else got == want
    assert np.all(ok), (what, "first mismatches", np.flatnonzero(~np.asarray(ok).reshape(-1))[:5])


def skew(op_dtype, elems):
    return int(elems) * np.dtype(op_dtype).itemsize


TALLY = {}


def run(case):
    TALLY[case.entry] = TALLY.get(case.entry, 0) + 1
    return ga.run(case, "cuda")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if TALLY:
        print(f"\nbounds: {sum(TALLY.values())} cases of 4 calls each over {len(TALLY)} entry points: "
              + ", ".join(f"{k[5:]} {v}" for k, v in sorted(TALLY.items())))


# =========================================================================== completeness (no GPU)
def test_every_device_entry_point_has_a_case():
    """Every *_dev name of the ABI and the five exec entry points without the
    suffix are in the case table or exempt with a reason; nothing is both."""
    want = {n for n in _lib.SIGNATURES if n.endswith("_dev")} | set(EXEC_ENTRIES)
    assert set(EXEC_ENTRIES) <= set(_lib.SIGNATURES)
    assert want == set(TABLE) | set(EXEMPT), (sorted(want - set(TABLE) - set(EXEMPT)),
                                               sorted((set(TABLE) | set(EXEMPT)) - want))
    assert not set(TABLE) & set(EXEMPT)
    assert sorted(EXEMPT) == ["vsig_copy_dev", "vsig_xcorr_bank_create_dev"]
    assert all(len(r.splitlines()) == 1 and r for r in EXEMPT.values())
    assert not any(n.startswith("vsig_chain_") for n in TABLE)


# =========================================================================== the harness on CPU tensors
def _view(addr, n, dt):
    return np.ctypeslib.as_array((C.c_ubyte * (n * np.dtype(dt).itemsize)).from_address(addr)).view(dt)


def _cpu_case(fake, n=100, holes=None, inplace=False):
    """y = 2 x over float32 by a host function standing in for an entry point."""
    x = np.arange(1, n + 1, dtype=np.float32)
    ins = {"x": In(x, skew=4, holes=holes, inplace=inplace)}
    outs = {} if inplace else {"y": Out(n, np.float32, skew=8)}
    used = np.ones(n, bool) if holes is None else ~np.asarray(holes)

    def check(o):
        got = o["x" if inplace else "y"]
        assert np.array_equal(got[used], 2 * x[used])
    return Case("fake_entry", f"n={n}", ins, outs, lambda p: fake(p, n), check)


def _good(p, n):
    _view(p["y"], n, np.float32)[:] = 2 * _view(p["x"], n, np.float32)
    return 0


def test_harness_passes_a_correct_call():
    out = ga.run(_cpu_case(_good), "cpu")
    assert np.array_equal(out["y"], 2 * np.arange(1, 101, dtype=np.float32))


@pytest.mark.parametrize("which,bound,operand,offset", [
    ("write_after", "write", "y", 400), ("write_before", "write", "y", -1), ("read_after", "read", "y", 396),
    ("read_before", "read", "y", 0), ("read_hole", "read", "y", 28), ("writes_input", "const", "x", 14),
    ("writes_input_guard", "const", "x", -4), ("status", "status", None, None),
    ("unstable", "stable", "y", 2), ("wrong", "value", None, None)])
def test_harness_reports_each_violation(which, bound, operand, offset):
    n = 100
    state = {"calls": 0}

    def fake(p, n):
        x, y = _view(p["x"], n, np.float32), _view(p["y"], n, np.float32)
        state["calls"] += 1
        with np.errstate(over="ignore"):
            y[:] = 2 * x
        if which == "write_after":
            _view(p["y"] + 4 * n, 1, np.float32)[0] = 1.0
        if which == "write_before":
            _view(p["y"] - 1, 1, np.uint8)[0] = 0
        if which == "read_after":
            y[n - 1] += _view(p["x"] + 4 * n, 1, np.float32)[0]
        if which == "read_before":
            y[0] += _view(p["x"] - 4, 1, np.float32)[0]
        if which == "read_hole":
            y[7] += x[7]
        if which == "writes_input":
            x[3] = 0
        if which == "writes_input_guard":
            _view(p["x"] - 4, 1, np.float32)[0] = 5.0
        if which == "unstable":
            y[0] += state["calls"]
        if which == "wrong":
            y[5] = 0
        return -2 if which == "status" else 0

    holes = np.zeros(n, bool)
    holes[7] = True
    case = _cpu_case(fake, n, holes if which == "read_hole" else None)
    with pytest.raises(GuardViolation) as e:
        ga.run(case, "cpu")
    v = e.value
    assert (v.bound, v.operand, v.offset) == (bound, operand, offset), str(v)
    assert v.entry == "fake_entry" and "fake_entry [n=100]" in str(v) and bound in str(v)


def test_harness_in_place_operand_and_unstable_mode():
    def fake(p, n):
        _view(p["x"], n, np.float32)[:] *= 2
        return 0
    out = ga.run(_cpu_case(fake, 50, inplace=True), "cpu")
    assert np.array_equal(out["x"], 2 * np.arange(1, 51, dtype=np.float32))
    # not bit-stable, but right under every fill: passes only with stable=False
    state = {"k": 0}

    def jitter(p, n):
        state["k"] += 1
        _view(p["y"], n, np.float32)[:] = 2 * _view(p["x"], n, np.float32)
        _view(p["y"], n, np.float32)[0] = np.nextafter(np.float32(2), np.float32(2 + state["k"] % 2))
        return 0
    case = _cpu_case(jitter, 20)
    case.check = lambda o: np.testing.assert_allclose(o["y"], 2 * np.arange(1, 21), rtol=1e-6)
    with pytest.raises(GuardViolation, match="stable"):
        ga.run(case, "cpu")
    case.stable = False
    ga.run(case, "cpu")

    def leaks(p, n):            # a stray read in the unstable mode: the NaN fill shows as a non-finite output
        _view(p["y"], n, np.float32)[:] = 2 * _view(p["x"], n, np.float32)
        _view(p["y"], n, np.float32)[3] += 0 * _view(p["x"] + 4 * n, 1, np.float32)[0]
        return 0
    case = _cpu_case(leaks, 20)
    case.stable = False
    with pytest.raises(GuardViolation, match="non-finite"):
        ga.run(case, "cpu")


def corr_ref(a, v, mode):
    """np.correlate(a, v, mode) in complex128 by one FFT of the whole length
    (np.correlate itself is O(na nv)): the full sequence is the same for
    either operand order; 'valid' and 'same' are numpy's slices of it, 'same'
    taken after numpy's operand swap when a is the shorter."""
    a, v = np.asarray(a).astype(np.complex128), np.asarray(v).astype(np.complex128)
    na, nv = len(a), len(v)
    full = scipy.signal.fftconvolve(a, np.conj(v[::-1]), "full")
    lo, hi = min(na, nv), max(na, nv)
    if mode == "full":
        return full
    if mode == "valid":
        return full[lo - 1:hi]
    s = (lo - 1) // 2 if na >= nv else lo - 1 - (lo - 1) // 2
    return full[s:s + hi]


def corr_want(a, v, mode):
    """np.correlate itself in complex128 where it is affordable: its rounding
    decides exact ties of |c| (a stream shorter than a constant-modulus
    template has many), and the refine reproduces numpy's choice.  Beyond
    that the FFT form; those cases plant one clear maximum."""
    if len(a) * len(v) <= 4e6:
        return np.correlate(np.asarray(a).astype(np.complex128), np.asarray(v).astype(np.complex128), mode)
    return corr_ref(a, v, mode)


@pytest.mark.parametrize("na,nv", [(1, 1), (1, 5), (5, 1), (7, 4), (4, 7), (8, 5), (5, 8), (40, 40), (33, 12),
                                   (12, 33)])
def test_corr_ref_is_np_correlate(na, nv):
    a, v = iq(na, 1, np.complex128), iq(nv, 2, np.complex128)
    for mode in ("valid", "full", "same"):
        want = np.correlate(a, v, mode)
        got = corr_ref(a, v, mode)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (mode, na, nv)


# =========================================================================== stream ops
STREAM_N = [1, 255, 256, 257, 4095, 4096, 4097]
BIG_N = (1 << 21) + 5       # the 8192-block grid-stride loops of stream_ops.hip take a second trip


def scale_case(ctx, n, si=0, so=0, extra_in=0, short_out=0):
    x, s = iq(n, 11), np.float32(0.37)

    def call(p):
        return ctx.lib.vsig_scale_c64_dev(ctx.h, P(p["x"]), n + extra_in, float(s), P(p["y"]))

    def check(o):       # tests/test_gpu_formats.py test_transplant_matches_reference: 1e-6 of max |want|
        normwise(o["y"][:n], x.astype(np.complex128) * float(s), 1e-6, "scale")
    return Case("vsig_scale_c64_dev", f"n={n} skew=({si},{so})", {"x": In(x, skew(x.dtype, si))},
                {"y": Out(n + extra_in - short_out, np.complex64, skew(np.complex64, so))}, call, check)


@covers("vsig_scale_c64_dev")
@pytest.mark.parametrize("n", STREAM_N + [BIG_N])
def test_scale(gpu, n):
    ctx = gpu.get_context()
    for si, so in SKEW2 if n != BIG_N else SKEW2[:1]:
        run(scale_case(ctx, n, si, so))


@covers("vsig_mix_c64_dev")
@pytest.mark.parametrize("n", STREAM_N + [BIG_N])
def test_mix(gpu, n):
    ctx = gpu.get_context()
    f, sr, i0 = 1.25e6, 56e6, 12345
    w = 2 * np.pi * f
    for si, so in SKEW2 if n != BIG_N else SKEW2[:1]:
        x = iq(n, 12)
        want = x.astype(np.complex128) * np.exp(1j * w * (i0 + np.arange(n)) / sr)

        def call(p):
            return ctx.lib.vsig_mix_c64_dev(ctx.h, P(p["x"]), n, float(w), sr, i0, P(p["y"]))

        def check(o):   # tests/test_gpu_formats.py test_frequency_shift_matches_reference: 1e-6 |x| per sample
            err = np.abs(o["y"].astype(np.complex128) - want) / np.maximum(np.abs(x), 1e-30)
            assert err.max() <= 1e-6, err.max()
        run(Case("vsig_mix_c64_dev", f"n={n} skew=({si},{so})", {"x": In(x, skew(x.dtype, si))},
                 {"y": Out(n, np.complex64, skew(np.complex64, so))}, call, check))


@covers("vsig_wv_quantize_dev")
@pytest.mark.parametrize("n", STREAM_N + [BIG_N])
def test_wv_quantize(gpu, n):
    ctx = gpu.get_context()
    for k, (si, so) in enumerate(SKEW2 if n != BIG_N else SKEW2[:1]):
        x, norm = iq(n, 13, scale=0.2), (0.0, 1.7)[k % 2]
        want = ref.mat2wv_fields(x / np.float32(norm) if norm else x, False)[0]

        def call(p):
            return ctx.lib.vsig_wv_quantize_dev(ctx.h, P(p["x"]), n, float(norm), P(p["q"]))

        def check(o):   # tests/test_gpu_special_values.py test_a3_wv_quantize_is_numpys_cast: exact
            same_bits(o["q"], want, "wv")
        run(Case("vsig_wv_quantize_dev", f"n={n} norm={norm} skew=({si},{so})", {"x": In(x, skew(x.dtype, si))},
                 {"q": Out(2 * n, np.int16, skew(np.int16, so))}, call, check))


def _plane(np_t, n, seed):
    rng = np.random.default_rng([seed, n])
    dt = np.dtype(np_t)
    if dt.kind in "iu":
        ii = np.iinfo(dt)
        return rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
    return (rng.standard_normal(n) * 100).astype(dt)


@covers("vsig_planar_to_c64_dev")
@pytest.mark.parametrize("mi", [1, 2, 3, 4, 5, 6, 7, 9, 12, 13])
def test_planar_to_c64(gpu, mi):
    from vector_amd.vectors import _MI_NP
    assert sorted(_MI_NP) == [1, 2, 3, 4, 5, 6, 7, 9, 12, 13]       # every mi_type of the ABI
    ctx, np_t = gpu.get_context(), _MI_NP[mi]
    sizes = STREAM_N + ([BIG_N] if mi == 7 else [])
    for n in sizes:
        re, im = _plane(np_t, n, mi), _plane(np_t, n, 100 + mi)
        for with_im in (True, False):
            def call(p):
                return ctx.lib.vsig_planar_to_c64_dev(ctx.h, mi, P(p["re"]), P(p["im"]) if with_im else None, n,
                                                      P(p["y"]))

            def check(o):   # tests/test_gpu_special_values.py test_a4_planar_to_c64_every_storage_type: exact
                same_bits(np.ascontiguousarray(o["y"].real), re.astype(np.float32), "re")
                same_bits(np.ascontiguousarray(o["y"].imag),
                          im.astype(np.float32) if with_im else np.zeros(n, np.float32), "im")
            for si, so in SKEW2 if n != BIG_N else SKEW2[:1]:
                ins = {"re": In(re, skew(np_t, si))}
                if with_im:
                    ins["im"] = In(im, skew(np_t, 1 - si))
                run(Case("vsig_planar_to_c64_dev", f"mi={mi} n={n} im={with_im} skew=({si},{so})", ins,
                         {"y": Out(n, np.complex64, skew(np.complex64, so))}, call, check))


@covers("vsig_c64_to_planar_dev")
@pytest.mark.parametrize("n", STREAM_N + [BIG_N])
def test_c64_to_planar(gpu, n):
    ctx = gpu.get_context()
    for si, so in SKEW2 if n != BIG_N else SKEW2[:1]:
        x = iq(n, 14)

        def call(p):
            return ctx.lib.vsig_c64_to_planar_dev(ctx.h, P(p["x"]), n, P(p["re"]), P(p["im"]))

        def check(o):   # save_vector's planes are the parts themselves: exact
            same_bits(o["re"], np.ascontiguousarray(x.real), "re")
            same_bits(o["im"], np.ascontiguousarray(x.imag), "im")
        run(Case("vsig_c64_to_planar_dev", f"n={n} skew=({si},{so})", {"x": In(x, skew(x.dtype, si))},
                 {"re": Out(n, np.float32, skew(np.float32, so)), "im": Out(n, np.float32, skew(np.float32, 1 - so))},
                 call, check))


@covers("vsig_normalize_c64_dev")
@pytest.mark.parametrize("n", STREAM_N + [BIG_N])
def test_normalize(gpu, n):
    ctx = gpu.get_context()
    for k, (si, so) in enumerate(SKEW2 if n != BIG_N else SKEW2[:1]):
        for inplace in (False, True):
            x, m = iq(n, 15), np.array([2.5], np.float32)
            ins = {"x": In(x, skew(x.dtype, si), inplace=inplace), "m": In(m, skew(np.float32, k % 2))}
            outs = {} if inplace else {"y": Out(n, np.complex64, skew(np.complex64, so))}

            def call(p):
                return ctx.lib.vsig_normalize_c64_dev(ctx.h, P(p["x"]), n, P(p["m"]), P(p["x" if inplace else "y"]))

            def check(o):   # tests/test_gpu_vector_build.py test_max_and_normalize_bit_exact: numpy's x / m
                same_bits(o["x" if inplace else "y"], x / m[0], "normalize")
            run(Case("vsig_normalize_c64_dev", f"n={n} inplace={inplace} skew=({si},{so})", ins, outs, call, check))


@covers("vsig_vector_build_dev")
@pytest.mark.parametrize("n", STREAM_N + [BIG_N])
def test_vector_build(gpu, n):
    ctx = gpu.get_context()
    for k, (si, so) in enumerate(SKEW2 if n != BIG_N else SKEW2[:1]):
        for with_max in (True, False):
            la = min(n, 37)
            pa = la + 5
            ca = (n - la) // pa + 1
            sa = n - ((ca - 1) * pa + la)               # the last instance ends exactly at n
            lb = min(n, 100)
            ya, yb = iq(la, 16), iq(lb, 17)
            want = np.zeros(n, np.complex64)
            for j in range(ca):
                want[sa + j * pa:sa + j * pa + la] += ya
            want[0:lb] += yb
            assert sa + (ca - 1) * pa + la == n
            ins = {"ya": In(ya, skew(ya.dtype, si)), "yb": In(yb, skew(yb.dtype, 1 - si))}
            outs = {"out": Out(n, np.complex64, skew(np.complex64, so))}
            if with_max:
                outs["max"] = Out(1, np.float32, skew(np.float32, k % 2))

            def call(p):
                places = (_lib.PacketPlace * 2)(_lib.PacketPlace(p["ya"], la, sa, pa, ca),
                                                _lib.PacketPlace(p["yb"], lb, 0, lb, 1))
                return ctx.lib.vsig_vector_build_dev(ctx.h, places, 2, P(p["out"]), n,
                                                     P(p["max"]) if with_max else None)

            def check(o):   # tests/test_gpu_vector_build.py test_accumulate_is_numpy_bit_exact / test_max_...: exact
                same_bits(o["out"], want, "vector")
                if with_max:
                    same_bits(o["max"], np.array([np.max(np.abs(want))], np.float32), "max")
            run(Case("vsig_vector_build_dev", f"n={n} max={with_max} skew=({si},{so})", ins, outs, call, check))


# =========================================================================== FIR
def _fir_handle(ctx, taps, decim):
    h = P()
    t = np.ascontiguousarray(taps, np.complex64)
    ctx.check(ctx.lib.vsig_fir_create(ctx.h, t.ctypes.data_as(P), len(t), decim, C.byref(h)), "fir_create")
    return h


def _fir_sizes(M, ntaps, decim):
    """Input lengths around every hop the launchers may take for block M:
    the block's outputs M - (ntaps - 1) (a multiple of decim), the same after
    the tap overlap is rounded up to 16 (lo16), and 768 (the 1024-point pair)."""
    lo = ntaps - 1
    lo16 = ((lo + decim - 1) // decim * decim + 15) // 16 * 16
    hops = {(M - lo) // decim * decim, (M - lo16) // decim * decim}
    if M == 1024:
        hops.add(768)
    hops = sorted(h for h in hops if h >= 1)
    ns = {1, 5 * hops[0] + 3}
    for h in hops:
        ns |= {h - 1, h, h + 1, 2 * h + 1}
        # segment b starts lo_eff samples before output b h (after any history) and is M long: it ends at the
        # stream's end, one short of it and one past it when n = M - lo_eff + b h + d -- the unchecked / checked
        # choice of load_segment and load_pair_x4 -- for every overlap the launchers may take
        for lo_eff in {lo, (lo + 15) // 16 * 16, (lo + decim - 1) // decim * decim, lo16}:
            for b in (0, 1):
                ns |= {M - lo_eff + b * h + d for d in (-1, 0, 1)}
    return sorted(n for n in ns if n >= 1)


def _fir_ref(xe, taps, nhist, n, decim):
    t = np.asarray(taps).astype(np.complex128)
    x = xe.astype(np.complex128)
    y = scipy.signal.fftconvolve(x, t) if len(t) > 1024 else np.convolve(x, t)
    return y[nhist:nhist + n][::decim]


def _fir_case(f, ctx, entry, taps, decim, n, nhist, si, so, mix=None, extra_in=0, short_out=0):
    xe = iq(nhist + n, 21)
    ny = -(-(n + extra_in) // decim)

    def call(p):
        if entry == "vsig_fir_exec_dev":
            return ctx.lib.vsig_fir_exec_dev(f, P(p["x"]), n + extra_in, P(p["y"]), ny)
        if entry == "vsig_fir_exec_hist_dev":
            return ctx.lib.vsig_fir_exec_hist_dev(f, P(p["x"]), nhist, n, P(p["y"]), ny)
        return ctx.lib.vsig_fir_exec_mix_dev(f, P(p["x"]), nhist, n, P(p["y"]), ny, mix[0], mix[1], mix[2])

    def check(o):       # tests/test_gpu_parity.py FIR_TOL (tests/test_gpu_mixfir.py for the mixed form): 1e-5 normwise
        src = xe
        if mix:
            src = xe.astype(np.complex128) * np.exp(2j * np.pi * mix[0] * (mix[2] + np.arange(len(xe))) / mix[1])
        want = _fir_ref(src, taps, nhist, n, decim)
        normwise(o["y"][:len(want)], want, 1e-5, "fir")
    return Case(entry, f"ntaps={len(taps)} decim={decim} n={n} nhist={nhist} skew=({si},{so})",
                {"x": In(xe, skew(xe.dtype, si))}, {"y": Out(ny - short_out, np.complex64, skew(np.complex64, so))},
                call, check)


def _taps(ntaps):
    rng = np.random.default_rng(ntaps)
    return (rng.standard_normal(ntaps) / math.sqrt(ntaps)).astype(np.float32)


@covers("vsig_fir_exec_dev")
@pytest.mark.parametrize("decim", [1, 2, 3, 4])
@pytest.mark.parametrize("ntaps", [1, 64, 255, 257])
def test_fir_exec(gpu, ntaps, decim):
    """nhist = 0: the NaN in front of x must read as the zeros of the contract."""
    ctx, taps = gpu.get_context(), _taps(ntaps)
    f = _fir_handle(ctx, taps, decim)
    try:
        M = ctx.lib.vsig_fir_block(f)
        for n in _fir_sizes(M, ntaps, decim):
            for si, so in SKEW2:
                run(_fir_case(f, ctx, "vsig_fir_exec_dev", taps, decim, n, 0, si, so))
    finally:
        ctx.lib.vsig_fir_free(f)


@covers("vsig_fir_exec_hist_dev")
@pytest.mark.parametrize("decim", [1, 2, 3, 4])
@pytest.mark.parametrize("ntaps", [1, 64, 255, 257])
def test_fir_exec_hist(gpu, ntaps, decim):
    ctx, taps = gpu.get_context(), _taps(ntaps)
    f = _fir_handle(ctx, taps, decim)
    try:
        M = ctx.lib.vsig_fir_block(f)
        for nhist in sorted({0, 1, ntaps - 1, (ntaps - 1 + 15) // 16 * 16}):
            for n in _fir_sizes(M, ntaps, decim):
                for si, so in SKEW2:
                    run(_fir_case(f, ctx, "vsig_fir_exec_hist_dev", taps, decim, n, nhist, si, so))
    finally:
        ctx.lib.vsig_fir_free(f)


@covers("vsig_fir_exec_mix_dev")
@pytest.mark.parametrize("decim", [1, 2, 3, 4])
@pytest.mark.parametrize("ntaps", [1, 64, 255])
def test_fir_exec_mix(gpu, ntaps, decim):
    """The fused mixer: the default variant, ntaps <= 256."""
    ctx, taps = gpu.get_context(), _taps(ntaps)
    f = _fir_handle(ctx, taps, decim)
    try:
        M = ctx.lib.vsig_fir_block(f)
        for nhist in sorted({0, 1, ntaps - 1, (ntaps - 1 + 15) // 16 * 16}):
            for n in _fir_sizes(M, ntaps, decim):
                for si, so in SKEW2:
                    run(_fir_case(f, ctx, "vsig_fir_exec_mix_dev", taps, decim, n, nhist, si, so,
                                  mix=(1.25e6, 56e6, 1000 + n)))
    finally:
        ctx.lib.vsig_fir_free(f)


@covers("vsig_fir_exec_dev", "vsig_fir_exec_hist_dev")
@pytest.mark.parametrize("decim,n,nhist", [(1, 20_000, 0), (3, 20_000, 0), (1, 20_000, 8299), (4, 20_000, 8304),
                                           (1, BIG_N, 0)])
def test_fir_parts(gpu, decim, n, nhist):
    """Over 8192 taps: 8192-tap parts summed with their delays (fir_part_accum),
    at 2^21 + 5 samples with a second trip of its grid-stride loop."""
    ctx, taps = gpu.get_context(), _taps(8300)
    f = _fir_handle(ctx, taps, decim)
    try:
        entry = "vsig_fir_exec_hist_dev" if nhist else "vsig_fir_exec_dev"
        for si, so in SKEW2 if n != BIG_N else SKEW2[:1]:
            run(_fir_case(f, ctx, entry, taps, decim, n, nhist, si, so))
    finally:
        ctx.lib.vsig_fir_free(f)


# =========================================================================== PSD and its traces
NFFTS = [64, 1024, 8192, 16384, 32768, 100, 1000]


def _psd_setup(nfft, nperseg, hop, stride, nframes, tail, shift, seed):
    """(payload, holes, window, n, reference Sxx[nframes][nfft] in float64)."""
    n = (nframes - 1) * hop + nperseg + tail
    assert tail < hop and (n - nperseg) // hop + 1 == nframes
    span = (n - 1) * stride + 1
    x = iq(span, seed)
    used = np.zeros(span, bool)
    idx = (np.arange(nframes)[:, None] * hop + np.arange(nperseg)[None, :]) * stride
    used[idx.reshape(-1)] = True
    win = scipy.signal.get_window("hann", nperseg).astype(np.float32)
    scale = np.float32(1.0 / float(win.astype(np.float64).sum()) ** 2)
    X = np.fft.fft(x[idx].astype(np.complex128) * win.astype(np.float64)[None, :], nfft, axis=1)
    S = (X.real ** 2 + X.imag ** 2) * float(scale)
    if shift:
        S = np.fft.fftshift(S, axes=1)
    return x, ~used, win, n, float(scale), S


def _psd_combos(nfft, full, stride):
    """The whole product nperseg x hop x nframes x tail x shift of the issue
    for one stride; the skews of x, the output and the window rotate so that
    every combination of the first two meets every (nperseg, hop)."""
    k = 0
    nperseg = nfft if full else nfft - 37
    for hop in (nperseg, nperseg // 2 + 1, 2 * nfft + 3):
        for nframes in (1, 2, 3):
            for tail in (0, min(nperseg, hop) - 1):
                for shift in (0, 1):
                    yield nperseg, hop, stride, nframes, tail, shift, SKEW2[(k + k // 12) % 4], (k // 3) % 2
                    k += 1


PSD_PARAMS = [(nfft, full, stride) for nfft in NFFTS for full in (True, False) for stride in (1, 3)]


@covers("vsig_psd_c64_dev")
@pytest.mark.parametrize("nfft,full,stride", PSD_PARAMS)
def test_psd(gpu, nfft, full, stride):
    ctx = gpu.get_context()
    for nperseg, hop, stride, nframes, tail, shift, _, sw in _psd_combos(nfft, full, stride):
        x, holes, win, n, scale, S = _psd_setup(nfft, nperseg, hop, stride, nframes, tail, shift, nfft + hop)
        for si, so in SKEW2:
            run(psd_case(ctx, x, holes, win, n, stride, nperseg, hop, nfft, scale, shift, nframes, S, si, so, sw))


def psd_case(ctx, x, holes, win, n, stride, nperseg, hop, nfft, scale, shift, nframes, S, si, so, sw,
             extra_in=0, short_out=0):
    def call(p):
        return ctx.lib.vsig_psd_c64_dev(ctx.h, P(p["x"]), n + extra_in, stride, P(p["win"]), nperseg, hop, nfft,
                                        scale, shift, P(p["sxx"]), (n + extra_in - nperseg) // hop + 1)

    def check(o):       # tests/test_gpu_parity.py assert_spectra_close: 1e-5 of each frame's maximum
        got = o["sxx"][:nframes * nfft].reshape(nframes, nfft).astype(np.float64)
        err = (np.abs(got - S).max(axis=1) / np.maximum(S.max(axis=1), 1e-30)).max()
        assert err <= 1e-5, f"spectrum error {err:.3e}"
    nf_lib = (n + extra_in - nperseg) // hop + 1
    return Case("vsig_psd_c64_dev", f"nfft={nfft} nperseg={nperseg} hop={hop} stride={stride} nframes={nframes} "
                f"n={n} shift={shift} skew=({si},{so},{sw})",
                {"x": In(x, skew(x.dtype, si), holes=holes), "win": In(win, skew(np.float32, sw))},
                {"sxx": Out(nf_lib * nfft - short_out, np.float32, skew(np.float32, so))}, call, check)


def _traces_case(ctx, nfft, nperseg, hop, stride, nframes, tail, shift, si, so, sw, which, setup=None):
    x, holes, win, n, scale, S = setup or _psd_setup(nfft, nperseg, hop, stride, nframes, tail, shift,
                                                     nfft + hop + 1)
    outs = {}
    for k, (name, dt) in enumerate((("mean", np.float64), ("max", np.float32), ("min", np.float32))):
        if name in which:
            outs[name] = Out(nfft, dt, skew(dt, (so + k) % 2))

    def call(p):
        return ctx.lib.vsig_psd_traces_c64_dev(ctx.h, P(p["x"]), n, stride, P(p["win"]), nperseg, hop, nfft, scale,
                                               shift, nframes, *(P(p[k]) if k in which else None
                                                                 for k in ("mean", "max", "min")))

    def check(o):
        # max, min and mean over frames are 1-Lipschitz in the sup norm (tests/spectrum_traces_ref.py bound), so
        # test_gpu_parity.py's 1e-5 of the largest frame maximum carries over
        tol = 1e-5 * S.max()
        want = {"mean": S.mean(axis=0), "max": S.max(axis=0), "min": S.min(axis=0)}
        for name in which:
            err = np.abs(o[name].astype(np.float64) - want[name]).max()
            assert err <= tol, f"{name} error {err:.3e} > {tol:.3e}"
    return Case("vsig_psd_traces_c64_dev", f"nfft={nfft} nperseg={nperseg} hop={hop} stride={stride} "
                f"nframes={nframes} n={n} shift={shift} out={'+'.join(which)} skew=({si},{so},{sw})",
                {"x": In(x, skew(x.dtype, si), holes=holes), "win": In(win, skew(np.float32, sw))}, outs, call, check)


WHICH = [("mean", "max", "min"), ("mean",), ("max",), ("min",), ("max", "min"), ("mean", "min")]


@covers("vsig_psd_traces_c64_dev")
@pytest.mark.parametrize("nfft,full,stride", PSD_PARAMS)
def test_psd_traces(gpu, nfft, full, stride):
    """Every shape under all four skew pairs; which of mean / max / min are
    NULL rotates over the product (each is present and NULL at every nfft)."""
    ctx = gpu.get_context()
    combos = _psd_combos(nfft, full, stride)
    for k, (nperseg, hop, stride, nframes, tail, shift, _, sw) in enumerate(combos):
        setup = _psd_setup(nfft, nperseg, hop, stride, nframes, tail, shift, nfft + hop + 1)
        for j, (si, so) in enumerate(SKEW2):
            run(_traces_case(ctx, nfft, nperseg, hop, stride, nframes, tail, shift, si, so, sw,
                             WHICH[(k + j) % len(WHICH)], setup))


def _traces_plan(lib, nfft, nframes):
    b, step, fpb = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.vsig_psd_traces_plan(nfft, nframes, C.byref(b), C.byref(step), C.byref(fpb)) == 0
    return b.value, step.value, fpb.value


@covers("vsig_psd_traces_c64_dev")
@pytest.mark.parametrize("nfft", [64, 1024, 8192])
def test_psd_traces_block_edges(gpu, nfft):
    """Frame counts at which, by vsig_psd_traces_plan queried for that very
    count, the last of several blocks owns one frame, all but one of its
    frames_per_block, and all of them: the nearest such counts below 2^20
    samples.  Each runs under all four skew pairs with all three outputs."""
    ctx = gpu.get_context()
    n0 = (1 << 20) // nfft
    fpb0 = _traces_plan(ctx.lib, nfft, n0)[2]
    found = {}
    for nframes in range(n0, max(1, n0 - 4 * fpb0 - 4), -1):
        b, step, fpb = _traces_plan(ctx.lib, nfft, nframes)
        assert fpb >= 1 and b >= 1 and (b - 1) * fpb < nframes <= b * fpb
        owned = nframes - (b - 1) * fpb
        if b >= 2:
            for kind, hit in (("one", owned == 1), ("all but one", owned == fpb - 1), ("all", owned == fpb)):
                if hit:
                    found.setdefault(kind, nframes)
    assert "one" in found and "all" in found and (fpb0 < 3 or "all but one" in found), (found, fpb0)
    for k, nframes in enumerate(sorted(set(found.values()))):
        setup = _psd_setup(nfft, nfft, nfft, 1, nframes, 0, k % 2, nfft + 1)
        for si, so in SKEW2:
            run(_traces_case(ctx, nfft, nfft, nfft, 1, nframes, 0, k % 2, si, so, k % 2, WHICH[0], setup))


# =========================================================================== correlators
XC_L = [1, 64, 1000, 4096, 4097, 8192, 9000]
XC_L_STREAM = XC_L + [17_000]               # over 16384: one pass per 8192-sample chunk, accumulated in c


def _xc_plan(L):
    """(M, [hop, ...]) of the single-template correlator.  The library has no
    query for it, so this restates the rule of api_xcorr.hip (os_size_xcorr and
    xcorr_run): M = 4096 up to L = 1024, 8192 up to 2048, 16384 up to 8192,
    32768 up to 16384; hop = M - L + 1 outputs per block, rounded down to even
    at M = 16384.  Longer templates run one M = 16384 pass per 8192-sample
    chunk, each with the hop of its own chunk length."""
    if L > 16384:
        chunks = [min(8192, L - p) for p in range(0, L, 8192)]
        return 16384, sorted({16384 - lp + 1 for lp in chunks})
    M = 4096 if L <= 1024 else 8192 if L <= 2048 else 16384 if L <= 8192 else 32768
    hop = M - L + 1
    if M == 16384 and hop > 1:
        hop &= ~1
    return M, [hop]


def _xc_sizes(L, mode):
    """Stream lengths for np.correlate(s, p, mode) with len(p) = L: L and
    L + 1.  In outputs: 1, 2, one block's outputs - 1 / + 0 / + 1, two blocks' likewise,
    three blocks + 5.  In samples: block b reads M samples from b hop - off
    (off = 0 for valid, L - 1 for full, either half of L - 1 for same), so it
    ends with the stream, one sample short of it and one past it at
    n = M - off + b hop + d: the choice between the unchecked and the checked
    loads, for the first two blocks."""
    M, hops = _xc_plan(L)
    offs = {"valid": [0], "full": [L - 1], "same": sorted({(L - 1) // 2, L - 1 - (L - 1) // 2})}[mode]
    ns = {L, L + 1}
    for hop in hops:
        nouts = {1, 2, hop - 1, hop, hop + 1, 2 * hop - 1, 2 * hop, 2 * hop + 1, 3 * hop + 5}
        # outputs -> samples: n - L + 1 (valid), n + L - 1 (full), n (same, the stream the longer operand)
        ns |= {nout + {"valid": L - 1, "full": 1 - L, "same": 0}[mode] for nout in nouts}
        ns |= {M - off + b * hop + d for off in offs for b in (0, 1) for d in (-1, 0, 1)}
    return sorted(n for n in ns if n >= (1 if mode == "full" else L))


def _planted(n, tmpl, seed):
    """Noise with the template added where it fits: one clear maximum."""
    s = iq(n, seed, scale=0.3)
    if n >= len(tmpl):
        at = (n - len(tmpl)) // 3
        s[at:at + len(tmpl)] += tmpl.astype(s.dtype)
    return s


def _check_peak(rec, cref, what):
    """The 32-byte record against |c| of the reference: index and, to 1e-9, the
    refined maximum (tests/test_gpu_alignment.py); the sums to 1e-5
    (tests/test_gpu_xcorr_bank.py test_values)."""
    a = np.abs(cref)
    peak, s1, s2 = rec.view(np.float64)[[0, 2, 3]]
    idx = int(rec.view(np.int64)[1])
    assert idx == int(np.argmax(a)), (what, idx, int(np.argmax(a)))
    assert abs(peak / a.max() - 1) <= 1e-9, (what, peak, a.max())
    assert abs(s1 / a.sum() - 1) <= 1e-5 and abs(s2 / (a * a).sum() - 1) <= 1e-5, (what, s1, a.sum(), s2)


def xcorr_case(ctx, h, tmpl, n, mode, with_c, si, so, extra_in=0, short_out=0, want=None):
    L = len(tmpl)
    s = _planted(n, tmpl, 31)
    want = corr_want(s, tmpl, mode) if want is None else want
    nout = n + extra_in - L + 1 if mode == "valid" else n + extra_in + L - 1
    outs = {"peak": Out(4, np.float64, skew(np.float64, so))}
    if with_c:
        outs["c"] = Out(nout - short_out, np.complex64, skew(np.complex64, so))

    def call(p):
        return ctx.lib.vsig_xcorr_exec_dev(h, P(p["s"]), n + extra_in, _lib.MODES[mode], P(p["c"]) if with_c else None,
                                           P(p["peak"]))

    def check(o):       # tests/test_gpu_parity.py XC_TOL: 1e-5 normwise
        if with_c:
            normwise(o["c"][:len(want)], want, 1e-5, "xcorr")
        _check_peak(o["peak"], want, "xcorr")
    return Case("vsig_xcorr_exec_dev", f"L={L} n={n} mode={mode} c={with_c} skew=({si},{so})",
                {"s": In(s, skew(s.dtype, si))}, outs, call, check)


def _xcorr_handle(ctx, tmpl):
    h = P()
    ctx.sync_blas_threads()
    ctx.check(ctx.lib.vsig_xcorr_create(ctx.h, tmpl.ctypes.data_as(P), len(tmpl), C.byref(h)), "xcorr_create")
    return h


@covers("vsig_xcorr_exec_dev")
@pytest.mark.parametrize("mode", ["valid", "full"])
@pytest.mark.parametrize("L", XC_L_STREAM)
def test_xcorr_exec(gpu, L, mode):
    ctx, tmpl = gpu.get_context(), ref.qpsk_preamble(L, seed=L)
    h = _xcorr_handle(ctx, tmpl)
    try:
        for n in _xc_sizes(L, mode):
            want = corr_want(_planted(n, tmpl, 31), tmpl, mode)
            for with_c in (True, False):
                for si, so in SKEW2:
                    run(xcorr_case(ctx, h, tmpl, n, mode, with_c, si, so, want=want))
    finally:
        ctx.lib.vsig_xcorr_free(h)


def _correlate_case(ctx, entry, a, v, mode, in128, out128, with_c, with_peak, si, so, want=None):
    dt_in = np.complex128 if in128 else np.complex64
    dt_out = np.complex128 if out128 else np.complex64
    a, v = a.astype(dt_in), v.astype(dt_in)
    want = corr_want(a, v, mode) if want is None else want
    outs = {}
    if with_c:
        outs["c"] = Out(len(want), dt_out, skew(dt_out, so))
    if with_peak:
        outs["peak"] = Out(4, np.float64, skew(np.float64, so))

    def call(p):
        c, pk = P(p["c"]) if with_c else None, P(p["peak"]) if with_peak else None
        if entry == "vsig_correlate_c64_dev":
            return ctx.lib.vsig_correlate_c64_dev(ctx.h, P(p["a"]), len(a), P(p["v"]), len(v), _lib.MODES[mode], c, pk)
        return ctx.lib.vsig_correlate_dev(ctx.h, CODE["c128" if in128 else "c64"], P(p["a"]), len(a), P(p["v"]),
                                          len(v), _lib.MODES[mode], CODE["c128" if out128 else "c64"], c, pk)

    def check(o):       # tests/test_gpu_parity.py XC_TOL: 1e-5 normwise
        if with_c:
            normwise(o["c"], want, 1e-5, "correlate")
        if with_peak:
            _check_peak(o["peak"], want, "correlate")
    return Case(entry, f"na={len(a)} nv={len(v)} mode={mode} in128={in128} out128={out128} c={with_c} "
                f"peak={with_peak} skew=({si},{so})",
                {"a": In(a, skew(dt_in, si)), "v": In(v, skew(dt_in, 1 - si))}, outs, call, check)


# (in128, out128, c present, peak present, operands swapped)
CORR_VARIANTS = [(False, False, True, True, False), (False, False, False, True, False),
                 (False, False, True, True, True), (True, False, True, True, False),
                 (False, True, True, True, False), (True, True, True, False, True)]


@covers("vsig_correlate_dev")
@pytest.mark.parametrize("mode", ["valid", "full", "same"])
@pytest.mark.parametrize("L", XC_L)
def test_correlate(gpu, L, mode):
    """Every size of _xc_sizes for the mode (the handle is built by the same
    rule as the streaming correlator's), every variant, all four skew pairs."""
    ctx, tmpl = gpu.get_context(), ref.qpsk_preamble(L, seed=L)
    ctx.sync_blas_threads()
    for n in _xc_sizes(L, mode):
        s = _planted(n, tmpl, 32)
        want = {sw: corr_want(*((tmpl, s) if sw else (s, tmpl)), mode) for sw in (False, True)}
        for in128, out128, with_c, with_peak, swapped in CORR_VARIANTS:
            a, v = (tmpl, s) if swapped else (s, tmpl)
            for si, so in SKEW2:
                run(_correlate_case(ctx, "vsig_correlate_dev", a, v, mode, in128, out128, with_c, with_peak, si, so,
                                    want[swapped]))


@covers("vsig_correlate_c64_dev")
@pytest.mark.parametrize("mode", ["valid", "full", "same"])
@pytest.mark.parametrize("L", [1, 64, 1000, 4097])
def test_correlate_c64(gpu, L, mode):
    ctx, tmpl = gpu.get_context(), ref.qpsk_preamble(L, seed=L)
    ctx.sync_blas_threads()
    sizes = _xc_sizes(L, "valid")
    for k, n in enumerate([sizes[0], sizes[1], sizes[2], sizes[-1]]):
        s = _planted(n, tmpl, 33)
        _, _, with_c, with_peak, swapped = CORR_VARIANTS[k % 3]
        a, v = (tmpl, s) if swapped else (s, tmpl)
        si, so = SKEW2[k % 4]
        run(_correlate_case(ctx, "vsig_correlate_c64_dev", a, v, mode, False, False, with_c, with_peak, si, so))


@covers("vsig_correlate_stats_dev")
@pytest.mark.parametrize("mode", ["valid", "full", "same"])
@pytest.mark.parametrize("L", XC_L)
def test_correlate_stats(gpu, L, mode):
    """Every output in numpy's operation order: np.mean / np.std of
    |np.correlate| in complex128 to the bit (tests/test_gpu_refine.py
    test_flat_valid_confidence_exact).  From L = 4096 (sums past one
    8192-element pairwise buffer at 8192 and 9000) the reference np.correlate
    is O(n L) on the host, so the stream is L, L + 1 and L + 300 and the
    precision and the operand order rotate instead of being crossed."""
    ctx = gpu.get_context()
    ctx.sync_blas_threads()
    k = 0
    long_ = L >= 4096
    rot = [(False, False), (True, True), (False, True), (True, False)]
    for i, n in enumerate((L, L + 1, L + (300 if long_ else 2500))):
        for in128 in (False, True):
            for swapped in (False, True):
                if long_ and (in128, swapped) != rot[(i + ["valid", "full", "same"].index(mode)) % 4]:
                    continue
                dt = np.complex128 if in128 else np.complex64
                s, t = iq(n, 34, dt), iq(L, 35, dt)
                a, v = (t, s) if swapped else (s, t)
                m = np.abs(np.correlate(a.astype(np.complex128), v.astype(np.complex128), mode))
                want = np.array([np.mean(m), np.std(m)])
                si, so = SKEW2[k % 4]
                k += 1

                def call(p):
                    return ctx.lib.vsig_correlate_stats_dev(ctx.h, CODE["c128" if in128 else "c64"], P(p["a"]), len(a),
                                                            P(p["v"]), len(v), _lib.MODES[mode], P(p["st"]))

                def check(o):
                    same_bits(o["st"], want, "mean / std")
                run(Case("vsig_correlate_stats_dev", f"na={len(a)} nv={len(v)} mode={mode} in128={in128} "
                         f"skew=({si},{so})", {"a": In(a, skew(dt, si)), "v": In(v, skew(dt, 1 - si))},
                         {"st": Out(2, np.float64, skew(np.float64, so))}, call, check))


@covers("vsig_xcorr_bank_exec_dev")
@pytest.mark.parametrize("mode", ["valid", "full"])
@pytest.mark.parametrize("L", [64, 1025])
@pytest.mark.parametrize("K", [1, 3])
def test_xcorr_bank(gpu, K, L, mode):
    """Each call builds the bank from template rows in an arena
    (vsig_xcorr_bank_create_dev), runs it and frees it."""
    ctx = gpu.get_context()
    tm = np.stack([ref.qpsk_preamble(L, seed=L + k) for k in range(K)])
    probe = P()
    ctx.check(ctx.lib.vsig_xcorr_bank_create(ctx.h, tm.ctypes.data_as(P), K, L, C.byref(probe)), "bank")
    M, hop, nb, grid = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
    assert ctx.lib.vsig_xcorr_bank_plan(probe, 4 * L, _lib.MODES[mode], C.byref(M), C.byref(hop), C.byref(nb),
                                        C.byref(grid)) == 0
    ctx.lib.vsig_xcorr_bank_free(probe)
    hop, off = hop.value, 0 if mode == "valid" else L - 1
    assert hop == M.value - L + 1
    nouts = {1, 2, hop - 1, hop, hop + 1, 3 * hop + 5}
    # block b reads M samples from b hop - off: the stream ends with it, one short of it, one past it
    nouts |= {M.value - off + b * hop + d + 2 * off - L + 1 for b in (0, 1) for d in (-1, 0, 1)}
    for k, nout in enumerate(sorted(nouts)):
        n = nout + L - 1 - 2 * off
        if n < (L if mode == "valid" else 1):
            continue
        s = _planted(n, tm[0], 36)
        want = np.stack([corr_want(s, t, mode) for t in tm])
        for with_c in (True, False):
            si, so = SKEW2[(k + with_c) % 4]
            outs = {"peaks": Out(4 * K, np.float64, skew(np.float64, so))}
            if with_c:
                outs["c"] = Out(K * want.shape[1], np.complex64, skew(np.complex64, so))

            def call(p):
                h = P()
                rc = ctx.lib.vsig_xcorr_bank_create_dev(ctx.h, P(p["tm"]), K, L, C.byref(h))
                if rc:
                    return rc
                rc = ctx.lib.vsig_xcorr_bank_exec_dev(h, P(p["s"]), n, _lib.MODES[mode], P(p["c"]) if with_c else None,
                                                      P(p["peaks"]))
                ctx.check(ctx.lib.vsig_synchronize(ctx.h), "sync")
                ctx.lib.vsig_xcorr_bank_free(h)
                return rc

            def check(o):   # tests/test_gpu_xcorr_bank.py test_values: 1e-5 for c, the peak and the sums
                if with_c:
                    normwise(o["c"].reshape(want.shape), want, 1e-5, "bank")
                for r in range(K):
                    a = np.abs(want[r])
                    rec = o["peaks"][4 * r:4 * r + 4]
                    assert int(rec.view(np.int64)[1]) == int(np.argmax(a)), r
                    assert abs(rec[0] / a.max() - 1) <= 1e-5 and abs(rec[2] / a.sum() - 1) <= 1e-5 \
                        and abs(rec[3] / (a * a).sum() - 1) <= 1e-5, (r, rec, a.max(), a.sum())
            run(Case("vsig_xcorr_bank_exec_dev", f"K={K} L={L} n={n} mode={mode} c={with_c} skew=({si},{so})",
                     {"tm": In(tm, skew(np.complex64, 1 - si)), "s": In(s, skew(np.complex64, si))}, outs, call,
                     check))


# =========================================================================== transforms of any length
XF_N = [1, 7, 256, 257, 513, 1000, 16384, 32768, 20_000]


@covers("vsig_dft_dev")
@pytest.mark.parametrize("n", XF_N)
def test_dft(gpu, n):
    ctx = gpu.get_context()
    for batch in (1, 3):
        for inverse in (0, 1):
            for code in ("c64", "c128"):
                x = iq(n * batch, 41, DT[code])
                f = np.fft.ifft if inverse else np.fft.fft
                want = f(x.reshape(batch, n).astype(np.complex128), axis=1).reshape(-1)

                for out in ("c64", "c128"):         # the 8-byte and the 16-byte store
                    def call(p):
                        return ctx.lib.vsig_dft_dev(ctx.h, CODE[code], P(p["x"]), n, batch, inverse, CODE[out],
                                                    P(p["y"]))

                    def check(o):   # tests/test_gpu_transforms.py TOL: 1e-5 normwise
                        normwise(o["y"], want, 1e-5, "dft")
                    for si, so in SKEW2:
                        run(Case("vsig_dft_dev", f"n={n} batch={batch} inverse={inverse} in={code} out={out} "
                                 f"skew=({si},{so})", {"x": In(x, skew(x.dtype, si))},
                                 {"y": Out(n * batch, DT[out], skew(DT[out], so))}, call, check))


@covers("vsig_resample_dev")
@pytest.mark.parametrize("n", XF_N)
def test_resample(gpu, n):
    ctx = gpu.get_context()
    for num in sorted({max(1, n - n // 4 - 1), n + n // 4 + 1}):
        for code in ("c64", "c128"):
            for real in (0, 1):
                x = iq(n, 42, DT[code])
                if real:
                    x = (x.real + 0j).astype(DT[code])
                want = scipy.signal.resample(x.real.astype(np.float64) if real else x.astype(np.complex128), num)

                def call(p):
                    return ctx.lib.vsig_resample_dev(ctx.h, CODE[code], P(p["x"]), n, num, real, P(p["y"]))

                def check(o):   # tests/test_gpu_transforms.py TOL: 1e-5 normwise
                    normwise(o["y"], want, 1e-5, "resample")
                    if real:
                        assert not o["y"].imag.any()
                for si, so in SKEW2:
                    run(Case("vsig_resample_dev", f"n={n} num={num} in={code} real={real} skew=({si},{so})",
                             {"x": In(x, skew(x.dtype, si))}, {"y": Out(num, np.complex64, skew(np.complex64, so))},
                             call, check))


@covers("vsig_filter_channel_dev")
@pytest.mark.parametrize("n", [n for n in XF_N if n == 1 or n % 2 == 0])
def test_filter_channel(gpu, n):
    """Odd n > 1 is refused by the contract (numpy's shape mismatch).  With
    sample_rate = sqrt(n) the reference's axis is CENTER_FREQ + k; the band
    keeps bins 1 .. n / 4, its edges a quarter bin away from any bin."""
    ctx = gpu.get_context()
    sr = math.sqrt(n)
    args = (ref.CENTER_FREQ + n / 8 + 0.25 * sr * sr / n, sr, n / 4 * sr * sr / n)
    for k, code in enumerate(("c64", "c128", "c64", "c128")):
        x = iq(n, 43, DT[code])
        want = ref.filter_channel(x.astype(np.complex128), *args)
        si, so = SKEW2[k % 4]

        def call(p):
            return ctx.lib.vsig_filter_channel_dev(ctx.h, CODE[code], P(p["x"]), n, *args, P(p["y"]))

        def check(o):   # tests/test_gpu_transforms.py TOL: 1e-5 normwise
            normwise(o["y"], want, 1e-5, "filter_channel")
        run(Case("vsig_filter_channel_dev", f"n={n} in={code} skew=({si},{so})", {"x": In(x, skew(x.dtype, si))},
                 {"y": Out(n, np.float64, skew(np.float64, so))}, call, check))


# =========================================================================== |a| kernels
ALL4 = ["c128", "c64", "f64", "f32"]


def _abs_sizes(lib):
    ns = {1, 2, 3, 5}
    for T in (lib.vsig_peaks_tile(), lib.vsig_runs_tile()):
        ns |= {T - 1, T, T + 1, 2 * T + 3}
    return sorted(ns)


def _mag(a):
    return np.abs(a).astype(np.float64)


def _abs_data(n, code, seed):
    """Noise with a burst, so that thresholds, peaks and runs have structure."""
    a = iq(n, seed, DT[code], scale=0.1)
    if n >= 8:
        a[n // 3:n // 3 + max(1, n // 7)] *= 9
    a[(2 * n) // 3] *= 30
    return a


def _each(gpu, code, skews=4):
    for k, n in enumerate(_abs_sizes(gpu.load_library())):
        for s in range(skews):
            yield n, s, (k + s) % 2


@covers("vsig_peak_dev")
@pytest.mark.parametrize("code", ALL4)
def test_peak(gpu, code):
    ctx = gpu.get_context()
    for n, s, so in _each(gpu, code):
        run(peak_case(ctx, code, n, s, so))


def peak_case(ctx, code, n, s, so, extra_in=0, short_out=0):
    a = _abs_data(n, code, 51)

    def call(p):
        return ctx.lib.vsig_peak_dev(ctx.h, CODE[code], P(p["a"]), n + extra_in, P(p["rec"]))

    def check(o):       # tests/test_gpu_special_values.py test_b6: numpy's argmax and maximum; the sums as _check_peak
        m = _mag(a)
        rec = o["rec"]
        assert int(rec.view(np.int64)[1]) == int(np.argmax(m)) and rec[0] == m.max(), (rec, m.max())
        assert abs(rec[2] / m.sum() - 1) <= 1e-5 and abs(rec[3] / (m * m).sum() - 1) <= 1e-5
    return Case("vsig_peak_dev", f"{code} n={n} skew=({s},{so})", {"a": In(a, skew(a.dtype, s))},
                {"rec": Out(4 - short_out, np.float64, skew(np.float64, so))}, call, check)


@covers("vsig_peaks_dev")
@pytest.mark.parametrize("code", ALL4)
def test_peaks(gpu, code):
    ctx = gpu.get_context()
    for n, s, so in _each(gpu, code):
        a = _abs_data(n, code, 52)
        m = _mag(a)
        thr_used = 0.5 * m.max()
        wi, wv = ref_peaks(m, thr_used, 7)
        cap = len(wi) + 3

        def call(p):
            return ctx.lib.vsig_peaks_dev(ctx.h, CODE[code], P(p["a"]), n, 0.5, 1, 7, P(p["out"]), cap, P(p["info"]))

        def check(o):   # tests/test_gpu_peaks.py check: exact; records past the count stay unwritten
            info = o["info"]
            assert info.view(np.int64)[:2].tolist() == [len(wi), int(np.argmax(m))]
            assert info[2] == m.max() and info[3] == thr_used
            rec = o["out"].reshape(cap, 2)
            assert np.array_equal(rec.view(np.int64)[:len(wi), 0], wi) and np.array_equal(rec[:len(wi), 1], wv)
            assert (rec[len(wi):].view(np.uint8) == ga.OUT_FILL).all()
        run(Case("vsig_peaks_dev", f"{code} n={n} skew=({s},{so})", {"a": In(a, skew(a.dtype, s))},
                 {"out": Out(2 * cap, np.float64, skew(np.float64, so)), "info": Out(4, np.float64, 8 * (1 - so))},
                 call, check))


@covers("vsig_runs_dev")
@pytest.mark.parametrize("code", ALL4)
def test_runs(gpu, code):
    ctx = gpu.get_context()
    for n, s, so in _each(gpu, code):
        a = _abs_data(n, code, 53)
        m = _mag(a)
        thr_used = 0.25 * m.max()
        gap = (0, 3)[s % 2]
        ws, we = runs_ref(m, thr_used, gap)
        wa, wm, wsum = run_stats(m, ws, we)
        cap = len(ws) + 3

        def call(p):
            return ctx.lib.vsig_runs_dev(ctx.h, CODE[code], P(p["a"]), n, 0.25, 1, gap, P(p["out"]), cap, P(p["info"]))

        def check(o):   # tests/test_gpu_runs.py check: exact, a run's sum within 2 len 2^-53 sum
            info = o["info"]
            assert info.view(np.int64)[:3].tolist() == [len(ws), int(np.count_nonzero(m >= thr_used)),
                                                        int(np.argmax(m))]
            assert info[3] == m.max() and info[4] == thr_used
            rec = o["out"].reshape(cap, 5)
            k = len(ws)
            ri = rec.view(np.int64)
            assert np.array_equal(ri[:k, 0], ws) and np.array_equal(ri[:k, 1], we) and np.array_equal(ri[:k, 2], wa)
            assert np.array_equal(rec[:k, 3], wm)
            assert (np.abs(rec[:k, 4] - wsum) <= 2 * (we - ws + 1) * 2.0 ** -53 * wsum).all()
            assert (rec[k:].view(np.uint8) == ga.OUT_FILL).all()
        run(Case("vsig_runs_dev", f"{code} n={n} gap={gap} skew=({s},{so})", {"a": In(a, skew(a.dtype, s))},
                 {"out": Out(5 * cap, np.float64, skew(np.float64, so)), "info": Out(5, np.float64, 8 * (1 - so))},
                 call, check))


@covers("vsig_trace_envelope_dev")
@pytest.mark.parametrize("code", ALL4)
def test_trace_envelope(gpu, code):
    """shift x bin x (whole array / a sub-range with holes outside it) at every
    size, input skew 0 .. 3 and output skew 0 / 1; the four (env_min, info)
    present / NULL pairs and the two kinds rotate through that product."""
    ctx = gpu.get_context()
    nulls = [(True, True), (False, True), (True, False), (False, False)]
    c = 0
    for n, s, _ in _each(gpu, code):
        for so in (0, 1):
            for shift in (0, 1):
                for bin_ in (1, 7):
                    for sub in (False, True):
                        c += 1
                        if sub and n < 5:
                            continue
                        with_min, with_info = nulls[(c + c // 8) % 4]
                        _trace_run(ctx, code, n, s, so, shift, bin_, sub, with_min, with_info, (c // 4 + c // 16) % 2)


def _trace_run(ctx, code, n, s, so, shift, bin_, sub, with_min, with_info, db):
    odt = np.float32 if code in ("c64", "f32") else np.float64
    a = _abs_data(n, code, 54)
    lo, hi = (n // 5 + 1, n - n // 7 - 1) if sub else (0, n)
    kind, eps = ((_lib.TRACE_ABS, 0.0), (_lib.TRACE_DB20, 1e-12))[db]
    rot = (n + 1) // 2 if shift else 0
    used = np.zeros(n, bool)
    used[(np.arange(lo, hi) + rot) % n] = True
    cols = -(-(hi - lo) // bin_)
    wmin, wmax, winfo = tr.restate(a, bool(shift), lo, hi, bin_, kind, eps)
    outs = {"max": Out(cols, odt, skew(odt, so))}
    if with_min:
        outs["min"] = Out(cols, odt, skew(odt, 1 - so))
    if with_info:
        outs["info"] = Out(4, np.float64, skew(np.float64, so))

    def call(p):
        return ctx.lib.vsig_trace_envelope_dev(ctx.h, CODE[code], P(p["a"]), n, shift, lo, hi, bin_, kind, eps,
                                               P(p["min"]) if with_min else None, P(p["max"]),
                                               P(p["info"]) if with_info else None)

    def check(o):   # tests/test_gpu_traces.py: VSIG_TRACE_ABS exact, VSIG_TRACE_DB20 within 8 ulps
        for name, want in (("max", wmax), ("min", wmin)):
            if name in o:
                if kind == _lib.TRACE_ABS:
                    same_bits(o[name], want.astype(odt), name)
                else:
                    assert tr.ulps(o[name], want).max() <= 8, name
        if with_info:
            assert o["info"].view(np.int64)[:2].tolist() == list(winfo[:2]), (o["info"], winfo)
            if kind == _lib.TRACE_ABS:
                assert o["info"][2:].tolist() == list(winfo[2:])
            else:
                assert tr.ulps(o["info"][2:].astype(odt), np.array(winfo[2:], odt)).max() <= 8
    run(Case("vsig_trace_envelope_dev", f"{code} n={n} shift={shift} [{lo},{hi}) bin={bin_} kind={kind} "
             f"min={with_min} info={with_info} skew=({s},{so})",
             {"a": In(a, skew(a.dtype, s), holes=~used)}, outs, call, check))


@covers("vsig_abs_stats_dev")
@pytest.mark.parametrize("code", ["c128", "f64"])
def test_abs_stats(gpu, code):
    ctx = gpu.get_context()
    for n, s, so in _each(gpu, code):
        a = _abs_data(n, code, 55)

        def call(p):
            return ctx.lib.vsig_abs_stats_dev(ctx.h, CODE[code], P(p["a"]), n, P(p["st"]))

        def check(o):   # tests/test_gpu_refine.py test_abs_stats_numpy_order: numpy's to the bit
            same_bits(o["st"], np.array([np.mean(np.abs(a)), np.std(np.abs(a))]), "mean / std")
        run(Case("vsig_abs_stats_dev", f"{code} n={n} skew=({s},{so})", {"a": In(a, skew(a.dtype, s))},
                 {"st": Out(2, np.float64, skew(np.float64, so))}, call, check))


@covers("vsig_select_dev")
@pytest.mark.parametrize("code", ["f64", "f32"])
def test_select(gpu, code):
    ctx = gpu.get_context()
    for n, s, _ in _each(gpu, code):
        a = _abs_data(n, code, 56)
        rk = sorted({0, n // 2, (n - 1) // 3, n - 1})

        def call(p):
            ranks, vals = (C.c_int64 * len(rk))(*rk), (C.c_double * len(rk))()
            rc = ctx.lib.vsig_select_dev(ctx.h, CODE[code], P(p["a"]), n, ranks, len(rk), vals)
            return rc, {"values": np.array(list(vals), np.float64)}

        def check(o):   # tests/test_gpu_analysis.py test_order_statistics_exact
            same_bits(o["values"], np.sort(np.abs(a))[rk].astype(np.float64), "select")
        run(Case("vsig_select_dev", f"{code} n={n} skew={s}", {"a": In(a, skew(a.dtype, s))}, {}, call, check))


@covers("vsig_threshold_dev")
@pytest.mark.parametrize("code", ["f64", "f32"])
def test_threshold(gpu, code):
    ctx = gpu.get_context()
    for n, s, _ in _each(gpu, code):
        a = _abs_data(n, code, 57)
        thr = float(np.median(np.abs(a)))

        def call(p):
            cnt, first, last, mx = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
            rc = ctx.lib.vsig_threshold_dev(ctx.h, CODE[code], P(p["a"]), n, thr, C.byref(cnt), C.byref(first),
                                            C.byref(last), C.byref(mx))
            return rc, {"stats": np.array([cnt.value, first.value, last.value, mx.value], np.float64)}

        def check(o):   # tests/test_gpu_analysis.py test_threshold_stats_exact
            want = sv.np_threshold_stats(a, thr)
            assert tuple(o["stats"][:3].astype(np.int64)) == tuple(want[:3]) and o["stats"][3] == float(want[3]), \
                (o["stats"], want)
        run(Case("vsig_threshold_dev", f"{code} n={n} skew={s}", {"a": In(a, skew(a.dtype, s))}, {}, call, check))


@covers("vsig_boxcar_energy_dev")
@pytest.mark.parametrize("code", ALL4)
def test_boxcar_energy(gpu, code):
    ctx = gpu.get_context()
    for n, s, so in _each(gpu, code):
        a = _abs_data(n, code, 58)
        for w in (3, n + 7):
            want = np.convolve(np.abs(a) ** 2, np.ones(w) / w, mode="same")     # |x|^2 in x's precision, as numpy
            assert len(want) == max(n, w)

            def call(p):
                return ctx.lib.vsig_boxcar_energy_dev(ctx.h, CODE[code], P(p["x"]), n, w, P(p["sm"]))

            def check(o):   # tests/test_gpu_analysis.py test_boxcar_energy_matches_numpy: 1e-12 of the maximum
                assert np.abs(o["sm"] - want).max() <= 1e-12 * max(want.max(), 1e-300)
            run(Case("vsig_boxcar_energy_dev", f"{code} n={n} w={w} skew=({s},{so})", {"x": In(a, skew(a.dtype, s))},
                     {"sm": Out(max(n, w), np.float64, skew(np.float64, so))}, call, check))


@covers("vsig_db_dev")
@pytest.mark.parametrize("code", ["f64", "f32"])
def test_db(gpu, code):
    ctx = gpu.get_context()
    for n, s, so in _each(gpu, code):
        a = _abs_data(n, code, 59)
        dt = DT[code]
        want = 10 * np.log10(np.abs(a) + dt(1e-12))

        def call(p):
            return ctx.lib.vsig_db_dev(ctx.h, CODE[code], P(p["a"]), n, 1e-12, P(p["out"]))

        def check(o):   # tests/test_gpu_special_values.py test_a2_db_map_classes_and_ulps: 8 ulps
            assert np.all(np.abs(o["out"] - want) <= 8 * np.spacing(np.abs(want)) + 1e-30)
        run(Case("vsig_db_dev", f"{code} n={n} skew=({s},{so})", {"a": In(a, skew(a.dtype, s))},
                 {"out": Out(n, dt, skew(dt, so))}, call, check))


@covers("vsig_abs_c64_dev", "vsig_abs_c128_dev")
@pytest.mark.parametrize("entry,code", [("c64", "c64"), ("c64", "f32")] + [("c128", c) for c in ALL4])
def test_abs(gpu, entry, code):
    """vsig_abs_c64_dev takes the 32-bit types (np.abs as float32), vsig_abs_c128_dev all four."""
    ctx = gpu.get_context()
    odt = np.complex64 if entry == "c64" else np.complex128
    fn = ctx.lib.vsig_abs_c64_dev if entry == "c64" else ctx.lib.vsig_abs_c128_dev
    for n, s, so in _each(gpu, code):
        a = _abs_data(n, code, 60)

        def call(p):
            return fn(ctx.h, CODE[code], P(p["a"]), n, P(p["out"]))

        def check(o):   # tests/test_gpu_special_values.py test_a1_abs_is_numpy_to_the_bit
            same_bits(o["out"], (np.abs(a) + 0j).astype(odt), "abs")
        run(Case(f"vsig_abs_{entry}_dev", f"{code} n={n} skew=({s},{so})", {"a": In(a, skew(a.dtype, s))},
                 {"out": Out(n, odt, skew(odt, so))}, call, check))


@covers("vsig_region_power_dev")
def test_region_power(gpu):
    """Operands on 8-byte boundaries: skews of 0 .. 3 complex64 elements each."""
    ctx = gpu.get_context()
    for n, s, so in _each(gpu, "c64"):
        a, b = iq(n, 61), iq(n, 62)

        def call(p):
            return ctx.lib.vsig_region_power_dev(ctx.h, P(p["a"]), P(p["b"]), n, P(p["sums"]))

        def check(o):   # tests/test_gpu_transplant.py RTOL 1e-10 against math.fsum of numpy's float32 |.|^2
            want = [math.fsum((np.abs(v) ** 2).astype(np.float64).tolist()) for v in (a, b, a - b)]
            for g, w in zip(o["sums"], want):
                assert abs(g - w) <= 1e-10 * w, (g, w)
        run(Case("vsig_region_power_dev", f"n={n} skew=({s},{3 - s},{so})",
                 {"a": In(a, 8 * s), "b": In(b, 8 * (3 - s))}, {"sums": Out(3, np.float64, 8 * so)}, call, check))


# =========================================================================== display
IMG_OPTS = [(m, f, pf, pt) for m in (0, 1) for f in (0, 1) for pf in (1, 3) for pt in (1, 3)]


@covers("vsig_spectrogram_image_dev")
@pytest.mark.parametrize("extent", [(1, 1), (5, 7), (130, 517)])
@pytest.mark.parametrize("freq_fast", [0, 1])
@pytest.mark.parametrize("code", ["f32", "f64"])
def test_spectrogram_image(gpu, code, freq_fast, extent):
    FLOOR, VMIN, VMAX = dr.FLOOR, dr.VMIN, dr.VMAX
    ctx, dt = gpu.get_context(), DT[code]
    nf, nt = extent
    S = dr.centred(nf, nt, dt)
    lut = gpu.colormap_table("turbo").copy()
    fast, slow = (nf, nt) if freq_fast else (nt, nf)
    k = 0
    for pad in (0, 3):
        ld = fast + pad
        mem = np.zeros((slow, ld), dt)
        mem[:, :fast] = S.T if freq_fast else S
        hole = np.zeros((slow, ld), bool)
        hole[:, fast:] = True
        span = (slow - 1) * ld + fast               # the last row's pad lies past the operand
        for median, flip, pf, pt in IMG_OPTS:
            k += 1
            rows, cols = -(-nf // pf), -(-nt // pt)
            want = dr.restate(S, FLOOR, VMIN, VMAX, lut, bool(median), bool(flip), (pf, pt))

            def call(p):
                return ctx.lib.vsig_spectrogram_image_dev(ctx.h, CODE[code], P(p["sxx"]), nf, nt, freq_fast, ld, FLOOR,
                                                          VMIN, VMAX, median, flip, pf, pt, P(p["lut"]), P(p["rgba"]))

            def check(o):   # tests/test_gpu_display.py check_exact: byte for byte on centred values
                assert np.array_equal(o["rgba"].reshape(rows, cols, 4), want)
            for j, (si, so) in enumerate(SKEW2):
                run(Case("vsig_spectrogram_image_dev", f"{code} {nf}x{nt} freq_fast={freq_fast} ld={ld} "
                         f"median={median} flip={flip} pool=({pf},{pt}) skew=({si},{so})",
                         {"sxx": In(mem.reshape(-1)[:span], skew(dt, si), holes=hole.reshape(-1)[:span]),
                          "lut": In(lut, 4 * ((k + j) % 2))},
                         {"rgba": Out(rows * cols * 4, np.uint8, 4 * so)}, call, check))


# =========================================================================== channelizer
@covers("vsig_pfb_c64_dev")
@pytest.mark.parametrize("pt", [4, 8, 16])
@pytest.mark.parametrize("nchan", [64, 128, 256])
def test_pfb(gpu, nchan, pt):
    """Group g of vsig_pfb_plan's frames_per_group frames reads up to sample
    ((g + 1) fpg + pt - 1) nchan: the stream ends there, one sample short and
    one past, for the first two groups (the per-group `inside` choice) and for
    the first whole block of groups_per_block groups (`inside_blk`; 17 344
    samples at nchan 64, pt 16, tests/test_gpu_analysis.py)."""
    from scipy.signal import firwin
    ctx = gpu.get_context()
    ntaps = pt * nchan
    h = firwin(ntaps, 1.0 / nchan).astype(np.float32)
    fpg, gpb, nb = C.c_int64(), C.c_int64(), C.c_int64()
    assert ctx.lib.vsig_pfb_plan(nchan, ntaps, 1, C.byref(fpg), C.byref(gpb), C.byref(nb)) == 0
    fpg, gpb = fpg.value, gpb.value
    assert fpg >= 1 and gpb == 256 // nchan and nb.value == 1
    ends = [((g + 1) * fpg + pt - 1) * nchan for g in sorted({0, 1, gpb - 1})]
    sizes = {ntaps, ntaps + 1, 17_343, 17_344} | {e + d for e in ends for d in (-1, 0, 1)}
    for k, n in enumerate(sorted(sizes)):
        x = iq(n, 71)
        M = (n - ntaps) // nchan + 1
        used = np.zeros(n, bool)
        used[:(M - 1) * nchan + ntaps] = True
        # oracle.ref.pfb_channelize's definition, kept in complex128
        want = np.fft.fft((np.lib.stride_tricks.sliding_window_view(x.astype(np.complex128), ntaps)[::nchan][:M]
                           * h.astype(np.float64)[None, :]).reshape(M, pt, nchan).sum(axis=1), axis=1)

        def call(p):
            return ctx.lib.vsig_pfb_c64_dev(ctx.h, P(p["x"]), n, P(p["h"]), ntaps, nchan, P(p["y"]), M)

        def check(o):   # tests/test_gpu_analysis.py test_pfb_matches_definition: 1e-5 of max |Y|
            normwise(o["y"].reshape(M, nchan), want, 1e-5, "pfb")
        for j, (si, so) in enumerate(SKEW2):
            run(Case("vsig_pfb_c64_dev", f"nchan={nchan} pt={pt} n={n} skew=({si},{so})",
                     {"x": In(x, skew(x.dtype, si), holes=~used), "h": In(h, 4 * ((k + j) % 2))},
                     {"y": Out(M * nchan, np.complex64, skew(np.complex64, so))}, call, check))


# =========================================================================== detector self-tests
def _self_cases(ctx, extra_in, short_out):
    """One entry point per family, told one element more than the harness is
    (the element lies inside the arena: nothing is out of bounds)."""
    yield scale_case(ctx, 257, extra_in=extra_in, short_out=short_out)
    taps = _taps(64)
    f = _fir_handle(ctx, taps, 1)
    yield _fir_case(f, ctx, "vsig_fir_exec_dev", taps, 1, 1000, 0, 0, 0, extra_in=extra_in, short_out=short_out)
    ctx.lib.vsig_fir_free(f)
    # a tail of 63 samples (data, not holes): one more sample completes a fourth frame
    x, holes, win, n, scale, S = _psd_setup(64, 64, 64, 1, 3, 63 if extra_in else 0, 0, 1)
    yield psd_case(ctx, x, holes if not extra_in else None, win, n, 1, 64, 64, 64, scale, 0, 3, S, 0, 0, 0,
                   extra_in=extra_in, short_out=short_out)
    tmpl = ref.qpsk_preamble(64, seed=64)
    h = _xcorr_handle(ctx, tmpl)
    yield xcorr_case(ctx, h, tmpl, 500, "valid", True, 0, 0, extra_in=extra_in, short_out=short_out)
    ctx.lib.vsig_xcorr_free(h)
    yield peak_case(ctx, "c64", 300, 0, 0, extra_in=extra_in, short_out=short_out)


@gpu_test
@pytest.mark.parametrize("j", range(5))
def test_detector_sees_a_read_past_the_operand(gpu, j):
    ctx = gpu.get_context()
    for k, case in enumerate(_self_cases(ctx, 1, 0)):
        if k == j:
            with pytest.raises(GuardViolation) as e:
                run(case)
            assert e.value.bound == "read", str(e.value)


@gpu_test
@pytest.mark.parametrize("j", range(5))
def test_detector_sees_a_write_past_the_output(gpu, j):
    ctx = gpu.get_context()
    for k, case in enumerate(_self_cases(ctx, 0, 1)):
        if k == j:
            with pytest.raises(GuardViolation) as e:
                run(case)
            assert (e.value.bound, e.value.offset) == ("write", case.outs[e.value.operand].nbytes), str(e.value)
