"""The numpy-exact kernels at non-finite and extreme inputs.

A (elementwise) and B (reductions, selections, detectors): every expectation
is numpy's own value, computed on the host at test time, or the CPU oracle's;
comparisons are bitwise (NaN equal to NaN) unless a tolerance of the existing
suite is named.  C (frame-based FFT kernels): containment, not parity -- an
FFT spreads a NaN over its frame, so frames that hold the poisoned sample have
no finite value and all others are bit-identical to the clean run.

test_special_values_cpu.py proves the poisoned inputs change numpy's answers.
Each test gathers every mismatch (GPU value, numpy value) before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import special_values as sv
import test_gpu_peaks as tp
from oracle import ref
from test_gpu_formats import _wv_parts
from test_transplant_cpu import ref_validate
from vector_amd import _lib
from vector_amd.vectors import _MI_NP

pytestmark = pytest.mark.gpu

CODE = {np.dtype(np.complex128): "c128", np.dtype(np.complex64): "c64",
        np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}
NAN, INF = float("nan"), float("inf")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _report(bad):
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(str(b) for b in bad[:40])


# =========================================================================== A1
def _abs_dev(va, a, wide):
    ctx = va.get_context()
    t = _dev(a)
    out = torch.full((len(a),), 7 + 7j, dtype=torch.complex128 if wide else torch.complex64, device="cuda")
    fn = ctx.lib.vsig_abs_c128_dev if wide else ctx.lib.vsig_abs_c64_dev
    ctx.check(fn(ctx.h, _lib.DTYPES[CODE[a.dtype]], _ptr(t), len(a), _ptr(out)), "abs")
    return out.cpu().numpy()


@pytest.mark.parametrize("entry,dt", [("c64", np.complex64), ("c64", np.float32),
                                      ("c128", np.complex64), ("c128", np.float32),
                                      ("c128", np.complex128), ("c128", np.float64)])
def test_a1_abs_is_numpy_to_the_bit(gpu, entry, dt):
    """vsig_abs_c64_dev writes np.abs(a) as float32, vsig_abs_c128_dev as
    float64 (np.abs in a's precision, widened exactly), imaginary part +0."""
    rt = sv.real_of(dt)
    z = np.concatenate([sv.grid(rt), sv.wide(65_536 + 3, rt, 3)])
    assert len(z) % 256 and len(z) % 4096
    a = z if np.dtype(dt).kind == "c" else np.concatenate([z.real, z.imag])
    with np.errstate(all="ignore"):
        want = np.abs(a).astype(np.float32 if entry == "c64" else np.float64)
    got = _abs_dev(gpu, a, entry == "c128")
    ok = sv.same_bits(got.real, want)
    bad = [("|a|", i, a[i], "gpu", got.real[i], "numpy", want[i]) for i in np.flatnonzero(~ok)[:40]]
    assert not sv.bits(got.imag).any(), "imaginary part must be +0.0"
    assert not bad, f"{np.count_nonzero(~ok)} of {len(a)} differ:\n" + "\n".join(map(str, bad))


# =========================================================================== A2
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("floor", [1e-12, 1.0])
def test_a2_db_map_classes_and_ulps(gpu, dt, floor):
    a = sv.specials(dt)
    ctx = gpu.get_context()
    t = _dev(a)
    out = torch.empty(len(a), dtype=t.dtype, device="cuda")
    ctx.check(ctx.lib.vsig_db_dev(ctx.h, _lib.DTYPES[CODE[a.dtype]], _ptr(t), len(a), float(floor), _ptr(out)), "db")
    got = out.cpu().numpy()
    with np.errstate(all="ignore"):
        want = 10 * np.log10(np.abs(a) + dt(floor))
    assert want.dtype == got.dtype
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(want)), (f.__name__, a, got, want)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 8 * np.spacing(np.abs(want[fin])) + 1e-30), (got, want)


# =========================================================================== A3
def _quantize_inputs():
    f = np.float32
    one = f(1)
    vals = np.array([0.5, -0.25, 1, np.nextafter(one, f(2)), np.nextafter(one, f(0)), -1,
                     np.nextafter(-one, f(-2)), np.nextafter(-one, f(0)), 0.99999, -0.99999,
                     1.5, -1.7, 3.0, -2.5,                     # beyond int16: wraps
                     70000.0, -70000.0, 1e10, -3e38,            # beyond int32
                     INF, -INF, NAN, -0.0, 1e-45, 1e-40], dtype=f)
    k = len(vals)
    x = np.zeros(3 * k, np.complex64)
    x.real[:k], x.imag[:k] = vals, 0.25
    x.real[k:2 * k], x.imag[k:2 * k] = -0.125, vals
    x.real[2 * k:], x.imag[2 * k:] = vals, vals[::-1]
    x = np.tile(x, 5)
    assert len(x) % 256
    return x


@pytest.mark.parametrize("norm", [0.0, 1.7, 0.3, INF, NAN])
def test_a3_wv_quantize_is_numpys_cast(gpu, norm):
    """(x * 32767).astype(int16), after signal / norm when norm != 0, formed as
    ref.mat2wv_fields forms it: numpy has no complex-by-real loop, so each part
    also takes the other part times zero (NaN when that part is not finite)."""
    x = _quantize_inputs()
    with np.errstate(all="ignore"):
        want = ref.mat2wv_fields(x / np.float32(norm) if norm != 0 else x, False)[0]
    ctx = gpu.get_context()
    t = _dev(x)
    q = torch.full((2 * len(x),), 12345, dtype=torch.int16, device="cuda")
    ctx.check(ctx.lib.vsig_wv_quantize_dev(ctx.h, _ptr(t), len(x), float(norm), _ptr(q)), "wv")
    got = q.cpu().numpy()
    bad = [("norm", norm, "x", x[i // 2], "part", i % 2, "gpu", got[i], "numpy", want[i])
           for i in np.flatnonzero(got != want)[:40]]
    _report(bad)


@pytest.mark.parametrize("normalize", [False, True])
def test_a3_save_vector_wv_with_non_finite_samples(gpu, tmp_path, normalize):
    base = sv.base_signal(np.complex64)
    cases = {"nan": [(4096, NAN)], "inf": [(17, INF)], "1e20": [(8000, 1e20)],
             "all_three": [(4096, NAN), (17, INF), (8000, 1e20)]}
    bad = []
    for name, spots in cases.items():
        x = base.copy()
        for at, v in spots:
            x[at] = v
        with np.errstate(all="ignore"):
            want, rms, peak = ref.mat2wv_fields(x, normalize)
        out = tmp_path / f"{name}.wv"
        with np.errstate(all="ignore"):
            gpu.save_vector_wv(x, str(out), 56e6, normalize=normalize)
        hdr, payload, _ = _wv_parts(out)
        if not np.array_equal(payload, want):
            i = np.flatnonzero(payload != want)
            bad.append((name, "payload", len(i), "first", int(i[0]), "gpu", payload[i[0]], "numpy", want[i[0]]))
        lvl = [float(s) for s in hdr[hdr.index("{LEVEL OFFS: ") + 13:].split("}")[0].split(", ")]
        for what, g, w in (("rms", lvl[0], float(rms)), ("peak", lvl[1], float(peak))):
            same = (np.isnan(g) and np.isnan(w)) or g == w or abs(g - w) <= 1e-5
            if not same:
                bad.append((name, what, "gpu", g, "numpy", w))
    _report(bad)


# =========================================================================== A4
def _plane(np_t, seed):
    """257 storage values of one MAT type: extremes, float32 ties, single
    rounding, then seeded values over the whole range."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(np_t)
    if dt.kind in "iu":
        ii = np.iinfo(dt)
        want = [ii.min, ii.max, 0, 1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 24 + 2, 2 ** 25 + 2, 2 ** 25 + 6,
                2 ** 53 + 1, 2 ** 53 + 3, 2 ** 63 - 1, 2 ** 63 + 2 ** 39, 2 ** 64 - 2 ** 39 - 1,
                -1, -(2 ** 24) - 1, -(2 ** 24) - 3, -(2 ** 53) - 1]
        head = [v for v in want if ii.min <= v <= ii.max]
        body = rng.integers(ii.min, ii.max, 257 - len(head), dtype=dt, endpoint=True)
        return np.concatenate([np.array(head, dtype=dt), body])
    s = sv.specials(dt)
    if dt == np.float64:
        fmax = float(np.finfo(np.float32).max)
        extra = [1e39, -1e39, fmax * (1 + 2.0 ** -25), fmax * (1 + 2.0 ** -26), 1e-40, -1e-44,
                 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -52), 2.0 ** -151, 3 * 2.0 ** -150,
                 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -52, -(1 + 2.0 ** -24)]
        s = np.concatenate([s, np.array(extra)])
    body = sv.wide(257 - len(s), dt, seed).real
    return np.concatenate([s, body]).astype(dt)


@pytest.mark.parametrize("mi", sorted(_MI_NP))
def test_a4_planar_to_c64_every_storage_type(gpu, mi):
    np_t = _MI_NP[mi]
    re, im = _plane(np_t, mi), _plane(np_t, 100 + mi)[::-1].copy()
    assert len(re) == 257
    ctx = gpu.get_context()
    bad = []
    for planes in ((re, None), (re, im)):
        y = torch.full((257,), 9 + 9j, dtype=torch.complex64, device="cuda")
        dr = _dev(planes[0].view(np.uint8))
        di = _dev(planes[1].view(np.uint8)) if planes[1] is not None else None
        ctx.check(ctx.lib.vsig_planar_to_c64_dev(ctx.h, mi, _ptr(dr), _ptr(di) if di is not None else None,
                                                 257, _ptr(y)), "planar")
        got = y.cpu().numpy()
        with np.errstate(all="ignore"):
            wr = planes[0].astype(np.float32)
            wi = planes[1].astype(np.float32) if planes[1] is not None else np.zeros(257, np.float32)
        for what, g, w, src in (("re", got.real, wr, planes[0]), ("im", got.imag, wi, planes[1])):
            ok = sv.same_bits(np.ascontiguousarray(g), w)
            bad += [(np_t.__name__, what, "in", src[i] if src is not None else None, "gpu", g[i], "numpy", w[i])
                    for i in np.flatnonzero(~ok)[:10]]
    _report(bad)


@pytest.mark.parametrize("mi", [m for m in sorted(_MI_NP) if np.dtype(_MI_NP[m]).kind in "iu"])
def test_a4_load_packet_integer_files(gpu, tmp_path, mi):
    from scipy.io import loadmat, savemat
    data = _plane(_MI_NP[mi], mi)
    path = str(tmp_path / f"t{mi}.mat")
    savemat(path, {"Y": data})
    want = loadmat(path)["Y"].flatten().astype(np.complex64)
    got = gpu.load_packet(path)
    ok = sv.same_bits(got, want)
    assert ok.all(), (np.dtype(_MI_NP[mi]).name, np.count_nonzero(~ok))


# =========================================================================== B1
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4099])
def test_b1_order_statistics_sort_nan_last(gpu, dt, n):
    rng = np.random.default_rng(n)
    base = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3, n)).astype(dt)
    tiny = np.finfo(dt).smallest_subnormal
    variants = {"one_nan": sv.poison(base, n // 2, NAN), "inf": sv.poison(base, n - 1, INF),
                "neg_nan": sv.poison(base, 0, -NAN), "all_nan": np.full(n, NAN, dt)}
    if n >= 4:
        variants["two_nan"] = sv.poison(base, [1, n - 1], NAN)
        variants["mixed"] = sv.poison(base, [0, 1, 2, 3], [-0.0, tiny, -INF, NAN])
    ranks = sorted({0, n - 1, n // 2, max(0, n - 2), (n - 1) // 3})
    bad = []
    for name, a in variants.items():
        want = np.sort(np.abs(a))[ranks].astype(np.float64)
        got = np.array(gpu.order_statistics(a, ranks), np.float64)
        ok = sv.same_bits(got, want)
        bad += [(name, "rank", ranks[i], "gpu", got[i], "numpy", want[i]) for i in np.flatnonzero(~ok)]
    _report(bad)


# =========================================================================== B2
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_b2_threshold_stats(gpu, dt):
    base = sv.base_signal(dt)
    tiny = float(np.finfo(dt).smallest_subnormal)
    bad = []
    for name, at, v in [("clean", [], 0.0)] + sv.poison_cases(len(base)):
        a = sv.poison(base, at, v)
        for thr in (0.0, tiny, 1.0, INF, NAN):
            want = sv.np_threshold_stats(a, thr)
            got = gpu.threshold_stats(a, thr)
            if tuple(got[:3]) != want[:3] or not sv.same_scalar(got[3], want[3]):
                bad.append((name, "thr", thr, "gpu", got, "numpy", want))
    _report(bad)


# =========================================================================== B3
@pytest.mark.parametrize("dt", sv.DTYPES)
def test_b3_boxcar_energy_classes(gpu, dt):
    base = sv.base_signal(dt)
    n = len(base)
    bad = []
    for name, at, v in sv.poison_cases(n, energy=True, cplx=np.dtype(dt).kind == "c"):
        x = sv.poison(base, at, v)
        for w in (1, 3, 56, n + 7):
            want = sv.np_boxcar(x, w)
            got = gpu.boxcar_energy(x, w).cpu().numpy()
            assert got.shape == want.shape and got.dtype == want.dtype
            for f in (np.isnan, np.isposinf, np.isneginf):
                if not np.array_equal(f(got), f(want)):
                    i = np.flatnonzero(f(got) != f(want))
                    bad.append((name, "w", w, f.__name__, len(i), "first", int(i[0]), "gpu", got[i[0]],
                                "numpy", want[i[0]]))
            fin = np.isfinite(want) & np.isfinite(got)
            if fin.any():
                err = np.abs(got[fin] - want[fin]).max()
                if err > 1e-12 * max(np.abs(want[fin]).max(), 1e-300):
                    bad.append((name, "w", w, "finite error", err, "of", np.abs(want[fin]).max()))
    _report(bad)


# =========================================================================== B4
@pytest.mark.parametrize("dt", sv.DTYPES)
def test_b4_packet_detectors_equal_the_oracle(gpu, dt):
    base = sv.base_signal(dt)
    bad = []
    for name, at, v in sv.poison_cases(len(base), energy=True, cplx=np.dtype(dt).kind == "c"):
        x = sv.poison(base, at, v)
        with np.errstate(all="ignore"):
            for ws in (None, 1, 150):
                want = ref.find_packet_start(x, window_size=ws)
                got = gpu.find_packet_start(x, window_size=ws)
                if got != want:
                    bad.append((name, "find_packet_start", ws, "gpu", got, "oracle", want))
            want = tuple(int(t) for t in ref.detect_packet_bounds(x, 56e6))
            got = tuple(int(t) for t in gpu.detect_packet_bounds(x, 56e6))
            if got != want:
                bad.append((name, "detect_packet_bounds", "gpu", got, "oracle", want))
    _report(bad)


# =========================================================================== B5
@pytest.mark.parametrize("dt,shape", [(np.float32, (64, 33)), (np.float64, (32, 17))])
def test_b5_spectrogram_levels_and_db_map(gpu, dt, shape):
    S = np.random.default_rng(5).exponential(size=shape).astype(dt)
    bad = []
    for name, at, v in (("one_nan", (3, 7), NAN), ("one_inf", (3, 7), INF), ("all_nan", slice(None), NAN)):
        P = sv.poison(S, at, v)
        with np.errstate(all="ignore"):
            rdb, rvmin, rvmax = ref.normalize_spectrogram(P)
            db, vmin, vmax = gpu.normalize_spectrogram(P)
            _, lmin, lmax = gpu.spectrogram_levels(P)
        for what, g, w in (("vmin", vmin, rvmin), ("vmax", vmax, rvmax), ("levels vmin", lmin, rvmin),
                           ("levels vmax", lmax, rvmax)):
            if type(g) is not type(w) or not sv.same_scalar(g, w):
                bad.append((name, what, "gpu", repr(g), type(g).__name__, "oracle", repr(w), type(w).__name__))
        assert db.dtype == rdb.dtype and db.shape == rdb.shape
        for f in (np.isnan, np.isposinf, np.isneginf):
            if not np.array_equal(f(db), f(rdb)):
                bad.append((name, "dB map", f.__name__, int(f(db).sum()), "oracle", int(f(rdb).sum())))
        fin = np.isfinite(rdb) & np.isfinite(db)
        if not np.all(np.abs(db[fin] - rdb[fin]) <= 8 * np.spacing(np.abs(rdb[fin])) + 1e-30):
            bad.append((name, "dB map beyond 8 ulp"))
    _report(bad)


# =========================================================================== B6
def _peak_cases(dt, n):
    rng = np.random.default_rng(n)
    c = rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(dt).kind == "c" else 0)
    c = c.astype(dt)
    if n > 3:
        c[n // 3] = 100                                     # a larger finite value earlier
    cases = {"nan_mid": sv.poison(c, n // 2, NAN), "nan_last": sv.poison(c, n - 1, NAN),
             "inf": sv.poison(c, n // 2, INF), "all_nan": np.full(n, NAN, dt)}
    if n > 3:
        cases["two_nan"] = sv.poison(c, [n // 2, n - 1], NAN)          # different blocks from n = 8193
        cases["inf_then_nan"] = sv.poison(sv.poison(c, n // 4, INF), n - 2, NAN)
        cases["nan_then_inf"] = sv.poison(sv.poison(c, n // 4, NAN), n - 2, INF)
    if np.dtype(dt).kind == "c":
        cases["nanj"] = sv.poison(c, n // 2, complex(0.0, NAN))
        cases["inf_nanj"] = sv.poison(c, n // 2, complex(INF, NAN))      # |.| is inf
    return cases


@pytest.mark.parametrize("dt", sv.DTYPES)
@pytest.mark.parametrize("n", [1, 300, 8193, 70_001])
def test_b6_peak_argmax_is_numpys(gpu, dt, n):
    ctx = gpu.get_context()
    lags = np.arange(n) - 7
    bad = []
    for name, c in _peak_cases(dt, n).items():
        wi, wm, wmean, wstd = sv.np_peak(c)
        wm = float(wm)
        gi, gm, _, _, gn = gpu.peak_stats(c)
        if gi != wi or not sv.same_scalar(gm, wm) or gn != n:
            bad.append((name, "peak_stats", "gpu", (gi, gm), "numpy", (wi, wm)))
        t = _dev(c)
        rec = torch.zeros(4, dtype=torch.float64, device="cuda")
        ctx.check(ctx.lib.vsig_peak_dev(ctx.h, _lib.DTYPES[CODE[c.dtype]], _ptr(t), n, _ptr(rec)), "peak")
        r = rec.cpu()
        if int(r.view(torch.int64)[1]) != wi or not sv.same_scalar(float(r[0]), wm):
            bad.append((name, "vsig_peak_dev", "gpu", (int(r.view(torch.int64)[1]), float(r[0])), "numpy", (wi, wm)))
        with np.errstate(all="ignore"):
            rl, rp, rc = ref.find_correlation_peak(c, lags)
            gl, gp, gc = gpu.find_correlation_peak(c, lags)
        if gl != rl or not sv.same_scalar(gp, rp) or not abs(float(gc) - float(rc)) <= 1e-5:
            bad.append((name, "find_correlation_peak", "gpu", (gl, gp, gc), "oracle", (rl, rp, rc)))
        if CODE[c.dtype] in ("c128", "f64"):
            st = torch.zeros(2, dtype=torch.float64, device="cuda")
            ctx.check(ctx.lib.vsig_abs_stats_dev(ctx.h, _lib.DTYPES[CODE[c.dtype]], _ptr(t), n, _ptr(st)), "stats")
            gmean, gstd = st.cpu().tolist()
            if not sv.same_scalar(gmean, wmean) or not sv.same_scalar(gstd, wstd):
                bad.append((name, "mean/std", "gpu", (gmean, gstd), "numpy", (wmean, wstd)))
    _report(bad)


# =========================================================================== B7
def _same_validation(got, want):
    bad = []
    for k in ("transplant_length_samples", "vector_location", "success", "transplant_length_us",
              "time_precision_us"):
        if got[k] != want[k]:
            bad.append((k, got[k], want[k]))
    if got["criteria"] != want["criteria"]:
        bad.append(("criteria", got["criteria"], want["criteria"]))
    if not sv.same_scalar(got["reference_correlation"], want["reference_correlation"]):
        bad.append(("reference_correlation", got["reference_correlation"], want["reference_correlation"]))
    if not abs(float(got["reference_confidence"]) - float(want["reference_confidence"])) <= 1e-5:
        bad.append(("reference_confidence", got["reference_confidence"], want["reference_confidence"]))
    for k, tol, rel in (("power_ratio", 1e-5, True), ("snr_improvement_db", 1e-4, False)):
        g, w = float(got[k]), float(want[k])
        if np.isfinite(w) and w != 0.0:
            if not abs(g - w) <= tol * (abs(w) if rel else 1.0):
                bad.append((k, g, w))
        elif not sv.same_scalar(g, w):
            bad.append((k, g, w))
    return bad


def test_b7_validate_transplant_quality(gpu):
    """Inside the region the reference segment is empty: with one, the score
    would come from the fused correlator's peak record, which is undefined on
    a non-finite stream.  Outside the region the poison must
    change nothing, with the correlation on."""
    rng = np.random.default_rng(9)
    orig = (rng.standard_normal(4099) + 1j * rng.standard_normal(4099)).astype(np.complex64)
    packet = (rng.standard_normal(700) + 1j * rng.standard_normal(700)).astype(np.complex64)
    new = orig.copy()
    new[1001:1701] = packet
    empty, seg = np.zeros(0, np.complex64), packet[100:400].copy()
    bad = []
    for v in (NAN, INF):
        for name, o, t, r in (("new inside", orig, sv.poison(new, 1300, v), empty),
                              ("orig inside", sv.poison(orig, 1001, v), new, empty),
                              ("both inside", sv.poison(orig, 1700, v), sv.poison(new, 1700, v), empty),
                              ("outside", sv.poison(orig, 1701, v), sv.poison(new, 1000, v), seg)):
            with np.errstate(all="ignore"):
                want = ref_validate(o, t, packet, 1001, r, 56e6)
                got = gpu.validate_transplant_quality(o, t, packet, 1001, r, 56e6)
            bad += [(name, v) + b for b in _same_validation(got, want)]
    _report(bad)


# =========================================================================== B8
def test_b8_build_vector_normalize(gpu):
    rng = np.random.default_rng(10)
    packet = (rng.standard_normal(700) + 1j * rng.standard_normal(700)).astype(np.complex64)
    sr = 1e6
    bad = []
    for name, v in (("nan", NAN), ("inf", INF), ("nanj", complex(0.0, NAN)), ("infj", complex(1.0, -INF))):
        pk = sv.poison(packet, 5, v)
        cfg = dict(signal=pk, period=1000.5 / sr, start_time=3.2 / sr)
        with np.errstate(all="ignore"):
            got, _ = gpu.build_vector([cfg], 4099.5 / sr, sr, normalize=True)
            want = sv.np_normalized_vector(pk, 1000, 4099, 3)
        ok = sv.same_bits(got, want).reshape(-1, 2).all(axis=1)
        bad += [(name, int(i), "gpu", got[i], "numpy", want[i]) for i in np.flatnonzero(~ok)[:8]]
    _report(bad)


# =========================================================================== B9
@pytest.mark.parametrize("dt", [np.float32, np.complex64])
def test_b9_peaks_treat_nan_as_minus_one(gpu, dt):
    """peaks.hip's rule: a NaN magnitude is never an instance, never beats a
    neighbour and never becomes a maximum -- the existing oracle run on |a|
    with NaN replaced by -1."""
    T = gpu.load_library().vsig_peaks_tile()
    n = 3 * T + 5
    base = sv.base_signal(dt, n=n, seed=2024)
    cases = {"scattered": [5, T // 2, 2 * T + 9], "tile_boundary": [T - 1, T], "next_tile_first": [2 * T],
             "whole_tile": np.arange(T, 2 * T), "at_the_peak": [int(np.argmax(np.abs(base)))],
             "all_nan": np.arange(n)}
    bad = []
    for name, at in cases.items():
        a = sv.poison(base, at, NAN)
        with np.errstate(all="ignore"):
            m = sv.nan_to_minus_one(np.abs(a).astype(np.float64))
        for d in (7, T + 1):
            for thr, relative in ((0.5, True), (0.3, False)):
                thr_used = thr * m.max() if relative else thr
                wi, wv = tp.ref_peaks(m, thr_used, d)
                want = dict(count=len(wi), argmax=int(np.argmax(m)), max=float(m.max()), thr_used=float(thr_used))
                rc, gi, gv, inf, _, _ = tp.dev_peaks(gpu, _dev(a), CODE[a.dtype], thr, relative, d, len(wi) + 3)
                if rc or inf != want or not np.array_equal(gi, wi) or not np.array_equal(gv, wv):
                    bad.append((name, d, thr, relative, "gpu", inf, list(gi[:4]), "oracle", want, list(wi[:4])))
                pi, pv = gpu.find_peaks(a, thr, d, relative)
                if not np.array_equal(pi, wi) or not np.array_equal(pv, wv):
                    bad.append((name, d, thr, relative, "find_peaks", list(pi[:4]), "oracle", list(wi[:4])))
        if name == "all_nan":
            assert (want["count"], want["argmax"], want["max"]) == (0, 0, -1.0)
    _report(bad)


# =========================================================================== C
def _split(got, clean, hit, axis):
    """(frames with a finite value among those that hold the sample, frames
    that differ from the clean run among the others); axis: the frame axis."""
    got, clean = np.moveaxis(got, axis, 0), np.moveaxis(clean, axis, 0)
    flat = got.reshape(len(got), -1)
    finite = np.isfinite(flat.view(sv.real_of(flat.dtype))).any(axis=1)
    same = sv.same_bits(got, clean).reshape(len(got), -1).all(axis=1)
    return np.flatnonzero(hit & finite), np.flatnonzero(~hit & ~same)


@pytest.mark.parametrize("nperseg,noverlap", [(256, 0), (1024, 512), (8192, 4096)])
def test_c1_spectrum_contains_a_non_finite_sample(gpu, nperseg, noverlap):
    hop = nperseg - noverlap
    n = nperseg + 4 * hop + 13
    x = ref.synth_iq(n, seed=nperseg)
    _, _, clean = gpu.spectrum(x, 1.0, "hann", nperseg, noverlap, nperseg)
    assert clean.shape == (nperseg, 5) and np.isfinite(clean).all()
    k = 2 * hop + 37
    m = np.arange(5)
    hit = (m * hop <= k) & (k < m * hop + nperseg)
    assert hit.any() and not hit.all()
    for v in (NAN, INF):
        _, _, S = gpu.spectrum(sv.poison(x, k, v), 1.0, "hann", nperseg, noverlap, nperseg)
        leak_in, leak_out = _split(S, clean, hit, 1)
        assert not len(leak_in), (v, "frames holding the sample with a finite bin", leak_in)
        assert not len(leak_out), (v, "clean frames that changed", leak_out)


@pytest.mark.parametrize("nchan,pt,n,k", [(64, 16, 17_344, 64 * 100 + 3), (256, 4, 256 * 24 + 3, 256 * 7 + 5)])
def test_c2_pfb_contains_a_non_finite_sample(gpu, nchan, pt, n, k):
    from scipy.signal import firwin
    h = firwin(pt * nchan, 1.0 / nchan).astype(np.float32)
    x = ref.synth_iq(n, seed=nchan)
    clean = gpu.pfb_channelize(x, h, nchan)
    assert np.isfinite(clean).all()
    m = np.arange(clean.shape[1])
    hit = (m * nchan <= k) & (k < m * nchan + pt * nchan)
    assert hit.sum() == pt and not hit.all()
    for v in (NAN, INF):
        y = gpu.pfb_channelize(sv.poison(x, k, v), h, nchan)
        parts = np.ascontiguousarray(y.T).view(np.float32).reshape(len(m), nchan, 2)
        some_finite = np.flatnonzero(hit & np.isfinite(parts).all(axis=2).any(axis=1))
        assert not len(some_finite), (v, "frames holding the sample with a finite channel", some_finite)
        _, leak_out = _split(y, clean, hit, 1)
        assert not len(leak_out), (v, "clean frames that changed", leak_out)


@pytest.mark.parametrize("decim", [1, 4])
def test_c3_fir_contains_a_non_finite_sample(gpu, decim):
    taps = np.hamming(255).astype(np.float32)
    taps /= taps.sum()
    f = gpu.FirFilter(taps, decim)
    block = f.block
    n = 4 * block + 77
    x = ref.synth_iq(n, seed=decim)
    clean = f(_dev(x)).cpu().numpy()
    assert np.isfinite(clean.view(np.float32)).all()
    k = block + block // 2 + 3
    j = np.arange(len(clean)) * decim                      # the input index of output j
    covered = (j >= k) & (j <= k + 254)
    far = np.abs(j - k) > block + 255
    assert covered.any() and far.sum() > len(j) // 4
    for v in (NAN, INF):
        y = f(_dev(sv.poison(x, k, v))).cpu().numpy()
        fin = np.isfinite(y.view(np.float32)).reshape(-1, 2).all(axis=1)
        assert not (covered & fin).any(), (v, "finite outputs under the taps", np.flatnonzero(covered & fin)[:8])
        same = sv.same_bits(y, clean).reshape(-1, 2).all(axis=1)
        assert same[far].all(), (v, "far outputs that changed", np.flatnonzero(far & ~same)[:8])


def test_c4_stored_correlation_contains_a_non_finite_sample(gpu):
    L, n, seg = 512, 3 * 8192, 16_384                      # seg: the largest correlator segment
    tm = ref.qpsk_preamble(L)
    x = ref.synth_iq(n, seed=44)
    td = _dev(tm)
    clean, _ = gpu.cross_correlate_signals(td, _dev(x), "valid")
    clean = clean.cpu().numpy()
    assert clean.dtype == np.complex64 and np.isfinite(clean.view(np.float32)).all()
    k = 1500
    o = np.arange(len(clean))
    covered = (o <= k) & (o >= k - L + 1)
    far = np.abs(o - k) > seg + L
    assert covered.sum() == L and far.sum() > 1000
    for v in (NAN, INF):
        c, _ = gpu.cross_correlate_signals(td, _dev(sv.poison(x, k, v)), "valid")
        c = c.cpu().numpy()
        fin = np.isfinite(c.view(np.float32)).reshape(-1, 2).all(axis=1)
        assert not (covered & fin).any(), (v, np.flatnonzero(covered & fin)[:8])
        same = sv.same_bits(c, clean).reshape(-1, 2).all(axis=1)
        assert same[far].all(), (v, np.flatnonzero(far & ~same)[:8])


# =========================================================================== D
# An unknown dtype code at every *_dev entry point that takes one: the status
# the C-ABI layer gives it (most refuse it themselves; vsig_db_dev and the two
# abs entry points hand it to their launcher, whose hipErrorInvalidValue comes
# back as VSIG_E_HIP), and the context goes on working.
E_INVALID, E_HIP, E_UNSUPPORTED = -1, -2, -4
_EPS32, _EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
_DX = (np.random.default_rng(7).standard_normal(16) + 1j * np.random.default_rng(8).standard_normal(16))
_DV = _DX[3:7].copy()
_DR = np.ascontiguousarray(_DX.real)
_DROWS = np.array([3, 17, 40, 64, 99, 100, 128, 150, 177, 200, 201, 222, 240, 250, 254, 255])
_DMAG = np.abs(_DX)
# every FFT-based entry point below is one or two 16-point complex64
# transforms of _DX: an output's error is at most n eps32 sum|x| a transform
# (n terms, each off by at most n / 2 roundings), doubled for margin
_FFT_TOL = 4 * 16 * _EPS32 * float(_DMAG.sum())


def _zeros(n, dt):
    return torch.zeros(n, dtype=dt, device="cuda")


def _d_peak(ctx, code):
    x, pk = _dev(_DX), _zeros(4, torch.float64)
    rc = ctx.lib.vsig_peak_dev(ctx.h, code, _ptr(x), 16, _ptr(pk))
    return rc, lambda: (pk[0].item() == _DMAG.max() and pk.view(torch.int64)[1].item() == _DMAG.argmax())


def _d_peaks(ctx, code):
    x, out, info = _dev(_DX), _zeros(8, torch.int64), _zeros(4, torch.int64)
    rc = ctx.lib.vsig_peaks_dev(ctx.h, code, _ptr(x), 16, 0.0, 0, 16, _ptr(out), 4, _ptr(info))
    return rc, lambda: (info[:2].tolist() == [1, _DMAG.argmax()] and out[0].item() == _DMAG.argmax()
                        and out.view(torch.float64)[1].item() == _DMAG.max())


def _d_runs(ctx, code):
    x, out, info = _dev(_DX), _zeros(10, torch.int64), _zeros(5, torch.int64)
    rc = ctx.lib.vsig_runs_dev(ctx.h, code, _ptr(x), 16, 0.0, 0, 0, _ptr(out), 2, _ptr(info))
    am, mx = int(_DMAG.argmax()), float(_DMAG.max())
    return rc, lambda: (info[:3].tolist() == [1, 16, am] and out[:3].tolist() == [0, 15, am]
                        and out.view(torch.float64)[3].item() == mx)


def _d_trace(ctx, code):
    x, lo, hi, info = _dev(_DX), _zeros(4, torch.float64), _zeros(4, torch.float64), _zeros(4, torch.int64)
    rc = ctx.lib.vsig_trace_envelope_dev(ctx.h, code, _ptr(x), 16, 0, 0, 16, 4, _lib.TRACE_ABS, 0.0, _ptr(lo),
                                         _ptr(hi), _ptr(info))
    m = _DMAG.reshape(4, 4)
    return rc, lambda: (np.array_equal(lo.cpu().numpy(), m.min(1)) and np.array_equal(hi.cpu().numpy(), m.max(1))
                        and info[:2].tolist() == [_DMAG.argmin(), _DMAG.argmax()])


def _d_abs_stats(ctx, code):
    x, st = _dev(_DX), _zeros(2, torch.float64)
    rc = ctx.lib.vsig_abs_stats_dev(ctx.h, code, _ptr(x), 16, _ptr(st))
    # 16 magnitudes of at most 4 roundings each, summed: 64 eps64 max|a| covers mean and std
    return rc, lambda: np.allclose(st.cpu().numpy(), [_DMAG.mean(), _DMAG.std()], rtol=0,
                                   atol=64 * _EPS64 * _DMAG.max())


def _d_select(ctx, code):
    x, ranks, vals = _dev(_DR), (C.c_int64 * 3)(0, 8, 15), (C.c_double * 3)()
    rc = ctx.lib.vsig_select_dev(ctx.h, code, _ptr(x), 16, ranks, 3, vals)
    return rc, lambda: list(vals) == np.sort(np.abs(_DR))[[0, 8, 15]].tolist()


def _d_threshold(ctx, code):
    x, thr = _dev(_DR), float(np.median(np.abs(_DR)))
    cnt, first, last, mx = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
    rc = ctx.lib.vsig_threshold_dev(ctx.h, code, _ptr(x), 16, thr, C.byref(cnt), C.byref(first), C.byref(last),
                                    C.byref(mx))
    hit = np.flatnonzero(np.abs(_DR) >= thr)
    return rc, lambda: (cnt.value, first.value, last.value, mx.value) == (len(hit), hit[0], hit[-1],
                                                                           np.abs(_DR).max())


def _d_boxcar(ctx, code):
    x, sm = _dev(_DX), _zeros(16, torch.float64)
    rc = ctx.lib.vsig_boxcar_energy_dev(ctx.h, code, _ptr(x), 16, 5, _ptr(sm))
    e = _DMAG ** 2
    # differences of prefix sums, each off by at most n eps64 sum(e)
    return rc, lambda: np.allclose(sm.cpu().numpy(), np.convolve(e, np.ones(5) / 5, "same"), rtol=0,
                                   atol=2 * 16 * _EPS64 * e.sum())


def _d_db(ctx, code):
    x, out = _dev(_DR), _zeros(16, torch.float64)
    rc = ctx.lib.vsig_db_dev(ctx.h, code, _ptr(x), 16, 1e-12, _ptr(out))
    want = 10 * np.log10(np.abs(_DR) + 1e-12)
    return rc, lambda: bool(np.all(np.abs(out.cpu().numpy() - want) <= 8 * np.spacing(np.abs(want))))   # as A2


def _d_abs(ctx, code, wide):
    x, out = _dev(_DX), _zeros(16, torch.complex128 if wide else torch.complex64)
    fn = ctx.lib.vsig_abs_c128_dev if wide else ctx.lib.vsig_abs_c64_dev
    rc = fn(ctx.h, code, _ptr(x), 16, _ptr(out))
    want = _DMAG if wide else _DMAG.astype(np.float32)
    return rc, lambda: np.array_equal(out.cpu().numpy(), want + 0j)


def _d_image(ctx, code):
    # a 4 x 4 map whose pixels sit in the middle of colour rows _DROWS; the table's entry i is the number i
    vmin, vmax = -40.0, 0.0
    s = 10.0 ** (((_DROWS + 0.5) / 256 * (vmax - vmin) + vmin) / 10)
    x, lut, out = _dev(s), torch.arange(259, dtype=torch.int32, device="cuda"), _zeros(16, torch.int32)
    rc = ctx.lib.vsig_spectrogram_image_dev(ctx.h, code, _ptr(x), 4, 4, 0, 4, 0.0, vmin, vmax, 0, 0, 1, 1, _ptr(lut),
                                            _ptr(out))
    return rc, lambda: out.tolist() == _DROWS.tolist()


def _d_dft(ctx, code):
    x, y = _dev(_DX), _zeros(16, torch.complex64)
    rc = ctx.lib.vsig_dft_dev(ctx.h, code, _ptr(x), 16, 1, 0, _lib.DTYPES["c64"], _ptr(y))
    return rc, lambda: np.allclose(y.cpu().numpy(), np.fft.fft(_DX), rtol=0, atol=_FFT_TOL)


def _d_resample(ctx, code):
    x, y = _dev(_DX), _zeros(8, torch.complex64)
    rc = ctx.lib.vsig_resample_dev(ctx.h, code, _ptr(x), 16, 8, 0, _ptr(y))
    return rc, lambda: np.allclose(y.cpu().numpy(), ref.resample_signal(_DX, 2.0, 1.0), rtol=0, atol=_FFT_TOL)


def _d_channel(ctx, code):
    # sample_rate 4, n 16: the reference's axis is CENTER_FREQ + k, the band keeps k = 1, 2, 3
    x, y, args = _dev(_DX), _zeros(16, torch.float64), (ref.CENTER_FREQ + 2.0, 4.0, 3.0)
    rc = ctx.lib.vsig_filter_channel_dev(ctx.h, code, _ptr(x), 16, *args, _ptr(y))
    return rc, lambda: np.allclose(y.cpu().numpy(), ref.filter_channel(_DX, *args), rtol=0, atol=_FFT_TOL)


def _d_correlate(ctx, code):
    a, v, c = _dev(_DX), _dev(_DV), _zeros(13, torch.complex128)
    rc = ctx.lib.vsig_correlate_dev(ctx.h, code, _ptr(a), 16, _ptr(v), 4, _lib.MODES["valid"], _lib.DTYPES["c128"],
                                    _ptr(c), None)
    # complex64 transforms of any length the library may pick (at most 2^14 points: 14 passes)
    tol = 4 * 14 * _EPS32 * float(np.linalg.norm(_DX) * np.linalg.norm(_DV))
    return rc, lambda: np.allclose(c.cpu().numpy(), np.correlate(_DX, _DV, "valid"), rtol=0, atol=tol)


def _d_correlate_stats(ctx, code):
    a, v, st = _dev(_DX), _dev(_DV), _zeros(2, torch.float64)
    rc = ctx.lib.vsig_correlate_stats_dev(ctx.h, code, _ptr(a), 16, _ptr(v), 4, _lib.MODES["valid"], _ptr(st))
    m = np.abs(np.correlate(_DX, _DV, "valid"))
    # double sums of 4 products, then 13 magnitudes: 64 eps64 max|c| covers mean and std
    return rc, lambda: np.allclose(st.cpu().numpy(), [m.mean(), m.std()], rtol=0, atol=64 * _EPS64 * m.max())


# entry point -> (status for an unknown code, a valid code, the call)
_DTYPE_ENTRIES = {
    "vsig_peak_dev": (E_INVALID, "c128", _d_peak),
    "vsig_peaks_dev": (E_INVALID, "c128", _d_peaks),
    "vsig_runs_dev": (E_INVALID, "c128", _d_runs),
    "vsig_trace_envelope_dev": (E_INVALID, "c128", _d_trace),
    "vsig_abs_stats_dev": (E_UNSUPPORTED, "c128", _d_abs_stats),
    "vsig_select_dev": (E_INVALID, "f64", _d_select),
    "vsig_threshold_dev": (E_INVALID, "f64", _d_threshold),
    "vsig_boxcar_energy_dev": (E_INVALID, "c128", _d_boxcar),
    "vsig_db_dev": (E_HIP, "f64", _d_db),
    "vsig_abs_c64_dev": (E_HIP, "c128", lambda ctx, code: _d_abs(ctx, code, False)),
    "vsig_abs_c128_dev": (E_HIP, "c128", lambda ctx, code: _d_abs(ctx, code, True)),
    "vsig_spectrogram_image_dev": (E_INVALID, "f64", _d_image),
    "vsig_dft_dev": (E_INVALID, "c128", _d_dft),
    "vsig_resample_dev": (E_INVALID, "c128", _d_resample),
    "vsig_filter_channel_dev": (E_INVALID, "c128", _d_channel),
    "vsig_correlate_dev": (E_INVALID, "c128", _d_correlate),
    "vsig_correlate_stats_dev": (E_INVALID, "c128", _d_correlate_stats),
}


def test_d0_every_dtype_entry_point_is_listed():
    """The table above names every *_dev entry point of the ABI whose second
    argument is a dtype code (vsig_planar_to_c64_dev's is a MAT class)."""
    have = {n for n, (_, args) in _lib.SIGNATURES.items()
            if n.endswith("_dev") and len(args) > 2 and args[1] is _lib.I32 and n != "vsig_planar_to_c64_dev"}
    assert have == set(_DTYPE_ENTRIES)


@pytest.mark.parametrize("entry", sorted(_DTYPE_ENTRIES))
def test_d1_unknown_dtype_code(gpu, entry):
    status, code, call = _DTYPE_ENTRIES[entry]
    ctx = gpu.get_context()
    for bad in (4, -1):
        rc, _ = call(ctx, bad)
        assert rc == status, (entry, bad, rc, ctx.lib.vsig_last_error(ctx.h).decode())
    rc, right = call(ctx, _lib.DTYPES[code])
    assert rc == _lib.VSIG_OK, (entry, rc, ctx.lib.vsig_last_error(ctx.h).decode())
    assert right(), entry
