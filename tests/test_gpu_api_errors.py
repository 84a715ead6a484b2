"""The C-ABI layer's argument refusals, through ctypes: the status code and the
exact vsig_last_error text of checks that several entry points share (the
record lists, the two segment tables, the streaming span, 8-byte alignment,
the element-wise prologue).  Every refusal comes before anything is enqueued,
so those cases launch nothing.

Then the smallest runs that reach the shared host helpers: both record lists
through their host-pointer entry with cap below the count, an isolate plan of
2 filters x 3 taps over 3 segments (an odd frame count), a bank of K = 2, L = 8.
References and tolerances are those of the features' own GPU tests
(tests/peaks_ref.py, runs_ref.py, isolate_ref.py at 1e-5, xcorr_bank_ref.py at
1e-5)."""
import ctypes as C

import numpy as np
import pytest
import torch

import isolate_ref as iso
import xcorr_bank_ref as xb
from oracle import ref
from peaks_ref import ref_peaks
from runs_ref import run_stats, runs_ref
from vector_amd import _lib

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
VALID, SAME = 0, 2
C64 = _lib.DTYPES["c64"]
SR = 56e6
SENT = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.get_context()


@pytest.fixture(scope="module")
def mem():
    """128 bytes of device memory; ptr(mem) is 8-byte aligned."""
    return torch.zeros(16, dtype=torch.complex64, device="cuda")


def ptr(t, skew=0):
    return C.c_void_p(t.data_ptr() + skew)


def refused(ctx, rc, text, code=INVALID):
    assert rc == code, (rc, ctx.lib.vsig_last_error(ctx.h).decode())
    assert ctx.lib.vsig_last_error(ctx.h).decode() == text


# ---------------------------------------------------------------- record lists
LIST_CASES = [
    ("cap", dict(cap=-1), "need cap >= 0 and {reach} >= 0"),
    ("reach", dict(reach=-1), "need cap >= 0 and {reach} >= 0"),
    ("null out", dict(cap=1, out=None), "null out with cap > 0"),
    ("nan thr", dict(thr=float("nan")), "thr is NaN"),
    ("long n", dict(n=(1 << 40) + 1), "n above 2^40"),
    ("dtype", dict(dtype=99), "dtype"),
]


@pytest.mark.parametrize("entry", ["vsig_peaks_dev", "vsig_peaks", "vsig_runs_dev", "vsig_runs"])
@pytest.mark.parametrize("name,change,text", LIST_CASES, ids=[c[0] for c in LIST_CASES])
def test_record_list_refusals(ctx, mem, entry, name, change, text):
    host = np.zeros(16, np.complex64)
    a = ptr(mem) if entry.endswith("_dev") else C.c_void_p(host.ctypes.data)
    out = np.zeros(64, np.int64)
    info = np.zeros(8, np.int64)
    arg = dict(dtype=C64, n=16, thr=0.5, reach=0, out=C.c_void_p(out.ctypes.data), cap=0)
    arg.update(change)
    rc = getattr(ctx.lib, entry)(ctx.h, arg["dtype"], a, arg["n"], arg["thr"], 0, arg["reach"], arg["out"],
                                 arg["cap"], C.c_void_p(info.ctypes.data))
    refused(ctx, rc, text.format(reach="min_distance" if "peaks" in entry else "max_gap"))


# ---------------------------------------------------------------- segment tables
def psd_segments_create(ctx, segs, nseg, n):
    h = C.c_void_p()
    tab = (_lib.Segment * len(segs))(*[_lib.Segment(s, ln) for s, ln in segs]) if segs is not None else None
    return ctx.lib.vsig_psd_segments_create(ctx.h, tab, nseg, n, 64, 32, 64, C.byref(h)), h


def isolate_create(ctx, segs, nseg, n, taps=None, sr=SR):
    h = C.c_void_p()
    taps = np.full((1, 3), 1 / 3, np.float32) if taps is None else np.ascontiguousarray(taps, np.float32)
    tab = None
    if segs is not None:
        tab = (_lib.IsolateSeg * len(segs))(*[_lib.IsolateSeg(*s) for s in segs])
    rc = ctx.lib.vsig_isolate_create(ctx.h, tab, nseg, n, taps.ctypes.data_as(C.POINTER(C.c_float)),
                                     taps.shape[0], taps.shape[1], sr, C.byref(h))
    return rc, h


def test_segment_table_refusals(ctx):
    for create, seg in ((psd_segments_create, lambda s, ln: (s, ln)),
                        (isolate_create, lambda s, ln: (s, ln, 0.0, 0, 0))):
        rc, _ = create(ctx, [seg(0, 4)], -1, 10)
        refused(ctx, rc, "nseg must be in [0, 2^24]")
        rc, _ = create(ctx, None, 1, 10)
        refused(ctx, rc, "null segment table")
        rc, _ = create(ctx, [seg(0, 4)], 1, 0)
        refused(ctx, rc, "n must be in [1, 2^40]")
    rc, _ = psd_segments_create(ctx, [(0, 4), (5, 6)], 2, 10)
    refused(ctx, rc, "segment 1 {start 5, len 6} is outside [0, 10]")
    rc, _ = isolate_create(ctx, [(0, 4, 0.0, 0, 0), (5, 6, 0.0, 0, 0)], 2, 10)
    refused(ctx, rc, "segment 1 {start 5, len 6} is empty or outside [0, 10)")


def test_empty_segment_at_the_end_is_a_psd_row_and_no_burst(ctx, mem):
    rc, h = isolate_create(ctx, [(10, 0, 0.0, 0, 0)], 1, 10)
    refused(ctx, rc, "segment 0 {start 10, len 0} is empty or outside [0, 10)")
    assert not h.value
    rc, h = psd_segments_create(ctx, [(10, 0)], 1, 10)
    assert rc == 0 and h.value, ctx.lib.vsig_last_error(ctx.h).decode()
    try:
        v = [C.c_int64(-1) for _ in range(4)]
        assert ctx.lib.vsig_psd_segments_info(h, *(C.byref(a) for a in v)) == 0
        assert (v[0].value, v[1].value) == (0, 0)                # no frames, no blocks
        # the run's alignment check, on the same plan
        rc = ctx.lib.vsig_psd_segments_run(h, ptr(mem, 4), ptr(mem), 1.0, 0, ptr(mem), None, None)
        refused(ctx, rc, "x must be 8-byte aligned")
    finally:
        ctx.lib.vsig_psd_segments_free(h)


# ---------------------------------------------------------------- alignment
def test_alignment_refusals(ctx, mem):
    lib = ctx.lib
    refused(ctx, lib.vsig_band_measure_run(ctx.h, ptr(mem, 4), 1, 4, 4, 0.1, ptr(mem, 64)),
            "rows and out must be 8-byte aligned")
    refused(ctx, lib.vsig_band_measure_run(ctx.h, ptr(mem), 1, 4, 4, 0.1, ptr(mem, 68)),
            "rows and out must be 8-byte aligned")
    refused(ctx, lib.vsig_region_power_dev(ctx.h, ptr(mem, 4), ptr(mem), 4, ptr(mem, 64)),
            "region power: operands must be 8-byte aligned")
    refused(ctx, lib.vsig_region_power_dev(ctx.h, ptr(mem), ptr(mem, 4), 4, ptr(mem, 64)),
            "region power: operands must be 8-byte aligned")
    refused(ctx, lib.vsig_normalize_c64_dev(ctx.h, ptr(mem, 4), 4, ptr(mem, 120), ptr(mem, 64)),
            "x and y must be 8-byte aligned")
    refused(ctx, lib.vsig_normalize_c64_dev(ctx.h, ptr(mem), 4, ptr(mem, 120), ptr(mem, 68)),
            "x and y must be 8-byte aligned")
    refused(ctx, lib.vsig_vector_build_dev(ctx.h, None, 0, ptr(mem, 4), 4, None), "out must be 8-byte aligned")
    place = (_lib.PacketPlace * 1)(_lib.PacketPlace(mem.data_ptr() + 4, 1, 0, 1, 1))
    refused(ctx, lib.vsig_vector_build_dev(ctx.h, place, 1, ptr(mem, 64), 4, None),
            "place 0: packet must be 8-byte aligned")


# ---------------------------------------------------------------- element-wise prologue
def elementwise(lib, h, x, n, y, y2):
    return {
        "vsig_mix_c64_dev": lambda: lib.vsig_mix_c64_dev(h, x, n, 1.0, SR, 0, y),
        "vsig_scale_c64_dev": lambda: lib.vsig_scale_c64_dev(h, x, n, 2.0, y),
        "vsig_wv_quantize_dev": lambda: lib.vsig_wv_quantize_dev(h, x, n, 1.0, y),
        "vsig_planar_to_c64_dev": lambda: lib.vsig_planar_to_c64_dev(h, 7, x, x, n, y),
        "vsig_c64_to_planar_dev": lambda: lib.vsig_c64_to_planar_dev(h, x, n, y, y2),
    }


@pytest.mark.parametrize("entry", ["vsig_mix_c64_dev", "vsig_scale_c64_dev", "vsig_wv_quantize_dev",
                                   "vsig_planar_to_c64_dev", "vsig_c64_to_planar_dev"])
def test_elementwise_prologue(ctx, mem, entry):
    out = torch.full((16,), SENT, dtype=torch.int64, device="cuda")
    y, y2 = ptr(out), ptr(out, 64)
    refused(ctx, elementwise(ctx.lib, ctx.h, ptr(mem), -1, y, y2)[entry](),
            "need n >= 0 and sample_rate != 0" if entry == "vsig_mix_c64_dev" else "n < 0")
    refused(ctx, elementwise(ctx.lib, ctx.h, None, 4, y, y2)[entry](), "null pointer")
    refused(ctx, elementwise(ctx.lib, ctx.h, ptr(mem), 4, None, y2)[entry](), "null pointer")
    assert elementwise(ctx.lib, ctx.h, ptr(mem), 0, y, y2)[entry]() == 0
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "n = 0 wrote something"


def test_mix_refuses_a_zero_sample_rate(ctx, mem):
    refused(ctx, ctx.lib.vsig_mix_c64_dev(ctx.h, ptr(mem), 4, 1.0, 0.0, 0, ptr(mem, 64)),
            "need n >= 0 and sample_rate != 0")


# ---------------------------------------------------------------- record lists, host entry
def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def test_peaks_host_entry_copies_min_count_cap(ctx):
    n = ctx.lib.vsig_peaks_tile() + 1
    a = noise(n, 11)
    m = np.abs(a).astype(np.float64)
    thr, d, cap = float(np.quantile(m, 0.9)), 3, 2
    wi, wv = ref_peaks(m, thr, d)
    assert len(wi) > cap
    out = np.full((cap + 2, 2), SENT, np.int64)
    info = _lib.PeaksInfo()
    rc = ctx.lib.vsig_peaks(ctx.h, C64, C.c_void_p(a.ctypes.data), n, thr, 0, d, C.c_void_p(out.ctypes.data), cap,
                            C.byref(info))
    assert rc == 0, ctx.lib.vsig_last_error(ctx.h).decode()
    assert (info.count, info.argmax, info.max, info.thr_used) == (len(wi), int(np.argmax(m)), m.max(), thr)
    assert np.array_equal(out[:cap, 0], wi[:cap]) and np.array_equal(out[:cap, 1].view(np.float64), wv[:cap])
    assert (out[cap:] == SENT).all()


def test_runs_host_entry_copies_min_count_cap(ctx):
    n = ctx.lib.vsig_runs_tile() + 1
    a = noise(n, 12)
    m = np.abs(a).astype(np.float64)
    thr, gap, cap = float(np.quantile(m, 0.9)), 1, 2
    ws, we = runs_ref(m, thr, gap)
    assert len(ws) > cap
    out = np.full((cap + 2, 5), SENT, np.int64)
    info = _lib.RunsInfo()
    rc = ctx.lib.vsig_runs(ctx.h, C64, C.c_void_p(a.ctypes.data), n, thr, 0, gap, C.c_void_p(out.ctypes.data), cap,
                           C.byref(info))
    assert rc == 0, ctx.lib.vsig_last_error(ctx.h).decode()
    assert (info.count, info.covered, info.argmax, info.max, info.thr_used) == (
        len(ws), int(np.count_nonzero(m >= thr)), int(np.argmax(m)), m.max(), thr)
    wa, wm, wsum = run_stats(m, ws[:cap], we[:cap])
    f = out.view(np.float64)
    assert np.array_equal(out[:cap, 0], ws[:cap]) and np.array_equal(out[:cap, 1], we[:cap])
    assert np.array_equal(out[:cap, 2], wa) and np.array_equal(f[:cap, 3], wm)
    # tests/test_gpu_runs.py's bound on a run's sum: 2 length 2^-53 of it
    assert (np.abs(f[:cap, 4] - wsum) <= 2 * (we[:cap] - ws[:cap] + 1) * 2.0 ** -53 * wsum).all()
    assert (out[cap:] == SENT).all()


# ---------------------------------------------------------------- isolate plan
def test_small_isolate_plan(ctx):
    T, n = 3, 5000
    hop = iso.M - (T - 1)
    rng = np.random.default_rng(3)
    taps = np.stack([np.array([0.25, 0.5, 0.25], np.float32), rng.standard_normal(T).astype(np.float32) / np.sqrt(T)])
    segs = [(100, hop + 5, 0.11 * SR, 1, 0), (4000, 7, -0.3 * SR, 0, 0), (1501, 2 * hop, 0.02 * SR, 1, 0)]
    x = noise(n, 13)
    rc, h = isolate_create(ctx, segs, len(segs), n, taps)
    assert rc == 0, ctx.lib.vsig_last_error(ctx.h).decode()
    try:
        v = [C.c_int64() for _ in range(4)]
        assert ctx.lib.vsig_isolate_info(h, *(C.byref(a) for a in v)) == 0
        total, frames, blocks, hop2 = (a.value for a in v)
        assert (total, frames, blocks, hop2) == (sum(s[1] for s in segs), 5, 3, hop)
        off = np.zeros(len(segs) + 1, np.int64)
        assert ctx.lib.vsig_isolate_offsets(h, off.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        assert np.array_equal(off, np.r_[0, np.cumsum([s[1] for s in segs])])
        xd = torch.from_numpy(x).cuda()
        y = torch.full((total,), float("nan"), dtype=torch.complex64, device="cuda")
        refused(ctx, ctx.lib.vsig_isolate_run(h, ptr(xd, 4), ptr(y)), "x and y must be 8-byte aligned")
        refused(ctx, ctx.lib.vsig_isolate_run(h, ptr(xd), ptr(y, 4)), "x and y must be 8-byte aligned")
        assert ctx.lib.vsig_isolate_run(h, ptr(xd), ptr(y)) == 0, ctx.lib.vsig_last_error(ctx.h).decode()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
    finally:
        ctx.lib.vsig_isolate_free(h)
    for k, (start, ln, f, filt, _) in enumerate(segs):
        err = iso.rel_err(got[off[k]:off[k + 1]], iso.isolate(x, start, start + ln, f, taps[filt], SR))
        print(f"segment {k}: error {err:.3e}")
        assert err <= 1e-5, (k, err)


# ---------------------------------------------------------------- template bank
def test_small_bank_and_the_streaming_modes(ctx):
    K, L, n = 2, 8, 5000
    offs = xb.default_step(SR, L) / 8 * np.array([2.0, 3.0])
    T = np.ascontiguousarray(xb.hypotheses(ref.qpsk_preamble(L, seed=L), offs, SR))
    pos = 3210
    s, _ = xb.planted(L, n, offs, 0, pos, seed=14)
    s = np.ascontiguousarray(s, np.complex64)
    want = xb.bank_ref(s, T, "valid")
    widx, wpeak, ws1, ws2 = xb.records_ref(want)
    assert widx[0] == pos
    sd = torch.from_numpy(s).cuda()
    bank, one = C.c_void_p(), C.c_void_p()
    assert ctx.lib.vsig_xcorr_bank_create(ctx.h, C.c_void_p(T.ctypes.data), K, L, C.byref(bank)) == 0
    try:
        c = torch.full((K, n - L + 1), float("nan"), dtype=torch.complex64, device="cuda")
        pk = torch.zeros((K, 4), dtype=torch.float64, device="cuda")
        refused(ctx, ctx.lib.vsig_xcorr_bank_exec_dev(bank, ptr(sd), n, SAME, ptr(c), ptr(pk)),
                "the template bank supports VALID and FULL")
        rc = ctx.lib.vsig_xcorr_bank_exec_dev(bank, ptr(sd), n, VALID, ptr(c), ptr(pk))
        assert rc == 0, ctx.lib.vsig_last_error(ctx.h).decode()
        torch.cuda.synchronize()
        got, rec = c.cpu().numpy(), pk.cpu()
    finally:
        ctx.lib.vsig_xcorr_bank_free(bank)
    a = np.abs(want)
    e = np.abs(got - want).max(axis=1) / a.max(axis=1)
    idx = rec.view(torch.int64)[:, 1].numpy()
    peak, s1, s2 = (rec[:, j].numpy() for j in (0, 2, 3))
    top = a[np.arange(K), idx] / wpeak
    ep, e1, e2 = (np.abs(g / w - 1).max() for g, w in ((peak, wpeak), (s1, ws1), (s2, ws2)))
    print(f"bank K={K} L={L}: c {e.max():.2e} top {top.min():.7f} peak {ep:.2e} sum_abs {e1:.2e} sum_abs2 {e2:.2e}")
    assert np.all(e <= 1e-5) and np.all(top >= 1 - 1e-4) and idx[0] == widx[0]
    assert ep <= 1e-5 and e1 <= 1e-5 and e2 <= 1e-5
    # one template, streaming: the same span rule, its own message
    assert ctx.lib.vsig_xcorr_create(ctx.h, C.c_void_p(T.ctypes.data), L, C.byref(one)) == 0
    try:
        refused(ctx, ctx.lib.vsig_xcorr_exec_dev(one, ptr(sd), n, SAME, None, None),
                "streaming correlation supports VALID and FULL")
    finally:
        ctx.lib.vsig_xcorr_free(one)
