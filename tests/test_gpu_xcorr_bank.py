"""GPU checks of the template bank (xcorr_bank.hip behind vsig_xcorr_bank_* and
vector_amd.CorrelatorBank / frequency_search / find_packet_location_with_offset).

The reference is tests/xcorr_bank_ref.py: np.correlate in complex128 per
template.  XC_TOL = 1e-5 is the project's bound for a complex64 overlap-save
correlation (max error over max |c|; scipy's own complex64 overlap-save of the
same data sits at 2.6e-7).  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import xcorr_bank_ref as xb
from oracle import ref
from vector_amd import _lib

pytestmark = pytest.mark.gpu

XC_TOL = 1e-5
SR = 56e6
KS = (1, 3, 17)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(bank, s, mode, store=True):
    """(c[K][nout] or None, peaks tensor) of one call, synchronised."""
    nout = bank.out_len(int(s.shape[0]), mode)
    out = torch.full((bank.K, nout), float("nan"), dtype=torch.complex64, device="cuda") if store else None
    c, pk = bank(s, mode, out=out)
    torch.cuda.synchronize()
    return (c.cpu().numpy() if store else None), pk


def records(bank, pk):
    peak, idx, s1, s2 = bank.read_peaks(pk)
    return idx, peak, s1, s2


def search_templates(L, K=17):
    """K hypotheses of qpsk_preamble(L) on a grid of an eighth of the default
    step (a refining search), the planted one first, so that every leading
    sub-bank holds it.  Every hypothesis is then within half a cycle of the
    planted one over the template and keeps sinc(1/2) = 0.64 of its peak: the
    error bound is relative to each hypothesis' own max |c|, and fp32 rounding
    is relative to the energy under the template, so a hypothesis a whole
    number of cycles off -- whose only output at n = L is a cancellation to
    1e-3 of that energy -- would measure the cancellation, not the kernel.
    (Weak hypotheses on the default grid, over a long vector: the front-end
    tests below.)"""
    step = xb.default_step(SR, L) / 8
    offs = step * np.r_[2, np.arange(-8, 2), np.arange(3, 9)][:K]
    return offs, xb.hypotheses(ref.qpsk_preamble(L, seed=L), offs, SR)


# ---------------------------------------------------------------- 1. values
def _n_of(kind, L, hop):
    return {"L": L, "L+hop-1": L + hop - 1, "L+hop": L + hop, "3hop+77": 3 * hop + 77}[kind]


@pytest.mark.parametrize("nkind", ["L", "L+hop-1", "L+hop", "3hop+77"])
@pytest.mark.parametrize("L", [1, 2, 1000, 1024, 1025, 3000, 4096])
def test_values(gpu, L, nkind):
    offs, T = search_templates(L)
    banks = {K: gpu.CorrelatorBank(T[:K]) for K in KS}
    M, hop, _, _ = banks[1].plan(L, "valid")
    assert M == (4096 if L <= 1024 else 8192) and hop == M - L + 1
    n = _n_of(nkind, L, hop)
    pos = (2 * (n - L)) // 3
    s, _ = xb.planted(L, n, offs, 0, pos, seed=L + n)
    full = xb.bank_ref(s, T, "full")                       # once; 'valid' is its middle
    refs = {"full": full, "valid": full[:, L - 1:n]}
    buf = torch.empty(n + 1, dtype=torch.complex64, device="cuda")
    buf[1:] = dev(s)
    streams = {"aligned": dev(s), "8 bytes in": buf[1:]}
    worst = dict(c=0.0, top=1.0, peak=0.0, s1=0.0, s2=0.0)
    for mode, want in refs.items():
        a = np.abs(want)
        widx, wpeak, ws1, ws2 = xb.records_ref(want)
        assert wpeak[0] > 0.5 * L and widx[0] == pos + (L - 1 if mode == "full" else 0)
        for K, bank in banks.items():
            assert bank.plan(n, mode)[:2] == (M, hop)
            for name, st in streams.items():
                c, pk = run(bank, st, mode)
                _, pk0 = run(bank, st, mode, store=False)
                idx, peak, s1, s2 = records(bank, pk)
                tag = f"L={L} n={n} K={K} {mode} {name}"
                assert c.shape == (K, want.shape[1])
                e = np.abs(c - want[:K]).max(axis=1) / a[:K].max(axis=1)
                top = a[np.arange(K), idx] / wpeak[:K]
                ep, e1, e2 = (np.abs(g / w - 1).max() for g, w in
                              ((peak, wpeak[:K]), (s1, ws1[:K]), (s2, ws2[:K])))
                print(f"{tag}: c {e.max():.2e} top {top.min():.7f} peak {ep:.2e} "
                      f"sum_abs {e1:.2e} sum_abs2 {e2:.2e}")
                worst = dict(c=max(worst["c"], e.max()), top=min(worst["top"], top.min()),
                             peak=max(worst["peak"], ep), s1=max(worst["s1"], e1), s2=max(worst["s2"], e2))
                assert np.all(e <= XC_TOL), tag
                assert np.all((idx >= 0) & (idx < want.shape[1])), tag
                assert np.all(top >= 1 - 1e-4), tag
                assert idx[0] == widx[0], tag
                assert ep <= 1e-5 and e1 <= 1e-5 and e2 <= 1e-5, tag
                assert torch.equal(pk.view(torch.int64), pk0.view(torch.int64)), tag + ": c = NULL"
    print(f"worst L={L} {nkind}: {worst}")


# ------------------------------------------------ 2. many frames per block
def test_second_walk_of_a_persistent_block(gpu):
    L, K = 1024, 2
    offs = xb.default_step(SR, L) * np.array([2.0, 3.0])   # the planted hypothesis and its neighbour
    T = xb.hypotheses(ref.qpsk_preamble(L, seed=L), offs, SR)
    bank = gpu.CorrelatorBank(T)
    n = 1 << 21
    while True:
        M, hop, nblocks, grid = bank.plan(n, "valid")
        if nblocks > grid:
            break
        n *= 2
        assert n <= 1 << 25, (nblocks, grid)
    pos = (grid + 3) * hop + 100                           # a frame reached on a second walk
    assert pos + L <= n and pos // hop >= grid
    s, _ = xb.planted(L, n, offs, 0, pos, seed=21)
    _, pk = run(bank, dev(s), "valid", store=False)
    idx, peak, _, _ = records(bank, pk)
    # the planted |c| (about L; 0.64 L for the neighbour hypothesis) against the
    # largest noise-only |c|: Rayleigh of scale 0.1 sqrt(L) = 3.2 over n lags, < 25
    want = np.abs([np.vdot(T[k].astype(np.complex128), s[pos:pos + L].astype(np.complex128))
                   for k in range(K)])
    print(f"n={n} M={M} hop={hop} nblocks={nblocks} grid={grid} pos={pos} idx={idx} "
          f"peak={peak} want={want} err={np.abs(peak / want - 1)}")
    assert want[0] > 0.9 * L and want[1] > 0.5 * L
    assert np.array_equal(idx, [pos, pos])
    assert np.all(np.abs(peak / want - 1) <= 1e-5)


# ---------------------------------------------------------- 3. independence
def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def test_rows_do_not_depend_on_the_other_templates(gpu):
    L = 1000
    A, B, Cc = (ref.synth_iq(L, seed=k) for k in (31, 32, 33))
    zero = np.zeros(L, np.complex64)
    nan = B.copy()
    nan[L // 2] = complex(np.nan, 0.0)
    probe = gpu.CorrelatorBank(np.stack([B]))
    hop = probe.plan(L, "valid")[1]
    n = 3 * hop + 77
    s = dev(ref.synth_iq(n, seed=30))
    got = {}
    for name, rows in dict(ABC=[A, B, Cc], B=[B], CB=[Cc, B], AZC=[A, zero, Cc], ANC=[A, nan, Cc]).items():
        bank = gpu.CorrelatorBank(np.stack(rows))
        c, pk = run(bank, s, "valid")
        got[name] = (c, pk.cpu().numpy())
    c0, r0 = got["ABC"]
    for name, row in (("B", 0), ("CB", 1)):
        c, r = got[name]
        assert np.array_equal(_bits(c[row]), _bits(c0[1])), name
        assert np.array_equal(_bits(r[row]), _bits(r0[1])), name
    for name in ("AZC", "ANC"):                            # the neighbours of the odd row are untouched
        c, r = got[name]
        for row in (0, 2):
            assert np.array_equal(_bits(c[row]), _bits(c0[row])), name
            assert np.array_equal(_bits(r[row]), _bits(r0[row])), name
    cz, rz = got["AZC"]
    assert not cz[1].any()
    assert np.array_equal(_bits(rz[1]), _bits(np.zeros(4)))          # (0, 0, 0, 0)
    _, rn = got["ANC"]
    print("NaN template record:", rn[1], rn[1].view(np.int64)[1])
    assert np.isnan(rn[1][2]) and np.isnan(rn[1][3])
    assert np.all(np.isfinite(rn[[0, 2]][:, [0, 2, 3]]))


# ----------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("L", [1024, 4096])
def test_same_call_same_bits(gpu, L):
    offs, T = search_templates(L, 5)
    bank = gpu.CorrelatorBank(T)
    hop = bank.plan(L, "valid")[1]
    s = dev(xb.planted(L, 3 * hop + 77, offs, 0, hop + 5, seed=4)[0])
    c1, p1 = run(bank, s, "full")
    c2, p2 = run(bank, s, "full")
    assert np.array_equal(_bits(c1), _bits(c2))
    assert torch.equal(p1.view(torch.int64), p2.view(torch.int64))


# ------------------------------------------- 5. K = 1 against the Correlator
@pytest.mark.parametrize("mode", ["valid", "full"])
@pytest.mark.parametrize("L", [1000, 3000, 4096])
def test_single_template_matches_the_correlator(gpu, L, mode):
    p = ref.qpsk_preamble(L, seed=L)
    bank = gpu.CorrelatorBank(p[None, :])
    hop = bank.plan(L, "valid")[1]
    n = 3 * hop + 77
    s, _ = xb.planted(L, n, [0.0], 0, hop + 11, seed=5)
    st = dev(s)
    c, pk = run(bank, st, mode)
    idx, peak, s1, s2 = records(bank, pk)
    single = gpu.Correlator(p)
    out = torch.empty(bank.out_len(n, mode), dtype=torch.complex64, device="cuda")
    _, rec = single(st, mode, out=out)
    torch.cuda.synchronize()
    wpeak, widx, ws1, ws2 = gpu.dsp._read_peak(rec)
    w = out.cpu().numpy()
    e = np.abs(c[0] - w).max() / np.abs(w).max()
    print(f"L={L} {mode}: c {e:.2e} idx {idx[0]} / {widx} peak {peak[0] / wpeak - 1:.2e} "
          f"sum_abs {s1[0] / ws1 - 1:.2e} sum_abs2 {s2[0] / ws2 - 1:.2e}")
    assert e <= 1e-5
    assert idx[0] == widx == hop + 11 + (L - 1 if mode == "full" else 0)
    assert abs(peak[0] / wpeak - 1) <= 1e-5
    assert abs(s1[0] / ws1 - 1) <= 1e-5 and abs(s2[0] / ws2 - 1) <= 1e-5


# ------------------------------------------------------------- 6. front end
FE_L, FE_N, FE_START = 1024, 20000, 6000


def _built(gpu, packet, f, sigma, seed):
    """build_vector's output for one instance of packet at freq_shift f, plus
    complex noise of sigma per component; the packet's first sample."""
    cfg = dict(signal=packet, freq_shift=f, period=1.0, start_time=FE_START / SR)
    vl = (FE_N + 0.5) / SR
    start = gpu.vector_plan([cfg], vl, SR).places[0][0]
    v, _ = gpu.build_vector([cfg], vl, SR)
    assert v.shape == (FE_N,) and start == FE_START
    rng = np.random.default_rng(seed)
    return (v + sigma * (rng.standard_normal(FE_N) + 1j * rng.standard_normal(FE_N))).astype(np.complex64), start


def test_frequency_search_finds_offset_and_start(gpu):
    p = ref.qpsk_preamble(FE_L, seed=FE_L)
    step = xb.default_step(SR, FE_L)
    v, start = _built(gpu, p, 3 * step, 0.1, 61)
    fs = gpu.frequency_search(v, p, SR, max_offset=4 * step)
    want = xb.frequency_search_ref(v, p, SR, xb.offset_grid(4 * step, step))
    print("on grid:", fs.offset_hz, fs.lag, fs.peak, fs.confidence, "ref", want[:3])
    assert np.array_equal(fs.offsets, np.arange(-4, 5) * step)
    assert fs.offset_hz == 3 * step == want[0] and fs.lag == start == want[1]
    assert abs(fs.peak / want[2] - 1) <= 1e-5 and fs.confidence == 1.0
    assert np.all(fs.lags[6:9] == start) and np.all(want[3][6:9] == start)   # 0.64, 1, 0.64 of the peak
    assert np.all(np.abs(fs.peaks / want[4] - 1) <= 1e-5)
    assert fs.peaks.shape == fs.lags.shape == fs.confidences.shape == (9,)
    # the same from an explicit grid, in 'full' mode, on device tensors
    ft = gpu.frequency_search(dev(v), dev(p), SR, offsets=fs.offsets, mode="full")
    assert ft.offset_hz == fs.offset_hz and ft.lag == start
    fn = gpu.frequency_search(v, p, SR, offsets=fs.offsets, mode="full")
    assert np.array_equal(fn.peaks, ft.peaks) and np.array_equal(fn.lags, ft.lags)
    assert np.array_equal(fn.confidences, ft.confidences)
    # half-way between two grid points: one of the two, sinc(1/4) = 0.90 of the peak
    vh, _ = _built(gpu, p, 2.5 * step, 0.1, 62)
    fh = gpu.frequency_search(vh, p, SR, max_offset=4 * step)
    print("half way:", fh.offset_hz / step, fh.lag, fh.peak / fs.peak)
    assert fh.offset_hz in (2 * step, 3 * step) and fh.lag == start
    assert fh.peak >= 0.85 * fs.peak


def test_frequency_search_correlates_max_template_samples(gpu):
    p = ref.qpsk_preamble(3000, seed=9)
    step = xb.default_step(SR, 512)
    v, start = _built(gpu, p, -2 * step, 0.1, 63)
    fs = gpu.frequency_search(v, p, SR, max_offset=3 * step, max_template=512)
    assert len(fs.offsets) == 7 and fs.offset_hz == -2 * step and fs.lag == start
    assert abs(fs.peak / 512 - 1) < 0.05


def test_find_packet_location_with_offset(gpu):
    """Noise of sigma 2 per component: |c| of noise is Rayleigh of scale
    2 sqrt(1024) = 64, its maximum over 2e4 lags about 64 sqrt(2 ln 2e4) = 285,
    a z-score of (4.45 - 1.25) / 0.655 = 4.9.  On frequency the peak is 1024
    (z = 22: confidence clipped to 1); 3 steps off it is sinc(1.5) = 0.21 of
    that, 217, under the noise maximum: the plain search locks onto noise with
    a confidence near 0.49."""
    pkt = ref.qpsk_preamble(3000, seed=77)
    seg = pkt[500:500 + FE_L]
    step = xb.default_step(SR, FE_L)
    v0, start = _built(gpu, pkt, 0.0, 2.0, 12)
    plain = gpu.find_packet_location_in_vector(v0, pkt, seg)
    loc, f, conf = gpu.find_packet_location_with_offset(v0, pkt, seg, SR, 4 * step)
    print("offset 0:", plain, (loc, f, conf))
    assert loc == plain[0] == start and f == 0.0 and conf == plain[2] == 1.0
    v3, _ = _built(gpu, pkt, 3 * step, 2.0, 12)
    plain = gpu.find_packet_location_in_vector(v3, pkt, seg)
    loc, f, conf = gpu.find_packet_location_with_offset(v3, pkt, seg, SR, 4 * step)
    print("offset 3 steps:", plain, (loc, f, conf))
    assert plain[0] != start and plain[2] <= 0.6
    assert loc == start and f == 3 * step and conf >= 0.99
    loc, f, _ = gpu.find_packet_location_with_offset(v3, pkt, seg, SR, 4 * step,
                                                     search_window=(2000, 15000))
    assert loc == start and f == 3 * step


# ---------------------------------------------------------------- 7. errors
def _create(ctx, K, L, rows=None):
    rows = np.zeros((max(K, 1), max(L, 1)), np.complex64) if rows is None else rows
    h = C.c_void_p()
    rc = ctx.lib.vsig_xcorr_bank_create(ctx.h, rows.ctypes.data_as(C.c_void_p), K, L, C.byref(h))
    return rc, h, ctx.lib.vsig_last_error(ctx.h).decode()


def test_error_codes_and_texts(gpu):
    ctx = gpu.get_context()
    E_INVALID, E_UNSUPPORTED = -1, -4
    rc, h, msg = _create(ctx, 1, 4097)
    assert rc == E_UNSUPPORTED and not h.value and "4096" in msg, msg
    rc, h, msg = _create(ctx, 0, 16)
    assert rc == E_INVALID and not h.value and "K" in msg, msg
    rc, h, msg = _create(ctx, 4097, 16)
    assert rc == E_INVALID and not h.value and "4096" in msg, msg
    rc, h, msg = _create(ctx, 1, 0)
    assert rc == E_INVALID and not h.value, msg
    assert ctx.lib.vsig_xcorr_bank_create(ctx.h, None, 1, 16, C.byref(h)) == E_INVALID
    rc, h, msg = _create(ctx, 2, 16)
    assert rc == 0 and h.value
    try:
        s = torch.zeros(64, dtype=torch.complex64, device="cuda")
        pk = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
        exe = ctx.lib.vsig_xcorr_bank_exec_dev
        sp, pp = C.c_void_p(s.data_ptr()), C.c_void_p(pk.data_ptr())
        assert exe(h, sp, 15, _lib.MODES["valid"], None, pp) == E_INVALID         # nout < 1
        assert "shorter" in ctx.lib.vsig_last_error(ctx.h).decode()
        assert exe(h, sp, 0, _lib.MODES["full"], None, pp) == E_INVALID
        assert exe(h, sp, 64, _lib.MODES["same"], None, pp) == E_INVALID
        assert exe(h, None, 64, _lib.MODES["valid"], None, pp) == E_INVALID
        assert exe(h, sp, 64, _lib.MODES["valid"], None, None) == E_INVALID       # records are required
        M, hop, nb, grid = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        plan = ctx.lib.vsig_xcorr_bank_plan
        assert plan(h, 15, 0, C.byref(M), C.byref(hop), C.byref(nb), C.byref(grid)) == E_INVALID
        assert plan(h, 64, 0, C.byref(M), C.byref(hop), C.byref(nb), C.byref(grid)) == 0
        assert (M.value, hop.value, nb.value, grid.value) == (4096, 4081, 1, 1)
        assert exe(h, sp, 64, _lib.MODES["valid"], None, pp) == 0
        torch.cuda.synchronize()
        assert not pk.cpu().numpy().any()                                         # zeros in, (0, 0, 0, 0) out
    finally:
        ctx.lib.vsig_xcorr_bank_free(h)
    with pytest.raises(NotImplementedError, match="4096"):
        gpu.CorrelatorBank(torch.zeros((1, 4097), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):
        gpu.CorrelatorBank(np.zeros((2, 16), np.complex64))(torch.zeros(8, dtype=torch.complex64, device="cuda"))
