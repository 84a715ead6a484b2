"""The parity-split form of the M = 16384 correlator (xcorr.hip, PS) on the
GPU against a complex128 valid correlation on the CPU: 1 to 4 blocks at
L = 4096 (hop 12288), peaks planted on even and odd outputs, the first and
last output, around a block seam and in a short last block; exact ties
inside one thread column (outputs 2 (m + 256 rank) + parity); L = 4097 (same
hop) and L = 3000 (run-time epilogue split); and a stream view one sample
off 16-byte alignment, which takes the split by halves.

Bars: the lag exact; max |c| (refined: numpy's complex128 dot) at 1e-12
against the direct dot, and max |c|, sum |c|, sum |c|^2 at the project's
rel 1e-5 against the reference correlation (test_gpu_chain.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref

pytestmark = pytest.mark.gpu

HOP = 12288                 # M - L + 1 rounded down to even, L = 4096 / 4097


def _valid_corr128(s, t):
    """np.correlate(s, t, 'valid') in complex128 by np.fft (error ~1e-15 of the max)."""
    n = len(s) + len(t) - 1
    nf = 1 << (n - 1).bit_length()
    S = np.fft.fft(s.astype(np.complex128), nf)
    T = np.fft.fft(np.conj(t.astype(np.complex128)[::-1]), nf)
    return np.fft.ifft(S * T)[len(t) - 1: len(s)]


@functools.lru_cache(maxsize=None)
def _case(L, ns, lag, seed=0):
    """(template, stream, reference |c|): noise with 4 x the template at `lag`."""
    pre = ref.qpsk_preamble(L, seed=L + seed)
    s = ref.synth_iq(ns, seed=ns + lag + seed)
    s[lag:lag + L] += 4 * pre
    return pre, s, np.abs(_valid_corr128(s, pre))


def _run(gpu, pre, sdev, out=None):
    xc = gpu.Correlator(pre)
    _, pk = xc(sdev, "valid", out=out)
    rec = gpu.dsp._read_peak(pk)
    gpu.dsp.check_refine()
    return rec


def _check(rec, pre, s, a, lag):
    m, idx, s1, s2 = rec
    assert int(np.argmax(a)) == lag            # the reference's own peak is the planted one
    print(f"lag {idx} want {lag}  max {m!r} ref {a[lag]!r}  "
          f"s1 rel {s1 / a.sum() - 1:.2e}  s2 rel {s2 / (a * a).sum() - 1:.2e}")
    assert idx == lag
    direct = abs(np.vdot(pre.astype(np.complex128), s[lag:lag + len(pre)].astype(np.complex128)))
    assert m == pytest.approx(direct, rel=1e-12)
    assert m == pytest.approx(a[lag], rel=1e-5)
    assert s1 == pytest.approx(a.sum(), rel=1e-5)
    assert s2 == pytest.approx((a * a).sum(), rel=1e-5)


# ns -> nout = ns - 4095: 16383 -> one whole block; 20000 -> 12288 + 3617 (a
# last block shorter than a hop); 30000 -> two blocks + 1329; 53247 -> four.
@pytest.mark.parametrize("ns,lag", [
    (20_000, 5000), (20_000, 5001),                       # even / odd output
    (16_383, 0), (16_383, HOP - 1),                       # first / last output, one block
    (20_000, 0), (20_000, 20_000 - 4096),                 # ... with a short last block
    (30_000, HOP - 1), (30_000, HOP), (30_000, HOP + 1),  # either side of a block seam
    (20_000, 15_000), (20_000, 15_001),                   # inside the short last block
    (53_247, 3 * HOP + 4001), (53_247, 4 * HOP - 1),      # four whole blocks
])
def test_planted_peak_every_position(gpu, ns, lag):
    pre, s, a = _case(4096, ns, lag)
    _check(_run(gpu, pre, torch.from_numpy(s).cuda()), pre, s, a, lag)


@pytest.mark.parametrize("L,ns,lag", [
    (4097, 30_001, 12_289), (4097, 30_001, 12_288),       # hop 12288 again
    (3000, 30_000, 13_383), (3000, 30_000, 13_384),       # hop 13384: the run-time split,
    (3000, 30_000, 13_385), (3000, 30_000, 27_000),       #   its seam and its last output
])
def test_other_template_lengths(gpu, L, ns, lag):
    pre, s, a = _case(L, ns, lag)
    _check(_run(gpu, pre, torch.from_numpy(s).cuda()), pre, s, a, lag)


@pytest.mark.parametrize("L,ns,lag", [(4096, 30_000, HOP + 1), (4096, 30_000, 5000),
                                      (3000, 30_000, 13_385)])
def test_view_off_alignment_takes_the_other_kernel(gpu, L, ns, lag):
    """The same samples behind a 16-byte aligned base and behind one 8 bytes
    off it: the second launch cannot use 16-byte segment loads (the split by
    halves runs), and both give the reference's answer and each other's."""
    pre, s, a = _case(L, ns, lag)
    buf = torch.zeros(ns + 2, dtype=torch.complex64, device="cuda")
    buf[1:ns + 1] = torch.from_numpy(s).cuda()
    view = buf[1:ns + 1]
    assert view.data_ptr() % 16 == 8
    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0
    r0 = _run(gpu, pre, aligned)
    r1 = _run(gpu, pre, view)
    _check(r0, pre, s, a, lag)
    _check(r1, pre, s, a, lag)
    assert r0[1] == r1[1]
    assert r0[0] == r1[0]                      # both refined to numpy's value
    assert r0[2] == pytest.approx(r1[2], rel=1e-5)
    assert r0[3] == pytest.approx(r1[3], rel=1e-5)


def _mid_bucket_scale(energy):
    """Amplitude A (within 4e-6 of 1) that puts (A energy)^2 at the middle of
    a 64-ulp bucket of fp32: the kernel's argmax key drops the 6 low mantissa
    bits of |c|^2, so two outputs of that exact value tie in it whatever
    their fp32 rounding (a few ulps)."""
    v = np.float32(energy * energy)
    mid = ((v.view(np.uint32) & np.uint32(0xFFFFFFC0)) | np.uint32(32)).view(np.float32)
    return float(np.sqrt(np.float64(mid) / (energy * energy)))


def _tie_stream(pre, ns, p1, p2, quiet=9500):
    """Two bit-equal copies of the template at p1 and p2 over zeros, noise from
    `quiet` on (past both copies' windows: the sums are those of a live stream,
    the two peaks' dot products stay bit-equal)."""
    assert max(p1, p2) + len(pre) <= quiet
    e = float((np.abs(pre.astype(np.complex128)) ** 2).sum())
    s = np.zeros(ns, np.complex64)
    s[quiet:] = ref.synth_iq(ns - quiet, seed=p1 + p2)
    cp = (_mid_bucket_scale(e) * pre.astype(np.complex128)).astype(np.complex64)
    s[p1:p1 + len(pre)] = cp
    s[p2:p2 + len(pre)] = cp
    return s


def _refine(gpu, on):
    ctx = gpu.get_context()
    ctx.check(ctx.lib.vsig_set_option(ctx.h, b"refine", 1 if on else 0), "refine option")


@pytest.mark.parametrize("refine", [True, False])
def test_equal_maxima_in_one_column_first_wins(gpu, refine):
    """Two bit-equal copies of the template (_tie_stream), at outputs 2 m and
    2 (m + 256 * 9) + 1 of block 0 (thread column m = 100: an even and an odd
    output, 4609 apart so the copies do not overlap): |c| ties exactly, and
    the lower lag wins -- by the kernel's key alone (refine off) and after the
    exact re-rank (np.argmax's first maximum)."""
    L, ns = 4096, 20_000
    p1, p2 = 2 * 100, 2 * (100 + 256 * 9) + 1
    pre = ref.qpsk_preamble(L, seed=7)
    s = _tie_stream(pre, ns, p1, p2)
    a = np.abs(_valid_corr128(s, pre))
    assert a[p1] == pytest.approx(a[p2], rel=1e-12) and a[p1] > 10 * np.delete(a, [p1, p2]).max()
    _refine(gpu, refine)
    try:
        m, idx, s1, s2 = _run(gpu, pre, torch.from_numpy(s).cuda())
    finally:
        _refine(gpu, True)
    assert idx == p1
    assert m == pytest.approx(a[p1], rel=1e-5)
    assert s1 == pytest.approx(a.sum(), rel=1e-5)
    assert s2 == pytest.approx((a * a).sum(), rel=1e-5)


@pytest.mark.parametrize("refine", [True, False])
def test_equal_maxima_reversed_order_first_wins(gpu, refine):
    """The same tie with the operands swapped (np.correlate(template, stream,
    'full'): the kernel's outputs run backwards, raw = p + L - 1 for a copy at
    p).  L = 4097 keeps the segment starts 16-byte aligned (off = L - 1 even).
    Copies at raw 2 (100 + 256 * 8) and 2 (100 + 256 * 17) + 1 of block 0: the
    first maximum of the reversed space is the higher raw output."""
    L, ns = 4097, 20_000
    r1, r2 = 2 * (100 + 256 * 8), 2 * (100 + 256 * 17) + 1
    p1, p2 = r1 - (L - 1), r2 - (L - 1)
    assert p2 - p1 >= L and r2 < HOP
    pre = ref.qpsk_preamble(L, seed=8)
    s = _tie_stream(pre, ns, p1, p2)
    c, lags = ref.cross_correlate_signals(s, pre, "full")     # np.correlate(pre, s, 'full')
    want = ref.find_correlation_peak(c, lags)
    k = int(np.argmax(np.abs(c)))
    assert k == ns - 1 - p2 and np.abs(c)[ns - 1 - p1] == np.abs(c)[k]    # an exact tie in numpy
    _refine(gpu, refine)
    try:
        lag, val, _ = gpu.correlate_peak(s, pre, "full")
    finally:
        _refine(gpu, True)
    assert lag == want[0]
    assert val == pytest.approx(want[1], rel=1e-12 if refine else 1e-5)


@pytest.mark.parametrize("L,mode,swapped", [(4096, "valid", False), (4097, "full", True)])
def test_stored_correlation(gpu, L, mode, swapped):
    """The stored array of the same launches (even / odd outputs side by
    side; swapped: conj, reversed) at 1e-5 of the largest |c|."""
    pre, s, _ = _case(L, 30_000 + (L - 4096), 12_289)
    a, b = (s, pre) if swapped else (pre, s)
    c, lags = gpu.cross_correlate_signals(a, b, mode)
    r, rl = ref.cross_correlate_signals(a, b, mode)
    assert (lags == rl).all()
    assert np.abs(c - r).max() <= 1e-5 * np.abs(r).max()
