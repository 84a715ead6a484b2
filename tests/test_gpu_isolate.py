"""GPU tests of the burst isolation (vsig_isolate_run, isolate_packets): which
frame owns which output, two filters in one workgroup, a long phase,
determinism, NaN, memory bounds, graph capture and the front end's round trip.

Tolerance throughout: max |z_gpu - z_ref| / max |z_ref| <= 1e-5 per segment (the
FIR's bar, tests/test_gpu_mixfir.py::_close: the same kernel body)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import accuracy_ref as acc
import isolate_ref as iso
from guard_arena import Case, In, Out, run
from vector_amd import _lib
from vector_amd import packets as pk

pytestmark = pytest.mark.gpu

TOL = 1e-5
SR = 56e6
P = C.c_void_p
SKEW2 = [(0, 0), (1, 0), (0, 1), (1, 1)]          # (input, output) skew in elements


def ptr(t):
    return P(t.data_ptr())


def table(starts, lens, freqs, filters):
    t = np.zeros(len(starts), pk.ISOLATE_SEG_DTYPE)
    t["start"], t["len"], t["freq"], t["filter"] = starts, lens, freqs, filters
    return t


class IsoPlan:
    """vsig_isolate_create / _free around a block."""

    def __init__(self, gpu, tab, n, taps, sr):
        self.gpu, self.ctx = gpu, gpu.get_context()
        self.tab = tab
        taps = np.ascontiguousarray(np.atleast_2d(taps), np.float32)
        self.h = P()
        self.ctx.check(self.ctx.lib.vsig_isolate_create(
            self.ctx.h, tab.ctypes.data_as(C.POINTER(_lib.IsolateSeg)), tab.size, n,
            taps.ctypes.data_as(C.POINTER(C.c_float)), taps.shape[0], taps.shape[1], sr, C.byref(self.h)), "create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.lib.vsig_isolate_free(self.h)

    def info(self):
        """(out_total, frames, blocks, hop)"""
        v = [C.c_int64() for _ in range(4)]
        self.ctx.check(self.ctx.lib.vsig_isolate_info(self.h, *(C.byref(a) for a in v)), "info")
        return tuple(a.value for a in v)

    def offsets(self):
        off = np.zeros(self.tab.size + 1, np.int64)
        self.ctx.check(self.ctx.lib.vsig_isolate_offsets(self.h, off.ctypes.data_as(C.POINTER(C.c_int64))), "offsets")
        return off

    def run(self, xd, y=None):
        y = torch.empty(self.info()[0], dtype=torch.complex64, device="cuda") if y is None else y
        self.gpu.get_context()                     # binds the context to the current stream
        self.ctx.check(self.ctx.lib.vsig_isolate_run(self.h, ptr(xd), ptr(y)), "run")
        return y


def plan_hop(gpu, T):
    with IsoPlan(gpu, table([0], [1], [0.0], [0]), 1, np.ones((1, T), np.float32), 1.0) as p:
        return p.info()[3]


def check_segments(got, off, x, tab, taps, sr, what):
    worst = 0.0
    for k, s in enumerate(tab):
        want = iso.isolate(x, int(s["start"]), int(s["start"] + s["len"]), float(s["freq"]), taps[s["filter"]], sr)
        err = iso.rel_err(got[off[k]:off[k + 1]], want)
        worst = max(worst, err)
        assert err <= TOL, f"{what}: segment {k} {s}: error {err:.3e}"
    return worst


# ---------------------------------------------------------------------------
# T1. frame ownership (and T4, T5 on the same plan)
# ---------------------------------------------------------------------------
N1 = 10_007


def ownership_case(T, hop):
    """Lengths around the hop; starts at 0 (left zero fill), ending at n - 1
    (right zero fill), odd, overlapping, repeated; shuffled."""
    n = N1
    segs = [(4001, 1), (n - 2, 2), (17, hop - 1), (n - hop, hop), (3001, hop + 1), (1000, 2 * hop - 1),
            (1500, 2 * hop), (0, 2 * hop + 1), (5000, 3 * hop + 1),
            (3001, hop + 1),                      # the fifth again
            (5003, 2 * hop - 1)]                  # inside the ninth
    rng = np.random.default_rng(T)
    freqs = rng.uniform(-0.45, 0.45, len(segs)) * SR
    filters = rng.integers(0, 2, len(segs))
    freqs[9], filters[9] = freqs[4], filters[4]
    order = rng.permutation(len(segs))
    taps = np.stack([pk.design_lowpass(SR / 20, SR, T), rng.standard_normal(T).astype(np.float32) / np.sqrt(T)])
    tab = table([segs[i][0] for i in order], [segs[i][1] for i in order], freqs[order], filters[order])
    twin = (int(np.flatnonzero(order == 4)[0]), int(np.flatnonzero(order == 9)[0]))
    return acc.noise(n, seed=100 + T), tab, taps, twin


@functools.lru_cache(maxsize=None)
def ownership_run(T):
    """One plan, two runs on the clean capture: (x, tab, taps, twin, offsets, frames, y, y again)."""
    import vector_amd as gpu
    hop = plan_hop(gpu, T)
    assert hop == 1025 - T
    x, tab, taps, twin = ownership_case(T, hop)
    xd = torch.from_numpy(x).cuda()
    with IsoPlan(gpu, tab, N1, taps, SR) as plan:
        total, frames, blocks, hop2 = plan.info()
        off = plan.offsets()
        y0 = plan.run(xd).cpu().numpy()
        y1 = plan.run(xd).cpu().numpy()
    fr = pk.isolate_frames(tab["start"], tab["len"], T)
    assert hop2 == hop == fr.hop and frames == fr.seg.size and blocks == (frames + 1) // 2
    assert total == fr.offsets[-1] and np.array_equal(off, fr.offsets)
    for a in (x, y0, y1):
        a.setflags(write=False)
    return x, tab, taps, twin, off, fr, y0, y1


@pytest.mark.parametrize("T", [255, 3, 63, 511])
def test_frame_ownership(gpu, T):
    x, tab, taps, twin, off, fr, y, _ = ownership_run(T)
    assert fr.seg.size % 2 == 1, "the last workgroup must hold one frame"
    err = check_segments(y, off, x, tab, taps, SR, f"T={T}")
    print(f"T={T}: frames {fr.seg.size}, worst segment error {err:.3e}")
    a, b = twin                                    # the repeated segment agrees sample for sample
    assert np.array_equal(y[off[a]:off[a + 1]], y[off[b]:off[b + 1]])


def test_determinism(gpu):
    """Two runs of one plan, and a second plan of the same table, give the same bytes."""
    x, tab, taps, _, off, _, y0, y1 = ownership_run(255)
    assert np.array_equal(y0.view(np.uint8), y1.view(np.uint8))
    with IsoPlan(gpu, tab, N1, taps, SR) as plan:
        y2 = plan.run(torch.from_numpy(x.copy()).cuda()).cpu().numpy()
    assert np.array_equal(y0.view(np.uint8), y2.view(np.uint8))


def test_nan_poisons_the_frames_that_hold_it(gpu):
    """A NaN at capture index i: every output of every frame whose input window
    holds i is non-finite, every other frame's outputs keep their bits."""
    x, tab, taps, _, off, fr, clean, _ = ownership_run(255)
    lo, hi = np.maximum(fr.x0, 0), np.minimum(fr.x0 + iso.M, N1)
    K = tab.size
    for i in range(0, N1, 97):                     # the planner says which segments an index touches
        hit = (lo <= i) & (i < hi)
        segs_hit = np.unique(fr.seg[hit])
        if segs_hit.size >= 2 and K - segs_hit.size >= 2:
            break
    else:
        pytest.fail("no index with two segments on each side")
    bad = x.copy()
    bad[i] = np.nan
    with IsoPlan(gpu, tab, N1, taps, SR) as plan:
        y = plan.run(torch.from_numpy(bad).cuda()).cpu().numpy()
    for f in range(fr.seg.size):
        a, b = clean[fr.y0[f]:fr.y0[f] + fr.keep[f]], y[fr.y0[f]:fr.y0[f] + fr.keep[f]]
        if hit[f]:
            assert not np.isfinite(b).any(), f"frame {f} holds the NaN"
        else:
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"frame {f} does not hold the NaN"
    untouched = [k for k in range(K) if k not in segs_hit]
    assert len(untouched) >= 2
    for k in untouched:
        assert np.array_equal(clean[off[k]:off[k + 1]].view(np.uint8), y[off[k]:off[k + 1]].view(np.uint8))
    assert any(np.isnan(y[off[k]:off[k + 1]]).any() for k in segs_hit)


# ---------------------------------------------------------------------------
# T2. two filters in one workgroup
# ---------------------------------------------------------------------------
def test_two_filters_in_one_workgroup(gpu):
    T = 255
    hop = plan_hop(gpu, T)
    n, K = 20_000, 12
    taps = np.stack([pk.design_lowpass(SR / 50, SR, T), pk.design_lowpass(SR / 8, SR, T), pk.design_lowpass(SR, SR, T)])
    assert np.count_nonzero(taps[2]) == 1
    freqs = np.array([(-1.0) ** k * (k + 1) * 1.7e6 for k in range(K)])
    freqs[4], freqs[7], freqs[10] = 0.0, SR / 2 * (1 - 1e-6), -SR / 2 * (1 - 1e-6)
    filters = np.arange(K) % 3                     # a pair's frames (2b, 2b + 1) differ in filter and frequency
    tab = table([3 + 1500 * k for k in range(K)], [hop // 2] * K, freqs, filters)
    assert all(filters[2 * b] != filters[2 * b + 1] and freqs[2 * b] != freqs[2 * b + 1] for b in range(K // 2))
    x = acc.noise(n, seed=2)
    with IsoPlan(gpu, tab, n, taps, SR) as plan:
        assert plan.info()[1] == K                 # one frame a segment
        y = plan.run(torch.from_numpy(x).cuda()).cpu().numpy()
        err = check_segments(y, plan.offsets(), x, tab, taps, SR, "two filters")
    print(f"two filters: worst segment error {err:.3e}")


# ---------------------------------------------------------------------------
# T3. long phase
# ---------------------------------------------------------------------------
def test_long_phase(gpu):
    """2^23 samples at sr = 1: |theta| reaches 2^23 * 2 pi * 0.31 (the phase is
    reduced in double before the fp32 rotation)."""
    n = 1 << 23
    x = acc.noise(n, seed=3)
    taps = scipy.signal.firwin(255, 0.3).astype(np.float32)[None, :]
    tab = table([n - 5000], [5000], [0.31], [0])
    with IsoPlan(gpu, tab, n, taps, 1.0) as plan:
        y = plan.run(torch.from_numpy(x).cuda()).cpu().numpy()
        err = check_segments(y, plan.offsets(), x, tab, taps, 1.0, "long phase")
    print(f"long phase: error {err:.3e}")


# ---------------------------------------------------------------------------
# T6. memory bounds
# ---------------------------------------------------------------------------
def test_bounds_isolate_run(gpu):
    """x is read inside [0, n) only -- and nowhere outside the union of the
    frames' windows --, y is written at [0, out_total) exactly, x is not written."""
    T, n = 255, 6000
    ctx = gpu.get_context()
    tab = table([0, n - 500, 2900], [300, 500, 1], [3e6, -11e6, 0.0], [0, 1, 0])
    taps = np.stack([pk.design_lowpass(2e6, SR, T), pk.design_lowpass(SR / 8, SR, T)])
    x = acc.noise(n, seed=6)
    fr = pk.isolate_frames(tab["start"], tab["len"], T)
    used = np.zeros(n, bool)
    for x0 in fr.x0:
        used[max(0, x0):min(n, x0 + iso.M)] = True
    assert used[0] and used[-1] and not used.all()
    refs = [iso.isolate(x, int(s["start"]), int(s["start"] + s["len"]), float(s["freq"]), taps[s["filter"]], SR)
            for s in tab]
    with IsoPlan(gpu, tab, n, taps, SR) as plan:
        total, off = plan.info()[0], plan.offsets()

        def call(p):
            return ctx.lib.vsig_isolate_run(plan.h, P(p["x"]), P(p["y"]))

        def check(o):
            for k, want in enumerate(refs):
                err = iso.rel_err(o["y"][off[k]:off[k + 1]], want)
                assert err <= TOL, f"segment {k}: error {err:.3e}"
        for si, so in SKEW2:
            run(Case("vsig_isolate_run", f"T={T} n={n} skew=({si},{so})", {"x": In(x, 8 * si, holes=~used)},
                     {"y": Out(total, np.complex64, 8 * so)}, call, check))


# ---------------------------------------------------------------------------
# T7. capture
# ---------------------------------------------------------------------------
def test_run_captures_into_a_graph(gpu):
    """vsig_isolate_run neither allocates nor synchronises: one capture on a
    single stream, replayed twice on new contents, gives the bytes of plain calls."""
    T = 255
    x, tab, taps, _ = ownership_case(T, 1025 - T)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(x).cuda()
        with IsoPlan(gpu, tab, N1, taps, SR) as plan:
            y = torch.zeros(plan.info()[0], dtype=torch.complex64, device="cuda")
            plan.run(xd, y)
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                plan.run(xd, y)
            for shift in (4321, 77):
                new = np.roll(x, shift) * np.float32(0.5)
                xd.copy_(torch.from_numpy(new))
                y.zero_()
                graph.replay()
                stream.synchronize()
                replayed = y.cpu().numpy().copy()
                y.zero_()
                plan.run(xd, y)
                stream.synchronize()
                assert np.array_equal(replayed.view(np.uint8), y.cpu().numpy().view(np.uint8))
                assert np.abs(replayed).min() > 0
            del graph


# ---------------------------------------------------------------------------
# T8. front end, round trip
# ---------------------------------------------------------------------------
FE_N, FE_L = 20_000, 3000


def _packet(seed):
    """3000 samples of 2 MHz band-limited complex noise, peak-normalised."""
    rng = np.random.default_rng(seed)
    h = scipy.signal.firwin(129, 1e6, fs=SR)
    w = rng.standard_normal(FE_L + 128) + 1j * rng.standard_normal(FE_L + 128)
    p = np.convolve(w, h, "valid")
    return p / np.abs(p).max()


def _capture(places):
    """Noise floor 1e-3 and the packets mixed to their carriers (global phase)."""
    rng = np.random.default_rng(99)
    x = 1e-3 * (rng.standard_normal(FE_N) + 1j * rng.standard_normal(FE_N)) * np.sqrt(0.5)
    t = np.arange(FE_N) / SR
    for p, at, f in places:
        x[at:at + FE_L] += p * np.exp(2j * np.pi * f * t[at:at + FE_L])
    return x.astype(np.complex64)


def rho(z, p, pre):
    z = np.asarray(z[pre:pre + FE_L], np.complex128)
    return abs(np.vdot(p, z)) / (np.linalg.norm(z) * np.linalg.norm(p))


def test_isolate_packets_round_trip(gpu):
    p = [_packet(11), _packet(12)]
    fs = [8e6, -6e6]
    at = [4000, 5000]                              # 2000 samples of time overlap
    x = _capture(list(zip(p, at, fs)))
    starts, ends = np.array(at), np.array(at) + FE_L - 1
    out = gpu.isolate_packets(x, (starts, ends), SR, freqs=fs, bandwidths=[2e6, 2e6], pre_samples=100,
                              post_samples=50)
    assert isinstance(out, pk.IsolatedPackets) and len(out.packets) == 2
    assert out.pre.tolist() == [100, 100] and out.center_freq.tolist() == fs and out.bandwidth.tolist() == [2e6, 2e6]
    assert np.all(out.cutoff == 1e6 + 1.65 * SR / 255)
    h = pk.design_lowpass(2e6, SR, 255)
    for k in range(2):
        z = out.packets[k]
        assert isinstance(z, np.ndarray) and z.dtype == np.complex64 and z.shape == (FE_L + 150,)
        lo, hi = at[k] - 100, at[k] + FE_L + 50
        want = iso.isolate(x, lo, hi, fs[k], h, SR)
        err = iso.rel_err(z, want)
        mixed = iso.isolate(x, lo, hi, fs[k], [0.0, 1.0, 0.0], SR)       # mixed, not filtered
        r, r_ref, r_mix = rho(z, p[k], 100), rho(want, p[k], 100), rho(mixed, p[k], 100)
        print(f"packet {k}: rho {r:.4f} (float64 reference {r_ref:.4f}, mix only {r_mix:.4f}), error {err:.3e}")
        assert err <= TOL
        assert r >= 0.99 and r > r_mix
    assert out.packets[0].base is out.packets[1].base is not None       # views into one packed buffer


def test_isolate_packets_forms(gpu):
    p = _packet(11)
    x = _capture([(p, 4000, 8e6)])
    # pre is clamped at the capture's start
    out = gpu.isolate_packets(x, ([20], [500]), SR, freqs=[8e6], bandwidths=[2e6], pre_samples=100, post_samples=50)
    assert out.pre.tolist() == [20] and out.packets[0].shape == (551,)
    want = iso.isolate(x, 0, 551, 8e6, pk.design_lowpass(2e6, SR, 255), SR)
    assert iso.rel_err(out.packets[0], want) <= TOL
    # and post at its end
    out = gpu.isolate_packets(x, ([FE_N - 300], [FE_N - 10]), SR, freqs=[8e6], bandwidths=[2e6], post_samples=50)
    assert out.pre.tolist() == [0] and out.packets[0].shape == (300,)
    # a device tensor in gives device views
    xd = torch.from_numpy(x).cuda()
    host = gpu.isolate_packets(x, ([4000, 100], [6999, 900]), SR, freqs=[8e6, 1e6], bandwidths=[2e6, SR])
    dev = gpu.isolate_packets(xd, ([4000, 100], [6999, 900]), SR, freqs=[8e6, 1e6], bandwidths=[2e6, SR])
    assert all(isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.complex64 for z in dev.packets)
    assert dev.packets[0].untyped_storage().data_ptr() == dev.packets[1].untyped_storage().data_ptr()
    for a, b in zip(host.packets, dev.packets):
        assert np.array_equal(a, b.cpu().numpy())
    assert isinstance(dev.pre, np.ndarray) and isinstance(dev.cutoff, np.ndarray)
    # a PacketMeasurements is used as given; an unmeasurable burst is the plain slice
    m2 = gpu.measure_packets(x, ([4000, 10], [6999, 40]), SR, nperseg=1024)
    assert np.isnan(m2.center_freq[1])
    out = gpu.isolate_packets(x, ([4000, 10], [6999, 40]), SR, measurements=m2)
    assert np.isnan(out.cutoff[1]) and not np.isnan(out.cutoff[0])
    assert iso.rel_err(out.packets[1], x[10:41].astype(np.complex128)) <= TOL
    # no burst: empty lists
    out = gpu.isolate_packets(xd, (np.zeros(0, np.int64), np.zeros(0, np.int64)), SR)
    assert out.packets == [] and out.pre.size == 0 and out.cutoff.size == 0


def test_default_path_measures_the_centre(gpu):
    """No freqs: measure_packets (its defaults) finds the centre and the band of
    a single burst, within one of its bins (sr / 1024) of +8 MHz.

    The isolated burst is then the packet at the residual offset delta = 8 MHz -
    centre, so rho is taken against the packet mixed by delta.  Against the
    packet itself a residual of a fraction of a bin already decorrelates the two
    (|sinc(delta * 3000 / sr)|: 0.99 needs |delta| < 1.5 kHz, a bin is 54.7 kHz;
    the centroid of 2 frames of 2 MHz noise scatters by tens of kHz), whatever the
    filter does: on the MI355X the centre came back as 8 038 173 Hz and the
    uncompensated figure was 0.103; both are printed."""
    p = _packet(11)
    x = _capture([(p, 4000, 8e6)])
    out = gpu.isolate_packets(x, ([4000], [6999]), SR)
    m = gpu.measure_packets(x, ([4000], [6999]), SR)
    assert pk.default_nperseg([FE_L]) == 1024                           # measure_packets' bin: SR / 1024
    assert abs(out.center_freq[0] - 8e6) <= SR / 1024 and out.center_freq[0] == m.center_freq[0]
    assert out.bandwidth[0] == m.bandwidth[0] and out.cutoff[0] == m.bandwidth[0] / 2 + 1.65 * SR / 255
    delta = 8e6 - out.center_freq[0]
    residual = p * np.exp(2j * np.pi * delta * np.arange(4000, 4000 + FE_L) / SR)
    r, r_plain = rho(out.packets[0], residual, 0), rho(out.packets[0], p, 0)
    print(f"default path: centre {out.center_freq[0]:.0f} Hz, bandwidth {out.bandwidth[0]:.0f} Hz, rho {r:.4f} "
          f"(against the packet without the residual {delta:.0f} Hz: {r_plain:.4f})")
    want = iso.isolate(x, 4000, 7000, out.center_freq[0], pk.design_lowpass(out.bandwidth[0], SR, 255), SR)
    assert iso.rel_err(out.packets[0], want) <= TOL
    assert r >= 0.99


def test_c_abi_errors(gpu):
    ctx = gpu.get_context()
    good = table([0], [10], [1e6], [0])
    taps = np.ones((1, 255), np.float32)

    def create(tab, n=100, taps=taps, sr=SR, nf=None, T=None):
        h = P()
        rc = ctx.lib.vsig_isolate_create(ctx.h, tab.ctypes.data_as(C.POINTER(_lib.IsolateSeg)), tab.size, n,
                                         taps.ctypes.data_as(C.POINTER(C.c_float)),
                                         taps.shape[0] if nf is None else nf, taps.shape[1] if T is None else T, sr,
                                         C.byref(h))
        if rc == 0:
            ctx.lib.vsig_isolate_free(h)
        return rc, ctx.lib.vsig_last_error(ctx.h).decode()
    assert create(good)[0] == 0
    for tab, word in ((table([0], [0], [0.0], [0]), "segment 0"), (table([0, 95], [10, 6], [0.0, 0.0], [0, 0]), "segment 1"),
                      (table([-1], [5], [0.0], [0]), "segment 0"), (table([0], [5], [0.0], [1]), "filter"),
                      (table([0], [5], [np.nan], [0]), "freq"), (table([0], [5], [np.inf], [0]), "freq")):
        rc, msg = create(tab)
        assert rc == -1 and word in msg, (rc, msg)
    assert create(good, sr=0.0)[0] == -1 and create(good, sr=np.inf)[0] == -1 and create(good, n=0)[0] == -1
    assert create(good, T=254)[0] == -1 and create(good, T=1)[0] == -1 and create(good, nf=0)[0] == -1
    big = np.ones((1, 513), np.float32)
    assert create(good, taps=big)[0] == -4
    bad = taps.copy()
    bad[0, 7] = np.nan
    assert create(good, taps=bad)[0] == -1
    # an empty table is a valid plan that does nothing
    with IsoPlan(gpu, table([], [], [], []), 100, taps, SR) as plan:
        assert plan.info() == (0, 0, 0, 770) and plan.offsets().tolist() == [0]
        y = torch.full((4,), 7, dtype=torch.complex64, device="cuda")
        plan.run(y, y)
        assert torch.all(y == 7)
    with IsoPlan(gpu, good, 100, taps, SR) as plan:
        xd = torch.zeros(101, dtype=torch.complex64, device="cuda")
        y = torch.zeros(11, dtype=torch.complex64, device="cuda")
        assert ctx.lib.vsig_isolate_run(plan.h, None, ptr(y)) == -1
        assert ctx.lib.vsig_isolate_run(plan.h, P(xd.data_ptr() + 4), ptr(y)) == -1
        assert ctx.lib.vsig_isolate_run(plan.h, ptr(xd), P(y.data_ptr() + 4)) == -1
