"""GPU tests of the all-pairs burst similarity (vsig_match_run, packet_similarity,
match_packets): values against the float64 definition at every transform
length, the mirror rule, determinism, independence of the list, the grid hook,
special values, memory bounds, graph capture, the C-ABI errors and the front
ends' recovery of a vector plan.

Tolerances: |rho - rho_ref| <= 1e-5 (the project's float bar), energy 1e-6
relative, lags equal wherever the reference itself is decided (rho_ref >= 0.5
and its largest |c| above the second by >= 1e-3 relative)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import match_ref as mr
from guard_arena import Case, In, Out, run
from vector_amd import match as mt
from vector_amd.packets import PacketMeasurements

pytestmark = pytest.mark.gpu

TOL_RHO, TOL_E, MARGIN = 1e-5, 1e-6, 1e-3
P = C.c_void_p


def ptr(t):
    return P(t.data_ptr())


class MatchPlan:
    """vsig_match_create / _free around a block."""

    def __init__(self, gpu, lens):
        self.gpu, self.ctx = gpu, gpu.get_context()
        self.lens = np.ascontiguousarray(lens, np.int64)
        self.K = int(self.lens.size)
        self.h = P()
        self.ctx.check(self.ctx.lib.vsig_match_create(self.ctx.h, self.lens.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      self.K, C.byref(self.h)), "create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.lib.vsig_match_free(self.h)

    def info(self):
        """(N, pairs, units, grid, workspace_bytes)"""
        n = C.c_int32()
        v = [C.c_int64() for _ in range(4)]
        self.ctx.check(self.ctx.lib.vsig_match_info(self.h, C.byref(n), *(C.byref(a) for a in v)), "info")
        return (n.value,) + tuple(a.value for a in v)

    def outputs(self):
        K = self.K
        return (torch.full((K, K), 7, dtype=torch.float32, device="cuda"),
                torch.full((K, K), 7, dtype=torch.int32, device="cuda"),
                torch.full((K,), 7, dtype=torch.float64, device="cuda"))

    def run(self, packed, out=None):
        peak, lag, energy = self.outputs() if out is None else out
        self.gpu.get_context()                     # binds the context to the current stream
        self.ctx.check(self.ctx.lib.vsig_match_run(self.h, ptr(packed), ptr(peak), ptr(lag), ptr(energy)), "run")
        return peak, lag, energy


def host(out):
    return tuple(t.cpu().numpy() for t in out)


def match_gpu(gpu, packets):
    """(peak, lag, energy) host arrays and the plan's info: one plan, one run."""
    with MatchPlan(gpu, [p.size for p in packets]) as plan:
        out = host(plan.run(torch.from_numpy(np.concatenate(packets)).cuda()))
        return out, plan.info()


def same_bytes(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def case(lmax):
    """The 15 packets at lmax, their reference, one plan run twice and a second plan."""
    import vector_amd as gpu
    pk, who = mr.emitters(lmax)
    ref = mr.match(pk)
    packed = torch.from_numpy(np.concatenate(pk)).cuda()
    with MatchPlan(gpu, [p.size for p in pk]) as plan:
        info = plan.info()
        first, second = host(plan.run(packed)), host(plan.run(packed))
    other, _ = match_gpu(gpu, pk)
    for a in first + second + other:
        a.setflags(write=False)
    return pk, who, ref, info, first, second, other


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [512, 2048, 4096, 8192])
def test_values_against_the_definition(gpu, lmax):
    pk, who, ref, info, (peak, lag, energy), _, _ = case(lmax)
    K = len(pk)
    assert K == 15 and info[0] == mt.match_size(lmax) == {512: 1024, 2048: 4096, 4096: 8192, 8192: 16384}[lmax]
    assert info[1] == K * (K - 1) // 2 and info[2] >= 1 and info[3] >= 1 and info[4] == K * info[0] * 8
    rho = mt.rho_from(peak, energy)
    e_rho = np.abs(rho - ref.rho).max()
    e_en = (np.abs(energy - ref.energy) / ref.energy).max()
    off = ~np.eye(K, dtype=bool)
    decided = off & (ref.rho >= 0.5) & (ref.margin >= MARGIN)
    same = off & (who[:, None] == who[None, :]) & (who[:, None] >= 0)
    print(f"lmax {lmax} N {info[0]} units {info[2]} grid {info[3]}: max |rho - ref| {e_rho:.3e}, energy {e_en:.3e}, "
          f"lags compared {np.count_nonzero(np.triu(decided))}, same-emitter pairs "
          f"{np.count_nonzero(np.triu(same))}, their min margin {ref.margin[same].min():.3f}")
    assert e_rho <= TOL_RHO and e_en <= TOL_E
    assert np.count_nonzero(np.triu(same)) == 18 and np.all(decided[same]), "the filter leaves out a same-emitter pair"
    assert np.array_equal(lag[decided], ref.lag[decided])
    assert np.all(rho[same] >= 0.9) and np.all(rho[off & ~same & (who[:, None] >= 0) & (who[None, :] >= 0)] < 0.5)


def test_mirror_diagonal_and_lag_range(gpu):
    pk, _, ref, _, (peak, lag, energy), _, _ = case(512)
    assert np.array_equal(peak.view(np.uint32), peak.T.copy().view(np.uint32)) and np.array_equal(lag, -lag.T)
    assert np.array_equal(np.diag(peak), energy.astype(np.float32)) and np.all(np.diag(lag) == 0)
    L = np.array([p.size for p in pk])
    assert np.all(lag <= L[:, None] - 1) and np.all(lag >= -(L[None, :] - 1))


def test_same_bytes_twice_and_from_a_second_plan(gpu):
    for lmax in (512, 2048):
        _, _, _, _, first, second, other = case(lmax)
        assert same_bytes(first, second) and same_bytes(first, other)


def test_a_pair_does_not_depend_on_the_list(gpu):
    """Record (a, b) from a list of the two packets alone (a < b kept, the same
    N: a is a longest packet) has the bits it has inside the 15."""
    pk, who, _, info, (peak, lag, energy), _, _ = case(512)
    longest = [k for k, p in enumerate(pk) if p.size == 512]
    pairs = [(a, b) for a in longest for b in range(a + 1, 15)][:4] + [(a, b) for b in longest for a in range(b)][:4]
    assert len(pairs) >= 4
    for a, b in pairs:
        (p2, l2, e2), info2 = match_gpu(gpu, [pk[a], pk[b]])
        assert info2[0] == info[0]
        assert p2[0, 1].view(np.uint32) == peak[a, b].view(np.uint32) and l2[0, 1] == lag[a, b]
        assert e2[0] == energy[a] and e2[1] == energy[b]


@pytest.mark.parametrize("K", [1, 2, 3])
def test_small_lists(gpu, K):
    rng = np.random.default_rng(K)
    base = np.exp(2j * np.pi * rng.random(100)).astype(np.complex64)
    pk = [base, base[7:], np.exp(2j * np.pi * rng.random(60)).astype(np.complex64)][:K]
    (peak, lag, energy), info = match_gpu(gpu, pk)
    ref = mr.match(pk)
    assert info[:3] == (1024, K * (K - 1) // 2, K * (K - 1) // 2)
    assert np.abs(mt.rho_from(peak, energy) - ref.rho).max() <= TOL_RHO
    assert np.abs(energy - ref.energy).max() <= TOL_E * ref.energy.max()
    if K >= 2:
        assert lag[0, 1] == 7 and lag[1, 0] == -7


def test_match_grid_hook_changes_no_byte(gpu):
    """K = 48 at L <= 512: three blocks walk all the units."""
    rng = np.random.default_rng(48)
    pk = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
          for n in rng.integers(1, 513, 48)]
    pk[5] = pk[20][2:].copy()
    ctx = gpu.get_context()
    default, info = match_gpu(gpu, pk)
    ctx.check(ctx.lib.vsig_set_option(ctx.h, b"match_grid", 3), "option")
    try:
        v = C.c_int()
        assert ctx.lib.vsig_get_option(ctx.h, b"match_grid", C.byref(v)) == 0 and v.value == 3
        capped, info3 = match_gpu(gpu, pk)
    finally:
        ctx.check(ctx.lib.vsig_set_option(ctx.h, b"match_grid", 0), "option")
    assert info[3] > 3 and info3[3] == 3 and info3[:3] == info[:3] and info[2] > 3 * 8
    assert same_bytes(default, capped)
    ref = mr.match(pk)
    assert np.abs(mt.rho_from(default[0], default[2]) - ref.rho).max() <= TOL_RHO and default[1][20, 5] == 2
    assert ctx.lib.vsig_set_option(ctx.h, b"match_grid", -1) == -1


# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------
def test_nan_inf_and_zero_packets(gpu):
    pk, who, _, _, clean, _, _ = case(512)
    k = int(np.flatnonzero(who == 1)[0])            # a packet with partners of its own emitter
    for what in ("nan_inf", "zero"):
        bad = [p.copy() for p in pk]
        if what == "zero":
            bad[k][:] = 0
        else:
            bad[k][3] = np.nan
            bad[k][bad[k].size // 2] = np.inf
        (peak, lag, energy), _ = match_gpu(gpu, bad)
        others = np.ones(15, bool)
        others[k] = False
        if what == "zero":
            assert energy[k] == 0 and np.all(peak[k] == 0) and np.all(peak[:, k] == 0)
            assert np.all(mt.rho_from(peak, energy)[k] == 0)
        else:
            assert not np.isfinite(energy[k]) and np.isnan(peak[k]).all() and np.isnan(peak[:, k]).all()
        assert np.all(lag[k] == 0) and np.all(lag[:, k] == 0)
        sub = np.ix_(others, others)
        assert same_bytes((peak[sub].copy(), lag[sub].copy(), energy[others].copy()),
                          (clean[0][sub].copy(), clean[1][sub].copy(), clean[2][others].copy())), what


# ---------------------------------------------------------------------------
# memory bounds
# ---------------------------------------------------------------------------
def test_bounds_match_run(gpu):
    """packed is read at [0, sum lens) only (the buffer's tail and the guards
    are poisoned), peak / lag / energy are written exactly."""
    ctx = gpu.get_context()
    rng = np.random.default_rng(7)
    base = np.exp(2j * np.pi * rng.random(257)).astype(np.complex64)
    pk = [base, base[5:200].copy(), np.ones(1, np.complex64), base[::-1][:130].copy(), (2 * base[:-1]).astype(np.complex64)]
    K, total, tail = len(pk), sum(p.size for p in pk), 300
    ref = mr.match(pk)
    data = np.concatenate(pk + [np.zeros(tail, np.complex64)])
    holes = np.arange(total + tail) >= total
    with MatchPlan(gpu, [p.size for p in pk]) as plan:
        def call(p):
            return ctx.lib.vsig_match_run(plan.h, P(p["packed"]), P(p["peak"]), P(p["lag"]), P(p["energy"]))

        def check(o):
            peak, lag, energy = o["peak"].reshape(K, K), o["lag"].reshape(K, K), o["energy"]
            assert np.abs(mt.rho_from(peak, energy) - ref.rho).max() <= TOL_RHO
            assert np.abs(energy - ref.energy).max() <= TOL_E * ref.energy.max()
            assert lag[0, 1] == 5 and lag[1, 0] == -5 and lag[0, 4] == 0
        for skew in range(4):
            run(Case("vsig_match_run", f"K={K} skew={skew}", {"packed": In(data, 8 * skew, holes=holes)},
                     {"peak": Out(K * K, np.float32, 4 * skew), "lag": Out(K * K, np.int32, 4 * (3 - skew)),
                      "energy": Out(K, np.float64, 8 * skew)}, call, check))


# ---------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------
def test_run_captures_into_a_graph(gpu):
    """vsig_match_run neither allocates nor synchronises: one capture on a single
    stream, replayed twice on new contents, gives the bytes of plain calls."""
    pk, _ = mr.emitters(512)
    x = np.concatenate(pk)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(x).cuda()
        with MatchPlan(gpu, [p.size for p in pk]) as plan:
            out = plan.outputs()
            plan.run(xd, out)
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                plan.run(xd, out)
            for shift in (321, 77):
                xd.copy_(torch.from_numpy(np.roll(x, shift) * np.float32(0.5)))
                for t in out:
                    t.fill_(7)
                graph.replay()
                stream.synchronize()
                replayed = host(out)
                for t in out:
                    t.fill_(7)
                plan.run(xd, out)
                stream.synchronize()
                assert same_bytes(replayed, host(out))
                assert np.all(replayed[2] > 0) and np.all(np.diag(replayed[1]) == 0)
            del graph


# ---------------------------------------------------------------------------
# C-ABI errors
# ---------------------------------------------------------------------------
def test_c_abi_errors(gpu):
    ctx = gpu.get_context()

    def create(lens, K=None, null_lens=False, null_out=False):
        lens = np.ascontiguousarray(lens, np.int64)
        h = P()
        rc = ctx.lib.vsig_match_create(ctx.h, None if null_lens else lens.ctypes.data_as(C.POINTER(C.c_int64)),
                                       lens.size if K is None else K, None if null_out else C.byref(h))
        if rc == 0:
            ctx.lib.vsig_match_free(h)
        return rc, ctx.lib.vsig_last_error(ctx.h).decode()
    assert create([5, 8192, 1])[0] == 0 and create([1])[0] == 0
    assert create([5], K=0)[0] == -1 and create(np.ones(4097), K=4097)[0] == -1 and create([5], K=-1)[0] == -1
    rc, msg = create([5, 0, 7])
    assert rc == -1 and "packet 1" in msg
    rc, msg = create([5, 7, -3])
    assert rc == -1 and "packet 2" in msg
    rc, msg = create([8193, 7])
    assert rc == -4 and "packet 0" in msg
    assert create([5], null_lens=True)[0] == -1 and create([5], null_out=True)[0] == -1
    h = P()
    one = np.ones(1, np.int64)
    assert ctx.lib.vsig_match_create(None, one.ctypes.data_as(C.POINTER(C.c_int64)), 1, C.byref(h)) == -1
    with MatchPlan(gpu, [10, 20]) as plan:
        xd = torch.zeros(31, dtype=torch.complex64, device="cuda")
        peak, lag, energy = plan.outputs()
        args = [ptr(xd), ptr(peak), ptr(lag), ptr(energy)]
        for i in range(4):                          # a NULL, then a misaligned pointer in every place
            a = list(args)
            a[i] = None
            assert ctx.lib.vsig_match_run(plan.h, *a) == -1
            a[i] = P(args[i].value + (4 if i in (0, 3) else 2))
            assert ctx.lib.vsig_match_run(plan.h, *a) == -1
        torch.cuda.synchronize()
        assert torch.all(peak == 7) and torch.all(lag == 7) and torch.all(energy == 7)     # nothing was enqueued
        n = C.c_int32()
        v = [C.c_int64() for _ in range(4)]
        assert ctx.lib.vsig_match_info(plan.h, None, *(C.byref(a) for a in v)) == -1
        assert ctx.lib.vsig_match_info(None, C.byref(n), *(C.byref(a) for a in v)) == -1
    assert ctx.lib.vsig_match_run(None, *args) == -1
    ctx.lib.vsig_match_free(None)


# ---------------------------------------------------------------------------
# front ends
# ---------------------------------------------------------------------------
PLAN_SR, PLAN_LEN = 1e6, 0.05
PLAN_L = (300, 411, 500)
PLAN_PERIOD = (6000, 12000, 18000)
PLAN_START = (200, 1000, 2000)


def plan_configs():
    rng = np.random.default_rng(31)
    return [{"signal": np.exp(2j * np.pi * rng.random(L)).astype(np.complex64), "name": f"e{i}",
             "start_time": s / PLAN_SR, "period": p / PLAN_SR}
            for i, (L, p, s) in enumerate(zip(PLAN_L, PLAN_PERIOD, PLAN_START))]


def plan_instances(gpu, configs):
    """(position, length, emitter) of every instance, sorted by position; the
    plan's instances never overlap in time."""
    plan = gpu.vector_plan(configs, PLAN_LEN, PLAN_SR)
    inst = sorted((start + k * period, L, e) for e, ((start, period, count), L) in enumerate(zip(plan.places, PLAN_L))
                  for k in range(count))
    assert [pl[2] for pl in plan.places] == [9, 5, 3]
    assert all(a[0] + a[1] < b[0] for a, b in zip(inst, inst[1:])), "instances overlap"
    return plan, inst


def test_grouping_recovers_the_plan(gpu):
    configs = plan_configs()
    vector, _ = gpu.build_vector(configs, PLAN_LEN, PLAN_SR, device=True)
    plan, inst = plan_instances(gpu, configs)
    rng = np.random.default_rng(32)
    cut = rng.integers(-7, 8, len(inst))            # burst k starts cut[k] samples before its instance
    cut[:3] = (0, 7, -7)
    starts = np.array([pos - c for (pos, _, _), c in zip(inst, cut)])
    ends = np.array([pos + L - 1 + rng.integers(0, 8) for pos, L, _ in inst])
    slices = [s for s, _ in gpu.extract_packets(vector, list(zip(starts, ends)))]
    sim = gpu.packet_similarity(slices)
    assert isinstance(sim.rho, torch.Tensor) and sim.rho.is_cuda and sim.rho.dtype == torch.float64
    assert sim.lag.dtype == torch.int64 and sim.energy.dtype == torch.float64
    host_sim = gpu.packet_similarity([s.cpu().numpy() for s in slices])           # numpy in, numpy out, the same
    assert isinstance(host_sim.rho, np.ndarray) and np.array_equal(host_sim.rho, sim.rho.cpu().numpy())
    assert np.array_equal(host_sim.lag, sim.lag.cpu().numpy())
    groups = gpu.group_packets(sim.rho, 0.7, sim.energy)
    timing = gpu.group_timing(groups, starts, sim.lag, PLAN_SR)
    who = np.array([e for _, _, e in inst])
    assert len(groups.groups) == 3
    for g, members in enumerate(groups.groups):
        e = who[members[0]]
        assert np.all(who[members] == e) and members.size == np.count_nonzero(who == e)
        start, period, count = plan.places[e]
        rep = groups.representative[g]
        assert timing.count[g] == count and abs(timing.period[g] - period) < 1e-6 and timing.jitter[g] < 1e-6
        assert abs(timing.start[g] - (start - cut[rep])) < 1e-6, (g, timing.start[g], start, cut[rep])
        assert abs(timing.seconds.period[g] - period / PLAN_SR) < 1e-12


def test_detect_then_match_recovers_the_plan(gpu):
    configs = plan_configs()
    vector, _ = gpu.build_vector(configs, PLAN_LEN, PLAN_SR)
    plan, inst = plan_instances(gpu, configs)
    rng = np.random.default_rng(33)
    x = (vector + 1e-3 * (rng.standard_normal(vector.size) + 1j * rng.standard_normal(vector.size)) * np.sqrt(0.5))
    x = x.astype(np.complex64)
    packets = gpu.detect_packets(x, PLAN_SR)
    assert packets.starts.size == len(inst)
    m = gpu.match_packets(x, packets, PLAN_SR)
    assert isinstance(m, mt.PacketMatches) and len(m.groups.groups) == 3 and m.carriers.size == 1
    who = np.array([e for _, _, e in inst])
    for g, members in enumerate(m.groups.groups):
        e = who[members[0]]
        assert np.all(who[members] == e) and members.size == np.count_nonzero(who == e)
        start, period, count = plan.places[e]
        assert m.timing.count[g] == count and abs(m.timing.period[g] - period) <= 1e-6 * period
        assert abs(m.timing.start[g] - start) <= packets.window
        cfg = m.configs[g]
        assert cfg["signal"] is m.isolated.packets[m.groups.representative[g]]
        assert cfg["freq_shift"] == m.carriers[0]
    again = gpu.vector_plan(m.configs, PLAN_LEN, PLAN_SR)
    for g, (start, period, count) in enumerate(again.places):
        arrivals = np.round(m.timing.arrivals[g]).astype(np.int64)
        assert count >= arrivals.size
        assert np.array_equal(start + period * np.arange(arrivals.size), arrivals), (g, start, period, arrivals)
    rebuilt, _ = gpu.build_vector(m.configs, PLAN_LEN, PLAN_SR)
    assert rebuilt.shape == vector.shape and np.abs(rebuilt[inst[0][0] + 10]) > 0.5


FE_SR, FE_N, FE_L = 56e6, 20_000, 3000


def _packet(seed):
    """3000 samples of 2 MHz band-limited complex noise, peak-normalised."""
    rng = np.random.default_rng(seed)
    h = scipy.signal.firwin(129, 1e6, fs=FE_SR)
    w = rng.standard_normal(FE_L + 128) + 1j * rng.standard_normal(FE_L + 128)
    p = np.convolve(w, h, "valid")
    return p / np.abs(p).max()


def test_two_carriers_that_overlap_in_time(gpu):
    """Two emitters at +8 and -6 MHz whose bursts share 2000 samples, two bursts
    each; the centres as a measurement scatters them (tens of kHz apart).  The
    carriers' common centres make one emitter's bursts differ by a constant
    phase only: two carriers, two groups, the periods."""
    pa, pb = _packet(11), _packet(12)
    places = [(pa, 4000, 8e6), (pb, 5000, -6e6), (pa, 12000, 8e6), (pb, 13500, -6e6)]
    rng = np.random.default_rng(99)
    x = 1e-3 * (rng.standard_normal(FE_N) + 1j * rng.standard_normal(FE_N)) * np.sqrt(0.5)
    t = np.arange(FE_N) / FE_SR
    for p, at, f in places:
        x[at:at + FE_L] += p * np.exp(2j * np.pi * f * (t[at:at + FE_L] - t[at]))
    x = x.astype(np.complex64)
    starts = np.array([at for _, at, _ in places])
    centres = np.array([8e6 + 21e3, -6e6 - 17e3, 8e6 - 30e3, -6e6 + 25e3])
    nan = np.full(4, np.nan)
    meas = PacketMeasurements(centres, nan, nan, nan, np.full(4, 2e6), nan, np.ones(4, np.int64), None)
    m = gpu.match_packets(x, (starts, starts + FE_L - 1), FE_SR, measurements=meas, max_samples=FE_L)
    assert m.carrier_of.tolist() == [1, 0, 1, 0]
    assert m.carriers.tolist() == [np.median(centres[[1, 3]]), np.median(centres[[0, 2]])]
    assert [g.tolist() for g in m.groups.groups] == [[0, 2], [1, 3]]
    rho = m.similarity.rho
    print(f"two carriers: rho same emitter {rho[0, 2]:.4f} {rho[1, 3]:.4f}, across {rho[0, 1]:.4f} {rho[2, 3]:.4f}")
    assert rho[0, 2] >= 0.95 and rho[1, 3] >= 0.95 and max(rho[0, 1], rho[0, 3], rho[1, 2], rho[2, 3]) < 0.5
    assert abs(m.timing.period[0] - 8000) < 1e-6 and abs(m.timing.period[1] - 8500) < 1e-6
    assert [c["freq_shift"] for c in m.configs] == [m.carriers[1], m.carriers[0]]
