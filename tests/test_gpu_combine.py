"""GPU tests of the coherent averaging of an emitter's repeats (vsig_combine_*,
combine_packets, match_packets(combine=True)): values against the float64
definition (combine_ref.py) at every chunk boundary, the planted scene, the
bit-level properties, memory bounds, graph capture, the C-ABI errors and the
front ends.

Tolerances, all the project's float bar: max |y - y_ref| <= 1e-5 max |y_ref|;
Ep, Ev 1e-6 relative; |a - a_ref| <= 1e-5 |a_ref|, |freq - freq_ref| n <= 1e-5
and |rho - rho_ref| <= 1e-5 for the members the reference decides (rho_ref >=
0.5); used and n equal for every member."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import combine_ref as cr
from guard_arena import Case, In, Out, run
from vector_amd import _lib
from vector_amd import match as mt

pytestmark = pytest.mark.gpu

TOL, TOL_E, MIN_RHO = 1e-5, 1e-6, 0.3
P = C.c_void_p
I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
REC = _lib.COMBINE_MEMBER


def ptr(t):
    return None if t is None else P(t.data_ptr())


class CombinePlan:
    """vsig_combine_create / _free around a block."""

    def __init__(self, gpu, packets, group, lag, rep):
        self.gpu, self.ctx = gpu, gpu.get_context()
        self.lens = np.array([p.size for p in packets], np.int64)
        self.group, self.lag = np.ascontiguousarray(group, np.int32), np.ascontiguousarray(lag, np.int64)
        self.rep = np.ascontiguousarray(rep, np.int32)
        self.K, self.G = int(self.lens.size), int(self.rep.size)
        self.h = P()
        self.ctx.check(self.ctx.lib.vsig_combine_create(
            self.ctx.h, self.lens.ctypes.data_as(I64P), self.group.ctypes.data_as(I32P), self.lag.ctypes.data_as(I64P),
            self.K, self.rep.ctypes.data_as(I32P), self.G, C.byref(self.h)), "create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.lib.vsig_combine_free(self.h)

    def info(self):
        """(out_total, S, est_items, sum_items, workspace_bytes)"""
        v = [C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()]
        self.ctx.check(self.ctx.lib.vsig_combine_info(self.h, *(C.byref(a) for a in v)), "info")
        return tuple(a.value for a in v)

    def offsets(self):
        o = np.zeros(self.G + 1, np.int64)
        self.ctx.check(self.ctx.lib.vsig_combine_offsets(self.h, o.ctypes.data_as(I64P)), "offsets")
        return o

    def records(self):
        return torch.full((self.K * REC.itemsize,), 7, dtype=torch.uint8, device="cuda")

    def output(self):
        return torch.full((self.info()[0],), 7, dtype=torch.complex64, device="cuda")

    def estimate(self, packed, ref=None, f0=None, min_rho=MIN_RHO, rec=None):
        rec = self.records() if rec is None else rec
        self.gpu.get_context()                     # binds the context to the current stream
        self.ctx.check(self.ctx.lib.vsig_combine_estimate(self.h, ptr(packed), ptr(ref), ptr(f0), min_rho, ptr(rec)),
                       "estimate")
        return rec

    def sum(self, packed, rec, y=None):
        y = self.output() if y is None else y
        self.gpu.get_context()
        self.ctx.check(self.ctx.lib.vsig_combine_sum(self.h, ptr(packed), ptr(rec), ptr(y)), "sum")
        return y


def freq_of(rec):
    """The records' freq column as a contiguous device float64 tensor."""
    return rec.view(torch.float64).view(-1, REC.itemsize // 8)[:, 2].contiguous()


def host_rec(rec):
    return rec.cpu().numpy().view(REC).reshape(-1).copy()


def path(gpu, packets, group, lag, rep, min_rho=MIN_RHO):
    """first records, y, second records, refined y as host arrays, and the plan's
    info and offsets: one plan, the four launches of combine_packets."""
    packed = torch.from_numpy(np.concatenate(packets)).cuda()
    with CombinePlan(gpu, packets, group, lag, rep) as plan:
        r1 = plan.estimate(packed, min_rho=min_rho)
        y1 = plan.sum(packed, r1)
        r2 = plan.estimate(packed, y1, freq_of(r1), min_rho)
        y2 = plan.sum(packed, r2)
        torch.cuda.synchronize()
        return host_rec(r1), y1.cpu().numpy(), host_rec(r2), y2.cpu().numpy(), plan.info(), plan.offsets()


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def chunk_size(gpu):
    one = [np.ones(3, np.complex64)]
    with CombinePlan(gpu, one, [0], [0], [0]) as plan:
        return plan.info()[1]


def values_scene(S):
    """Two groups and one packet in no group.  Group 0's representative has
    2 S + 3 samples, group 1's S.  Names -> what each member is there for."""
    rng = np.random.default_rng(77)

    def junk(n):
        return 0.7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))

    def unit(n):
        return np.exp(2j * np.pi * rng.random(n))

    def copy(seg, gain, f):
        """seg by a complex gain and a frequency offset |f| n <= 0.3, plus a little noise"""
        t = np.arange(seg.size)
        return gain * np.exp(2j * np.pi * (f / max(seg.size, 1)) * t) * seg + 0.02 * junk(seg.size)
    L0, L1 = 2 * S + 3, S
    b0, b1 = unit(L0), unit(L1)
    members = [  # (name, samples, group, lag)
        ("rep0", b0, 0, 0),
        ("n=S+1", copy(b0[5:5 + S + 1], 0.8 - 0.3j, 0.25), 0, -5),
        ("n=S", np.concatenate([junk(3), copy(b0[:S], -0.4 + 1.1j, -0.2)]), 0, 3),
        ("n=S-1", np.concatenate([copy(b0[L0 - S + 1:], 1.5j, 0.3), junk(10)]), 0, -(L0 - S + 1)),
        ("n=2", np.concatenate([copy(b0[L0 - 2:], 0.9, 0.1), junk(4)]), 0, -(L0 - 2)),
        ("n=1", np.concatenate([junk(7), copy(b0[:1], 1.2 + 0.5j, 0.0)]), 0, 7),
        ("none", junk(40), 0, L0 + 5),
        ("noise", junk(L0), 0, 0),
        ("full", np.concatenate([junk(2), copy(b0, 0.6 + 0.6j, -0.28), junk(2)]), 0, 2),
        ("alone", junk(50), -1, 4),
        ("rep1", b1, 1, 0),
        ("longer", np.concatenate([junk(10), copy(b1, 2.0, 0.22), junk(10)]), 1, 10),
        ("shorter", copy(b1[4:S - 3], -1.0j, -0.15), 1, -4),
    ]
    names = [m[0] for m in members]
    packets = [m[1].astype(np.complex64) for m in members]
    group = np.array([m[2] for m in members], np.int32)
    lag = np.array([m[3] for m in members], np.int64)
    rep = np.array([names.index("rep0"), names.index("rep1")], np.int32)
    return names, packets, group, lag, rep


@functools.lru_cache(maxsize=None)
def values_case():
    import vector_amd as gpu
    S = chunk_size(gpu)
    names, packets, group, lag, rep = values_scene(S)
    ref = cr.combine(packets, group, lag, rep, MIN_RHO, refine=True)
    got = path(gpu, packets, group, lag, rep)
    again = path(gpu, packets, group, lag, rep)
    for a in got[:4] + again[:4]:
        a.setflags(write=False)
    return S, names, packets, group, lag, rep, ref, got, again


def check_records(names, rec, want, what):
    """The bars of the module docstring on one pass's records."""
    n = want.n
    assert np.array_equal(rec["n"], n) and np.array_equal(rec["used"] != 0, want.used), what
    assert np.all(rec["pad"] == 0)
    assert np.abs(want.rho - MIN_RHO).min() >= 1e-3, "min_rho too close to a reference rho"
    for f in ("Ep", "Ev"):
        w = getattr(want, f)
        e = np.abs(rec[f] - w) / np.where(w > 0, w, 1.0)
        assert e.max() <= TOL_E, (what, f, e.max(), names[int(e.argmax())])
    assert np.array_equal(rec["m"], want.m)
    decided = want.rho >= 0.5
    out = {names[k] for k in np.flatnonzero(~decided)}
    a = rec["a_re"] + 1j * rec["a_im"]
    e_a = np.abs(a - want.a)[decided] / np.abs(want.a[decided])
    e_f = (np.abs(rec["freq"] - want.freq) * n)[decided]
    e_r = np.abs(rec["rho"] - want.rho)[decided]
    print(f"{what}: decided {int(decided.sum())} of {n.size}, max |a - ref| / |ref| {e_a.max():.2e}, "
          f"|freq - ref| n {e_f.max():.2e}, |rho - ref| {e_r.max():.2e}; outside: {sorted(out)}")
    assert out <= {"noise", "none", "alone"}, out
    assert e_a.max() <= TOL and e_f.max() <= TOL and e_r.max() <= TOL, what
    und = ~(rec["used"] != 0)
    assert np.all(a[und] == 0) and np.all((rec["rho"][und] == 0) | np.isnan(rec["rho"][und]))


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
def test_values_against_the_definition(gpu):
    S, names, packets, group, lag, rep, ref, (r1, y1, r2, y2, info, offsets), _ = values_case()
    L0, L1 = 2 * S + 3, S
    assert S >= 64 and info[0] == L0 + L1 and offsets.tolist() == [0, L0, L0 + L1]
    n = ref.first.n
    assert [int(n[names.index(k)]) for k in ("n=1", "n=2", "n=S-1", "n=S", "n=S+1", "none", "alone", "full")] == \
        [1, 2, S - 1, S, S + 1, 0, 0, L0]
    # a sum item is (group, chunk of its output), the chunk no longer than S
    assert info[2] == int(np.sum((n + S - 1) // S)) and info[3] >= 3 + 1 and info[4] == 64 * info[2]
    alone = names.index("alone")
    assert r1["used"][alone] == 0 and r1["n"][alone] == 0 and r1["a_re"][alone] == 0 and r1["Ep"][alone] == 0
    for k in rep:                                  # by definition, not estimated
        assert (r1["a_re"][k], r1["a_im"][k], r1["freq"][k], r1["rho"][k], r1["res"][k], r1["used"][k]) == (1, 0, 0, 1, 0, 1)
    check_records(names, r1, ref.first, "first pass")
    check_records(names, r2, ref.second, "second pass")
    assert not ref.first.used[names.index("noise")] and ref.first.used.sum() == len(names) - 3
    for what, y, want in (("y", y1, ref.y_first), ("refined y", y2, ref.y)):
        for g in range(2):
            yg, wg = y[offsets[g]:offsets[g + 1]], want[g]
            e = np.abs(yg - wg).max() / np.abs(wg).max()
            print(f"{what} group {g}: max |y - ref| / max |ref| {e:.2e}")
            assert e <= TOL, (what, g, e)
    gain = np.array([np.sum((r1["a_re"] ** 2 + r1["a_im"] ** 2)[(group == g) & (r1["used"] != 0)]) for g in range(2)])
    assert np.all(np.abs(gain - ref.gain) <= TOL * ref.gain)


@pytest.mark.parametrize("seed", cr.SCENE_SEEDS)
def test_planted_scene(gpu, seed):
    """The scene of test_combine_cpu.py through combine_packets: the same three
    conditions, and gain_g within 1e-5 relative of the reference's."""
    sc = cr.planted_scene(seed)
    want = cr.combine(sc.packets, sc.group, sc.lag, sc.rep)
    K = len(sc.packets)
    lag = np.zeros((K, K), np.int64)
    lag[:, sc.rep[0]] = sc.lag
    for refine in (False, True):
        out = gpu.combine_packets(sc.packets, [np.r_[sc.rep[0], np.delete(np.arange(K), sc.rep[0])]], lag, refine=refine)
        ratio, ferr, factor = cr.scene_figures(sc, out.packets[0], out.gain[0], out.members.freq, out.members.snr)
        print(f"seed {seed} refine {refine}: gain_g {out.gain[0]:.4f} (ref {want.gain[0]:.4f}), measured / gain_g "
              f"{ratio:.3f}, max |freq - planted| L {ferr:.2e}, snr factor {factor:.3f}")
        assert out.members.used.all() and np.array_equal(out.members.overlap, want.first.n)
        assert abs(out.gain[0] - want.gain[0]) <= TOL * want.gain[0]
        assert 0.9 <= ratio <= 1.2 and ferr <= 2e-2 and factor <= cr.SNR_FACTOR_BAR
        assert np.all(np.abs(out.members.snr - want.snr) <= 1e-3 * want.snr)


# ---------------------------------------------------------------------------
# bit-level properties
# ---------------------------------------------------------------------------
def test_a_group_of_one_returns_its_packet(gpu):
    S = chunk_size(gpu)
    rng = np.random.default_rng(3)
    pk = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) for n in (2 * S + 5, 90, 1, 80)]
    pk[3][:70] = pk[1][10:80]
    pk[0][7] = complex(-0.0, 5.0)
    group, lag, rep = [0, 1, 2, 1], [0, 0, 0, -10], [0, 1, 2]
    r1, y1, r2, y2, _, off = path(gpu, pk, group, lag, rep, 0.0)
    for g in (0, 2):
        assert same_bytes([y1[off[g]:off[g + 1]]], [pk[g]]) and same_bytes([y2[off[g]:off[g + 1]]], [pk[g]])
        assert (r2["a_re"][g], r2["a_im"][g], r2["freq"][g], r2["used"][g]) == (1, 0, 0, 1)
    assert r1["used"].tolist() == [1, 1, 1, 1] and r1["n"].tolist() == [2 * S + 5, 90, 1, 80]


def test_same_bytes_twice_and_from_a_second_plan(gpu):
    S, names, packets, group, lag, rep, _, got, again = values_case()
    assert same_bytes(got[:4], again[:4])
    packed = torch.from_numpy(np.concatenate(packets)).cuda()
    with CombinePlan(gpu, packets, group, lag, rep) as plan:
        a = plan.estimate(packed)
        b = plan.estimate(packed)
        ya, yb = plan.sum(packed, a), plan.sum(packed, b)
        torch.cuda.synchronize()
        assert same_bytes([host_rec(a), ya.cpu().numpy()], [host_rec(b), yb.cpu().numpy()])
        assert same_bytes([host_rec(a), ya.cpu().numpy()], got[:2])


def test_a_group_does_not_depend_on_the_list(gpu):
    """Group 0's records and output from a list of its members alone have the
    bytes they have inside the full list, and so has group 1."""
    S, names, packets, group, lag, rep, _, (r1, y1, r2, y2, _, off), _ = values_case()
    for g in range(2):
        idx = np.flatnonzero(group == g)
        sub = path(gpu, [packets[k] for k in idx], np.zeros(idx.size, np.int32), lag[idx],
                   [int(np.flatnonzero(idx == rep[g])[0])])
        assert same_bytes(sub[:4], (r1[idx], y1[off[g]:off[g + 1]], r2[idx], y2[off[g]:off[g + 1]])), g


def test_nan_zero_and_a_nan_representative(gpu):
    S, names, packets, group, lag, rep, _, (r1, y1, r2, y2, _, off), _ = values_case()
    k_nan, k_zero = names.index("n=S+1"), names.index("full")
    bad = [p.copy() for p in packets]
    bad[k_nan][S // 2] = np.nan
    bad[k_zero][:] = 0
    b1, by1, b2, by2, _, _ = path(gpu, bad, group, lag, rep)
    assert b1["used"][k_nan] == 0 and np.isnan(b1["rho"][k_nan]) and b1["a_re"][k_nan] == 0
    assert b1["used"][k_zero] == 0 and b1["rho"][k_zero] == 0 and b2["used"][k_zero] == 0 and b2["used"][k_nan] == 0
    keep = np.array([k for k in range(len(names)) if k not in (k_nan, k_zero)])
    new_rep = [int(np.flatnonzero(keep == r)[0]) for r in rep]
    s1, sy1, s2, sy2, _, soff = path(gpu, [packets[k] for k in keep], group[keep], lag[keep], new_rep)
    assert soff.tolist() == off.tolist()
    assert same_bytes((by1, by2, b1[keep], b2[keep]), (sy1, sy2, s1, s2))
    assert np.isfinite(by1.view(np.float32)).all()
    # with min_rho = 0 an all-zero member still is not used (rho is 0 / 0)
    z1 = path(gpu, bad, group, lag, rep, 0.0)[0]
    assert z1["used"][k_zero] == 0 and z1["used"][names.index("noise")] == 1
    # a NaN in group 0's representative stays in group 0
    bad = [p.copy() for p in packets]
    bad[rep[0]][11] = np.nan
    n1, ny1, n2, ny2, _, _ = path(gpu, bad, group, lag, rep)
    g1 = slice(off[1], off[2])
    in1 = group == 1
    assert same_bytes((ny1[g1], ny2[g1], n1[in1], n2[in1]), (y1[g1], y2[g1], r1[in1], r2[in1]))
    others = (group == 0) & (np.arange(len(names)) != rep[0]) & (r1["n"] > 0)
    covers = others & (11 + lag >= 0) & (11 + lag < np.array([p.size for p in packets]))
    assert covers.sum() >= 4
    assert np.all(n1["used"][covers] == 0) and n1["used"][rep[0]] == 1 and np.isnan(ny1[11])


# ---------------------------------------------------------------------------
# memory bounds
# ---------------------------------------------------------------------------
def test_bounds_estimate_and_sum(gpu):
    """packed and ref are read inside their extents only (their tails and the
    guards are poisoned), records and y are written exactly, no input is
    written."""
    ctx = gpu.get_context()
    S, names, packets, group, lag, rep, ref, (r1, y1, r2, _, info, _), _ = values_case()
    K, total, tail = len(packets), sum(p.size for p in packets), 300
    data = np.concatenate(packets + [np.zeros(tail, np.complex64)])
    holes = np.arange(total + tail) >= total
    ydata = np.concatenate([y1, np.zeros(tail, np.complex64)])
    yholes = np.arange(info[0] + tail) >= info[0]
    f0 = np.ascontiguousarray(r1["freq"])
    with CombinePlan(gpu, packets, group, lag, rep) as plan:
        def first(p):
            return ctx.lib.vsig_combine_estimate(plan.h, P(p["packed"]), None, None, MIN_RHO, P(p["records"]))

        def second(p):
            return ctx.lib.vsig_combine_estimate(plan.h, P(p["packed"]), P(p["ref"]), P(p["f0"]), MIN_RHO, P(p["records"]))

        def total_sum(p):
            return ctx.lib.vsig_combine_sum(plan.h, P(p["packed"]), P(p["records"]), P(p["y"]))

        def is_first(o):
            assert same_bytes([o["records"]], [r1])

        def is_second(o):
            assert same_bytes([o["records"]], [r2])

        def is_y(o):
            assert same_bytes([o["y"]], [y1])
        for skew in range(4):
            run(Case("vsig_combine_estimate", f"ref=NULL skew={skew}", {"packed": In(data, 8 * skew, holes=holes)},
                     {"records": Out(K, REC, 8 * (3 - skew))}, first, is_first))
            run(Case("vsig_combine_estimate", f"ref=y skew={skew}",
                     {"packed": In(data, 8 * skew, holes=holes), "ref": In(ydata, 8 * ((skew + 1) % 4), holes=yholes),
                      "f0": In(f0, 8 * ((skew + 2) % 4))},
                     {"records": Out(K, REC, 8 * (3 - skew))}, second, is_second))
            run(Case("vsig_combine_sum", f"skew={skew}",
                     {"packed": In(data, 8 * skew, holes=holes), "records": In(r1, 8 * ((skew + 1) % 4))},
                     {"y": Out(info[0], np.complex64, 8 * (3 - skew))}, total_sum, is_y))


# ---------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------
def test_the_passes_capture_into_a_graph(gpu):
    """Estimate, sum and estimate neither allocate nor synchronise: one capture
    on a single stream, replayed on new contents, gives the bytes of plain
    calls."""
    S, names, packets, group, lag, rep, *_ = values_case()
    x = np.concatenate(packets)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(x).cuda()
        with CombinePlan(gpu, packets, group, lag, rep) as plan:
            r1, r2, y = plan.records(), plan.records(), plan.output()
            f0 = torch.zeros(plan.K, dtype=torch.float64, device="cuda")

            def passes():
                plan.estimate(xd, rec=r1)
                plan.sum(xd, r1, y)
                f0.copy_(r1.view(torch.float64).view(-1, REC.itemsize // 8)[:, 2])
                plan.estimate(xd, y, f0, rec=r2)
            passes()
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                passes()
            for scale in (0.5, 3.0):
                xd.copy_(torch.from_numpy(x * np.float32(scale)))
                for t in (r1, r2, y):
                    t.fill_(7)
                graph.replay()
                stream.synchronize()
                replayed = (host_rec(r1), host_rec(r2), y.cpu().numpy())
                for t in (r1, r2, y):
                    t.fill_(7)
                passes()
                stream.synchronize()
                assert same_bytes(replayed, (host_rec(r1), host_rec(r2), y.cpu().numpy()))
                assert replayed[0]["used"].sum() == len(names) - 3 and np.all(replayed[0]["Ep"] >= 0)
            del graph


# ---------------------------------------------------------------------------
# C-ABI errors
# ---------------------------------------------------------------------------
def test_c_abi_errors(gpu):
    ctx = gpu.get_context()

    def create(lens, group, lag, rep, K=None, G=None, null=None, null_ctx=False):
        lens, lag = np.ascontiguousarray(lens, np.int64), np.ascontiguousarray(lag, np.int64)
        group, rep = np.ascontiguousarray(group, np.int32), np.ascontiguousarray(rep, np.int32)
        h = P()
        args = {"lens": lens.ctypes.data_as(I64P), "group": group.ctypes.data_as(I32P), "lag": lag.ctypes.data_as(I64P),
                "rep": rep.ctypes.data_as(I32P), "out": C.byref(h)}
        if null:
            args[null] = None
        rc = ctx.lib.vsig_combine_create(None if null_ctx else ctx.h, args["lens"], args["group"], args["lag"],
                                         lens.size if K is None else K, args["rep"], rep.size if G is None else G,
                                         args["out"])
        if rc == 0:
            ctx.lib.vsig_combine_free(h)
        return rc, ctx.lib.vsig_last_error(ctx.h).decode()
    ok = ([5, 9, 7], [0, 0, -1], [0, 2, 0], [0])
    assert create(*ok)[0] == 0 and create([1], [0], [0], [0])[0] == 0
    assert create([5, 9, 7], [0, 0, -1], [0, 1 << 60, -(1 << 62)], [0])[0] == 0       # a lag beyond every length
    assert create(*ok, K=0)[0] == -1 and create(*ok, K=-1)[0] == -1
    assert create(np.ones(4097), np.zeros(4097), np.zeros(4097), [0])[0] == -1
    assert create(*ok, G=0)[0] == -1 and create([5, 9], [0, 1], [0, 0], [0, 1, 0], G=3)[0] == -1
    for lens, name in (([5, 0, 7], "packet 1"), ([5, 9, -3], "packet 2")):
        rc, msg = create(lens, *ok[1:])
        assert rc == -1 and name in msg
    rc, msg = create([1 << 30, 1 << 30], [0, 0], [0, 0], [0])
    assert rc == -4 and "packet 1" in msg
    assert create([1 << 31], [0], [0], [0])[0] == -4
    for grp, name in (([0, 1, -1], "packet 1"), ([0, 0, -2], "packet 2")):
        rc, msg = create(ok[0], grp, ok[2], ok[3])
        assert rc == -1 and name in msg
    for lens, grp, lg, rp, name in (([5, 9, 7], [0, 0, 1], [0, 0, 0], [0, 1], "group 1"),      # another group's
                                    ([5, 9, 7], [0, 0, -1], [0, 0, 0], [2], "group 0"),        # in no group
                                    ([5, 9, 7], [0, 0, -1], [0, 0, 0], [3], "group 0"),        # no packet
                                    ([5, 9, 7], [0, 0, -1], [0, 0, 0], [-1], "group 0"),
                                    ([5, 9, 7], [0, 0, 0], [0, 0, 0], [0, 1], "group 1"),      # a group without members
                                    ([5, 9, 7], [0, 0, 1], [1, 0, 0], [0, 2], "group 0")):     # a lag of its own
        rc, msg = create(lens, grp, lg, rp)
        assert rc == -1 and name in msg, (rc, msg)
    for null in ("lens", "group", "lag", "rep", "out"):
        assert create(*ok, null=null)[0] == -1
    assert create(*ok, null_ctx=True)[0] == -1
    pk = [np.ones(10, np.complex64), np.ones(20, np.complex64)]
    with CombinePlan(gpu, pk, [0, 0], [0, -3], [0]) as plan:
        xd = torch.zeros(31, dtype=torch.complex64, device="cuda")
        rec, y = plan.records(), plan.output()
        ref = torch.zeros(11, dtype=torch.complex64, device="cuda")
        f0 = torch.zeros(3, dtype=torch.float64, device="cuda")
        est = [ptr(xd), ptr(ref), ptr(f0), ptr(rec)]
        for i in range(4):                          # a NULL (ref and f0 may be NULL), then a misaligned pointer
            a = list(est)
            if i in (0, 3):
                a[i] = None
                assert ctx.lib.vsig_combine_estimate(plan.h, a[0], a[1], a[2], 0.0, a[3]) == -1
            a[i] = P(est[i].value + 4)
            assert ctx.lib.vsig_combine_estimate(plan.h, a[0], a[1], a[2], 0.0, a[3]) == -1
        assert ctx.lib.vsig_combine_estimate(plan.h, est[0], est[1], est[2], float("nan"), est[3]) == -1
        sm = [ptr(xd), ptr(rec), ptr(y)]
        for i in range(3):
            a = list(sm)
            a[i] = None
            assert ctx.lib.vsig_combine_sum(plan.h, *a) == -1
            a[i] = P(sm[i].value + 4)
            assert ctx.lib.vsig_combine_sum(plan.h, *a) == -1
        torch.cuda.synchronize()
        assert torch.all(rec == 7) and torch.all(y == 7)                 # nothing was enqueued
        v = [C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()]
        assert ctx.lib.vsig_combine_info(plan.h, None, *(C.byref(a) for a in v[1:])) == -1
        assert ctx.lib.vsig_combine_info(None, *(C.byref(a) for a in v)) == -1
        assert ctx.lib.vsig_combine_offsets(plan.h, None) == -1 and ctx.lib.vsig_combine_offsets(None, None) == -1
    assert ctx.lib.vsig_combine_estimate(None, *est[:3], 0.0, est[3]) == -1
    assert ctx.lib.vsig_combine_sum(None, *sm) == -1
    ctx.lib.vsig_combine_free(None)


# ---------------------------------------------------------------------------
# front ends
# ---------------------------------------------------------------------------
def test_numpy_and_tensors_give_the_same(gpu):
    S, names, packets, group, lag, rep, ref, (r1, y1, r2, y2, _, off), _ = values_case()
    K = len(packets)
    lagm = np.zeros((K, K), np.int64)
    groups = []
    for g in range(2):
        idx = np.flatnonzero(group == g)
        lagm[idx, rep[g]] = lag[idx]
        groups.append(np.r_[rep[g], idx[idx != rep[g]]])
    for refine, y in ((False, y1), (True, y2)):
        h = gpu.combine_packets(packets, groups, lagm, min_rho=MIN_RHO, refine=refine)
        d = gpu.combine_packets([torch.from_numpy(p).cuda() for p in packets], groups, torch.from_numpy(lagm).cuda(),
                                min_rho=MIN_RHO, refine=refine)
        assert isinstance(h.packets[0], np.ndarray) and h.packets[0].dtype == np.complex64 and h.members.a.dtype == np.complex128
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in list(d.packets) + [d.gain] + list(d.members))
        assert d.packets[0].untyped_storage().data_ptr() == d.packets[1].untyped_storage().data_ptr()
        assert same_bytes(h.packets, [t.cpu().numpy() for t in d.packets])
        assert same_bytes([h.gain] + list(h.members), [d.gain.cpu().numpy()] + [t.cpu().numpy() for t in d.members])
        assert same_bytes(h.packets, [y[off[0]:off[1]], y[off[1]:off[2]]])
        assert np.array_equal(h.members.used, r1["used"] != 0) and np.array_equal(h.members.overlap, r1["n"])
        assert np.all(np.abs(h.gain - ref.gain) <= TOL * ref.gain)
        snr, want = h.members.snr, ref.snr
        # an overlap of one or two samples is fitted exactly: res is rounding, its sign either way
        big = ref.second.n > 2
        assert np.array_equal(np.isnan(snr), np.isnan(want))
        assert np.array_equal(np.isinf(snr[big]), np.isinf(want[big]))
        fin = np.isfinite(want) & ref.second.used & big
        assert np.all(np.abs(snr[fin] - want[fin]) <= 1e-2 * want[fin])
    # views of one packed device buffer are used in place
    packed = torch.from_numpy(np.concatenate(packets)).cuda()
    o = np.r_[0, np.cumsum([p.size for p in packets])]
    views = [packed[o[k]:o[k + 1]] for k in range(K)]
    v = gpu.combine_packets(views, groups, lagm, min_rho=MIN_RHO)
    assert same_bytes([t.cpu().numpy() for t in v.packets], [y1[off[0]:off[1]], y1[off[1]:off[2]]])
    # a PacketGroups names its representatives itself
    pg = mt.PacketGroups(np.where(group < 0, 2, group), [np.flatnonzero(group == 0), np.flatnonzero(group == 1)], rep)
    w = gpu.combine_packets(packets, pg, lagm, min_rho=MIN_RHO)
    assert same_bytes(w.packets, [y1[off[0]:off[1]], y1[off[1]:off[2]]])


PLAN_SR, PLAN_LEN, PLAN_NOISE = 1e6, 0.05, 0.05
PLAN_L = (300, 411, 500)
PLAN_PERIOD = (6000, 12000, 18000)
PLAN_START = (200, 1000, 2000)


def plan_configs():
    rng = np.random.default_rng(31)
    return [{"signal": np.exp(2j * np.pi * rng.random(L)).astype(np.complex64), "name": f"e{i}",
             "start_time": s / PLAN_SR, "period": p / PLAN_SR}
            for i, (L, p, s) in enumerate(zip(PLAN_L, PLAN_PERIOD, PLAN_START))]


def fit_error(x, s):
    """|x - c s|^2 / |c s|^2 with the one complex gain c that fits best."""
    x, s = np.asarray(x, np.complex128), np.asarray(s, np.complex128)
    c = np.vdot(s, x) / np.vdot(s, s)
    return np.sum(np.abs(x - c * s) ** 2) / np.sum(np.abs(c * s) ** 2)


def test_match_packets_combines_the_plan(gpu):
    configs = plan_configs()
    vector, _ = gpu.build_vector(configs, PLAN_LEN, PLAN_SR)
    plan = gpu.vector_plan(configs, PLAN_LEN, PLAN_SR)
    inst = sorted((start + k * period, L, e) for e, ((start, period, count), L) in enumerate(zip(plan.places, PLAN_L))
                  for k in range(count))
    assert [pl[2] for pl in plan.places] == [9, 5, 3]
    rng = np.random.default_rng(34)
    cut = rng.integers(-7, 8, len(inst))
    starts = np.array([pos - c for (pos, _, _), c in zip(inst, cut)])
    ends = np.array([pos + L - 1 + rng.integers(0, 8) for pos, L, _ in inst])
    noise = PLAN_NOISE * (rng.standard_normal(vector.size) + 1j * rng.standard_normal(vector.size)) * np.sqrt(0.5)
    x = (vector + noise).astype(np.complex64)
    plain = gpu.match_packets(x, (starts, ends), PLAN_SR)
    m = gpu.match_packets(x, (starts, ends), PLAN_SR, combine=True)
    assert plain.combined is None and isinstance(m.combined, mt.CombinedPackets) and len(m) == 8
    assert len(m.groups.groups) == 3
    assert all(np.array_equal(a, b) for a, b in zip(m.groups.groups, plain.groups.groups))
    assert np.array_equal(m.groups.representative, plain.groups.representative)
    assert np.array_equal(m.groups.labels, plain.groups.labels)
    for f in ("start", "period", "count", "jitter"):
        assert np.array_equal(getattr(m.timing, f), getattr(plain.timing, f), equal_nan=True)
    # the planted packets as the same path shows them: the noise-free capture, the same carriers and filters
    clean = gpu.match_packets(vector.astype(np.complex64), (starts, ends), PLAN_SR, measurements=m.measurements)
    who = np.array([e for _, _, e in inst])
    for g, members in enumerate(m.groups.groups):
        r = int(m.groups.representative[g])
        assert np.all(who[members] == who[r]) and members.size == np.count_nonzero(who == who[r])
        cfg, pcfg = m.configs[g], plain.configs[g]
        assert cfg["signal"] is m.combined.packets[g] and pcfg["signal"] is plain.isolated.packets[r]
        assert {k: v for k, v in cfg.items() if k != "signal"} == {k: v for k, v in pcfg.items() if k != "signal"}
        assert cfg["signal"].shape == m.isolated.packets[r].shape and cfg["signal"].dtype == np.complex64
        gain = m.combined.gain[g]
        want = clean.isolated.packets[r]
        e_rep, e_comb = fit_error(m.isolated.packets[r], want), fit_error(cfg["signal"], want)
        print(f"group {g}: {members.size} members, gain {gain:.3f}, error of the representative {e_rep:.3e}, "
              f"of the combined packet {e_comb:.3e} ({e_rep / e_comb:.2f} x)")
        assert gain >= 0.8 * members.size
        assert e_comb < e_rep
        assert np.all(m.combined.members.used[members])
    again = gpu.vector_plan(m.configs, PLAN_LEN, PLAN_SR)
    assert [pl[2] for pl in again.places] == [pl[2] for pl in gpu.vector_plan(plain.configs, PLAN_LEN, PLAN_SR).places]
    rebuilt, _ = gpu.build_vector(m.configs, PLAN_LEN, PLAN_SR)
    assert rebuilt.shape == vector.shape and np.abs(rebuilt[inst[0][0] + 10]) > 0.5
