"""Time the coherent averaging of grouped bursts through the C ABI against what a
caller could do with torch alone, in one process:

  A    vsig_combine_estimate, vsig_combine_sum, vsig_combine_estimate on one
       plan: five launches whatever K and G are
  B    a loop over the groups of torch ops on the device: the group's members
       gathered into an M x L matrix at their lags, the six masked sums in
       double, the gains and frequencies, the weighted sum, and the sums again
       against it (no host read inside the loop)

for K bursts of L samples in G groups: every group one unit-modulus random-phase
packet, its members cut at lags of +-7 samples with gains 0.5 - 2, frequency
offsets |f| L <= 0.3 and noise 0.1.  Both are timed by HIP events on the stream
(B's span holds its launch gaps: that is what its caller waits for).  A and B
alternate inside every repetition and the medians (min-max) are reported.
Before timing, A's packets and gains equal B's at 1e-4 relative (asserted).

Bytes: the algorithmic traffic of A, 8 B (3 sum n_k + 2 sum L_g) -- every
member's overlap read by both estimates and the sum, every output written once
and read once as the second reference; the re-reads of a reference by its
group's members are expected from L2 and not counted.  The share is of the
8 TB/s HBM roof.  No threshold: the table records what was measured.  A manual
tool: run it under its own time limit on one GPU, e.g.

    timeout -k 10 600 python tools/combine_ab.py [--out out/combine_ab.md]
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vector_amd as va  # noqa: E402
from vector_amd import _lib  # noqa: E402

ROOF_TBS = 8.0
P = C.c_void_p
I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
NREC = _lib.COMBINE_MEMBER.itemsize


def scene(K, L, G, seed):
    """(packets, group, lag, rep): member k of group k % G; the first member of
    a group is its representative."""
    rng = np.random.default_rng(seed)
    base = np.exp(2j * np.pi * rng.random((G, L + 14)))
    group = (np.arange(K) % G).astype(np.int32)
    rep = np.arange(G, dtype=np.int32)
    cut = rng.integers(-7, 8, K)
    cut[:G] = 0
    t = np.arange(L)
    packets = []
    for k in range(K):
        gain = rng.uniform(0.5, 2.0) * np.exp(2j * np.pi * rng.random())
        f = rng.uniform(-0.3, 0.3) / L
        noise = 0.1 * (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * np.sqrt(0.5)
        packets.append((gain * np.exp(2j * np.pi * f * t) * base[group[k], 7 - cut[k]:7 - cut[k] + L] + noise)
                       .astype(np.complex64))
    return packets, group, cut.astype(np.int64), rep      # p_k[i] = base[i + 7 - cut_k]: j + d_k = j + cut_k


class TorchLoop:
    """Method B: the tables it needs are built once, as A's plan is."""

    def __init__(self, packed, lens, group, lag, rep):
        dev = packed.device
        off = np.r_[0, np.cumsum(lens)]
        self.packed, self.groups = packed, []
        for g, r in enumerate(rep):
            mem = np.flatnonzero(group == g)
            Lg = int(lens[r])
            j = np.arange(Lg)
            idx = j[None, :] + lag[mem][:, None]
            valid = (idx >= 0) & (idx < lens[mem][:, None])
            lo = np.maximum(0, -lag[mem])
            n = valid.sum(1)
            self.groups.append(dict(
                src=torch.from_numpy(off[mem][:, None] + np.where(valid, idx, 0)).to(dev),
                valid=torch.from_numpy(valid).to(dev),
                first=torch.from_numpy(valid & (j[None, :] - lo[:, None] < (n // 2)[:, None])).to(dev),
                jm=torch.from_numpy(j[None, :] - (lo + (n - 1) / 2)[:, None]).to(dev),
                n=torch.from_numpy(n.astype(np.float64)).to(dev), rep=int(np.flatnonzero(mem == r)[0])))

    @staticmethod
    def estimate(t, X, v, f0):
        z = X * torch.conj(v)[None, :]
        if f0 is not None:
            z = z * torch.polar(torch.ones_like(t["jm"]), -2 * math.pi * f0[:, None] * t["jm"]).to(torch.complex64)
        first, rest = t["first"], t["valid"] & ~t["first"]
        A1 = (z * first).sum(1, dtype=torch.complex128)
        A2 = (z * rest).sum(1, dtype=torch.complex128)
        ev = (v.real ** 2 + v.imag ** 2)[None, :] * t["valid"]
        Ev = ev.sum(1, dtype=torch.float64)
        phi = torch.where((A1 != 0) & (A2 != 0), torch.angle(A2 * torch.conj(A1)), torch.zeros_like(Ev))
        half = torch.polar(torch.ones_like(phi), 0.5 * phi)
        a = (A1 * half + A2 * torch.conj(half)) / Ev
        return a, (0 if f0 is None else f0) + phi / (math.pi * t["n"])

    def run(self):
        out = []
        for t in self.groups:
            X = self.packed[t["src"]] * t["valid"]
            a, f = self.estimate(t, X, X[t["rep"]], None)
            a = a.clone()
            f = f.clone()
            a[t["rep"]], f[t["rep"]] = 1.0, 0.0
            w = torch.conj(a)[:, None] * torch.polar(torch.ones_like(t["jm"]), -2 * math.pi * f[:, None] * t["jm"])
            num = (w.to(torch.complex64) * X).sum(0)
            den = ((a.real ** 2 + a.imag ** 2)[:, None] * t["valid"]).sum(0)
            y = (num / den).to(torch.complex64)
            a2, f2 = self.estimate(t, X, y, f)
            out.append((y, a, f, a2, f2))
        return out


def case(ctx, K, L, G, warmup, reps):
    lib = ctx.lib
    packets, group, lag, rep = scene(K, L, G, K + L + G)
    lens = np.array([p.size for p in packets], np.int64)
    packed = torch.from_numpy(np.concatenate(packets)).cuda()
    ctx.bind_stream()
    plan = P()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.check(lib.vsig_combine_create(ctx.h, lens.ctypes.data_as(I64P), group.ctypes.data_as(I32P),
                                      lag.ctypes.data_as(I64P), K, rep.ctypes.data_as(I32P), G, C.byref(plan)), "create")
    create_ms = (time.perf_counter() - t0) * 1e3
    info = [C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()]
    ctx.check(lib.vsig_combine_info(plan, *(C.byref(v) for v in info)), "info")
    out_total, S, est_items, sum_items, wbytes = (v.value for v in info)
    rec1 = torch.empty(K * NREC, dtype=torch.uint8, device="cuda")
    rec2 = torch.empty(K * NREC, dtype=torch.uint8, device="cuda")
    y = torch.empty(out_total, dtype=torch.complex64, device="cuda")
    f0 = torch.empty(K, dtype=torch.float64, device="cuda")
    freq1 = rec1.view(torch.float64).view(K, NREC // 8)[:, 2]
    pp, p1, p2, py, pf = (P(t.data_ptr()) for t in (packed, rec1, rec2, y, f0))
    loop = TorchLoop(packed, lens, group, lag, rep)

    def method_a():
        ctx.check(lib.vsig_combine_estimate(plan, pp, None, None, 0.0, p1), "estimate")
        ctx.check(lib.vsig_combine_sum(plan, pp, p1, py), "sum")
        f0.copy_(freq1)
        ctx.check(lib.vsig_combine_estimate(plan, pp, py, pf, 0.0, p2), "estimate")

    try:
        method_a()
        got = loop.run()
        torch.cuda.synchronize()
        r1 = rec1.cpu().numpy().view(_lib.COMBINE_MEMBER)
        n_sum = int(r1["n"].sum())
        ya, diff_y, diff_a = y.cpu().numpy(), 0.0, 0.0
        off = np.r_[0, np.cumsum(lens[rep])]
        for g, (yb, a, _, _, _) in enumerate(got):
            yb = yb.cpu().numpy()
            diff_y = max(diff_y, float(np.abs(ya[off[g]:off[g + 1]] - yb).max() / np.abs(yb).max()))
            mem = np.flatnonzero(group == g)
            aa = r1["a_re"][mem] + 1j * r1["a_im"][mem]
            diff_a = max(diff_a, float((np.abs(aa - a.cpu().numpy()) / np.abs(aa)).max()))
        assert diff_y <= 1e-4 and diff_a <= 1e-4, (diff_y, diff_a)
        for _ in range(warmup):
            method_a()
            loop.run()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            for method, times in ((method_a, ta), (loop.run, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                method()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
    finally:
        lib.vsig_combine_free(plan)
    stat = lambda t: (statistics.median(t), min(t), max(t))    # noqa: E731
    nbytes = 8.0 * (3 * n_sum + 2 * out_total)
    return dict(K=K, L=L, G=G, S=S, est_items=est_items, sum_items=sum_items, wbytes=wbytes, a=stat(ta), b=stat(tb),
                diff_y=diff_y, diff_a=diff_a, create_ms=create_ms, nbytes=nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[512, 16384, 32, 24, 3000, 3], help="K L G triples")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "combine_ab.md"),
                    help="where the table goes (profiles/combine_ab.md holds a table of this tool's and the notes "
                         "written around it: it is not the default)")
    a = ap.parse_args()
    ctx = va.get_context(0)
    rows = []
    for K, L, G in zip(a.shapes[0::3], a.shapes[1::3], a.shapes[2::3]):
        rows.append(case(ctx, K, L, G, a.warmup, a.reps))
        print(rows[-1], flush=True)
        torch.cuda.empty_cache()
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"    # noqa: E731
    lines = [
        "# Grouped bursts averaged through `vsig_combine_*` against a per-group loop of torch ops",
        "",
        f"`tools/combine_ab.py`, one MI355X ({torch.cuda.get_device_name(0)}), K bursts of L samples in G groups.  "
        f"Medians (min-max) of {a.reps}",
        f"alternating runs after {a.warmup} warm-up runs, HIP events on the stream for both.  A: estimate, sum, estimate "
        "on one plan.",
        "B: per group, the members gathered at their lags and the same sums, gains and weighted sum as torch ops.  A's",
        "packets and gains equal B's at 1e-4 (asserted).  Bytes: 8 B (3 sum n_k + 2 sum L_g), algorithmic, no counter",
        f"behind them; the roof is {ROOF_TBS:g} TB/s.",
        "",
        "| K | L | G | S | estimate items | sum items | A ms | algorithmic MB | TB/s | share of roof | B ms | A / B | "
        "max diff y | max diff a | create ms |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        tbs = r["nbytes"] / r["a"][0] / 1e9
        lines.append(f"| {r['K']} | {r['L']} | {r['G']} | {r['S']} | {r['est_items']} | {r['sum_items']} | {fmt(r['a'])} | "
                     f"{r['nbytes'] / 1e6:.1f} | {tbs:.3f} | {100 * tbs / ROOF_TBS:.1f} % | {fmt(r['b'])} | "
                     f"{r['a'][0] / r['b'][0]:.2e} | {r['diff_y']:.1e} | {r['diff_a']:.1e} | {r['create_ms']:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
