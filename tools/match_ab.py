"""Time the all-pairs burst similarity in one pass against what a caller could do
before it existed, in one process:

  A    one vsig_match_run: K spectra, then every pair's product, transform and
       first maximum on a persistent grid (K + K (K - 1) / 2 transforms)
  B    the loop: correlate_peak(p_b, p_a, "full") for every a < b on device
       tensors (a handle, two transforms of the stream side, the exact-argmax
       refine and a host read per call)

for K packets of L unit-modulus random-phase samples.  A is timed by HIP events
on the stream; B reads its result on the host after every call, so it is timed
on the host clock between two device synchronisations: that is what the caller
waits for.  A and B alternate inside every repetition and the medians (min-max)
are reported.  Where the loop has more than --b-pairs pairs, B runs that many
of them, spread evenly over the list, and its time is scaled to all pairs: the
column says so.  Before timing, A's peak equals B's at 1e-5 relative on the
pairs B ran (asserted).

Transforms per second: (K + pairs) / A's median.  Flops: 5 N log2 N a transform,
plus 9 N a pair (the spectrum product and |c|^2); the FP32 roof is 157.3 TFLOP/s
(256 CUs x 128 lanes x 2 x 2.4 GHz).  A manual tool: run it under its own time
limit on one GPU, e.g.

    timeout -k 10 600 python tools/match_ab.py [--out out/match_ab.md]
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

ROOF_TFLOPS = 157.3
P = C.c_void_p


def case(ctx, K, L, warmup, reps, b_pairs):
    lib = ctx.lib
    gen = torch.Generator(device="cuda").manual_seed(K + L)
    ph = torch.rand(K * L, generator=gen, device="cuda", dtype=torch.float32) * (2 * math.pi)
    packed = torch.polar(torch.ones_like(ph), ph).contiguous()
    pk = [packed[k * L:(k + 1) * L] for k in range(K)]
    lens = np.full(K, L, np.int64)
    peak = torch.empty((K, K), dtype=torch.float32, device="cuda")
    lag = torch.empty((K, K), dtype=torch.int32, device="cuda")
    energy = torch.empty(K, dtype=torch.float64, device="cuda")
    ctx.bind_stream()
    plan = P()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.check(lib.vsig_match_create(ctx.h, lens.ctypes.data_as(C.POINTER(C.c_int64)), K, C.byref(plan)), "create")
    create_ms = (time.perf_counter() - t0) * 1e3
    n = C.c_int32()
    info = [C.c_int64() for _ in range(4)]
    ctx.check(lib.vsig_match_info(plan, C.byref(n), *(C.byref(v) for v in info)), "info")
    N, (pairs, units, grid, wbytes) = n.value, (v.value for v in info)
    every = [(a, b) for a in range(K) for b in range(a + 1, K)]
    ran = every if pairs <= b_pairs else [every[i] for i in np.linspace(0, pairs - 1, b_pairs).astype(np.int64)]
    ptrs = (P(packed.data_ptr()), P(peak.data_ptr()), P(lag.data_ptr()), P(energy.data_ptr()))
    got = {}

    def method_a():
        ctx.check(lib.vsig_match_run(plan, *ptrs), "match")

    def method_b():
        for a, b in ran:
            got[a, b] = va.correlate_peak(pk[b], pk[a], "full")

    try:
        method_a()
        method_b()
        torch.cuda.synchronize()
        pa, la = peak.cpu().numpy(), lag.cpu().numpy()
        diff = max(abs(pa[a, b] - v[1]) / v[1] for (a, b), v in got.items())
        assert diff <= 1e-5, diff
        lags_equal = sum(int(la[a, b] == v[0]) for (a, b), v in got.items())
        for _ in range(warmup):
            method_a()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            method_a()
            e1.record()
            e1.synchronize()
            ta.append(e0.elapsed_time(e1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            method_b()
            torch.cuda.synchronize()
            tb.append((time.perf_counter() - t0) * 1e3 * pairs / len(ran))
    finally:
        lib.vsig_match_free(plan)
    stat = lambda t: (statistics.median(t), min(t), max(t))    # noqa: E731
    flops = (K + pairs) * 5.0 * N * math.log2(N) + pairs * 9.0 * N
    return dict(K=K, L=L, N=N, pairs=pairs, units=units, grid=grid, wbytes=wbytes, a=stat(ta), b=stat(tb),
                b_ran=len(ran), diff=diff, lags_equal=lags_equal, create_ms=create_ms, flops=flops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[64, 2048, 1024, 512], help="K L pairs")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--b-pairs", type=int, default=2016, help="pairs the loop runs at most (scaled to all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "match_ab.md"),
                    help="where the table goes (profiles/match_ab.md holds a table of this tool's and the notes "
                         "written around it: it is not the default)")
    a = ap.parse_args()
    ctx = va.get_context(0)
    rows = []
    for K, L in zip(a.shapes[0::2], a.shapes[1::2]):
        rows.append(case(ctx, K, L, a.warmup, a.reps, a.b_pairs))
        print(rows[-1], flush=True)
        torch.cuda.empty_cache()
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"    # noqa: E731
    lines = [
        "# All pairs in one pass (`vsig_match_run`) against a loop of `correlate_peak`",
        "",
        f"`tools/match_ab.py`, one MI355X ({torch.cuda.get_device_name(0)}), K packets of L unit-modulus samples.  "
        f"Medians (min-max) of {a.reps}",
        f"alternating runs after {a.warmup} warm-up runs.  A: one `vsig_match_run`, HIP events.  B: `correlate_peak` for "
        "every a < b on",
        "device tensors, host clock between two synchronisations (every call reads its record on the host); where B ran",
        "fewer pairs than there are, its time is scaled by pairs / ran.  A's peaks equal B's at 1e-5 on the pairs B ran",
        f"(asserted).  Flops: 5 N log2 N a transform and 9 N a pair; the FP32 roof is {ROOF_TFLOPS:g} TFLOP/s.",
        "",
        "| K | L | N | pairs | units | grid | A ms | transforms / s | TFLOP/s | share of roof | B ms | B ran | A / B | "
        "max diff | lags equal | create ms |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        tf = r["flops"] / r["a"][0] / 1e9
        lines.append(f"| {r['K']} | {r['L']} | {r['N']} | {r['pairs']} | {r['units']} | {r['grid']} | {fmt(r['a'])} | "
                     f"{(r['K'] + r['pairs']) / r['a'][0] * 1e3:.3e} | {tf:.2f} | {100 * tf / ROOF_TFLOPS:.1f} % | "
                     f"{fmt(r['b'])} | {r['b_ran']} | {r['a'][0] / r['b'][0]:.2e} | {r['diff']:.1e} | "
                     f"{r['lags_equal']} / {r['b_ran']} | {r['create_ms']:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    late = [f"K {r['K']} L {r['L']}: {r['a'][0]:.3f} ms against {r['b'][0]:.3f} ms" for r in rows
            if r["a"][0] > r["b"][0]]
    if late:
        sys.exit("gate: A's median is above the loop's at " + "; ".join(late))


if __name__ == "__main__":
    main()
