"""Time the isolation of a burst list in one launch against what a caller could do
before it existed, in one process:

  A    one vsig_isolate_run: every burst mixed down by its own centre and
       filtered by its own low-pass, all frames of all bursts in one launch
  B    the loop: per burst one dsp.FirFilter(taps, 1, 0)(x[lo - d:hi + d],
       out=..., nhist=ntaps - 1, freq_shift=-f, sample_rate=sr, i0=lo - d), the
       handles built once per distinct filter outside the timed region, the
       outputs written in place (no copy-out)
  B0   B's library calls alone (vsig_fir_exec_mix_dev on the same handles and
       pointers, no Python front end around them): the loop at its cheapest

for K bursts of L samples at a stride of n / K in a complex64 capture of
2^--log2n samples of noise, 255 taps, 4 distinct filters, centres spread over
+-0.4 sr.  The three write the same samples (different frame grids: compared at
the FIR's 1e-5 bar before timing, the largest relative difference is reported).

Device times are HIP-event medians (min-max) over --reps runs after --warmup
runs; A, B and B0 alternate inside every repetition, so all see the same clock
and the same neighbours.  B's events bracket the whole loop, launch gaps
included: that is what the caller waits for.  The plan (vsig_isolate_create:
frame table, filter spectra, upload) is built once per burst list and is timed
apart, on the host clock.  Bytes per output sample: 8 read per frame sample
(frames x 1024) plus 8 written, over the outputs.  A manual tool: run it under
its own time limit on one GPU, e.g.

    timeout -k 10 600 python tools/isolate_ab.py [--out out/isolate_ab.md]
"""
import argparse
import ctypes as C
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
from vector_amd import packets as pk  # noqa: E402

ROOF_TBS = 8.0            # MI355X HBM3E peak
SR = 56e6
NTAPS = 255
BANDWIDTHS = (0.5e6, 2e6, 5e6, 10e6)
P = C.c_void_p


def timed(fns, warmup, reps):
    """Median / min / max ms of each fn, run in turn inside every repetition."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def case(ctx, x, n, K, L, warmup, reps):
    d = (NTAPS - 1) // 2
    rng = np.random.default_rng(K)
    lo = (n // K) * np.arange(K, dtype=np.int64) + 1001          # odd starts, clear of both ends by more than d
    hi = lo + L
    assert hi[-1] + d <= n and lo[0] >= d
    freqs = rng.uniform(-0.4, 0.4, K) * SR
    bws = np.array(BANDWIDTHS)[np.arange(K) % len(BANDWIDTHS)]
    table, taps, _ = pk.isolate_table(lo, hi, freqs, bws, SR, 0.0, NTAPS)
    assert taps.shape[0] == len(BANDWIDTHS)
    ya, yb = (torch.zeros(K * L, dtype=torch.complex64, device="cuda") for _ in "ab")
    ctx.bind_stream()
    lib = ctx.lib
    plan = P()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.check(lib.vsig_isolate_create(ctx.h, table.ctypes.data_as(C.POINTER(_lib.IsolateSeg)), K, n,
                                      taps.ctypes.data_as(C.POINTER(C.c_float)), taps.shape[0], NTAPS, SR,
                                      C.byref(plan)), "create")
    create_ms = (time.perf_counter() - t0) * 1e3
    info = [C.c_int64() for _ in range(4)]
    ctx.check(lib.vsig_isolate_info(plan, *(C.byref(v) for v in info)), "info")
    total, frames, blocks, hop = (v.value for v in info)
    assert total == K * L
    firs = [va.FirFilter(t, 1, 0) for t in taps]                  # one handle per distinct filter
    assert all(f.block == 1024 for f in firs)
    xs = [x[int(a) - d:int(b) + d] for a, b in zip(lo, hi)]
    outs = [yb[k * L:(k + 1) * L] for k in range(K)]
    fk = table["filter"].tolist()
    fl = [-float(f) for f in table["freq"]]
    xp, ap, bp = x.data_ptr(), ya.data_ptr(), yb.data_ptr()

    def method_a():
        ctx.check(lib.vsig_isolate_run(plan, P(xp), P(ap)), "isolate")

    def method_b():
        for k in range(K):
            firs[fk[k]](xs[k], out=outs[k], nhist=NTAPS - 1, freq_shift=fl[k], sample_rate=SR, i0=int(lo[k]) - d)

    def method_b0():
        for k in range(K):
            rc = lib.vsig_fir_exec_mix_dev(firs[fk[k]].h, P(xp + 8 * (int(lo[k]) - d)), NTAPS - 1, L, P(bp + 8 * k * L),
                                           L, fl[k], SR, int(lo[k]) - d)
            if rc:
                ctx.check(rc, "fir")

    try:
        method_a()
        method_b()
        torch.cuda.synchronize()
        diff = float((ya - yb).abs().max() / yb.abs().max())
        assert diff <= 1e-5, diff
        yb.zero_()
        method_b0()
        torch.cuda.synchronize()
        assert float((ya - yb).abs().max() / yb.abs().max()) <= 1e-5
        ta, tb, tb0 = timed([method_a, method_b, method_b0], warmup, reps)
    finally:
        lib.vsig_isolate_free(plan)
    return dict(K=K, L=L, frames=frames, blocks=blocks, hop=hop, a=ta, b=tb, b0=tb0, diff=diff, create_ms=create_ms,
                bytes_per_out=(8.0 * frames * 1024 + 8.0 * total) / total, total=total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1024, 4096, 64, 65536], help="K L pairs")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "isolate_ab.md"),
                    help="where the table goes (profiles/isolate_ab.md holds a table of this tool's and the notes "
                         "written around it: it is not the default)")
    a = ap.parse_args()
    ctx = va.get_context(0)
    n = 1 << a.log2n
    gen = torch.Generator(device="cuda").manual_seed(a.log2n)
    x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    rows = []
    for K, L in zip(a.shapes[0::2], a.shapes[1::2]):
        rows.append(case(ctx, x, n, K, L, a.warmup, a.reps))
        print(rows[-1], flush=True)
        torch.cuda.empty_cache()
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"    # noqa: E731
    lines = [
        "# Burst isolation in one launch (`vsig_isolate_run`) against a loop of mixed FIR calls",
        "",
        f"`tools/isolate_ab.py`, one MI355X ({torch.cuda.get_device_name(0)}), K bursts of L samples cut from 2^{a.log2n}",
        f"complex64 samples of noise, {NTAPS} taps, {len(BANDWIDTHS)} distinct filters, a centre per burst.  HIP-event "
        f"medians (min-max) of {a.reps}",
        f"runs after {a.warmup} warm-up runs; A, B and B0 alternate inside every repetition.  A: one `vsig_isolate_run`.",
        "B: one `FirFilter.__call__` (fused mixer, history) a burst, handles cached per filter, outputs in place, launch",
        "gaps included.  B0: B's `vsig_fir_exec_mix_dev` calls alone.  Before timing A's samples equal B's and B0's at the",
        "FIR's 1e-5 bar (asserted; the column is the largest relative difference).  B / out: A's bytes per output sample,",
        f"8 per frame sample read plus 8 written; TB/s: those bytes over A's median; the roof is {ROOF_TBS:g} TB/s.  create: "
        "the plan,",
        "built once per burst list, on the host clock.",
        "",
        "| K | L | frames | blocks | A ms | B / out | A TB/s | share of roof | B ms | B0 ms | A / B | A / B0 | max diff | "
        "create ms |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        tbs = r["bytes_per_out"] * r["total"] / r["a"][0] / 1e9
        lines.append(f"| {r['K']} | {r['L']} | {r['frames']} | {r['blocks']} | {fmt(r['a'])} | {r['bytes_per_out']:.1f} | "
                     f"{tbs:.3f} | {100 * tbs / ROOF_TBS:.1f} % | {fmt(r['b'])} | {fmt(r['b0'])} | "
                     f"{r['a'][0] / r['b'][0]:.4f} | {r['a'][0] / r['b0'][0]:.4f} | {r['diff']:.1e} | "
                     f"{r['create_ms']:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    # the gate: the single launch is not slower than the loop, in either form
    late = [f"K {r['K']} L {r['L']}: {r['a'][0]:.3f} ms against {min(r['b'][0], r['b0'][0]):.3f} ms" for r in rows
            if r["a"][0] > min(r["b"][0], r["b0"][0])]
    if late:
        sys.exit("gate: A's median is above the loop's at " + "; ".join(late))


if __name__ == "__main__":
    main()
