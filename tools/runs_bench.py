"""Time vsig_runs_dev at 2**28 complex64 samples against vsig_peak_dev (the
global-argmax reduction) on the same array, in one process:

  sparse   seeded noise with 64 planted bursts of 5000 samples, ratio 0.5,
           max_gap 100: the case a capture with packets in it gives
  dense    the alternating mask (1, 0, 1, 0, ...), threshold 0.5, max_gap 0:
           n / 2 runs, every tile mixed, a small cap
  flat     2**28 equal values, ratio 0.5: every element masked, one run
  peak     vsig_peak_dev on the same array: the yardstick, because it and the
           run list's tile pass each read the array exactly once

Device times are HIP-event medians over --reps runs after --warmup runs, the
two entry points alternating so that both see the same clock and neighbours.
Bytes: 8 B per sample read once (the tile table adds 32 B per 2048 samples;
a mixed tile is read a second time and leaves 256 B of mask words).
The run lists are checked: the sparse case must return the planted bursts, the
dense case n / 2 runs of one element, the flat case [0, n - 1].

    python tools/runs_bench.py [--log2n 28] [--out profiles/runs_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vector_amd as va  # noqa: E402
from vector_amd import _lib  # noqa: E402


def timed_pair(fns, warmup, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--max-gap", type=int, default=100)
    ap.add_argument("--planted", type=int, default=64)
    ap.add_argument("--burst", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, cap = 1 << a.log2n, 4096
    ctx = va.get_context(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    # noise |x| stays below ~6.5; the planted bursts sit at 40
    step = max(n // a.planted, 2 * a.burst)
    planted = torch.arange(a.planted, device="cuda") * step + 12345
    planted = planted[planted + a.burst <= n]
    for s in planted.tolist():
        x[s:s + a.burst] = 40.0
    alt = torch.zeros(n, dtype=torch.complex64, device="cuda")
    alt[0::2] = 1.0
    flat = torch.full((n,), 0.75 + 0j, dtype=torch.complex64, device="cuda")
    rec = torch.empty((cap, 5), dtype=torch.int64, device="cuda")
    info = torch.empty(5, dtype=torch.int64, device="cuda")
    pk = torch.empty(4, dtype=torch.float64, device="cuda")
    ctx.bind_stream()
    c64 = _lib.DTYPES["c64"]

    def runs(t, thr, rel, gap):
        ctx.check(ctx.lib.vsig_runs_dev(ctx.h, c64, C.c_void_p(t.data_ptr()), n, thr, rel, gap,
                                        C.c_void_p(rec.data_ptr()), cap, C.c_void_p(info.data_ptr())), "runs")

    def peak(t):
        ctx.check(ctx.lib.vsig_peak_dev(ctx.h, c64, C.c_void_p(t.data_ptr()), n, C.c_void_p(pk.data_ptr())),
                  "peak")

    try:
        clock = f"{torch.cuda.clock_rate()} MHz (torch.cuda.clock_rate before timing)"
    except Exception:                                        # noqa: BLE001
        clock = "not read"
    rows = []

    def row(name, t, count, gap):
        med, lo, hi = t
        r = dict(name=name, n=n, max_gap=gap, runs=count, ms_median=round(med, 4),
                 ms_min=round(lo, 4), ms_max=round(hi, 4), tbs=round(8 * n / med / 1e9, 3))
        rows.append(r)
        print(json.dumps(r), flush=True)

    cases = [("sparse", x, 0.5, 1, a.max_gap), ("dense", alt, 0.5, 0, 0), ("flat", flat, 0.5, 1, a.max_gap)]
    res = {}
    for name, t, thr, rel, gap in cases:
        tp, ty = timed_pair([lambda: runs(t, thr, rel, gap), lambda: peak(t)], a.warmup, a.reps)
        count, covered = int(info[0]), int(info[1])
        got = rec[:min(count, cap)]
        if name == "sparse":
            assert torch.equal(got[:, 0], planted) and torch.equal(got[:, 1], planted + a.burst - 1), \
                "sparse: the planted bursts were not returned"
            assert covered == len(planted) * a.burst
        if name == "dense":
            assert count == covered == n // 2 and torch.equal(got[:, 0], got[:, 1])
            assert torch.equal(got[:, 0], torch.arange(cap, device="cuda") * 2), "dense: runs 0, 2, 4, ... expected"
        if name == "flat":
            assert got[:, :2].tolist() == [[0, n - 1]] and covered == n, "flat: the run [0, n - 1] alone expected"
        row(name, tp, count, gap)
        row(f"peak_beside_{name}", ty, 1, gap)
        res[name] = (tp[0], ty[0])
    summary = dict(name="summary", n=n, clock=clock, tile=ctx.lib.vsig_runs_tile(),
                   sparse_over_peak=round(res["sparse"][0] / res["sparse"][1], 3),
                   dense_over_peak=round(res["dense"][0] / res["dense"][1], 3),
                   flat_over_peak=round(res["flat"][0] / res["flat"][1], 3))
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
