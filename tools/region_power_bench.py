"""Time vsig_region_power_dev on two operands of 2**26 complex64 samples against
what a caller could do before it existed, in one process:

  A   vsig_region_power_dev(a, b): one pass, 16 B read per sample, three sums
  B   vsig_peak_dev(a), vsig_peak_dev(b), torch's complex64 a - b into a
      temporary, vsig_peak_dev(a - b): the same three sums (sum_abs2 of each
      record) from three reductions and a materialised difference, 48 B of
      traffic per sample

Device times are HIP-event medians (min-max) over --reps runs after --warmup
runs; A and B alternate inside every repetition, so both see the same clock
and the same neighbours.  The two methods' sums are compared (relative 1e-6:
vsig_peak_dev squares |x| in double, A squares in float32 as numpy does).
A manual tool: run it under its own time limit on one GPU, e.g.

    timeout -k 10 300 python tools/region_power_bench.py [--log2n 26] [--out rows.jsonl]
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
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--offset", type=int, default=0, help="sample offset of both operands in their buffers")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = 1 << a.log2n
    ctx = va.get_context(0)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def operand():
        buf = torch.view_as_complex(torch.randn((n + a.offset, 2), generator=gen, device="cuda",
                                                dtype=torch.float32))
        return buf[a.offset:]

    x, y = operand(), operand()
    sums = torch.empty(3, dtype=torch.float64, device="cuda")
    pk = torch.empty((3, 4), dtype=torch.float64, device="cuda")
    ctx.bind_stream()
    c64 = _lib.DTYPES["c64"]
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def method_a():
        ctx.check(ctx.lib.vsig_region_power_dev(ctx.h, ptr(x), ptr(y), n, ptr(sums)), "region power")

    def method_b():
        ctx.check(ctx.lib.vsig_peak_dev(ctx.h, c64, ptr(x), n, ptr(pk[0])), "peak")
        ctx.check(ctx.lib.vsig_peak_dev(ctx.h, c64, ptr(y), n, ptr(pk[1])), "peak")
        d = x - y
        ctx.check(ctx.lib.vsig_peak_dev(ctx.h, c64, ptr(d), n, ptr(pk[2])), "peak")

    try:
        clock = f"{torch.cuda.clock_rate()} MHz (torch.cuda.clock_rate before timing)"
    except Exception:                                        # noqa: BLE001
        clock = "not read"
    ta, tb = timed_pair([method_a, method_b], a.warmup, a.reps)
    got, want = sums.cpu().tolist(), pk[:, 3].cpu().tolist()
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-6 * w, (got, want)
    rows = [dict(name="A region_power", n=n, offset=a.offset, ms_median=round(ta[0], 4), ms_min=round(ta[1], 4),
                 ms_max=round(ta[2], 4), tbs_16B=round(16 * n / ta[0] / 1e9, 3)),
            dict(name="B 3 x peak + subtract", n=n, offset=a.offset, ms_median=round(tb[0], 4),
                 ms_min=round(tb[1], 4), ms_max=round(tb[2], 4), tbs_48B=round(48 * n / tb[0] / 1e9, 3)),
            dict(name="summary", n=n, offset=a.offset, clock=clock, a_over_b=round(ta[0] / tb[0], 3),
                 warmup=a.warmup, reps=a.reps)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
