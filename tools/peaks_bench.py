"""Time vsig_peaks_dev at 2**28 complex64 samples against vsig_peak_dev (the
global-argmax reduction) on the same array, in one process:

  sparse   seeded noise with 64 planted peaks, ratio 0.5, min_distance 1e5:
           the case a correlation of a packet over a vector gives
  dense    the same noise, threshold 0 (every element a candidate), same d
  flat     2**28 equal values, ratio 0.5, same d: every element at the
           threshold and tied (a tone's |c|)
  peak     vsig_peak_dev on the sparse array: the yardstick, because it and
           the peak list's tile pass each read the array exactly once

Device times are HIP-event medians over --reps runs after --warmup runs, the
two entry points alternating so that both see the same clock and neighbours.
Bytes: 8 B per sample read once (the tile table adds 32 B per 2048 samples).
The instance lists are checked: the sparse case must return the planted
indices, the flat case index 0.

    python tools/peaks_bench.py [--log2n 28] [--out profiles/peaks_bench.jsonl]
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
    ap.add_argument("--min-distance", type=int, default=100000)
    ap.add_argument("--planted", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, d, cap = 1 << a.log2n, a.min_distance, 4096
    ctx = va.get_context(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    # noise |x| stays below ~6.5; the planted peaks sit at 40, 2 d + 1 apart or more
    step = max(n // a.planted, 2 * d + 1)
    planted = torch.arange(a.planted, device="cuda") * step + 12345
    planted = planted[planted < n]
    x[planted] = 40.0
    flat = torch.full((n,), 0.75 + 0j, dtype=torch.complex64, device="cuda")
    rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    info = torch.empty(4, dtype=torch.int64, device="cuda")
    pk = torch.empty(4, dtype=torch.float64, device="cuda")
    ctx.bind_stream()
    c64 = _lib.DTYPES["c64"]

    def peaks(t, thr, rel):
        ctx.check(ctx.lib.vsig_peaks_dev(ctx.h, c64, C.c_void_p(t.data_ptr()), n, thr, rel, d,
                                         C.c_void_p(rec.data_ptr()), cap, C.c_void_p(info.data_ptr())), "peaks")

    def peak():
        ctx.check(ctx.lib.vsig_peak_dev(ctx.h, c64, C.c_void_p(x.data_ptr()), n, C.c_void_p(pk.data_ptr())),
                  "peak")

    try:
        clock = f"{torch.cuda.clock_rate()} MHz (torch.cuda.clock_rate before timing)"
    except Exception:                                        # noqa: BLE001
        clock = "not read"
    rows = []

    def row(name, t, count):
        med, lo, hi = t
        r = dict(name=name, n=n, min_distance=d, instances=count, ms_median=round(med, 4),
                 ms_min=round(lo, 4), ms_max=round(hi, 4), tbs=round(8 * n / med / 1e9, 3))
        rows.append(r)
        print(json.dumps(r), flush=True)

    cases = [("sparse", x, 0.5, 1), ("dense", x, 0.0, 0), ("flat", flat, 0.5, 1)]
    res = {}
    for name, t, thr, rel in cases:
        tp, ty = timed_pair([lambda: peaks(t, thr, rel), peak], a.warmup, a.reps)
        count = int(info[0])
        got = rec[:min(count, cap), 0]
        if name == "sparse":
            assert torch.equal(got, planted), "sparse: the planted peaks were not returned"
        if name == "flat":
            assert got.tolist() == [0], "flat: instance 0 alone expected"
        row(name, tp, count)
        row(f"peak_beside_{name}", ty, 1)
        res[name] = (tp[0], ty[0])
    summary = dict(name="summary", n=n, min_distance=d, clock=clock, tile=ctx.lib.vsig_peaks_tile(),
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
