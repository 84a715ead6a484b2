"""Time vsig_vector_build_dev at 2**28 samples against what a caller could do
without it, in one process:

  build        one vsig_vector_build_dev launch (no max), the same with the
               fused max, and build + max + vsig_normalize_c64_dev
  torch loop   (a) the per-instance  v[a:b] += y  on the GPU (one launch each)
  numpy loop   (b) the reference's loop on the host

The packet mix is the golden fixture's (tests/golden/vector_build.npz: six
packets of 777..4101 samples, periods of 20k..45k samples), i.e. ~50k instances
in 2**28 samples.  Device times are HIP-event medians over --reps runs after
--warmup runs; the numpy loop is timed once per --host-reps with a host clock.
Bytes: the build writes 8 B per sample once (the packets are re-read from L2).
The write ceiling is the HBM rate of tools/membw.py's best non-temporal-store
copy probe on this box (bytes read + written per second; run here as a child
process when libvsig_tune.so is built, else --ceiling-gbs, else not reported).
torch's zero fill of the same vector, a pure write, is timed beside it.

    python tools/vector_build_bench.py [--log2n 28] [--out profiles/vector_build_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vector_amd as va  # noqa: E402
from vector_amd import _lib  # noqa: E402


def device_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def nt_copy_ceiling():
    """(GB/s moved by the best non-temporal-store copy probe, its name) from
    tools/membw.py in a child process, or None."""
    if not os.path.exists(os.path.join(ROOT, "vector_amd", "libvsig_tune.so")):
        return None
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "membw.py")], capture_output=True,
                           text=True, timeout=300)
        res = json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:                                   # noqa: BLE001
        print(f"membw.py gave no result ({e})", file=sys.stderr)
        return None
    nt = {k: v[1] for k, v in res.items() if k.startswith("probe_") and ("_nt_" in k or k.endswith("_nts"))}
    best = max(nt, key=nt.get)
    return nt[best], best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--ceiling-gbs", type=float, default=0.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = 1 << a.log2n
    g = np.load(os.path.join(ROOT, "tests", "golden", "vector_build.npz"))
    sr = float(g["sample_rate"])
    host = [g[f"packet{i}"] for i in range(len(g["files"]))]
    cfgs = [dict(length=len(y), pre_samples=int(g["pre_samples"][i]), freq_shift=0,
                 period=float(g["period"][i]), start_time=float(g["start_time"][i]))
            for i, y in enumerate(host)]
    plan = va.vector_plan(cfgs, (n + 0.5) / sr, sr)
    assert plan.total_samples == n
    ninst = sum(c for _, _, c in plan.places)
    ctx = va.get_context(0)
    dev = [torch.from_numpy(y).cuda() for y in host]
    places = (_lib.PacketPlace * len(dev))()
    for p, y, (s, per, c) in zip(places, dev, plan.places):
        p.y, p.len, p.start, p.period, p.count = y.data_ptr(), y.numel(), s, per, c
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    mx = torch.empty(1, dtype=torch.float32, device="cuda")
    ctx.bind_stream()

    def build(maxp=None):
        ctx.check(ctx.lib.vsig_vector_build_dev(ctx.h, places, len(dev), C.c_void_p(out.data_ptr()), n,
                                                maxp), "vector_build")

    def build_norm():
        build(C.c_void_p(mx.data_ptr()))
        ctx.check(ctx.lib.vsig_normalize_c64_dev(ctx.h, C.c_void_p(out.data_ptr()), n,
                                                 C.c_void_p(mx.data_ptr()), C.c_void_p(out.data_ptr())),
                  "normalize")

    v = torch.empty(n, dtype=torch.complex64, device="cuda")

    def torch_loop():
        v.zero_()
        for y, (s, per, c) in zip(dev, plan.places):
            m = y.numel()
            for k in range(c):
                v[s + k * per:s + k * per + m] += y

    try:
        clock = f"{torch.cuda.clock_rate()} MHz (torch.cuda.clock_rate before timing)"
    except Exception:                                        # noqa: BLE001
        clock = "not read"
    rows = []

    def row(name, med, lo, hi, bytes_):
        r = dict(name=name, n=n, instances=ninst, ms_median=round(med, 4), ms_min=round(lo, 4),
                 ms_max=round(hi, 4), gbs=round(bytes_ / med / 1e6, 1))
        rows.append(r)
        print(json.dumps(r), flush=True)

    row("build", *device_ms(build, a.warmup, a.reps), 8 * n)
    row("build+max", *device_ms(lambda: build(C.c_void_p(mx.data_ptr())), a.warmup, a.reps), 8 * n)
    row("build+max+normalize", *device_ms(build_norm, a.warmup, a.reps), 24 * n)
    row("torch_fill_zero", *device_ms(v.zero_, a.warmup, a.reps), 8 * n)
    row("torch_loop", *device_ms(torch_loop, 1, a.loop_reps), 8 * n)
    build()
    same = bool(torch.equal(out, v))                         # the torch loop adds in the same order
    ts = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        hv = np.zeros(n, dtype=np.complex64)
        for y, (s, per, c) in zip(host, plan.places):
            for k in range(c):
                hv[s + k * per:s + k * per + len(y)] += y
        ts.append((time.perf_counter() - t0) * 1e3)
    row("numpy_loop_host", statistics.median(ts), min(ts), max(ts), 8 * n)
    exact = bool(np.array_equal(out.cpu().numpy(), hv))
    del hv
    by = {r["name"]: r for r in rows}
    summary = dict(name="summary", n=n, instances=ninst, clock=clock,
                   build_equals_numpy=exact, build_equals_torch_loop=same,
                   speedup_vs_torch_loop=round(by["torch_loop"]["ms_median"] / by["build"]["ms_median"], 1),
                   build_share_of_torch_fill=round(by["torch_fill_zero"]["ms_median"] / by["build"]["ms_median"], 3),
                   speedup_vs_numpy_loop=round(by["numpy_loop_host"]["ms_median"] / by["build"]["ms_median"], 1))
    del v, out
    torch.cuda.empty_cache()
    ceil = (a.ceiling_gbs, "--ceiling-gbs") if a.ceiling_gbs > 0 else nt_copy_ceiling()
    if ceil:
        summary.update(nt_store_probe=ceil[1], write_ceiling_gbs=ceil[0],
                       build_share_of_write_ceiling=round(by["build"]["gbs"] / ceil[0], 3))
    else:
        summary.update(write_ceiling_gbs="not measured")
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
