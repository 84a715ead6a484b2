"""Time vsig_trace_envelope_dev on a whole-capture spectrum line against what a
caller could do before it existed, in one process:

  A   vsig_trace_envelope_dev(shift=1, 2048 columns, VSIG_TRACE_DB20): one
      pass, 8 B read per complex64 sample, 2 x 2048 floats written
  B   vsig_abs_c64_dev into a scratch array (|a| + 0j: 8 B read + 8 B
      written per sample), torch.roll of its real part (8 B strided read,
      4 B written), torch.amin / torch.amax over the (cols, bin) view (4 B read
      each), 20 log10(. + eps) of the 2 x 2048 results: about 36 B per sample

for 2^26 and 2^28 complex64 samples (the larger one only if it fits).  Device
times are HIP-event medians (min-max) over --reps runs after --warmup runs; A
and B alternate inside every repetition, so both see the same clock and the
same neighbours.  Before timing, A's VSIG_TRACE_ABS envelope must equal B's
bit for bit and the dB planes must agree to 1e-4 dB.  A manual tool: run it
under its own time limit on one GPU, e.g.

    timeout -k 10 600 python tools/trace_ab.py [--log2n 26 28] [--out profiles/trace_ab.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vector_amd as va  # noqa: E402
from vector_amd import _lib  # noqa: E402

ROOF_TBS = 8.0            # MI355X HBM3E peak
COLS, EPS = 2048, 1e-12


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


def case(ctx, log2n, warmup, reps):
    n = 1 << log2n
    bin_ = n // COLS
    gen = torch.Generator(device="cuda").manual_seed(log2n)
    x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    scratch = torch.empty_like(x)
    emin = torch.empty(COLS, dtype=torch.float32, device="cuda")
    emax = torch.empty(COLS, dtype=torch.float32, device="cuda")
    info = torch.empty(4, dtype=torch.int64, device="cuda")
    ctx.bind_stream()
    c64 = _lib.DTYPES["c64"]
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    out_b = {}

    def method_a(kind=_lib.TRACE_DB20):
        ctx.check(ctx.lib.vsig_trace_envelope_dev(ctx.h, c64, ptr(x), n, 1, 0, n, bin_, kind, EPS, ptr(emin),
                                                  ptr(emax), ptr(info)), "trace envelope")

    def method_b(db=True):
        ctx.check(ctx.lib.vsig_abs_c64_dev(ctx.h, c64, ptr(x), n, ptr(scratch)), "abs")
        m = torch.roll(torch.view_as_real(scratch)[:, 0], n // 2).view(COLS, bin_)      # fftshift, even n
        lo, hi = torch.amin(m, dim=1), torch.amax(m, dim=1)
        if db:
            lo, hi = 20 * torch.log10(lo + EPS), 20 * torch.log10(hi + EPS)
        out_b["lo"], out_b["hi"] = lo, hi

    method_a(_lib.TRACE_ABS)
    method_b(False)
    torch.cuda.synchronize()
    assert torch.equal(emin, out_b["lo"]) and torch.equal(emax, out_b["hi"]), "ABS envelopes differ"
    method_a()
    method_b()
    torch.cuda.synchronize()
    ddb = max(float((emin - out_b["lo"]).abs().max()), float((emax - out_b["hi"]).abs().max()))
    assert ddb <= 1e-4, ddb
    ta, tb = timed_pair([method_a, method_b], warmup, reps)
    del x, scratch, out_b
    torch.cuda.empty_cache()
    return dict(log2n=log2n, n=n, bin=bin_, a=ta, b=tb, ddb=ddb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_ab.md"))
    a = ap.parse_args()
    ctx = va.get_context(0)
    rows = []
    for log2n in a.log2n:
        free = torch.cuda.mem_get_info()[0]
        if 24 * (1 << log2n) > free:                         # x, scratch, the rolled line and slack
            print(f"2^{log2n} samples do not fit ({free >> 20} MiB free): skipped", flush=True)
            continue
        rows.append(case(ctx, log2n, a.warmup, a.reps))
        print(rows[-1], flush=True)
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"    # noqa: E731
    lines = [
        "# Line-trace envelope (`vsig_trace_envelope_dev`) against abs + roll + amin / amax",
        "",
        f"`tools/trace_ab.py`, one MI355X, complex64 samples, `shift = 1`, {COLS} columns, `VSIG_TRACE_DB20`,",
        f"eps {EPS:g}.  HIP-event medians (min-max) of {a.reps} runs after {a.warmup} warm-up runs; the two",
        "methods alternate inside every repetition.  A: the fused kernels",
        "(`trace_chunks`, `trace_merge`, `trace_info`).  B: `vsig_abs_c64_dev` into a scratch array,",
        "`torch.roll` of its real part, `torch.amin` / `torch.amax` over the `(cols, bin)` view, the dB map of",
        "the 2 x 2048 results.  The ABS envelopes of both are bit-equal and the dB planes agree to the",
        "difference shown (asserted by the tool).  TB/s is 8 B per sample over A's whole call; the roof is",
        f"{ROOF_TBS:g} TB/s.",
        "",
        "| samples | bin | A ms | A TB/s | share of roof | B ms | A / B | max dB difference |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        tbs = 8 * r["n"] / r["a"][0] / 1e9
        lines.append(f"| 2^{r['log2n']} | {r['bin']} | {fmt(r['a'])} | {tbs:.2f} | {100 * tbs / ROOF_TBS:.0f} % | "
                     f"{fmt(r['b'])} | {r['a'][0] / r['b'][0]:.3f} | {r['ddb']:.1e} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
