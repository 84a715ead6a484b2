"""Time vsig_psd_traces_c64_dev (mean / max-hold / min-hold of the block PSD in
one pass) against what a caller could do before it existed, in one process:

  A   vsig_psd_traces_c64_dev, all three detectors: 8 B read per complex64
      sample, O(nfft) written
  B   vsig_psd_c64_dev into an (nframes, nfft) float32 tensor (8 B read + 4 B
      written per sample), then torch.mean(dtype=float64), torch.amax and
      torch.amin over the frame axis (4 B read each): 16 to 24 B per sample
  C   vsig_psd_c64_dev alone, for scale

for complex64 noise of 2^26 and 2^28 samples, nfft 1024 and 8192, hop = nfft,
Hann window.  Device times are HIP-event medians (min-max) over --reps runs
after --warmup runs; A, B and C alternate inside every repetition, so all see
the same clock and the same neighbours.  Before timing, A's outputs are held
against B's: both are fp32 transforms within K e_ref of the complex128
spectrogram (tests/test_gpu_spectrum_traces.py's bound, K = 3 below 4096 points
and 8 from there), so they differ by at most 2 K e_ref plus a float32 rounding;
e_ref = max |S32 - S64| is taken with scipy.fft on the capture's first 64
frames (the input is stationary).  A manual tool: run it under its own time
limit on one GPU, e.g.

    timeout -k 10 600 python tools/psd_traces_ab.py [--log2n 26 28] [--out profiles/psd_traces_ab.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import scipy.fft
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vector_amd as va  # noqa: E402

ROOF_TBS = 8.0            # MI355X HBM3E peak
REF_FRAMES = 64


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


def reference_error(x_host, w32, nfft, scale):
    """max |S32 - S64| of the first frames, scipy.fft in complex64 / complex128."""
    fr = x_host.reshape(-1, nfft)
    X32 = scipy.fft.fft(fr * w32[None, :], axis=1)
    X64 = scipy.fft.fft(fr.astype(np.complex128) * w32.astype(np.float64)[None, :], axis=1)
    assert X32.dtype == np.complex64
    S32 = (X32.real * X32.real + X32.imag * X32.imag) * np.float32(scale)
    S64 = (X64.real * X64.real + X64.imag * X64.imag) * scale
    return float(np.abs(S32.astype(np.float64) - S64).max())


def case(ctx, log2n, nfft, warmup, reps):
    n = 1 << log2n
    nframes = n // nfft
    gen = torch.Generator(device="cuda").manual_seed(log2n + nfft)
    x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    w32 = scipy.signal.get_window("hann", nfft).astype(np.float32)
    scale = float(1.0 / float(np.sum(w32, dtype=np.float64)) ** 2)
    wd = torch.from_numpy(w32).cuda()
    S = torch.empty((nframes, nfft), dtype=torch.float32, device="cuda")
    mean = torch.empty(nfft, dtype=torch.float64, device="cuda")
    mx = torch.empty(nfft, dtype=torch.float32, device="cuda")
    mn = torch.empty(nfft, dtype=torch.float32, device="cuda")
    ctx.bind_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    out_b = {}

    def method_a():
        ctx.check(ctx.lib.vsig_psd_traces_c64_dev(ctx.h, ptr(x), n, 1, ptr(wd), nfft, nfft, nfft, scale, 0,
                                                  nframes, ptr(mean), ptr(mx), ptr(mn)), "psd traces")

    def method_c():
        ctx.check(ctx.lib.vsig_psd_c64_dev(ctx.h, ptr(x), n, 1, ptr(wd), nfft, nfft, nfft, scale, 0, ptr(S),
                                           nframes), "psd")

    def method_b():
        method_c()
        out_b["mean"] = torch.mean(S, dim=0, dtype=torch.float64)
        out_b["max"] = torch.amax(S, dim=0)
        out_b["min"] = torch.amin(S, dim=0)

    method_a()
    method_b()
    torch.cuda.synchronize()
    K = 8.0 if nfft >= 4096 else 3.0
    e_ref = reference_error(x[:REF_FRAMES * nfft].cpu().numpy(), w32, nfft, scale)
    worst = 0.0
    for name, got in (("mean", mean), ("max", mx), ("min", mn)):
        want = out_b[name].to(torch.float64)
        d = float((got.to(torch.float64) - want).abs().max())
        lim = 2 * K * e_ref + 2.0 ** -23 * float(want.abs().max())
        assert d <= lim, (name, d, lim)
        worst = max(worst, d / lim)
    ta, tb, tc = timed([method_a, method_b, method_c], warmup, reps)
    blocks, step, run = (C.c_int64() for _ in range(3))
    ctx.lib.vsig_psd_traces_plan(nfft, nframes, C.byref(blocks), C.byref(step), C.byref(run))
    del x, S, out_b
    torch.cuda.empty_cache()
    return dict(log2n=log2n, n=n, nfft=nfft, nframes=nframes, a=ta, b=tb, c=tc, agree=worst,
                blocks=blocks.value, run=run.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--nfft", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psd_traces_ab.md"))
    a = ap.parse_args()
    ctx = va.get_context(0)
    rows = []
    for log2n in a.log2n:
        for nfft in a.nfft:
            free = torch.cuda.mem_get_info()[0]
            if 20 * (1 << log2n) > free:                         # x, the spectrogram, torch's temporaries
                print(f"2^{log2n} samples do not fit ({free >> 20} MiB free): skipped", flush=True)
                continue
            rows.append(case(ctx, log2n, nfft, a.warmup, a.reps))
            print(rows[-1], flush=True)
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"    # noqa: E731
    lines = [
        "# Spectrum traces (`vsig_psd_traces_c64_dev`) against PSD + mean / amax / amin",
        "",
        "`tools/psd_traces_ab.py`, one MI355X, complex64 noise, `hop = nfft`, Hann window, all three detectors.",
        f"HIP-event medians (min-max) of {a.reps} runs after {a.warmup} warm-up runs; A, B and C alternate inside",
        "every repetition.  A: the fused call (the transform kernel with the reducing epilogue, then the merge).",
        "B: `vsig_psd_c64_dev` into an `(nframes, nfft)` float32 tensor, then `torch.mean(dtype=float64)`,",
        "`torch.amax`, `torch.amin` over the frame axis.  C: `vsig_psd_c64_dev` alone.  TB/s is 8 B per sample",
        f"over A's whole call; the roof is {ROOF_TBS:g} TB/s.  Agreement: the largest |A - B| over the three",
        "detectors as a share of its bound, 2 K e_ref plus a float32 rounding (asserted by the tool before",
        "timing).  blocks x run: A's grid and the frames a block owns (`vsig_psd_traces_plan`).",
        "",
        "| samples | nfft | blocks x run | A ms | A TB/s | share of roof | B ms | A / B | C ms | A / C | agreement |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        tbs = 8 * r["n"] / r["a"][0] / 1e9
        lines.append(f"| 2^{r['log2n']} | {r['nfft']} | {r['blocks']} x {r['run']} | {fmt(r['a'])} | {tbs:.2f} | "
                     f"{100 * tbs / ROOF_TBS:.0f} % | {fmt(r['b'])} | {r['a'][0] / r['b'][0]:.3f} | {fmt(r['c'])} | "
                     f"{r['a'][0] / r['c'][0]:.3f} | {r['agree']:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    assert all(r["a"][0] < r["b"][0] for r in rows), "gate: A must beat B at every size"


if __name__ == "__main__":
    main()
