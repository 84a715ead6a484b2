"""Time the display image (vsig_spectrogram_image_dev) on a 2048 x 18707 float32
frame-major spectrogram -- create_spectrogram of 2^20 samples at 56 MHz --
against what a device-side caller could do before it existed, in one process:

  A   spectrogram_image: one kernel from Sxx to RGBA bytes.  Timed twice: the
      kernel alone (levels given; `kernel` rows, the GB/s figures) and the whole
      call with its level selection (`call` rows)
  B   normalize_spectrogram on the tensor (level selection + a full dB map),
      the shifted torch.maximum, max_pool2d when pooled, normalise, clamp to a
      table row, table gather, permute(...).contiguous()

for full size and max_size = (1024, 2048) (pool 2 x 10), with and without the
median filter.  Device times are HIP-event medians (min-max) over --reps runs
after --warmup runs; A and B alternate inside every repetition, so both see
the same clock and the same neighbours.  The kernel rows enqueue --inner calls
between the two events (a pooled call is shorter than its launch path on the
host) and rotate over three copies of the input, 460 MB, so that no read is
served from the 256 MiB Infinity Cache.  Algorithmic traffic: 4 B read + 4 B
written per cell at full size, 4 B read per cell pooled; the roof is the
6.3 TB/s a streaming kernel reaches on this part (8 TB/s peak).  A's and B's
images are compared (they round alike: under 0.1 % of the pixels may differ).
A manual tool: run it under its own time limit on one GPU, e.g.

    timeout -k 10 300 python tools/display_bench.py [--out rows.jsonl]
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vector_amd as va  # noqa: E402
from vector_amd import _lib  # noqa: E402

HBM_ROOF = 6.3e12


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
    ap.add_argument("--n-freq", type=int, default=2048)
    ap.add_argument("--n-time", type=int, default=18707)
    ap.add_argument("--max-size", type=int, nargs=2, default=(1024, 2048))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    nf, nt = a.n_freq, a.n_time
    ctx = va.get_context(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    mem = torch.empty((nt, nf), device="cuda", dtype=torch.float32).exponential_(generator=gen).pow_(3).mul_(1e-6)
    copies = [mem, mem.clone(), mem.clone()]                 # frame-major memory, 3 x 153 MB
    views = [m.t() for m in copies]                          # (n_freq, n_time), as spectrum() returns it
    lut = torch.from_numpy(va.colormap_table("turbo").copy()).to("cuda")
    floor, vmin, vmax = va.spectrogram_levels(views[0], 5, 95, 25)
    ptr = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
    f32 = _lib.DTYPES["f32"]
    ctx.bind_stream()
    rows = []
    turn = [0]

    for pooled in (False, True):
        pf, pt = va.pool_factors((nf, nt), a.max_size if pooled else None)
        r, c = -(-nf // pf), -(-nt // pt)
        out = torch.empty((r, c, 4), dtype=torch.uint8, device="cuda")
        for median in (False, True):
            def kernel():
                for _ in range(a.inner):
                    turn[0] = (turn[0] + 1) % 3
                    ctx.check(ctx.lib.vsig_spectrogram_image_dev(
                        ctx.h, f32, ptr(copies[turn[0]]), nf, nt, 1, nf, floor, float(vmin), float(vmax),
                        int(median), 0, pf, pt, ptr(lut), ptr(out)), "image")

            def call_a():
                return va.spectrogram_image(views[0], low_percentile=5, high_percentile=95, median_filter=median,
                                            cmap="turbo", max_size=a.max_size if pooled else None).rgba

            def call_b():
                db, lo, hi = va.normalize_spectrogram(views[1], 5, 95, 25)
                m = db.t()                                   # memory order: (n_time, n_freq)
                if median:
                    m = torch.maximum(m, torch.cat([m[:, :1], m[:, :-1]], dim=1))
                if pooled:
                    m = F.max_pool2d(m[None, None], kernel_size=(pt, pf), ceil_mode=True)[0, 0]
                xa = (m - float(lo)) / (float(hi) - float(lo)) * 256
                k = torch.where(xa == 256, 255.0, xa).floor_().clamp_(-1, 256).to(torch.int64)
                row = torch.where(k < 0, 256, torch.where(k > 255, 257, k))
                return lut[row].permute(1, 0, 2).contiguous()

            with contextlib.redirect_stdout(io.StringIO()):  # normalize_spectrogram's message
                ia, ib = call_a(), call_b()
                differ = float((ia != ib).any(dim=-1).float().mean())
                assert ia.shape == ib.shape == out.shape and differ < 1e-3, (ia.shape, ib.shape, differ)
                tk, ta, tb = timed_pair([kernel, call_a, call_b], a.warmup, a.reps)
            ms = tk[0] / a.inner
            traffic = nf * nt * 4 + r * c * 4
            name = f"{'pooled' if pooled else 'full'}{' median' if median else ''}"
            rows.append(dict(name=f"A kernel {name}", n_freq=nf, n_time=nt, pool=[pf, pt], median=median,
                             ms_median=round(ms, 4), ms_min=round(tk[1] / a.inner, 4),
                             ms_max=round(tk[2] / a.inner, 4), gbs=round(traffic / ms / 1e6, 1),
                             hbm_roof_share=round(traffic / (ms * 1e-3) / HBM_ROOF, 3)))
            rows.append(dict(name=f"A call {name}", ms_median=round(ta[0], 3), ms_min=round(ta[1], 3),
                             ms_max=round(ta[2], 3)))
            rows.append(dict(name=f"B torch route {name}", ms_median=round(tb[0], 3), ms_min=round(tb[1], 3),
                             ms_max=round(tb[2], 3), a_over_b=round(ta[0] / tb[0], 3),
                             pixels_differ=differ))
    rows.append(dict(name="summary", warmup=a.warmup, reps=a.reps, inner=a.inner,
                     device=torch.cuda.get_device_name(0)))
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
