"""Time the per-burst spectra of a burst list in one pass against what a caller
could do before it existed, in one process:

  A   one vsig_psd_segments_run (all three detectors, every frame of every burst
      in one launch plus the segmented merge) and one vsig_band_measure_run
  S   A's first call alone, vsig_psd_segments_run: what B computes
  B   a loop of vsig_psd_traces_c64_dev over the same slices: two launches a
      burst, device pointers, each burst's rows written in place (no copy-out)
      -- and no band measurement, which had no device path

for K touching bursts that tile a complex64 capture of 2^--log2n samples (so the
total burst length is the same for every K), hop = nfft, Hann window.  Bursts
start at odd samples: a slice is then 8-byte aligned only and both paths run the
same plan at 8192 points (the single-slice path's 16-byte-load plan is not pinned
to the bit against the plain one), which the bit comparison below needs.

Device times are HIP-event medians (min-max) over --reps runs after --warmup
runs; A and B alternate inside every repetition, so both see the same clock and
the same neighbours.  B's events bracket the whole loop, launch gaps included:
that is what the caller waits for.  The plan (vsig_psd_segments_create: block
table, upload, scratch) is built once per burst list and is timed apart, on the
host clock.  Before timing A's rows must equal B's: max and min to the bit, the
mean within nframes * 2^-52 relative.  A manual tool: run it under its own time
limit on one GPU, e.g.

    timeout -k 10 900 python tools/packet_spectra_ab.py [--log2n 27] [--out out/packet_spectra_ab.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vector_amd as va  # noqa: E402
from vector_amd import _lib  # noqa: E402
from vector_amd.packets import BAND_DTYPE  # noqa: E402

ROOF_TBS = 8.0            # MI355X HBM3E peak


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


def case(ctx, x, log2n, K, nfft, warmup, reps):
    n = 1 << log2n
    slot = n // K
    starts = 1 + slot * np.arange(K, dtype=np.int64)          # x holds n + 1 samples
    lens = np.full(K, slot, np.int64)
    nframes = slot // nfft
    assert nframes >= 1, "a burst holds no frame"
    w32 = scipy.signal.get_window("hann", nfft).astype(np.float32)
    scale = float(1.0 / float(np.sum(w32, dtype=np.float64)) ** 2)
    wd = torch.from_numpy(w32).cuda()
    out = {}
    for tag in "ab":
        out[tag] = (torch.empty((K, nfft), dtype=torch.float64, device="cuda"),
                    torch.empty((K, nfft), dtype=torch.float32, device="cuda"),
                    torch.empty((K, nfft), dtype=torch.float32, device="cuda"))
    bands = torch.empty(K * BAND_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.bind_stream()
    lib = ctx.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    table = np.ascontiguousarray(np.stack([starts, lens], axis=1))
    plan = C.c_void_p()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.check(lib.vsig_psd_segments_create(ctx.h, table.ctypes.data_as(C.POINTER(_lib.Segment)), K, n + 1, nfft, nfft,
                                           nfft, C.byref(plan)), "create")
    create_ms = (time.perf_counter() - t0) * 1e3
    info = [C.c_int64() for _ in range(4)]
    ctx.check(lib.vsig_psd_segments_info(plan, *(C.byref(v) for v in info)), "info")
    xp = x.data_ptr()
    ma, xa, na = (t.data_ptr() for t in out["a"])
    mb, xb, nb = (t.data_ptr() for t in out["b"])
    P = C.c_void_p

    def method_a():
        ctx.check(lib.vsig_psd_segments_run(plan, P(xp), ptr(wd), scale, 1, P(ma), P(xa), P(na)), "segments")
        ctx.check(lib.vsig_band_measure_run(ctx.h, P(ma), K, nfft, nfft, 0.005, ptr(bands)), "band")

    def method_s():
        ctx.check(lib.vsig_psd_segments_run(plan, P(xp), ptr(wd), scale, 1, P(ma), P(xa), P(na)), "segments")

    def method_b():
        for k in range(K):
            rc = lib.vsig_psd_traces_c64_dev(ctx.h, P(xp + 8 * int(starts[k])), slot, 1, ptr(wd), nfft, nfft, nfft,
                                             scale, 1, nframes, P(mb + 8 * nfft * k), P(xb + 4 * nfft * k),
                                             P(nb + 4 * nfft * k))
            if rc:
                ctx.check(rc, "psd traces")

    try:
        method_a()
        method_b()
        torch.cuda.synchronize()
        assert torch.equal(out["a"][1], out["b"][1]) and torch.equal(out["a"][2], out["b"][2]), "max / min differ"
        rel = float(((out["a"][0] - out["b"][0]).abs() / out["b"][0]).max())
        assert rel <= nframes * 2.0 ** -52, (rel, nframes)
        rec = bands.cpu().numpy().view(BAND_DTYPE)
        assert np.all(rec["flags"] == 0) and np.all(rec["lo_bin"] >= 0) and np.all(rec["lo_bin"] < rec["hi_bin"])
        ta, ts, tb = timed([method_a, method_s, method_b], warmup, reps)
    finally:
        lib.vsig_psd_segments_free(plan)
    return dict(K=K, nfft=nfft, n=n, nframes=nframes, frame_samples=K * nframes * nfft, a=ta, s=ts, b=tb, mean_rel=rel,
                create_ms=create_ms, blocks=info[1].value, run=info[3].value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--bursts", type=int, nargs="+", default=[2, 64, 1024, 16384])
    ap.add_argument("--nfft", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "packet_spectra_ab.md"),
                    help="where the table goes (profiles/packet_spectra_ab.md holds a table of this tool's and the "
                         "notes written around it: it is not the default)")
    a = ap.parse_args()
    ctx = va.get_context(0)
    n = 1 << a.log2n
    gen = torch.Generator(device="cuda").manual_seed(a.log2n)
    x = torch.view_as_complex(torch.randn((n + 1, 2), generator=gen, device="cuda", dtype=torch.float32))
    rows = []
    for nfft in a.nfft:
        for K in a.bursts:
            if n // K < nfft:
                print(f"K={K}: a burst of {n // K} samples holds no {nfft}-point frame: skipped", flush=True)
                continue
            rows.append(case(ctx, x, a.log2n, K, nfft, a.warmup, a.reps))
            print(rows[-1], flush=True)
            torch.cuda.empty_cache()
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"    # noqa: E731
    lines = [
        "# Per-burst spectra in one pass (`vsig_psd_segments_run` + `vsig_band_measure_run`) against a loop of",
        "# `vsig_psd_traces_c64_dev`",
        "",
        f"`tools/packet_spectra_ab.py`, one MI355X, 2^{a.log2n} complex64 samples of noise tiled by K touching bursts",
        "(odd starts), `hop = nfft`, Hann window, all three detectors.  HIP-event medians (min-max) of "
        f"{a.reps} runs after {a.warmup}",
        "warm-up runs; A, S and B alternate inside every repetition.  A: one segmented pass and the band measurement.",
        "S: the segmented pass alone.  B: one `vsig_psd_traces_c64_dev` call a burst (device pointers, rows written",
        "in place, launch gaps included), and no band measurement.  Before timing A's max and min rows equal B's to",
        "the bit and the mean rows agree within `nframes * 2^-52` relative (asserted; the column is the largest",
        f"relative difference).  TB/s is 8 B per frame sample over A's two calls; the roof is {ROOF_TBS:g} TB/s.  create:",
        "the plan, built once per burst list, on the host clock.  blocks x run: A's grid and the longest run of",
        "frames a block owns.  overlap: whether A's and B's min-max ranges overlap.",
        "",
        "| nfft | K | frames / burst | blocks x run | A ms | A TB/s | share of roof | S ms | B ms | A / B | S / B | overlap | "
        "mean rel | create ms |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        tbs = 8 * r["frame_samples"] / r["a"][0] / 1e9
        overlap = "yes" if r["a"][1] <= r["b"][2] and r["b"][1] <= r["a"][2] else "no"
        lines.append(f"| {r['nfft']} | {r['K']} | {r['nframes']} | {r['blocks']} x {r['run']} | {fmt(r['a'])} | "
                     f"{tbs:.2f} | {100 * tbs / ROOF_TBS:.0f} % | {fmt(r['s'])} | {fmt(r['b'])} | "
                     f"{r['a'][0] / r['b'][0]:.4f} | {r['s'][0] / r['b'][0]:.4f} | {overlap} | {r['mean_rel']:.1e} | "
                     f"{r['create_ms']:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    # the gate: A, both calls, not above B wherever there are at least two bursts
    late = [f"nfft {r['nfft']} K {r['K']}: {r['a'][0]:.3f} ms against {r['b'][0]:.3f} ms" for r in rows
            if r["K"] >= 2 and r["a"][0] > r["b"][0]]
    if late:
        sys.exit("gate: A's median is above B's at " + "; ".join(late))


if __name__ == "__main__":
    main()
