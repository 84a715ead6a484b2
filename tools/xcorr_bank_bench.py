"""Time the template bank (vsig_xcorr_bank_exec_dev) against what a caller had
before it: K sequential vsig_xcorr_exec_dev calls, peak only, "refine" = 0, on
the same K templates (one reference mixed at K offsets beforehand).

  L in {1024, 2048, 4096}, K in {1, 8, 64, 512}, n = 2**26 complex64 samples;
  the bank at its default block size M and, for L > 1024, at both candidates
  (8192 and 16384, option "xcorr_bank_m").

Device times are HIP-event medians over the repetitions after warm-up runs,
the candidates and the baseline alternating inside every repetition, so all
see the same clock and neighbours.  `predicted` is the transform count alone:
(K + 1) M log2 M / hop of the bank over 2 K M' log2 M' / hop' of the K passes.
The bank's records are checked against the K passes' (same index, peak within
1e-5) before anything is timed.

Without --step the tool runs one child process per template length, each under
its own `timeout`, and stops at the first that fails:

    python tools/xcorr_bank_bench.py [--log2n 26] [--out out/xcorr_bank_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (1024, 2048, 4096)
KS = (1, 8, 64, 512)
SR = 56e6


def reps_for(K):
    return (2, 15) if K <= 8 else (2, 7) if K <= 64 else (1, 3)


def timed(fns, warmup, reps):
    """Median / min / max ms of each fn, run in turn inside every repetition."""
    import torch
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


def step(L, ks, log2n, out):
    import numpy as np
    import torch

    import vector_amd as va
    from vector_amd import _lib

    n = 1 << log2n
    ctx = va.get_context(0)
    ctx.bind_stream()
    lib = ctx.lib
    gen = torch.Generator(device="cuda").manual_seed(L)
    s = 0.1 * torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    bits = torch.randint(0, 2, (2, L), generator=gen, device="cuda").to(torch.float32)
    p = torch.complex(2 * bits[0] - 1, 2 * bits[1] - 1) / math.sqrt(2.0)
    df = SR / (2 * L)
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:                                        # noqa: BLE001
        clock = "not read"
    for K in ks:
        offs = (np.arange(K) - K // 2) * df
        T = torch.empty((K, L), dtype=torch.complex64, device="cuda")
        for k, f in enumerate(offs):
            if f == 0:
                T[k].copy_(p)
            else:
                ctx.check(lib.vsig_mix_c64_dev(ctx.h, C.c_void_p(p.data_ptr()), L, float((2j * np.pi * f).imag),
                                               SR, 0, C.c_void_p(T[k].data_ptr())), "mix")
        k0, pos = K // 3, n // 2 + 777
        x = s.clone()
        x[pos:pos + L] += T[k0]
        torch.cuda.synchronize()
        # the baseline: K handles, refine off
        ctx.check(lib.vsig_set_option(ctx.h, b"refine", 0), "refine")
        Th = T.cpu().numpy()
        singles = [va.Correlator(Th[k]) for k in range(K)]
        pk1 = torch.empty((K, 4), dtype=torch.float64, device="cuda")

        def passes():
            for k, h in enumerate(singles):
                ctx.check(lib.vsig_xcorr_exec_dev(h.h, C.c_void_p(x.data_ptr()), n, _lib.MODES["valid"], None,
                                                  C.c_void_p(pk1[k].data_ptr())), "xcorr")

        banks, fns, names = [], [], []
        for M in ((0,) if L <= 1024 else (8192, 16384)):
            ctx.check(lib.vsig_set_option(ctx.h, b"xcorr_bank_m", M), "xcorr_bank_m")
            b = va.CorrelatorBank(T)
            pk = torch.empty((K, 4), dtype=torch.float64, device="cuda")
            banks.append((b, pk))
            fns.append(lambda b=b, pk=pk: b(x, "valid", peaks=pk))
            names.append(b.plan(n, "valid"))
        ctx.check(lib.vsig_set_option(ctx.h, b"xcorr_bank_m", 0), "xcorr_bank_m")
        # same answers first
        passes()
        for f in fns:
            f()
        torch.cuda.synchronize()
        want = va.CorrelatorBank.read_peaks(pk1)
        assert want[1][k0] == pos, (want[1][k0], pos)
        for b, pk in banks:
            got = b.read_peaks(pk)
            strong = want[0] > 0.3 * L        # the planted hypothesis and its neighbours
            assert np.array_equal(got[1][strong], want[1][strong]), "bank and passes disagree on an index"
            assert np.all(np.abs(got[0][strong] / want[0][strong] - 1) <= 1e-5), \
                "bank and passes disagree on a peak"
        warmup, reps = reps_for(K)
        res = timed(fns + [passes], warmup, reps)
        # the single-template path's block size and hop (even at M = 16384)
        Mb = 4096 if L <= 1024 else 8192 if L <= 2048 else 16384
        hopb = Mb - L + 1
        if Mb == 16384:
            hopb -= hopb % 2
        base = res[-1]
        for (M, hop, nblocks, grid), t in zip(names, res[:-1]):
            pred = ((K + 1) * M * math.log2(M) / hop) / (2 * K * Mb * math.log2(Mb) / hopb)
            r = dict(L=L, K=K, n=n, M=M, hop=hop, nblocks=nblocks, grid=grid, reps=reps,
                     bank_ms=round(t[0], 4), bank_min=round(t[1], 4), bank_max=round(t[2], 4),
                     passes_M=Mb, passes_ms=round(base[0], 4), passes_min=round(base[1], 4),
                     passes_max=round(base[2], 4), ratio=round(t[0] / base[0], 4),
                     predicted=round(pred, 4), bank_ms_per_template=round(t[0] / K, 5), clock=clock)
            print(json.dumps(r), flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(json.dumps(r) + "\n")
        del singles, banks, fns
        ctx.check(lib.vsig_set_option(ctx.h, b"refine", 1), "refine")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--lengths", type=int, nargs="*", default=list(LENGTHS))
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per template length")
    ap.add_argument("--step", type=int, default=0, help="(internal) run one template length in this process")
    a = ap.parse_args()
    if a.step:
        step(a.step, a.ks, a.log2n, a.out)
        return 0
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    for L in a.lengths:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", str(L),
               "--log2n", str(a.log2n), "--ks", *map(str, a.ks)] + (["--out", a.out] if a.out else [])
        rc = subprocess.run(cmd).returncode
        if rc:
            print(f"L={L}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
