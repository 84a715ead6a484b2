"""Teardown of the C-ABI layer's device memory (vsig_ctx.hpp: DevBuf): contexts
and handles are created, driven through every large scratch family and freed,
over and over, and the device's free memory must not sink.

One cycle, on a private context (vsig_init .. vsig_free, not the per-thread
shared one), through the ctypes signatures:

* host-pointer vsig_peak on 2^20 complex64            -> stage (8 MB)
* complex128 vsig_correlate_dev, 2^19 x 64, c128 out  -> conv[0..2] (4 MB each),
                                                         lkeys, rscratch, partials
* a FIR handle of 8200 taps over 2^16 samples         -> the parts path, z (512 KB)
* an xcorr handle, 9000-sample template over 2^17     -> one M = 32768 pass: spectrum
  samples, no output array                               by the four-step plan, bigtmp
* the same with a 20000-sample template               -> chunked passes, the handle's
                                                         cbuf (0.85 MB)
* vsig_resample_dev 2^20 -> 2^20 - 24                 -> two Bluestein plans (8 + 16 MB
                                                         each), spec (8 MB each), bigtmp
                                                         (16 MB), the four-step table
* vsig_correlate_stats_dev 2^19 x 64                  -> vscratch (4 MB), sscratch

After one warm-up cycle the free memory is read, four more cycles run, and it
is read again.  A buffer leaked once per cycle costs four times its size; the
drop must stay below half of the smallest family above (z, 512 KB).  The small
tables and plan handles cannot be seen this way.

The cycle's results are asserted too (the peak of a planted spike, the
resampled signal against scipy.signal.resample at test_gpu_transforms.py's
tolerance), so a cycle cannot pass by doing nothing.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # test_gpu_transforms.py: of max |reference|
N_PEAK = 1 << 20
N_CORR, L_CORR = 1 << 19, 64
N_FIR, TAPS = 1 << 16, 8200
N_XC, L_XC, L_XC_LONG = 1 << 17, 9000, 20_000
N_RS, NUM_RS = 1 << 20, (1 << 20) - 24
SPIKE = 777_777
C128, C64 = 0, 1
VALID = 0

# bytes of the families a leak of which the threshold must catch
FAMILIES = {
    "stage": N_PEAK * 8,
    "conv": N_CORR * 8,
    "fir z": N_FIR * 8,
    "xcorr cbuf": (N_XC - L_XC_LONG + 1) * 8,
    "spec": NUM_RS * 8,
    "vscratch": (N_CORR - L_CORR + 1) * 8,
}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _noise(n, seed):
    """CN(0, 1): no tones, so the correlations have one clear peak."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)


@pytest.fixture(scope="module")
def data(gpu):
    """Operands (device tensors made once, so torch's allocator is quiet
    during the cycles) and the resample reference."""
    d = {}
    xp = ref.synth_iq(N_PEAK, seed=1).astype(np.complex64)
    xp *= np.complex64(0.5 / np.abs(xp).max())
    xp[SPIKE] = 3.0 + 4.0j
    d["peak_x"] = xp
    tm = _noise(L_CORR, 2)
    a = 0.01 * _noise(N_CORR, 3)
    d["corr_at"] = 123_456
    a[d["corr_at"]:d["corr_at"] + L_CORR] += tm
    d["corr_a"] = torch.from_numpy(a).cuda()
    d["corr_v"] = torch.from_numpy(tm).cuda()
    d["corr_out"] = torch.empty(N_CORR - L_CORR + 1, dtype=torch.complex128, device="cuda")
    d["taps"] = np.ascontiguousarray(ref.synth_iq(TAPS, seed=4), np.complex64)
    d["fir_x"] = torch.from_numpy(ref.synth_iq(N_FIR, seed=5).astype(np.complex64)).cuda()
    d["fir_y"] = torch.empty_like(d["fir_x"])
    d["xc_t"] = _noise(L_XC_LONG, 6).astype(np.complex64)
    d["xc_s"] = torch.from_numpy(_noise(N_XC, 7).astype(np.complex64)).cuda()
    xr = ref.synth_iq(N_RS, seed=8).astype(np.complex64)
    d["rs_x"] = torch.from_numpy(xr).cuda()
    d["rs_y"] = torch.empty(NUM_RS, dtype=torch.complex64, device="cuda")
    from scipy.signal import resample
    d["rs_ref"] = resample(xr.astype(np.complex128), NUM_RS)
    d["stats"] = torch.empty(2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return d


def _cycle(gpu, d):
    """vsig_init, every family once, vsig_free; -> (peak index of the spike,
    correlation peak index, resampled signal)."""
    _lib = gpu._lib
    ctx = _lib.Context(0)
    lib, h = ctx.lib, ctx.h
    pk = _lib.Peak()
    ctx.check(lib.vsig_peak(h, C64, d["peak_x"].ctypes.data_as(C.c_void_p), N_PEAK, C.byref(pk)), "peak")
    spike = int(pk.index)

    ctx.check(lib.vsig_correlate_dev(h, C128, _ptr(d["corr_a"]), N_CORR, _ptr(d["corr_v"]), L_CORR,
                                     VALID, C128, _ptr(d["corr_out"]), None), "correlate")

    fir = C.c_void_p()
    ctx.check(lib.vsig_fir_create(h, d["taps"].ctypes.data_as(C.c_void_p), TAPS, 1, C.byref(fir)), "fir")
    ctx.check(lib.vsig_fir_exec_dev(fir, _ptr(d["fir_x"]), N_FIR, _ptr(d["fir_y"]), N_FIR), "fir exec")

    xcs = []
    for L in (L_XC, L_XC_LONG):
        xc = C.c_void_p()
        ctx.check(lib.vsig_xcorr_create(h, d["xc_t"].ctypes.data_as(C.c_void_p), L, C.byref(xc)), "xcorr")
        xcs.append(xc)
        ctx.check(lib.vsig_xcorr_exec_dev(xc, _ptr(d["xc_s"]), N_XC, VALID, None, None), "xcorr exec")

    ctx.check(lib.vsig_resample_dev(h, C64, _ptr(d["rs_x"]), N_RS, NUM_RS, 0, _ptr(d["rs_y"])), "resample")
    ctx.check(lib.vsig_correlate_stats_dev(h, C128, _ptr(d["corr_a"]), N_CORR, _ptr(d["corr_v"]), L_CORR,
                                           VALID, _ptr(d["stats"])), "stats")
    ctx.check(lib.vsig_synchronize(h), "synchronize")
    corr_at = int(torch.argmax(d["corr_out"].abs()).item())
    y = d["rs_y"].cpu().numpy()

    lib.vsig_fir_free(fir)
    for xc in xcs:
        lib.vsig_xcorr_free(xc)
    lib.vsig_free(h)
    ctx.h = None
    return spike, corr_at, y


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_cycles_leave_free_memory_unchanged(gpu, data):
    def run():
        spike, corr_at, y = _cycle(gpu, data)
        assert spike == SPIKE
        assert corr_at == data["corr_at"]
        r = data["rs_ref"]
        assert y.shape == r.shape
        assert np.allclose(y, r, rtol=0.0, atol=TOL * np.abs(r).max())

    run()                                   # warm-up: the runtime's own pools, code objects
    before = _free_bytes()
    for _ in range(4):
        run()
    drop = before - _free_bytes()
    smallest = min(FAMILIES.values())
    print(f"free-memory drop over 4 cycles: {drop} B (smallest family {smallest} B)")
    assert drop < smallest // 2
