"""GPU tests of the spectrum traces (vsig_psd_traces_c64_dev, averaged_spectrum,
averaged_spectrum_trace): which frames a block owns (bit-exact), the accuracy
floor of every detector, many frames through the merge and the stored-batch
route, NaN, and the front end."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import accuracy_ref as acc
import spectrum_traces_ref as st
import trace_ref as tr

pytestmark = pytest.mark.gpu

IN_LDS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)


def plan(gpu, nfft, nframes):
    b, s, f = C.c_int64(), C.c_int64(), C.c_int64()
    assert gpu.load_library().vsig_psd_traces_plan(nfft, nframes, C.byref(b), C.byref(s), C.byref(f)) == 0
    return b.value, s.value, f.value


class batch_cap:
    """The "psd_traces_batch" option for the block, then automatic again."""

    def __init__(self, gpu, frames):
        self.ctx, self.frames = gpu.get_context(), frames

    def __enter__(self):
        self.ctx.check(self.ctx.lib.vsig_set_option(self.ctx.h, b"psd_traces_batch", self.frames), "option")

    def __exit__(self, *exc):
        self.ctx.check(self.ctx.lib.vsig_set_option(self.ctx.h, b"psd_traces_batch", 0), "option")


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


# ---------------------------------------------------------------------------
# T1. frame ownership, bit-exact
# ---------------------------------------------------------------------------
def _frame_counts(gpu, nfft):
    counts = [1, 2, 3, 7]
    if nfft in (1024, 8192):
        # a block's run, one frame more, and one frame short of whole runs
        _, step, _ = plan(gpu, nfft, 1)
        blocks, step, run = plan(gpu, nfft, 64 * step)
        assert blocks >= 3 and run >= step
        counts += [run, run + 1, blocks * run - 1]
    return counts


@pytest.mark.parametrize("nfft", IN_LDS)
def test_frame_ownership_bit_exact(gpu, nfft):
    """Frame m is the constant a_m = p_m + 1j q_m (small integers), the window
    is ones: only bin 0 is non-zero, and it is |a_m|^2 exactly (every non-zero
    value meets only W^0 products with a zero partner; nfft a_m and its square
    over nfft^2 are exact in fp32).  So the detectors must equal the numpy
    reductions of spectrum()'s own stored output to the bit, whatever the
    blocks' runs: a frame counted twice, dropped, or a zero frame past nframes
    folded in changes a bit of min or mean."""
    w = np.ones(nfft)
    for nframes in _frame_counts(gpu, nfft):
        x, p2 = st.constant_frames(nfft, nframes, seed=nfft + nframes)
        off = torch.from_numpy(np.concatenate([np.zeros(1, np.complex64), x])).cuda()[1:]   # 8 bytes in: x4 off
        x3 = np.zeros(3 * len(x), np.complex64)
        x3[::3] = x
        forms = [("plain", torch.from_numpy(x).cuda(), {}), ("offset", off, {}),
                 ("stride3", torch.from_numpy(x3).cuda(), dict(_stride=3, _nsamples=len(x)))]
        for shift in (False, True):
            for name, xd, kw in forms:
                case = f"nfft={nfft} nframes={nframes} shift={shift} {name}"
                _, _, S = gpu.spectrum(xd, 1.0, w, nfft, 0, nfft, fftshift=shift, **kw)
                want = st.reduce_frames(S.cpu().numpy())
                got = gpu.averaged_spectrum(xd, 1.0, w, nfft, 0, nfft, fftshift=shift, **kw)
                assert got.nframes == nframes == S.shape[1], case
                for d in st.DETECTORS:
                    y = host(getattr(got, d))
                    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), want[d].astype(np.float32)), \
                        (case, d)
                hot = nfft // 2 if shift else 0
                rest = np.delete(np.arange(nfft), hot)
                for d in st.DETECTORS:
                    assert np.all(host(getattr(got, d))[rest] == 0.0), (case, d)
                assert abs(float(host(got.max)[hot]) - p2.max()) <= 1e-6 * p2.max(), case
                assert abs(float(host(got.min)[hot]) - p2.min()) <= 1e-6 * p2.min(), case


# ---------------------------------------------------------------------------
# T2. accuracy floor, every bin distinct
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs(key, route):
    if route:
        nfft, nperseg, noverlap, stride = key
        x = acc.route_spectrum_input(nfft, nperseg, noverlap, stride)
    else:
        (nfft, nperseg, noverlap), stride = key, 1
        x = acc.spectrum_input(nfft, nperseg, noverlap)
    xs = x[::stride]
    S32 = acc.spectrum(xs, "hann", nperseg, noverlap, nfft)
    S64 = acc.spectrum(xs, "hann", nperseg, noverlap, nfft, np.complex128)
    assert S64.shape == (nfft, 3)
    return x, S32, S64


def _check_floor(case, got, S32, S64, K):
    want = st.reduce_frames(S64)
    e_ref = float(np.abs(S32.astype(np.float64) - S64).max())
    for d in st.DETECTORS:
        y = host(getattr(got, d)).astype(np.float64)
        err, lim = float(np.abs(y - want[d]).max()), st.bound(K, S32, S64, want[d])
        acc.say(f"{case} {d}", e_ref=e_ref, e_gpu=err, ratio=err / e_ref, bound=lim)
        assert err <= lim, (case, d, err, lim)


@pytest.mark.parametrize("key", list(acc.SPECTRUM_SEEDS))
def test_accuracy_floor(gpu, key):
    """Each detector within K max|S32 - S64| (+ one float32 rounding) of the
    detector of the complex128 spectrogram, K the class of the frame's route:
    3 frames, so the last pair (or lane groups of the last step) is partly
    inactive."""
    nfft, nperseg, noverlap = key
    x, S32, S64 = _refs(key, False)
    got = gpu.averaged_spectrum(x, 1.0, "hann", nperseg, noverlap, nfft)
    assert got.nframes == 3 and np.array_equal(got.f, np.fft.fftfreq(nfft, 1.0))
    _check_floor(f"traces nfft={nfft} nperseg={nperseg} noverlap={noverlap}", got, S32, S64,
                 acc.route_spectrum_class(nfft)[0])


@pytest.mark.parametrize("key", list(acc.ROUTE_SPECTRUM_SEEDS))
def test_accuracy_floor_routes(gpu, key):
    nfft, nperseg, noverlap, stride = key
    x, S32, S64 = _refs(key, True)
    xd = torch.from_numpy(x).cuda()
    got = gpu.averaged_spectrum(xd, 1.0, "hann", nperseg, noverlap, nfft, _stride=stride,
                                _nsamples=len(x[::stride]))
    assert got.nframes == 3 and got.mean.is_cuda
    _check_floor(f"traces nfft={nfft} nperseg={nperseg} noverlap={noverlap} stride={stride}", got, S32, S64,
                 acc.route_spectrum_class(nfft)[0])


# ---------------------------------------------------------------------------
# T3. many frames: the merge and the stored-batch route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [1024, 8192])
def test_many_frames_cross_block_runs(gpu, nfft):
    """The vetted 3-frame input tiled under exact power-of-two gains (the
    references' errors scale with them, so the seed table's premise carries
    over), enough repetitions that the frames cross at least three blocks'
    runs, the last one partly filled."""
    x, _, _ = _refs((nfft, nfft, 0), False)
    _, step, _ = plan(gpu, nfft, 1)
    reps = 1
    while True:
        blocks, step, run = plan(gpu, nfft, 3 * reps)
        if blocks >= 3 and 3 * reps > 2 * run and (3 * reps) % run != 0 and run > step:
            break
        reps += 1
        assert reps < 4096
    xt = st.tiled(x, reps, seed=nfft)
    S32 = acc.spectrum(xt, "hann", nfft, 0, nfft)
    S64 = acc.spectrum(xt, "hann", nfft, 0, nfft, np.complex128)
    got = gpu.averaged_spectrum(xt, 1.0, "hann", nfft, 0, nfft)
    assert got.nframes == 3 * reps
    _check_floor(f"traces tiled nfft={nfft} frames={3 * reps} blocks={blocks} run={run}", got, S32, S64,
                 acc.route_spectrum_class(nfft)[0])
    # the three detectors differ in every bin
    assert np.all(got.min < got.mean) and np.all(got.mean < got.max)


def test_many_frames_stored_batches_four_step(gpu):
    """32768-point frames take vsig_psd_c64_dev's four-step route into stored
    batches: 6 frames in three batches of 2."""
    nfft = 32768
    x, _, _ = _refs((nfft, nfft, 0, 1), True)
    xt = st.tiled(x, 2, seed=nfft)
    S32 = acc.spectrum(xt, "hann", nfft, 0, nfft)
    S64 = acc.spectrum(xt, "hann", nfft, 0, nfft, np.complex128)
    with batch_cap(gpu, 2):
        got = gpu.averaged_spectrum(xt, 1.0, "hann", nfft, 0, nfft)
    assert got.nframes == 6
    _check_floor(f"traces tiled nfft={nfft} frames=6 batch=2", got, S32, S64, acc.route_spectrum_class(nfft)[0])


def test_stored_batches_bluestein(gpu):
    """nfft = 1000 (Bluestein per frame), 5 frames in batches of 2, 2, 1: bounded
    as test_gpu_accuracy_routes.py bounds that route (noise, plain scipy
    references, the exact class)."""
    nfft = 1000
    x = acc.noise(5 * nfft, seed=2 * nfft)
    S32 = acc.spectrum(x, "hann", nfft, 0, nfft, fftshift=True)
    S64 = acc.spectrum(x, "hann", nfft, 0, nfft, np.complex128, fftshift=True)
    with batch_cap(gpu, 2):
        got = gpu.averaged_spectrum(x, 1.0, "hann", nfft, 0, nfft, fftshift=True)
    assert got.nframes == 5
    _check_floor("traces nfft=1000 frames=5 batch=2", got, S32, S64, acc.K_EXACT)


@pytest.mark.parametrize("nfft,batch", [(100, 2), (100, 0), (16384, 2)])
def test_stored_batches_equal_stored_spectrum(gpu, nfft, batch):
    """nfft = 100 is a direct sum in double, a route test_gpu_accuracy_routes.py
    has no spectrum class for: the traces are compared with the reductions of
    spectrum()'s own output instead.  This route stores P and folds the stored
    values, so max and min are those values to the bit and the mean is the
    same double sum in another order (within nframes 2^-53, then one float32
    rounding).  16384 points: the pair kernel's stored batches."""
    x = acc.noise(5 * nfft, seed=nfft)
    _, _, S = gpu.spectrum(x, 1.0, "hann", nfft, 0, nfft)
    want = st.reduce_frames(S)
    with batch_cap(gpu, batch):
        got = gpu.averaged_spectrum(x, 1.0, "hann", nfft, 0, nfft)
    assert got.nframes == 5
    assert np.array_equal(got.max, want["max"]) and np.array_equal(got.min, want["min"])
    assert np.abs(got.mean.astype(np.float64) - want["mean"]).max() <= 2.0 ** -23 * want["mean"].max()
    assert tr.ulps(got.mean, want["mean"].astype(np.float32)).max() <= 1


# ---------------------------------------------------------------------------
# T4. special values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [1024, 8192])
def test_nan_frame(gpu, nfft):
    x = acc.noise(5 * nfft, seed=nfft + 5).copy()
    x[2 * nfft + 5] = complex(np.nan, 0.0)
    _, _, S = gpu.spectrum(x, 1.0, "hann", nfft, 0, nfft)
    want = st.reduce_frames(S)
    got = gpu.averaged_spectrum(x, 1.0, "hann", nfft, 0, nfft)
    for d in st.DETECTORS:
        y = getattr(got, d)
        assert np.all(np.isnan(y)), d
        assert np.array_equal(y, want[d].astype(np.float32), equal_nan=True), d
    clean = gpu.averaged_spectrum(x[:2 * nfft], 1.0, "hann", nfft, 0, nfft)
    assert clean.nframes == 2
    for d in st.DETECTORS:
        assert np.all(np.isfinite(getattr(clean, d))), d


# ---------------------------------------------------------------------------
# T5. front end
# ---------------------------------------------------------------------------
def test_dtypes_and_return_forms(gpu):
    nfft = 256
    x = acc.noise(6 * nfft, seed=7)
    a = gpu.averaged_spectrum(x, 2e6, "hann", nfft, 0, nfft)
    assert isinstance(a, gpu.SpectrumTraces) and a.nframes == 6
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 and v.shape == (nfft,) for v in a[1:4])
    assert np.array_equal(a.f, np.fft.fftfreq(nfft, 1 / 2e6))
    b = gpu.averaged_spectrum(x.astype(np.complex128), 2e6, "hann", nfft, 0, nfft)
    assert all(v.dtype == np.float64 for v in b[1:4])
    assert np.array_equal(b.max, a.max.astype(np.float64)) and np.array_equal(b.mean.astype(np.float32), a.mean)
    r = gpu.averaged_spectrum(x.real.astype(np.float32), 2e6, "hann", nfft, 0, nfft)
    assert all(v.dtype == np.float32 for v in r[1:4])
    d = gpu.averaged_spectrum(torch.from_numpy(x).cuda(), 2e6, "hann", nfft, 0, nfft)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 for v in d[1:4])
    for k in st.DETECTORS:
        assert np.array_equal(host(getattr(d, k)), getattr(a, k)), k
    only = gpu.averaged_spectrum(x, 2e6, "hann", nfft, 0, nfft, detectors=("max",))
    assert only.mean is None and only.min is None and np.array_equal(only.max, a.max)
    one = gpu.averaged_spectrum(x, 2e6, "hann", nfft, 0, nfft, detectors="min")
    assert one.mean is None and one.max is None and np.array_equal(one.min, a.min)
    s = gpu.averaged_spectrum(x, 2e6, "hann", nfft, 0, nfft, fftshift=True)
    assert np.array_equal(s.mean, np.fft.fftshift(a.mean)) and np.array_equal(s.f, a.f)


def test_c_abi_host_twin_and_errors(gpu):
    nfft, nframes = 512, 9
    x = acc.noise(nframes * nfft, seed=9)
    w = acc.window32("hann", nfft)
    scale = float(1.0 / float(np.sum(w, dtype=np.float64)) ** 2)
    ctx = gpu.get_context()
    mean, mx, mn = np.zeros(nfft, np.float64), np.zeros(nfft, np.float32), np.zeros(nfft, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ctx.check(ctx.lib.vsig_psd_traces_c64(ctx.h, p(x), len(x), p(w), nfft, nfft, nfft, scale, 0, nframes,
                                          p(mean), p(mx), p(mn)), "host twin")
    a = gpu.averaged_spectrum(x, 1.0, "hann", nfft, 0, nfft)
    assert np.array_equal(mx, a.max) and np.array_equal(mn, a.min) and np.array_equal(mean.astype(np.float32), a.mean)
    assert np.all(mn <= mean) and np.all(mean <= mx)
    assert ctx.lib.vsig_psd_traces_c64(ctx.h, p(x), len(x), p(w), nfft, nfft, nfft, scale, 0, nframes,
                                       None, None, None) == -1
    assert ctx.lib.vsig_psd_traces_c64(ctx.h, p(x), len(x), p(w), nfft, nfft, nfft, scale, 0, nframes + 1,
                                       p(mean), None, None) == -1
    assert ctx.lib.vsig_set_option(ctx.h, b"psd_traces_batch", -1) == -1


@pytest.mark.parametrize("nfft", [1024, 8192, 16384])
def test_dev_call_captures_into_a_graph(gpu, nfft):
    """Warm, the call neither allocates nor synchronises: one capture on a
    single stream, replayed on new contents, gives the bytes of a plain call."""
    nframes = 21
    a = acc.noise(nframes * nfft, seed=nfft + 1)
    w = acc.window32("hann", nfft)
    scale = float(1.0 / float(np.sum(w, dtype=np.float64)) ** 2)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        x = torch.from_numpy(a).cuda()
        wd = torch.from_numpy(w).cuda()
        mean = torch.zeros(nfft, dtype=torch.float64, device="cuda")
        mx = torch.zeros(nfft, dtype=torch.float32, device="cuda")
        mn = torch.zeros(nfft, dtype=torch.float32, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731

        def step():
            ctx = gpu.get_context()
            ctx.check(ctx.lib.vsig_psd_traces_c64_dev(ctx.h, ptr(x), len(a), 1, ptr(wd), nfft, nfft, nfft, scale, 1,
                                                      nframes, ptr(mean), ptr(mx), ptr(mn)), "traces")
        step()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            step()
        new = np.roll(a, 4321) * np.float32(0.5)
        x.copy_(torch.from_numpy(new))
        for t in (mean, mx, mn):
            t.zero_()
        graph.replay()
        stream.synchronize()
        replayed = [t.cpu().numpy().copy() for t in (mean, mx, mn)]
        step()
        stream.synchronize()
        for r, t in zip(replayed, (mean, mx, mn)):
            assert np.array_equal(r, t.cpu().numpy()) and np.all(r > 0)
    want = gpu.averaged_spectrum(new, 1.0, "hann", nfft, 0, nfft, fftshift=True)
    assert np.array_equal(replayed[1], want.max) and np.array_equal(replayed[0].astype(np.float32), want.mean)


def test_averaged_spectrum_trace(gpu):
    nfft, sr, cf, eps = 1024, 20e6, 2.4e9, 1e-12
    x = acc.noise(40 * nfft + 100, seed=3)
    m = gpu.averaged_spectrum(x, sr, "hann", nfft, 0, nfft, fftshift=True)
    for det in st.DETECTORS:
        line = getattr(m, det)
        want = 10 * np.log10(line + np.float32(eps))
        t = gpu.averaged_spectrum_trace(x, sr, cf, nfft=nfft, detector=det, eps=eps)
        assert isinstance(t, gpu.Trace) and t.bin == 1 and t.lo is t.hi and t.hi.dtype == np.float32
        assert tr.ulps(t.hi, want).max() <= 8, det
        assert np.array_equal(t.x, np.fft.fftshift(np.fft.fftfreq(nfft, 1 / sr)) + cf)
        assert t.argmax == int(np.argmax(line)) and t.max == float(t.hi[t.argmax])
        # columns: the envelope of the mapped line is the mapped envelope
        c = gpu.averaged_spectrum_trace(x, sr, cf, nfft=nfft, detector=det, eps=eps, max_points=64)
        assert c.bin == 16 and c.hi.shape == (64,)
        assert np.array_equal(c.hi, t.hi.reshape(64, 16).max(axis=1)), det
        assert np.array_equal(c.lo, t.hi.reshape(64, 16).min(axis=1)), det
        assert np.array_equal(c.x, t.x[::16]) and c.argmax == t.argmax and c.max == t.max
    lin = gpu.averaged_spectrum_trace(x, sr, cf, nfft=nfft, scale="linear")
    assert np.array_equal(lin.hi, m.mean)
    nz = gpu.averaged_spectrum_trace(x, sr, cf, nfft=nfft, eps=eps, normalize=True)
    base = gpu.averaged_spectrum_trace(x, sr, cf, nfft=nfft, eps=eps)
    assert nz.max == 0.0 and np.array_equal(nz.hi, base.hi - np.float32(base.max))
    d = gpu.averaged_spectrum_trace(torch.from_numpy(x).cuda(), sr, cf, nfft=nfft, eps=eps, max_points=64)
    assert d.hi.is_cuda and np.array_equal(d.hi.cpu().numpy(), gpu.averaged_spectrum_trace(
        x, sr, cf, nfft=nfft, eps=eps, max_points=64).hi)
    wide = gpu.averaged_spectrum_trace(x.astype(np.complex128), sr, cf, nfft=nfft, eps=eps)
    assert wide.hi.dtype == np.float64
