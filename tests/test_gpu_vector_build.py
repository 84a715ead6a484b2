"""GPU checks of the vector assembly (vector_build.hip behind
vsig_vector_build_dev / vsig_normalize_c64_dev and vector_amd.build_vector)
against numpy's own loop, restated below from generate_vector
(unified_gui.py:1756-1769, 1779-1781):

    vector = np.zeros(n, complex64);  vector[a:b] += y  per packet, per instance
    vector / np.max(np.abs(vector))

The kernel performs the same fp32 adds in the same order, so every comparison
with that loop is np.array_equal on the complex64 arrays (max |v| and the
normalised vector included).  Only the comparison with the reference-made
golden has a tolerance, because there the packets pass through the GPU mixer,
which the project holds to 1e-5 absolute (tests/test_gpu_formats.py): k
contributions at a sample give k * 1e-5, and dividing by max_val (itself off
by at most k * 1e-5) gives 2 * k * 1e-5 / max_val for |v| <= max_val.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
from test_vector_build_cpu import _configs

pytestmark = pytest.mark.gpu

N = 100003


def _iq(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)


def np_build(n, items):
    """numpy's sequential accumulate: items = [(y, (start, period, count)), ...]."""
    v = np.zeros(n, dtype=np.complex64)
    for y, (start, period, count) in items:
        for k in range(count):
            a = start + k * period
            assert a + len(y) <= n
            v[a:a + len(y)] += y
    return v


def dev_build(va, packets, places, out, n, maxabs=None):
    """vsig_vector_build_dev on device packets (torch complex64 tensors)."""
    from vector_amd import _lib
    ctx = va.get_context()
    arr = (_lib.PacketPlace * max(1, len(packets)))()
    for p, y, (start, period, count) in zip(arr, packets, places):
        p.y, p.len, p.start, p.period, p.count = y.data_ptr(), y.numel(), start, period, count
    ctx.check(ctx.lib.vsig_vector_build_dev(ctx.h, arr, len(packets), C.c_void_p(out.data_ptr()), n,
                                            C.c_void_p(maxabs.data_ptr()) if maxabs is not None
                                            else None), "vector_build")


def dev_normalize(va, x, n, maxabs, y):
    ctx = va.get_context()
    ctx.check(ctx.lib.vsig_normalize_c64_dev(ctx.h, C.c_void_p(x.data_ptr()), n,
                                             C.c_void_p(maxabs.data_ptr()),
                                             C.c_void_p(y.data_ptr())), "normalize")


@pytest.fixture(scope="module")
def layout(gpu):
    """Packets of 1, 37, 4101 and 20000 samples (device tensors, fetched back
    for the numpy loop) and their placements in N = 100003 samples; amplitudes
    span 1e-3 .. 1e3 so that the order of three or more adds shows in fp32."""
    lens = dict(one=1, a37=37, b4101=4101, d4101=4101, c20000=20000, e20000=20000)
    scale = dict(one=1e3, a37=1.0, b4101=31.0, d4101=1e-3, c20000=0.07, e20000=5.0)
    dev = {k: torch.from_numpy(_iq(n, 100 + i, scale[k])).cuda()
           for i, (k, n) in enumerate(lens.items())}
    host = {k: t.cpu().numpy() for k, t in dev.items()}
    places = [("c20000", (3, 26667, 3)),            # [3, 20003), [26670, ..), [53337, 73337)
              ("b4101", (0, 4099, 3)),              # starts at 0; instances overlap by 2 samples
              ("a37", (1000, 5, 200)),              # period < len: up to 8 self-overlapping adds
              ("d4101", (1001, 30011, 3)),          # 4th packet over [1001, 2032)
              ("one", (53000, 3, 1000)),            # single samples across c's third instance
              ("e20000", (N - 20000, 1, 1)),        # ends exactly at N
              ("a37", (N - 37, 7, 1))]              # a second one ending at N, over e
    want = np_build(N, [(host[k], pl) for k, pl in places])
    return dict(dev=[dev[k] for k, _ in places], host=[host[k] for k, _ in places],
                places=[pl for _, pl in places], want=want)


def test_layout_covers_the_cases(layout):
    cover = np.zeros(N + 1, np.int64)
    for y, (s, p, c) in zip(layout["host"], layout["places"]):
        for k in range(c):
            cover[s + k * p] += 1
            cover[s + k * p + len(y)] -= 1
    cover = np.cumsum(cover)[:N]
    assert cover.max() >= 8 and cover[0] == 1 and cover[N - 1] >= 2 and (cover == 0).any()
    # the add order is observable: the same packets in reverse list order differ
    rev = np_build(N, list(zip(layout["host"], layout["places"]))[::-1])
    assert not np.array_equal(rev, layout["want"])


@pytest.mark.parametrize("offset", [0, 3])
def test_accumulate_is_numpy_bit_exact(gpu, layout, offset):
    """offset 3: out is an odd-sample view of a larger buffer (8-byte aligned
    only); the samples either side of it stay untouched."""
    buf = torch.full((N + 8,), 7.0 - 3.0j, dtype=torch.complex64, device="cuda")
    out = buf[offset:offset + N]
    assert out.data_ptr() % 16 == (8 if offset % 2 else 0)
    dev_build(gpu, layout["dev"], layout["places"], out, N)
    got = buf.cpu().numpy()
    assert np.array_equal(got[offset:offset + N], layout["want"])
    assert np.all(got[:offset] == np.complex64(7 - 3j)) and np.all(got[offset + N:] == np.complex64(7 - 3j))


@pytest.mark.parametrize("offset", [0, 1])
def test_more_places_than_one_launch(gpu, offset):
    """40 places (three launches of at most 16), all overlapping in one region."""
    n = 20011
    host = [_iq(300 + 11 * i, 200 + i, 10.0 ** ((i % 7) - 3)) for i in range(40)]
    places = [(5000 + 7 * i, 9000 - i, 2) for i in range(40)]
    places[17] = (0, 1, 0)                                     # an empty place in the list
    dev = [torch.from_numpy(y).cuda() for y in host]
    want = np_build(n, list(zip(host, places)))
    buf = torch.full((n + 2,), 1.0 + 1.0j, dtype=torch.complex64, device="cuda")
    mx = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    dev_build(gpu, dev, places, buf[offset:offset + n], n, mx)
    got = buf.cpu().numpy()
    assert np.array_equal(got[offset:offset + n], want)
    assert np.all(got[:offset] == np.complex64(1 + 1j)) and np.all(got[offset + n:] == np.complex64(1 + 1j))
    assert mx.cpu().numpy().view(np.uint32)[0] == np.max(np.abs(want)).view(np.uint32)


def test_max_and_normalize_bit_exact(gpu, layout):
    want = layout["want"]
    m = np.max(np.abs(want))
    assert m.dtype == np.float32
    buf = torch.empty(N + 1, dtype=torch.complex64, device="cuda")
    for offset in (0, 1):
        out = buf[offset:offset + N]
        mx = torch.full((1,), 123.0, dtype=torch.float32, device="cuda")
        dev_build(gpu, layout["dev"], layout["places"], out, N, mx)
        assert mx.cpu().numpy().view(np.uint32)[0] == m.view(np.uint32)
        other = torch.empty(N + 1, dtype=torch.complex64, device="cuda")
        dev_normalize(gpu, out, N, mx, other[:N])            # out of place: 8-byte or 16-byte lanes
        dev_normalize(gpu, out, N, mx, out)                  # in place
        assert np.array_equal(out.cpu().numpy(), want / m)
        assert np.array_equal(other[:N].cpu().numpy(), want / m)


def test_all_zero_build_stays_zero(gpu):
    cfg = dict(signal=_iq(5000, 1), freq_shift=1e6, period=1e-3, start_time=0.0)
    v, markers = gpu.build_vector([cfg], 4000.5 / 1e6, 1e6, normalize=True)   # packet longer than the vector
    assert v.dtype == np.complex64 and v.shape == (4000,) and markers == []
    assert np.all(np.isfinite(v)) and not v.any()
    z = torch.zeros(1, dtype=torch.float32, device="cuda")
    x = torch.from_numpy(_iq(1001, 2)).cuda()
    y = torch.empty_like(x)
    dev_normalize(gpu, x, 1001, z, y)                          # m == 0: unchanged
    assert torch.equal(x, y)


@pytest.mark.parametrize("scenario", ["a", "b"])
def test_build_vector_matches_reference_golden(gpu, scenario):
    g = golden("vector_build.npz")
    sr = float(g["sample_rate"])
    cfgs = _configs(g, "signal")
    vl = float(g[f"{scenario}_vector_length"])
    plan = gpu.vector_plan(cfgs, vl, sr)
    cover = np.zeros(plan.total_samples + 1, np.int64)
    for i, (s, p, c) in enumerate(plan.places):
        for j in range(c):
            cover[s + j * p] += 1
            cover[s + j * p + len(g[f"packet{i}"])] -= 1
    k = int(np.cumsum(cover).max())
    assert k >= (3 if scenario == "a" else 1)
    v, markers = gpu.build_vector(cfgs, vl, sr)
    want = g[f"{scenario}_vector"]
    assert v.dtype == np.complex64 and v.shape == want.shape
    print(f"golden {scenario}: k={k} max|diff|={np.abs(v - want).max():.3e} (atol {k * 1e-5:.1e})")
    np.testing.assert_allclose(v, want, rtol=0, atol=k * 1e-5)
    assert [m[0] for m in markers] == g[f"{scenario}_marker_times"].tolist()
    assert markers == plan.markers
    vn, _ = gpu.build_vector(cfgs, vl, sr, normalize=True)
    max_val = float(g[f"{scenario}_max_val"])
    wantn = g[f"{scenario}_normalised"]
    print(f"golden {scenario} normalised: max|diff|={np.abs(vn - wantn).max():.3e} "
          f"(atol {2 * k * 1e-5 / max_val:.1e})")
    np.testing.assert_allclose(vn, wantn, rtol=0, atol=2 * k * 1e-5 / max_val)


def test_invalid_places_are_refused_before_any_launch(gpu):
    y = torch.from_numpy(_iq(100, 3)).cuda()
    out = torch.full((1000,), 5.0 + 0j, dtype=torch.complex64, device="cuda")
    mx = torch.full((1,), 9.0, dtype=torch.float32, device="cuda")
    for places, msg in (([(0, 0, 1)], "period"), ([(901, 10, 1)], "past the vector"),
                        ([(1, 100, 10)], "past the vector"), ([(-1, 10, 1)], "start"),
                        ([(0, 10, -1)], "count")):
        with pytest.raises(gpu.VsigError, match=msg):
            dev_build(gpu, [y], places, out, 1000, mx)
    from vector_amd import _lib
    ctx = gpu.get_context()
    arr = (_lib.PacketPlace * 2)()
    arr[0].y, arr[0].len, arr[0].start, arr[0].period, arr[0].count = y.data_ptr(), 100, 0, 100, 2
    arr[1].y, arr[1].len, arr[1].start, arr[1].period, arr[1].count = None, 100, 0, 100, 1
    rc = ctx.lib.vsig_vector_build_dev(ctx.h, arr, 2, C.c_void_p(out.data_ptr()), 1000,
                                       C.c_void_p(mx.data_ptr()))
    assert rc == -1 and b"null packet pointer" in ctx.lib.vsig_last_error(ctx.h)
    with pytest.raises(gpu.VsigError):
        ctx.check(rc, "vector_build")
    torch.cuda.synchronize()
    assert torch.all(out == 5.0) and float(mx[0]) == 9.0          # nothing was enqueued
    dev_build(gpu, [y], [(900, 10, 1)], out, 1000, mx)             # the boundary itself is fine
    assert float(mx[0]) == float(np.max(np.abs(y.cpu().numpy())))


def test_device_vector_feeds_save_and_spectrogram(gpu, tmp_path):
    g = golden("vector_build.npz")
    sr = float(g["sample_rate"])
    cfgs = _configs(g, "signal")
    cfgs[1] = dict(cfgs[1], signal=torch.from_numpy(g["packet1"]).cuda())     # a device packet
    vec, markers = gpu.build_vector(cfgs, float(g["a_vector_length"]), sr, normalize=True, device=True)
    assert isinstance(vec, torch.Tensor) and vec.is_cuda and vec.dtype == torch.complex64
    host, _ = gpu.build_vector(cfgs, float(g["a_vector_length"]), sr, normalize=True)
    assert np.array_equal(vec.cpu().numpy(), host)
    assert float(np.max(np.abs(host))) == pytest.approx(1.0, abs=1e-6)
    path = str(tmp_path / "vector.mat")
    gpu.save_vector(vec, path)
    assert np.array_equal(gpu.load_packet(path), host)
    gpu.save_vector_wv(vec, str(tmp_path / "vector.wv"), sr)
    f, t, sxx = gpu.create_spectrogram(vec, sr)
    sxx = sxx.cpu().numpy() if isinstance(sxx, torch.Tensor) else sxx
    assert sxx.shape == (len(f), len(t)) and np.all(np.isfinite(sxx)) and sxx.max() > 0


def test_build_and_normalize_capture_into_a_graph(gpu, layout):
    """Neither call synchronises or allocates: build + max + normalise replays
    from a captured graph on new packet contents."""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pk = [t.clone() for t in layout["dev"]]
        out = torch.empty(N, dtype=torch.complex64, device="cuda")
        mx = torch.empty(1, dtype=torch.float32, device="cuda")

        def step():
            dev_build(gpu, pk, layout["places"], out, N, mx)
            dev_normalize(gpu, out, N, mx, out)
        step()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        for t in pk:
            t.mul_(0.5)                                   # exact in fp32: the sums halve
        graph.replay()
        st.synchronize()
        want = layout["want"] * np.float32(0.5)
        assert float(mx[0]) == float(np.max(np.abs(want)))
        assert np.array_equal(out.cpu().numpy(), want / np.max(np.abs(want)))
