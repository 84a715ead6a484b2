"""GPU tests of the per-burst spectra and measurements (vsig_psd_segments_run,
vsig_band_measure_run, segment_spectra, measure_packets): which frames a block
of the segmented pass owns (bit-exact), equality with the single-slice traces,
the accuracy floor, NaN, the band measurement on given rows, the front end,
memory bounds and graph capture."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import accuracy_ref as acc
import packet_spectra_ref as ps
import spectrum_traces_ref as st
from guard_arena import Case, In, Out, run
from vector_amd import _lib
from vector_amd.packets import BAND_DTYPE

pytestmark = pytest.mark.gpu

NFFTS = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
P = C.c_void_p


def ptr(t):
    return None if t is None else P(t.data_ptr())


class SegPlan:
    """vsig_psd_segments_create / _free around a block."""

    def __init__(self, gpu, starts, lens, n, nperseg, hop, nfft):
        self.ctx = gpu.get_context()
        self.K, self.nfft = len(starts), nfft
        tab = np.ascontiguousarray(np.stack([np.asarray(starts, np.int64), np.asarray(lens, np.int64)], axis=1))
        self.h = P()
        self.ctx.check(self.ctx.lib.vsig_psd_segments_create(
            self.ctx.h, tab.ctypes.data_as(C.POINTER(_lib.Segment)), self.K, n, nperseg, hop, nfft,
            C.byref(self.h)), "create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.lib.vsig_psd_segments_free(self.h)

    def info(self):
        """(frames_total, blocks, frames_per_step, max_run_frames)"""
        v = [C.c_int64() for _ in range(4)]
        self.ctx.check(self.ctx.lib.vsig_psd_segments_info(self.h, *(C.byref(a) for a in v)), "info")
        return tuple(a.value for a in v)

    def run(self, xd, wd, scale, shift):
        """(mean float64, max, min float32) host arrays (K, nfft)."""
        mean = torch.empty((self.K, self.nfft), dtype=torch.float64, device="cuda")
        mx = torch.empty((self.K, self.nfft), dtype=torch.float32, device="cuda")
        mn = torch.empty((self.K, self.nfft), dtype=torch.float32, device="cuda")
        self.ctx.check(self.ctx.lib.vsig_psd_segments_run(self.h, ptr(xd), ptr(wd), scale, shift, ptr(mean),
                                                          ptr(mx), ptr(mn)), "run")
        return {"mean": mean.cpu().numpy(), "max": mx.cpu().numpy(), "min": mn.cpu().numpy()}


def win_scale(window, nperseg):
    w = acc.window32(window, nperseg)
    return w, float(1.0 / float(np.sum(w, dtype=np.float64)) ** 2)


def slice_traces(gpu, xs, wd, nperseg, hop, nfft, scale, shift):
    """vsig_psd_traces_c64_dev on one device slice: the double mean, max, min."""
    ctx = gpu.get_context()
    n = int(xs.numel())
    mean = torch.empty(nfft, dtype=torch.float64, device="cuda")
    mx = torch.empty(nfft, dtype=torch.float32, device="cuda")
    mn = torch.empty(nfft, dtype=torch.float32, device="cuda")
    ctx.check(ctx.lib.vsig_psd_traces_c64_dev(ctx.h, ptr(xs), n, 1, ptr(wd), nperseg, hop, nfft, scale, shift,
                                              (n - nperseg) // hop + 1, ptr(mean), ptr(mx), ptr(mn)), "traces")
    return {"mean": mean.cpu().numpy(), "max": mx.cpu().numpy(), "min": mn.cpu().numpy()}


# ---------------------------------------------------------------------------
# T1. frame ownership, bit-exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [64, 1024, 2048, 4096, 8192])
def test_frame_ownership_bit_exact(gpu, nfft):
    """Frame m of a segment is the constant a_m = p_m + 1j q_m (small integers)
    under a ones window: only bin 0 is non-zero and it is |a_m|^2 exactly, so
    every detector must equal the numpy reduction of spectrum()'s own stored
    output on the slice to the bit, whatever block owns which frames (the sums
    are sums of small integers: exact in any order).  The gaps between the
    segments, and the tails some segments have past their last whole frame,
    hold NaN."""
    with SegPlan(gpu, [0], [nfft], nfft, nfft, nfft, nfft) as p:
        _, _, step, run_frames = p.info()
    assert step >= 1 and run_frames >= step
    long_frames = 2 * run_frames + 2
    counts = [1, 0, step + 1, step, max(step - 1, 1), long_frames]
    # (frames, gap of NaN samples before it, tail samples it extends into the gap after it)
    layout = [(counts[0], 0, 0), (counts[1], 1, 0), (counts[2], 0, 3), (counts[3], 4, 0), (counts[4], 0, 0),
              (counts[5], 3, 0)]
    pieces, starts, lens, pos = [], [], [], 0
    for j, (cnt, gap, tail) in enumerate(layout):
        pieces.append(np.full(gap, complex(np.nan, np.nan), np.complex64))
        pos += gap
        body = st.constant_frames(nfft, cnt, seed=nfft + j)[0] if cnt else \
            np.full(nfft - 1, 3 + 2j, np.complex64)                 # too short for a frame
        pieces.append(body)
        starts.append(pos)
        lens.append(len(body) + tail)
        pos += len(body)
    x = np.concatenate(pieces)
    n = len(x)
    assert n <= 1 << 20 and starts[0] == 0 and starts[1] % 2 == 1 and starts[2] == starts[1] + lens[1]
    assert starts[5] + lens[5] == n and starts[5] % 2 == 1          # the long segment: 8-byte aligned only
    # overlapping (whole frames inside the long segment) and identical segments
    starts += [starts[5] + 3 * nfft, starts[2]]
    lens += [(step + 1) * nfft, lens[2]]
    frames = ps.nframes(lens, nfft, nfft)
    assert list(frames) == counts + [step + 1, counts[2]]
    xd = torch.from_numpy(x).cuda()
    wd = torch.ones(nfft, dtype=torch.float32, device="cuda")
    scale = 1.0 / nfft ** 2
    for order in (1, -1):                                  # the table ascending, then descending
        s_, l_, f_ = starts[::order], lens[::order], frames[::order]
        with SegPlan(gpu, s_, l_, n, nfft, nfft, nfft) as p:
            total, blocks, step2, run2 = p.info()
            assert (total, step2, run2) == (int(frames.sum()), step, run_frames)
            assert blocks == sum(-(-int(f) // run_frames) for f in frames) and -(-long_frames // run_frames) >= 3
            for shift in (0, 1):
                got = p.run(xd, wd, scale, shift)
                for k, (s, ln, nf) in enumerate(zip(s_, l_, f_)):
                    case = f"nfft={nfft} order={order} shift={shift} segment {k} start={s} frames={nf}"
                    if nf == 0:
                        for d in st.DETECTORS:
                            assert np.all(np.isnan(got[d][k])), (case, d)
                        continue
                    _, _, S = gpu.spectrum(xd[s:s + nf * nfft], 1.0, np.ones(nfft), nfft, 0, nfft,
                                           fftshift=bool(shift))
                    assert S.shape == (nfft, nf), case
                    want = st.reduce_frames(S.cpu().numpy())
                    hot = nfft // 2 if shift else 0
                    for d in st.DETECTORS:
                        assert got[d][k].dtype == want[d].dtype and np.array_equal(got[d][k], want[d]), (case, d)
                        assert got[d][k][hot] > 0 and np.count_nonzero(got[d][k]) == 1, (case, d)


# ---------------------------------------------------------------------------
# T2. equality with the single-slice path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,nperseg,noverlap", [(n, n, 0) for n in NFFTS] + [(1024, 1000, 250), (8192, 8192, 4096)])
def test_equals_single_slice_traces(gpu, nfft, nperseg, noverlap):
    """Each segment's max and min rows are vsig_psd_traces_c64_dev's on the
    slice to the bit (the same P, and max / min do not depend on the order);
    the mean is the same non-negative double terms summed in another order:
    each order is within (nframes - 1) 2^-53 of the exact sum, so the two differ
    by at most nframes 2^-52 relative."""
    hop = nperseg - noverlap
    n = 40 * nfft + 11
    x = acc.noise(n, seed=nfft + nperseg)
    w, scale = win_scale("hann", nperseg)
    starts = [0, 2 * nfft + 1, 6 * nfft + 4, n - 9 * nperseg]
    if nfft == 8192:
        # a 16-byte aligned slice takes the single-slice path's interleaved plan, whose rows are
        # not pinned to the plain plan's bit for bit: odd starts here, and the aligned
        # placement is held to the accuracy floor (test_accuracy_floor's second segment)
        starts[0], starts[2] = 1, 6 * nfft + 5
    lens = [5 * nperseg, 21 * nperseg + 5, 9 * nperseg + hop // 2, 9 * nperseg]
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    with SegPlan(gpu, starts, lens, n, nperseg, hop, nfft) as p:
        for shift in (0, 1):
            got = p.run(xd, wd, scale, shift)
            for k, (s, ln) in enumerate(zip(starts, lens)):
                want = slice_traces(gpu, xd[s:s + ln], wd, nperseg, hop, nfft, scale, shift)
                nf = (ln - nperseg) // hop + 1
                case = f"nfft={nfft} nperseg={nperseg} hop={hop} shift={shift} segment {k}"
                assert np.array_equal(got["max"][k], want["max"]), case
                assert np.array_equal(got["min"][k], want["min"]), case
                rel = np.abs(got["mean"][k] - want["mean"]) / want["mean"]
                acc.say(case, mean_rel=float(rel.max()), bound=nf * 2.0 ** -52)
                assert rel.max() <= nf * 2.0 ** -52, case


# ---------------------------------------------------------------------------
# T3. accuracy floor
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs(key):
    nfft, nperseg, noverlap = key
    x = acc.spectrum_input(nfft, nperseg, noverlap)
    S32 = acc.spectrum(x, "hann", nperseg, noverlap, nfft)
    S64 = acc.spectrum(x, "hann", nperseg, noverlap, nfft, np.complex128)
    assert S64.shape == (nfft, 3)
    return x, S32, S64


@pytest.mark.parametrize("key", [k for k in acc.SPECTRUM_SEEDS if k[0] <= 8192])
def test_accuracy_floor(gpu, key):
    """The vetted 3-frame inputs of the spectrum's accuracy floor, placed twice
    (at an odd and at an even sample) inside a longer capture of noise: each
    detector within K max|S32 - S64| (+ one float32 rounding) of the detector
    of the complex128 spectrogram, K the class of the frame's route."""
    nfft, nperseg, noverlap = key
    x, S32, S64 = _refs(key)
    pad = acc.noise(37 + 101 + 51, seed=nfft)
    cap = np.concatenate([pad[:37], x, pad[37:138], x, pad[138:]]).astype(np.complex64)
    starts = np.array([37, 37 + len(x) + 101])
    assert starts[0] % 2 == 1 and starts[1] % 2 == 0
    ends = starts + len(x) - 1
    got = gpu.segment_spectra(cap, starts, ends, 1.0, window="hann", nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                              detectors=st.DETECTORS, fftshift=False)
    assert list(got.nframes) == [3, 3] and np.array_equal(got.f, np.fft.fftfreq(nfft, 1.0))
    want = st.reduce_frames(S64)
    K = acc.route_spectrum_class(nfft)[0]
    e_ref = float(np.abs(S32.astype(np.float64) - S64).max())
    for d in st.DETECTORS:
        rows = getattr(got, d)
        assert rows.shape == (2, nfft) and rows.dtype == np.float32
        for k in range(2):
            err, lim = float(np.abs(rows[k].astype(np.float64) - want[d]).max()), st.bound(K, S32, S64, want[d])
            acc.say(f"segments nfft={nfft} nperseg={nperseg} noverlap={noverlap} {d} segment {k}", e_ref=e_ref,
                    e_gpu=err, ratio=err / e_ref, bound=lim)
            assert err <= lim, (key, d, k, err, lim)


# ---------------------------------------------------------------------------
# T4. NaN
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [256, 8192])
def test_nan_poisons_the_segments_that_hold_it(gpu, nfft):
    n = 16 * nfft
    x = acc.noise(n, seed=nfft + 4).copy()
    #           A: 4 frames        B: overlaps A's frame 2   C: 3 frames + a tail    D: touches A, clean
    starts = [1, 2 * nfft + 1 + nfft // 2, 8 * nfft + 1, 4 * nfft + 1]
    lens = [4 * nfft, 2 * nfft, 3 * nfft + 9, 2 * nfft]
    x[2 * nfft + 1 + nfft // 2 + 5] = complex(np.nan, 0.0)        # A's frame 2, B's frame 0
    x[8 * nfft + 1 + 3 * nfft + 4] = complex(0.0, np.nan)         # C's tail: in no frame
    x[7 * nfft] = complex(np.nan, np.nan)                          # in no segment
    w, scale = win_scale("hann", nfft)
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    with SegPlan(gpu, starts, lens, n, nfft, nfft, nfft) as p:
        got = p.run(xd, wd, scale, 1)
    for d in st.DETECTORS:
        assert np.all(np.isnan(got[d][0])) and np.all(np.isnan(got[d][1])), d
        assert np.all(np.isfinite(got[d][2])) and np.all(np.isfinite(got[d][3])), d
    # (an odd start: at 8192 points an aligned slice takes the single-slice path's interleaved plan)
    clean = slice_traces(gpu, xd[starts[2]:starts[2] + 3 * nfft], wd, nfft, nfft, nfft, scale, 1)
    assert np.array_equal(got["max"][2], clean["max"]) and np.array_equal(got["min"][2], clean["min"])


# ---------------------------------------------------------------------------
# T5. band measurement on given rows
# ---------------------------------------------------------------------------
TAILS = (1e-4, 0.005, 0.05, 0.25)
GAINS = (2.0 ** -40, 1.0, 2.0 ** 40)


def band_call(gpu, rows_t, nrows, nbins, ld, tail):
    ctx = gpu.get_context()
    out = torch.zeros(nrows * BAND_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.vsig_band_measure_run(ctx.h, ptr(rows_t), nrows, nbins, ld, tail, ptr(out)), "band")
    return out.cpu().numpy().view(BAND_DTYPE)


def check_band(case, rec, row, tail):
    """One record against the sequential reference; the indices are exact under
    the premise asserted here for every row."""
    want = ps.band(row, tail)
    if want["lo_bin"] < 0:
        assert (rec["peak_bin"], rec["lo_bin"], rec["hi_bin"]) == (-1, -1, -1), case
        assert np.isnan(rec["centroid"]) and np.isnan(rec["peak"]), case
        assert np.array_equal(rec["power"], want["power"], equal_nan=True), case
        assert rec["flags"] != 0, case
        return
    nbins = len(row)
    margin = ps.band_margin(row, tail)
    assert margin > ps.PREMISE, (case, margin)
    assert rec["flags"] == 0, case
    assert abs(rec["power"] - want["power"]) <= nbins * 2.0 ** -52 * want["power"], case
    assert abs(rec["centroid"] - want["centroid"]) <= nbins * 2.0 ** -52 * want["centroid"], case
    assert rec["peak"] == want["peak"] and rec["peak_bin"] == want["peak_bin"], case
    assert (rec["lo_bin"], rec["hi_bin"]) == (want["lo_bin"], want["hi_bin"]), (case, margin)


@pytest.mark.parametrize("nbins", [64, 100, 1000, 1024, 8192])
def test_band_measure_rows(gpu, nbins):
    """power and centroid within nbins 2^-52 relative of numpy's sequential
    sums, peak and the three indices exact.  The rows' seeds are
    the first for which the reference alone keeps every cumulative sum 1e-9 of
    the total away from both targets of every tail."""
    rows, names = [], []
    for kind in ps.ROW_KINDS:
        for g in GAINS:
            m, seed = ps.vetted_row(kind, nbins, TAILS, g, nbins)
            rows.append(m)
            names.append(f"{kind} gain={g:g} seed={seed}")
    rows.append(np.zeros(nbins))
    names.append("zero")
    bad = ps.band_row("flat", nbins, 1)
    bad[nbins // 3] = np.nan
    rows.append(bad)
    names.append("nan")
    ld = nbins + 3
    arr = np.full((len(rows), ld), -7.0)
    arr[:, :nbins] = np.array(rows)
    rt = torch.from_numpy(arr).cuda()
    for tail in TAILS:
        rec = band_call(gpu, rt, len(rows), nbins, ld, tail)
        again = band_call(gpu, rt, len(rows), nbins, ld, tail)
        assert rec.tobytes() == again.tobytes()
        for r, row, name in zip(rec, rows, names):
            check_band(f"nbins={nbins} tail={tail} {name}", r, row, tail)
    assert rec[-2]["flags"] == 2 and rec[-1]["flags"] & 1


# bins of bit-equal maxima; the kernel gives a thread 16 contiguous bins, a wave 64 threads and a tile 4096 bins
TIES = {
    "one chunk": (40, 45),
    "an odd and the next even chunk of a wave": (16 * 1 + 3, 16 * 2 + 5),
    "an odd and a later even chunk of a wave": (16 * 1 + 3, 16 * 18 + 7),
    "an even and a later odd chunk of a wave": (16 * 6 + 15, 16 * 33),
    "three chunks of a wave": (16 * 63 + 2, 16 * 31 + 1, 16 * 47),
    "two waves": (16 * 5 + 1, 16 * (128 + 3) + 2),
    "the last and the first wave": (16 * 255 + 15, 16 * 7),
    "two tiles": (16 * 100 + 4, 4096 + 16 * 7 + 9),
    "two tiles, the later chunk first in its wave": (16 * 37 + 4, 4096 + 16 * 2),
}


@pytest.mark.parametrize("nbins", [1000, 8192])
def test_band_measure_tied_maxima(gpu, nbins):
    """peak_bin is the first of bit-equal maxima (np.argmax), wherever the
    kernel's chunks, waves and tiles put them."""
    names = [k for k, v in TIES.items() if max(v) < nbins]
    assert len(names) >= 4
    rows = []
    for j, name in enumerate(names):
        m = np.random.default_rng(nbins + j).random(nbins) * 0.5
        m[list(TIES[name])] = 2.0
        rows.append(m)
    rows.append(np.full(nbins, 0.25))                       # every bin a maximum
    names.append("flat")
    rt = torch.from_numpy(np.array(rows)).cuda()
    rec = band_call(gpu, rt, len(rows), nbins, nbins, 0.005)
    for r, row, name in zip(rec, rows, names):
        assert r["peak_bin"] == int(np.argmax(row)) and r["peak"] == row.max() and r["flags"] == 0, (nbins, name)
        assert abs(r["power"] - np.cumsum(row)[-1]) <= nbins * 2.0 ** -52 * r["power"], (nbins, name)


# ---------------------------------------------------------------------------
# T6. front end
# ---------------------------------------------------------------------------
FE = dict(nfft=256, sr=20e6, n=1 << 16)


@functools.lru_cache(maxsize=None)
def _planted():
    """Three complex tones at bin centres and one band-limited noise burst in
    noise 100 dB down: (signal, starts, ends (inclusive), tone bins, tone amplitudes)."""
    nfft, n = FE["nfft"], FE["n"]
    x = (acc.noise(n, seed=77) * np.float32(1e-5)).astype(np.complex64)
    starts = np.array([1001, 9000, 20001, 40000])
    length = 10 * nfft + 17
    bins = [-100, 0, 37]
    amps = [1.0, 0.5, 2.0]
    t = np.arange(length)
    for s, b, a in zip(starts[:3], bins, amps):
        x[s:s + length] += (a * np.exp(2j * np.pi * b * t / nfft)).astype(np.complex64)
    spec = np.fft.fft(acc.noise(length, seed=78).astype(np.complex128))
    f = np.fft.fftfreq(length)
    spec[(f < 0.05) | (f > 0.20)] = 0.0
    x[starts[3]:starts[3] + length] += np.fft.ifft(spec).astype(np.complex64)
    return x, starts, starts + length - 1, bins, amps


def test_measure_packets_planted_bursts(gpu):
    nfft, sr = FE["nfft"], FE["sr"]
    x, starts, ends, bins, amps = _planted()
    df = sr / nfft
    m = gpu.measure_packets(x, (starts, ends), sr, window="boxcar", nperseg=nfft, return_spectra=True)
    assert isinstance(m, gpu.PacketMeasurements) and isinstance(m.spectra, gpu.SegmentSpectra)
    assert list(m.nframes) == [10] * 4 and m.nframes.dtype == np.int64
    for k, (b, a) in enumerate(zip(bins, amps)):
        assert m.peak_freq[k] == b * df, k
        assert abs(m.power[k] - a * a) <= 1e-5 * a * a, (k, m.power[k])
        assert m.bandwidth[k] == df and m.f_lo[k] == (b - 0.5) * df and m.f_hi[k] == (b + 0.5) * df, k
        assert abs(m.center_freq[k] - b * df) <= 1e-3 * df, k
    # the noise burst: around its band [0.05, 0.20] sr (a boxcar frame leaks about a percent past the edges)
    assert 0.0 <= m.f_lo[3] < 0.05 * sr + 2 * df and 0.20 * sr - 2 * df < m.f_hi[3] <= 0.25 * sr
    assert m.f_lo[3] < m.center_freq[3] < m.f_hi[3] and abs(m.center_freq[3] - 0.125 * sr) < 0.02 * sr
    # every field is the band reference of the returned float64 mean rows
    sp = m.spectra
    assert sp.mean.dtype == np.float64 and sp.mean.shape == (4, nfft) and sp.max.dtype == np.float32
    assert np.array_equal(sp.f, np.fft.fftshift(np.fft.fftfreq(nfft, 1 / sr)))
    tail = (1 - 0.99) / 2
    w = np.ones(nfft, np.float32)
    for k in range(4):
        assert ps.band_margin(sp.mean[k], tail) > ps.PREMISE, k
        want = ps.to_hz(ps.band(sp.mean[k], tail), nfft, sr, 0.0, w)
        for name in ("peak_freq", "f_lo", "f_hi", "bandwidth"):
            assert getattr(m, name)[k] == want[name], (k, name)
        assert abs(m.power[k] - want["power"]) <= nfft * 2.0 ** -52 * want["power"], k
        assert abs(m.center_freq[k] - want["center_freq"]) <= nfft * 2.0 ** -52 * sr, k
    # a centre frequency moves every frequency field by the one addition
    cf = 2.4e9
    m2 = gpu.measure_packets(x, (starts, ends), sr, cf, window="boxcar", nperseg=nfft)
    assert m2.spectra is None
    for name in ("center_freq", "peak_freq", "f_lo", "f_hi"):
        assert np.array_equal(getattr(m2, name), cf + getattr(m, name)), name
    assert np.array_equal(m2.bandwidth, m.bandwidth) and np.array_equal(m2.power, m.power)
    # occupied: a wider share cannot narrow the band
    m90 = gpu.measure_packets(x, (starts, ends), sr, window="boxcar", nperseg=nfft, occupied=0.9)
    assert np.all(m90.bandwidth <= m.bandwidth) and m90.bandwidth[3] < m.bandwidth[3]


def test_measure_packets_input_forms(gpu):
    nfft, sr = FE["nfft"], FE["sr"]
    x, starts, ends, bins, _ = _planted()
    pk = gpu.detect_packets(x, sr, threshold=1e-3)
    assert len(pk.starts) == 4 and np.all(np.abs(pk.starts - starts) <= 64) and np.all(np.abs(pk.ends - ends) <= 64)
    a = gpu.measure_packets(x, pk, sr, window="boxcar", nperseg=nfft, return_spectra=True)
    b = gpu.measure_packets(x, (pk.starts, pk.ends), sr, window="boxcar", nperseg=nfft, return_spectra=True)
    d = gpu.measure_packets(torch.from_numpy(x).cuda(), pk, sr, window="boxcar", nperseg=nfft, return_spectra=True)
    assert [bn * sr / nfft for bn in bins] == list(a.peak_freq[:3])
    for name in gpu.PacketMeasurements._fields[:-1]:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
        assert np.array_equal(getattr(a, name), getattr(d, name), equal_nan=True), name
        assert isinstance(getattr(d, name), np.ndarray), name
    for name in st.DETECTORS:
        rows = getattr(d.spectra, name)
        assert isinstance(rows, torch.Tensor) and rows.is_cuda
        assert np.array_equal(rows.cpu().numpy(), getattr(a.spectra, name)), name
    # default nperseg: the largest power of two in [64, 1024] not above the shortest burst
    auto = gpu.measure_packets(x, (starts, ends), sr)
    assert list(auto.nframes) == [2] * 4                            # 2577 samples: nperseg 1024
    # a burst shorter than nperseg has no frame: NaN in every float field
    short = gpu.measure_packets(x, ([starts[0], starts[1]], [starts[0] + 100, ends[1]]), sr, nperseg=nfft)
    assert list(short.nframes) == [0, 10]
    for name in gpu.PacketMeasurements._fields[:-2]:
        v = getattr(short, name)
        assert np.isnan(v[0]) and np.isfinite(v[1]), name
    none = gpu.measure_packets(x, (np.zeros(0, np.int64), np.zeros(0, np.int64)), sr, nperseg=nfft)
    assert all(len(getattr(none, name)) == 0 for name in gpu.PacketMeasurements._fields[:-1])


def test_segment_spectra_dtypes_and_forms(gpu):
    nfft = 128
    x = acc.noise(6000, seed=11)
    starts, ends = np.array([5, 1000, 3000]), np.array([2000, 1000 + 3 * nfft - 1, 3050])
    a = gpu.segment_spectra(x, starts, ends, 2e6, nperseg=nfft, detectors=st.DETECTORS)
    assert isinstance(a, gpu.SegmentSpectra) and list(a.nframes) == [15, 3, 0]
    assert all(v.dtype == np.float32 and v.shape == (3, nfft) for v in a[1:4])
    assert np.array_equal(a.f, np.fft.fftshift(np.fft.fftfreq(nfft, 1 / 2e6)))
    assert all(np.all(np.isnan(v[2])) and np.all(np.isfinite(v[:2])) for v in a[1:4])
    one = gpu.averaged_spectrum(x[1000:1000 + 3 * nfft], 2e6, "hann", nfft, 0, nfft, fftshift=True)
    assert np.array_equal(a.max[1], one.max) and np.array_equal(a.min[1], one.min)
    wide = gpu.segment_spectra(x.astype(np.complex128), starts, ends, 2e6, nperseg=nfft, detectors=st.DETECTORS)
    assert all(v.dtype == np.float64 for v in wide[1:4])
    assert np.array_equal(wide.max, a.max.astype(np.float64), equal_nan=True)
    assert np.array_equal(wide.mean.astype(np.float32), a.mean, equal_nan=True)
    dflt = gpu.segment_spectra(x, starts, ends, 2e6, nperseg=nfft)
    assert dflt.max is None and dflt.min is None and np.array_equal(dflt.mean, a.mean, equal_nan=True)
    dev = gpu.segment_spectra(torch.from_numpy(x).cuda(), starts, ends, 2e6, nperseg=nfft, detectors=("max",))
    assert dev.mean is None and dev.max.is_cuda and dev.max.dtype == torch.float32
    assert np.array_equal(dev.max.cpu().numpy(), a.max, equal_nan=True)
    plain = gpu.segment_spectra(x, starts, ends, 2e6, nperseg=nfft, fftshift=False)
    assert np.array_equal(np.fft.fftshift(plain.mean, axes=1), a.mean, equal_nan=True)
    assert np.array_equal(plain.f, np.fft.fftfreq(nfft, 1 / 2e6))


def test_c_abi_errors_name_the_segment(gpu):
    ctx = gpu.get_context()
    lib = ctx.lib
    seg = (_lib.Segment * 3)(_lib.Segment(0, 100), _lib.Segment(50, 200), _lib.Segment(200, 57))
    h = P()
    for args, word in (((seg, 3, 256, 64, 64, 64), "segment 2"), ((seg, 3, 256, 64, 0, 64), "hop"),
                       ((seg, 2, 256, 128, 64, 64), "nfft"), ((seg, -1, 256, 64, 64, 64), "nseg"),
                       ((seg, 2, 0, 64, 64, 64), "n must")):
        assert lib.vsig_psd_segments_create(ctx.h, *args, C.byref(h)) == -1 and not h.value
        assert word in lib.vsig_last_error(ctx.h).decode(), args
    for nfft in (32, 100, 16384):
        assert lib.vsig_psd_segments_create(ctx.h, seg, 2, 256, 16, 16, nfft, C.byref(h)) == -4 and not h.value
    x = torch.zeros(300, dtype=torch.complex64, device="cuda")
    w = torch.ones(64, dtype=torch.float32, device="cuda")
    mean = torch.full((2, 64), 5.0, dtype=torch.float64, device="cuda")
    assert lib.vsig_psd_segments_create(ctx.h, seg, 2, 256, 64, 64, 64, C.byref(h)) == 0
    try:
        assert lib.vsig_psd_segments_run(h, ptr(x), ptr(w), 1.0, 0, None, None, None) == -1
        assert lib.vsig_psd_segments_run(h, None, ptr(w), 1.0, 0, ptr(mean), None, None) == -1
        assert lib.vsig_psd_segments_run(h, P(x.data_ptr() + 4), ptr(w), 1.0, 0, ptr(mean), None, None) == -1
        assert "aligned" in lib.vsig_last_error(ctx.h).decode()
        assert lib.vsig_psd_segments_run(h, ptr(x), ptr(w), 1.0, 0, ptr(mean), None, None) == 0
        torch.cuda.synchronize()
        assert np.all(mean.cpu().numpy() == 0.0)
    finally:
        lib.vsig_psd_segments_free(h)
    # an empty table is valid and does nothing
    e = P()
    assert lib.vsig_psd_segments_create(ctx.h, None, 0, 256, 64, 64, 64, C.byref(e)) == 0
    mean.fill_(5.0)
    assert lib.vsig_psd_segments_run(e, ptr(x), ptr(w), 1.0, 0, ptr(mean), None, None) == 0
    torch.cuda.synchronize()
    lib.vsig_psd_segments_free(e)
    assert np.all(mean.cpu().numpy() == 5.0)
    # the remaining refusals of create, each with a real context and its message
    neg = (_lib.Segment * 2)(_lib.Segment(0, 100), _lib.Segment(-1, 10))
    negl = (_lib.Segment * 1)(_lib.Segment(5, -1))
    for args, word in (((seg, (1 << 24) + 1, 256, 64, 64, 64), "nseg"), ((seg, 2, (1 << 40) + 1, 64, 64, 64), "n must"),
                       ((neg, 2, 256, 64, 64, 64), "segment 1"), ((negl, 1, 256, 64, 64, 64), "segment 0"),
                       ((seg, 2, 256, 0, 64, 64), "nperseg"), ((None, 2, 256, 64, 64, 64), "null segment table")):
        assert lib.vsig_psd_segments_create(ctx.h, *args, C.byref(h)) == -1 and not h.value, args
        assert word in lib.vsig_last_error(ctx.h).decode(), (args, lib.vsig_last_error(ctx.h).decode())
    assert lib.vsig_psd_segments_create(ctx.h, seg, 2, 256, 64, 64, 64, None) == -1
    assert "null pointer" in lib.vsig_last_error(ctx.h).decode()
    rec = torch.full((88,), 0xA5, dtype=torch.uint8, device="cuda")
    mean.fill_(1.0)
    for args, word in (((ptr(mean), -1, 64, 64, 0.005, ptr(rec)), "nrows"), ((ptr(mean), 1 << 31, 64, 64, 0.005, ptr(rec)), "nrows"),
                       ((ptr(mean), 2, 0, 64, 0.005, ptr(rec)), "nbins"), ((ptr(mean), 2, 64, 63, 0.005, ptr(rec)), "ld >= nbins"),
                       ((ptr(mean), 2, 64, 64, 0.0, ptr(rec)), "tail"), ((ptr(mean), 2, 64, 64, 0.5, ptr(rec)), "tail"),
                       ((ptr(mean), 2, 64, 64, -0.1, ptr(rec)), "tail"), ((ptr(mean), 2, 64, 64, float("nan"), ptr(rec)), "tail"),
                       ((None, 2, 64, 64, 0.005, ptr(rec)), "null pointer"), ((ptr(mean), 2, 64, 64, 0.005, None), "null pointer"),
                       ((P(mean.data_ptr() + 4), 1, 64, 64, 0.005, ptr(rec)), "aligned"),
                       ((ptr(mean), 2, 64, 64, 0.005, P(rec.data_ptr() + 4)), "aligned")):
        assert lib.vsig_band_measure_run(ctx.h, *args) == -1, args
        assert word in lib.vsig_last_error(ctx.h).decode(), (args, lib.vsig_last_error(ctx.h).decode())
    torch.cuda.synchronize()
    assert np.all(rec.cpu().numpy() == 0xA5)                  # no refusal enqueued anything
    assert lib.vsig_band_measure_run(ctx.h, ptr(mean), 0, 64, 64, 0.005, ptr(rec)) == 0
    assert lib.vsig_band_measure_run(ctx.h, ptr(mean), 2, 64, 64, 0.005, ptr(rec)) == 0
    torch.cuda.synchronize()
    got = rec.cpu().numpy()[:80].view(BAND_DTYPE)
    assert list(got["power"]) == [64.0, 64.0] and list(got["peak_bin"]) == [0, 0] and np.all(rec.cpu().numpy()[80:] == 0xA5)


# ---------------------------------------------------------------------------
# T7. memory bounds
# ---------------------------------------------------------------------------
SKEW2 = [(0, 0), (1, 0), (0, 1), (1, 1)]
WHICH = [("mean", "max", "min"), ("mean",), ("max",), ("min",), ("max", "min"), ("mean", "min")]
DT = {"mean": np.float64, "max": np.float32, "min": np.float32}


def _segments_case(gpu, plan, label, x, holes, win, scale, shift, starts, lens, nperseg, hop, nfft, si, so, which):
    ctx = gpu.get_context()
    K = len(starts)
    ref = ps.segment_traces(x, starts, [s + ln - 1 for s, ln in zip(starts, lens)], win, nperseg, nperseg - hop,
                            nfft, np.complex64, fftshift=bool(shift))
    tol = 1e-5 * np.nanmax(ref["max"])
    outs = {name: Out(K * nfft, DT[name], ((so + k) % 2) * np.dtype(DT[name]).itemsize)
            for k, name in enumerate(("mean", "max", "min")) if name in which}

    def call(p):
        return ctx.lib.vsig_psd_segments_run(plan.h, P(p["x"]), P(p["win"]), scale, shift,
                                             *(P(p[k]) if k in which else None for k in ("mean", "max", "min")))

    def check(o):
        for name in which:
            got = o[name].reshape(K, nfft).astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(ref[name])), f"{name}: NaN rows differ"
            err = np.nanmax(np.abs(got - ref[name]))
            assert err <= tol, f"{name} error {err:.3e} > {tol:.3e}"
    return Case("vsig_psd_segments_run", f"{label} shift={shift} out={'+'.join(which)} skew=({si},{so})",
                {"x": In(x, 8 * si, holes=holes), "win": In(win, 4 * si)}, outs, call, check)


@pytest.mark.parametrize("nfft,nperseg,hop", [(64, 64, 64), (256, 200, 77), (2048, 2048, 2048), (4096, 4096, 1024),
                                              (8192, 8192, 8192), (8192, 7000, 7000)])
def test_bounds_psd_segments(gpu, nfft, nperseg, hop):
    """x is declared with holes everywhere outside the union of the frames: the
    gaps between segments, a segment's tail past its last whole frame, and the
    samples of a segment too short for a frame."""
    with SegPlan(gpu, [0], [nperseg], nperseg, nperseg, hop, nfft) as p0:
        _, _, step, run_frames = p0.info()
    counts = [1, 0, step + 1, 2 * run_frames + 1, 2]
    tails = [0, 0, hop - 1, nperseg // 3 if hop > nperseg // 3 else hop - 1, 1]
    gaps = [0, 5, 0, 3, 2]
    starts, lens, pos = [], [], 0
    for cnt, tail, gap in zip(counts, tails, gaps):
        pos += gap
        ln = (cnt - 1) * hop + nperseg + tail if cnt else nperseg - 1
        starts.append(pos)
        lens.append(ln)
        pos += ln
    n = pos + 7                                           # and samples past the last segment
    starts.append(starts[3] + 2 * hop + 1)                # overlaps the long segment, off its frame grid
    lens.append(nperseg + hop)
    assert n <= 1 << 20 and list(ps.nframes(lens, nperseg, hop)) == counts + [2]
    x = acc.noise(n, seed=nfft + hop)
    used = np.zeros(n, bool)
    for s, ln in zip(starts, lens):
        for m in range(int(ps.nframes([ln], nperseg, hop)[0])):
            used[s + m * hop:s + m * hop + nperseg] = True
    assert not used.all()
    win, scale = win_scale("hann", nperseg)
    with SegPlan(gpu, starts, lens, n, nperseg, hop, nfft) as plan:
        for j, (si, so) in enumerate(SKEW2):
            run(_segments_case(gpu, plan, f"nfft={nfft} nperseg={nperseg} hop={hop} n={n}", x, ~used, win, scale,
                               j % 2, starts, lens, nperseg, hop, nfft, si, so, WHICH[(j + nfft // 64) % len(WHICH)]))


@pytest.mark.parametrize("nbins", [64, 100, 1000, 8192])
def test_bounds_band_measure(gpu, nbins):
    ctx = gpu.get_context()
    nrows, tail = 5, 0.005
    for si, so in SKEW2:
        ld = nbins + 1 + si
        rows = [ps.vetted_row(kind, nbins, (tail,), 1.0, nbins)[0] for kind in ps.ROW_KINDS] + [np.zeros(nbins)]
        arr = np.zeros((nrows, ld))
        arr[:, :nbins] = np.array(rows)
        holes = np.zeros((nrows, ld), bool)
        holes[:, nbins:] = True

        def call(p):
            return ctx.lib.vsig_band_measure_run(ctx.h, P(p["rows"]), nrows, nbins, ld, tail, P(p["out"]))

        def check(o):
            for k, (rec, row) in enumerate(zip(o["out"], rows)):
                check_band(f"bounds nbins={nbins} row {k}", rec, row, tail)
        run(Case("vsig_band_measure_run", f"nbins={nbins} ld={ld} skew=({si},{so})",
                 {"rows": In(arr, 8 * si, holes=holes)}, {"out": Out(nrows, BAND_DTYPE, 8 * so)}, call, check))


# ---------------------------------------------------------------------------
# T8. capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [1024, 8192])
def test_run_pair_captures_into_a_graph(gpu, nfft):
    """The two _run calls neither allocate nor synchronise: one capture on a
    single stream, replayed on new contents, gives the bytes of plain calls."""
    n = 30 * nfft
    a = acc.noise(n, seed=nfft + 2)
    starts, lens = [3, 9 * nfft, 4 * nfft + 1], [7 * nfft, 21 * nfft, 2 * nfft + 5]
    w, scale = win_scale("hann", nfft)
    K = len(starts)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        x = torch.from_numpy(a).cuda()
        wd = torch.from_numpy(w).cuda()
        mean = torch.zeros((K, nfft), dtype=torch.float64, device="cuda")
        mx = torch.zeros((K, nfft), dtype=torch.float32, device="cuda")
        rec = torch.zeros(K * BAND_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        with SegPlan(gpu, starts, lens, n, nfft, nfft, nfft) as plan:
            def step():
                ctx = gpu.get_context()
                ctx.check(ctx.lib.vsig_psd_segments_run(plan.h, ptr(x), ptr(wd), scale, 1, ptr(mean), ptr(mx), None),
                          "segments")
                ctx.check(ctx.lib.vsig_band_measure_run(ctx.h, ptr(mean), K, nfft, nfft, 0.005, ptr(rec)), "band")
            step()
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                step()
            new = np.roll(a, 4321) * np.float32(0.5)
            x.copy_(torch.from_numpy(new))
            for t in (mean, mx, rec):
                t.zero_()
            graph.replay()
            stream.synchronize()
            replayed = [t.cpu().numpy().copy() for t in (mean, mx, rec)]
            for t in (mean, mx, rec):
                t.zero_()
            step()
            stream.synchronize()
            for r, t in zip(replayed, (mean, mx, rec)):
                assert np.array_equal(r, t.cpu().numpy())
            del graph
    assert np.all(replayed[0] > 0) and np.all(replayed[1] >= replayed[0])
    bands = replayed[2].view(BAND_DTYPE)
    for k in range(K):
        want = ps.band(replayed[0][k], 0.005)
        assert bands[k]["peak_bin"] == want["peak_bin"] and bands[k]["peak"] == want["peak"]
        assert abs(bands[k]["power"] - want["power"]) <= nfft * 2.0 ** -52 * want["power"]
