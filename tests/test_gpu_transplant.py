"""GPU checks of the transplant workflow's scoring step: region.hip behind
vsig_region_power_dev, and vector_amd.validate_transplant_quality /
measure_packet_timing / extract_reference_segment / transplant_and_validate
on top of it.

ABI: the three sums against math.fsum over numpy's own float32 element
values (np.abs(x) ** 2 and np.abs(a - b) ** 2 in complex64).  The kernel forms
the same elements to the bit and adds them in double.  All terms are
non-negative, so a sum errs by at most (additions any one term passes through)
x 2^-53 relative.  The kernel's tree is shallow -- a thread's trips, six wave
steps, the block's waves, the same again in the finalize: under 64 additions
at the largest length below, 7e-15 -- and a plain left-to-right sum of that
length would stay under 2.4e-10.  The bound asserted is relative 1e-10 at
every length.

Front end: every case of tests/golden/transplant_quality.npz (the reference's
own results) numpy-in and device-in, then edges without goldens against the
numpy restatement test_transplant_cpu.py proves on those goldens."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import golden
from test_transplant_cpu import (CASES, CRITERIA, case_inputs, golden_dict, ref_timing,
                                 ref_validate)

pytestmark = pytest.mark.gpu

# launch geometry of region_power (region.hip): at most G blocks of 256
# threads, V samples per lane and trip by 16-byte loads.  At BIG every thread
# makes at least two trips and a ragged tail is left over.
G, V = 2048, 2
BIG = 2 * G * 256 * V + 257
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097, BIG]
OFFSETS = [(0, 0), (1, 1), (1, 0), (0, 1), (3, 2)]
RTOL = 1e-10


def _fsum(x32):
    return math.fsum(x32.astype(np.float64).tolist())


@pytest.fixture(scope="module")
def pairs():
    """n -> (a, b, (S0, S1, S2) by fsum): seeded complex64 pairs with a sample
    of magnitude 100 at either end of each operand; computed once per length."""
    rng = np.random.default_rng(77)
    base = (rng.standard_normal((2, BIG)) + 1j * rng.standard_normal((2, BIG))).astype(np.complex64)
    cache = {}

    def get(n):
        if n not in cache:
            a, b = base[0, :n].copy(), base[1, :n].copy()
            a[0], b[0] = 100, 100j
            a[-1], b[-1] = -60 + 80j, 100          # n == 1: the last write stands
            want = (_fsum(np.abs(a) ** 2), _fsum(np.abs(b) ** 2), _fsum(np.abs(a - b) ** 2))
            assert (np.abs(a) ** 2).dtype == np.float32
            cache[n] = (a, b, want)
        return cache[n]
    return get


def _place(x, off):
    """x on the device at sample offset off of a 64-byte-aligned allocation."""
    buf = torch.zeros(len(x) + off + 1, dtype=torch.complex64, device="cuda")
    assert buf.data_ptr() % 64 == 0
    t = buf[off:off + len(x)]
    t.copy_(torch.from_numpy(x))
    return t


def region_power(va, a, b, n, sums="alloc"):
    ctx = va.get_context()
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    rc = ctx.lib.vsig_region_power_dev(ctx.h, ptr(a), ptr(b), n, ptr(out if sums == "alloc" else sums))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def assert_sums(got, want, what):
    for k in range(3):
        err = abs(got[k] - want[k]) / want[k]
        print(f"{what} S{k}: got {got[k]!r} want {want[k]!r} rel {err:.3e}")
        assert err <= RTOL, (what, k)


@pytest.mark.parametrize("n", LENGTHS)
def test_region_power_exact(gpu, pairs, n):
    a, b, want = pairs(n)
    rc, got = region_power(gpu, _place(a, 0), _place(b, 0), n)
    assert rc == 0
    assert_sums(got, want, f"n={n}")


@pytest.mark.parametrize("n", [257, BIG])
@pytest.mark.parametrize("oa,ob", OFFSETS)
def test_region_power_alignment(gpu, pairs, n, oa, ob):
    a, b, want = pairs(n)
    rc, got = region_power(gpu, _place(a, oa), _place(b, ob), n)
    assert rc == 0
    assert_sums(got, want, f"n={n} offsets=({oa},{ob})")


@pytest.mark.parametrize("n", [257, BIG])
def test_region_power_deterministic(gpu, pairs, n):
    a, b, _ = pairs(n)
    ta, tb = _place(a, 1), _place(b, 1)
    first = region_power(gpu, ta, tb, n)[1]
    again = region_power(gpu, ta, tb, n)[1]
    assert first.tobytes() == again.tobytes()


@pytest.mark.parametrize("n", [1, 257, 4097])
def test_region_power_aliased(gpu, pairs, n):
    a, _, want = pairs(n)
    ta = _place(a, 0)
    rc, got = region_power(gpu, ta, ta, n)
    assert rc == 0
    assert got[2] == 0.0 and got[0] == got[1]
    assert abs(got[0] - want[0]) <= RTOL * want[0]


def test_region_power_bad_arguments(gpu, pairs):
    a, b, _ = pairs(64)
    ta, tb = _place(a, 0), _place(b, 0)
    assert region_power(gpu, ta, tb, 0)[0] == -1
    assert region_power(gpu, ta, tb, -3)[0] == -1
    assert region_power(gpu, None, tb, 64)[0] == -1
    assert region_power(gpu, ta, None, 64)[0] == -1
    assert region_power(gpu, ta, tb, 64, sums=None)[0] == -1
    rc, got = region_power(gpu, ta, tb, 64)              # the context still works
    assert rc == 0 and np.isfinite(got).all()


# ---------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def GD():
    return golden("transplant_quality.npz")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def assert_validation(got, want, what):
    """The issue's table: integers, booleans and criteria exact;
    reference_correlation bit-equal (the refine's contract);
    reference_confidence within 1e-5 (vsig.h's contract); power_ratio relative
    1e-5 (numpy's float32 pairwise mean errs by <= ~1.5e-6 at these sizes, the
    ratio doubles it, the GPU's double sums add nothing); a finite snr within
    1e-4 dB (4.34 x a 6e-6 ratio error plus float32 rounding of the value);
    inf and 0.0 exact."""
    assert set(got) == set(want) and set(got["criteria"]) == set(CRITERIA)
    for k in ("reference_correlation", "reference_confidence", "power_ratio", "snr_improvement_db"):
        print(f"{what} {k}: got {got[k]!r} want {want[k]!r}")
    for k in ("transplant_length_samples", "vector_location", "success", "transplant_length_us",
              "time_precision_us"):
        assert got[k] == want[k], (what, k)
    for k in CRITERIA:
        assert got["criteria"][k] == want["criteria"][k], (what, k)
    assert float(got["reference_correlation"]) == float(want["reference_correlation"]), what
    assert abs(float(got["reference_confidence"]) - float(want["reference_confidence"])) <= 1e-5, what
    for k, tol, rel in (("power_ratio", 1e-5, True), ("snr_improvement_db", 1e-4, False)):
        g, w = float(got[k]), float(want[k])
        if np.isfinite(w) and w != 0.0:
            assert abs(g - w) <= tol * (abs(w) if rel else 1.0), (what, k)
            assert np.asarray(got[k]).dtype == np.float32, (what, k)     # as the reference returns it
        else:
            assert g == w, (what, k)


@pytest.mark.parametrize("where", ["numpy", "cuda"])
@pytest.mark.parametrize("case", CASES)
def test_validate_golden(gpu, GD, case, where):
    orig, new, packet, loc, refseg, sr = case_inputs(GD, case)
    if where == "cuda":
        orig, new, packet, refseg = _dev(orig), _dev(new), _dev(packet), _dev(refseg)
    with np.errstate(divide="ignore"):
        got = gpu.validate_transplant_quality(orig, new, packet, loc, refseg, sr)
    assert_validation(got, golden_dict(GD, case), f"{case}/{where}")


def test_validate_numpy_and_device_agree(gpu, GD):
    for case in ("ok", "flat", "mid"):
        orig, new, packet, loc, refseg, sr = case_inputs(GD, case)
        h = gpu.validate_transplant_quality(orig, new, packet, loc, refseg, sr)
        d = gpu.validate_transplant_quality(_dev(orig), _dev(new), _dev(packet), loc, _dev(refseg), sr)
        assert h == d, case


def test_timing_and_segment_golden(gpu, GD):
    vector, packet = GD["vector"], GD["packet"]
    for v, p in ((vector, packet), (_dev(vector), _dev(packet))):
        assert list(gpu.measure_packet_timing(v, p[:256])) == GD["timing_tmpl"].tolist()
        assert list(gpu.measure_packet_timing(v)) == GD["timing_energy"].tolist()
    for j, (lo, hi) in enumerate(GD["segment_args"].tolist()):
        seg = gpu.extract_reference_segment(_dev(packet), lo, hi)
        assert seg.is_cuda and np.array_equal(seg.cpu().numpy(), GD[f"segment_{j}"])


EDGES = {
    "odd_location": dict(loc=5001),
    "even_location": dict(loc=5002),
    "length_1": dict(loc=16383),
    "negative_location": dict(loc=-1500, cut=2000),      # [-1500:1501] of 2000 samples: 1001 long
    "c128_reference": dict(loc=5003, c128=True),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_validate_edges(gpu, GD, edge):
    e = EDGES[edge]
    orig, new, packet, _, _, sr = case_inputs(GD, "ok")
    refseg = GD["mid_ref"]
    if e.get("c128"):
        refseg = refseg.astype(np.complex128) * (1 + 1e-9)       # not exact in complex64
    if "cut" in e:
        orig, new = orig[4000:4000 + e["cut"]].copy(), new[4000:4000 + e["cut"]].copy()
    want = ref_validate(orig, new, packet, e["loc"], refseg, sr)
    if edge == "length_1":
        assert want["transplant_length_samples"] == 1
    if edge == "negative_location":
        assert want["transplant_length_samples"] == 3001 and len(orig[-1500:1501]) == 1001
    for where in ("numpy", "cuda"):
        args = (orig, new, packet) if where == "numpy" else (_dev(orig), _dev(new), _dev(packet))
        got = gpu.validate_transplant_quality(*args, e["loc"], refseg, sr)
        assert_validation(got, want, f"{edge}/{where}")


def test_validate_errors(gpu, GD):
    orig, new, packet, _, refseg, sr = case_inputs(GD, "ok")
    empty = np.zeros(0, np.complex64)
    for loc in (len(orig), len(orig) + 10, -5):           # [-5:2996] of 16384 samples is empty
        with pytest.raises(ValueError):
            ref_validate(orig, new, packet, loc, refseg, sr)
        for r in (refseg, empty):
            with pytest.raises(ValueError):
                gpu.validate_transplant_quality(orig, new, packet, loc, r, sr)
            with pytest.raises(ValueError):
                gpu.validate_transplant_quality(_dev(orig), _dev(new), packet, loc, r, sr)
    wide = orig.astype(np.complex128)
    for a, b in ((wide, new), (orig, wide), (_dev(wide), _dev(new)), (_dev(orig), _dev(wide)),
                 (orig.view(np.float32), new)):
        with pytest.raises(NotImplementedError, match="complex64 vectors only"):
            gpu.validate_transplant_quality(a, b, packet, 5003, refseg, sr)


@pytest.mark.parametrize("where", ["numpy", "cuda"])
def test_transplant_and_validate(gpu, GD, where):
    vector, packet, sr = GD["vector"], GD["packet"], float(GD["sample_rate"])
    if where == "cuda":
        vector, packet = _dev(vector), _dev(packet)
    new, location, validation = gpu.transplant_and_validate(vector, packet, 200, 712, sr)
    # the four calls one by one
    refseg = gpu.extract_reference_segment(packet, 200, 712)
    vloc, ploc, conf = gpu.find_packet_location_in_vector(vector, packet, refseg)
    new1 = gpu.transplant_packet_in_vector(vector, packet, vloc, ploc, normalize_power=True)
    val1 = gpu.validate_transplant_quality(vector, new1, packet, vloc, refseg, sr)
    assert location == dict(vector_location=vloc, packet_location=ploc, confidence=conf)
    assert validation == val1
    if where == "cuda":
        assert new.is_cuda and torch.equal(new, new1)
        new = new.cpu().numpy()
    else:
        assert isinstance(new, np.ndarray) and np.array_equal(new, new1)
    # the ok golden
    assert [int(vloc), int(ploc)] == GD["ok_location"].tolist()
    assert abs(float(conf) - float(GD["ok_location_confidence"])) <= 1e-5
    want_new = case_inputs(GD, "ok")[1]
    print("transplant max |new - golden|:", np.abs(new - want_new).max())
    assert np.allclose(new, want_new, rtol=1e-6, atol=0)
    assert_validation(validation, golden_dict(GD, "ok"), f"workflow/{where}")
