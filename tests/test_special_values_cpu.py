"""CPU half of the non-finite / extreme-value tests: it pins the oracle on the
inputs test_gpu_special_values.py uses and proves those inputs are not vacuous.

  * oracle/npdot.c np_cabs against np.abs on the full special-value grid and on
    wide-range data, bit for bit;
  * every poisoned case of section B changes numpy's / the oracle's answer, so
    a kernel that ignores the poison cannot pass the GPU comparison;
  * wide() really holds subnormal, overflowing and NaN magnitudes;
  * this host's float32 -> int16 cast is the x86 pattern np_f32_to_i16
    (stream_ops.hip) restates -- the GPU quantiser tests compare with the host
    cast, so on a host that casts otherwise they fail (here first)."""
import numpy as np
import pytest

import special_values as sv
from oracle import npdot, ref
from test_gpu_peaks import ref_peaks
from test_transplant_cpu import ref_validate


# ---------------------------------------------------------------- the oracle's |c|
def test_oracle_cabs_on_the_grid():
    g = sv.grid(np.complex128)
    assert len(g) == 169
    with np.errstate(all="ignore"):
        want = np.abs(g)
    ok = sv.same_bits(npdot.cabs(g), want)
    assert ok.all(), sv.first_diff(ok, g, npdot.cabs(g), want)
    # the two inputs the device version lost
    assert np.isnan(want[(g.real == 0) & np.isnan(g.imag)]).all()
    assert np.isnan(want[np.isnan(g.real) & (g.imag == 0)]).all()
    assert np.isinf(want[np.isinf(g.real) & np.isnan(g.imag)]).all()


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_cabs_on_wide_data(seed):
    z = sv.wide(65_536 + 3, np.complex128, seed)
    with np.errstate(all="ignore"):
        want = np.abs(z)
    ok = sv.same_bits(npdot.cabs(z), want)
    assert ok.all(), sv.first_diff(ok, z, npdot.cabs(z), want)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_wide_holds_every_class(dt):
    z = sv.wide(65_536 + 3, dt, 1)
    fi = np.finfo(sv.real_of(dt))
    with np.errstate(all="ignore"):
        a = np.abs(z)
    finite_in = np.isfinite(z.real) & np.isfinite(z.imag)
    assert np.count_nonzero((a > 0) & (a < fi.smallest_normal)) > 0          # subnormal results
    assert np.count_nonzero(np.isinf(a) & finite_in) > 0                      # overflow of finite parts
    assert np.count_nonzero(np.isnan(a)) > 0
    assert np.count_nonzero(np.isinf(a) & (np.isnan(z.real) | np.isnan(z.imag))) > 0   # inf beats NaN
    # the exponents really span the dtype
    e = np.log10(np.abs(z.real[finite_in & (z.real != 0)]).astype(np.float64))
    assert e.min() < np.log10(float(fi.smallest_normal)) and e.max() > np.log10(float(fi.max)) - 1


def test_grid_keeps_signed_zeros_and_nan():
    for dt in (np.complex64, np.complex128):
        g = sv.grid(dt)
        s = sv.specials(dt)
        assert len(s) == 13 and g.dtype == dt
        assert sv.same_bits(g.real, np.repeat(s, 13)).all() and sv.same_bits(g.imag, np.tile(s, 13)).all()
        assert np.signbit(g.real[13]) and g.real[13] == 0


def test_same_bits_and_poison():
    a = np.array([0.0, -0.0, np.nan, 1.0], np.float32)
    b = np.array([-0.0, -0.0, -np.nan, 1.0], np.float32)
    assert sv.same_bits(a, b).tolist() == [False, True, True, True]
    with pytest.raises(AssertionError):
        sv.same_bits(a, a.astype(np.float64))
    x = np.arange(4.0)
    y = sv.poison(x, 2, np.nan)
    assert x[2] == 2 and np.isnan(y[2]) and y[3] == 3


# ---------------------------------------------------------------- the host cast
def test_host_f32_to_i16_cast_is_the_x86_pattern():
    with np.errstate(invalid="ignore"):
        got = np.array([np.nan, np.inf, 1e10, 4e9, 70000.7, -70000.7], np.float32).astype(np.int16)
    assert got.tolist() == [0, 0, 0, 0, 4464, -4464]


# ---------------------------------------------------------------- section B is not vacuous
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_poison_changes_order_statistics_and_thresholds(dt):
    base = sv.base_signal(dt)
    n = len(base)
    clean_sorted = np.sort(np.abs(base))
    for name, at, v in sv.poison_cases(n):
        a = sv.poison(base, at, v)
        assert sv.differs(np.sort(np.abs(a))[[n // 2, n - 1]], clean_sorted[[n // 2, n - 1]]), name
        assert sv.differs(sv.np_threshold_stats(a, 1.0), sv.np_threshold_stats(base, 1.0)), name


@pytest.mark.parametrize("dt", sv.DTYPES)
def test_poison_changes_boxcar_detectors_and_peaks(dt):
    base = sv.base_signal(dt)
    n = len(base)
    cplx = np.dtype(dt).kind == "c"
    clean_sm = sv.np_boxcar(base, 56)
    clean_start = ref.find_packet_start(base)
    clean_bounds = ref.detect_packet_bounds(base, 56e6)
    a, b = n // 3, 5200                               # the burst of base_signal
    assert a - 200 < clean_start <= a + 5 and a - 60 < clean_bounds[0] <= a + 5 and b - 5 < clean_bounds[1] < b + 60
    for name, at, v in sv.poison_cases(n, energy=True, cplx=cplx):
        x = sv.poison(base, at, v)
        with np.errstate(all="ignore"):
            assert sv.differs(sv.np_boxcar(x, 56), clean_sm), name
            assert ref.find_packet_start(x) != clean_start, name
            assert sv.differs(ref.detect_packet_bounds(x, 56e6), clean_bounds), name
            if not name.startswith("1e20"):
                assert sv.differs(sv.np_peak(x)[:2], sv.np_peak(base)[:2]), name


def test_one_nan_sample_gives_the_documented_oracle_answers():
    x = sv.poison(sv.base_signal(np.complex64), 4096, np.nan)
    with np.errstate(all="ignore"):
        assert ref.find_packet_start(x) == 0
        assert tuple(ref.detect_packet_bounds(x, 56e6)) == (0, len(x))
        payload, rms, peak = ref.mat2wv_fields(x, True)
    assert not payload.any() and np.isnan(rms) and np.isnan(peak)


def test_poison_changes_spectrogram_levels():
    rng = np.random.default_rng(5)
    for S in (rng.exponential(size=(64, 33)).astype(np.float32), rng.exponential(size=(32, 17))):
        clean = ref.normalize_spectrogram(S)
        for at, v in (((3, 7), np.nan), ((3, 7), np.inf), (slice(None), np.nan)):
            P = sv.poison(S, at, v)
            with np.errstate(all="ignore"):
                got = ref.normalize_spectrogram(P)
            assert sv.differs(got[0], clean[0])
            if not (isinstance(v, float) and np.isinf(v)):
                assert np.isnan(got[1]) and np.isnan(got[2])
                assert type(got[1]) is type(clean[1])


def test_poison_changes_transplant_scores_and_built_vectors():
    rng = np.random.default_rng(9)
    orig = (rng.standard_normal(4099) + 1j * rng.standard_normal(4099)).astype(np.complex64)
    packet = (rng.standard_normal(700) + 1j * rng.standard_normal(700)).astype(np.complex64)
    new = orig.copy()
    new[1001:1701] = packet
    empty = np.zeros(0, np.complex64)
    clean = ref_validate(orig, new, packet, 1001, empty, 56e6)
    for v in (np.nan, np.inf):
        with np.errstate(all="ignore"):
            inside = ref_validate(orig, sv.poison(new, 1300, v), packet, 1001, empty, 56e6)
            outside = ref_validate(orig, sv.poison(new, 10, v), packet, 1001, packet[100:400], 56e6)
        assert sv.differs([inside["power_ratio"], inside["snr_improvement_db"]],
                          [clean["power_ratio"], clean["snr_improvement_db"]])
        want = ref_validate(orig, new, packet, 1001, packet[100:400], 56e6)
        assert not sv.differs([outside[k] for k in ("power_ratio", "snr_improvement_db", "reference_correlation")],
                              [want[k] for k in ("power_ratio", "snr_improvement_db", "reference_correlation")])
        pk = sv.poison(packet, 5, v)
        assert sv.differs(sv.np_normalized_vector(pk, 1000, 4099, 3), sv.np_normalized_vector(packet, 1000, 4099, 3))


def test_peaks_rule_is_the_oracle_on_nan_as_minus_one():
    m = np.abs(sv.base_signal(np.float64))
    clean = ref_peaks(m, 0.5, 300)
    assert len(clean[0]) > 1
    p = sv.poison(m, clean[0][0], np.nan)
    got = ref_peaks(sv.nan_to_minus_one(p), 0.5, 300)
    assert sv.differs(got[0], clean[0]) and clean[0][0] not in got[0]
    allnan = sv.nan_to_minus_one(np.full(100, np.nan))
    assert len(ref_peaks(allnan, 0.5, 3)[0]) == 0 and int(np.argmax(allnan)) == 0 and allnan.max() == -1
