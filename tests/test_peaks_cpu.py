"""CPU-only checks of the peak-list feature's host side: the timing score
(validate_packet_timing) branch by branch on hand-made markers, the new C-ABI
names and struct sizes, and the argument errors find_packet_instances raises
before it touches the library."""
import ctypes as C

import numpy as np
import pytest

from vector_amd import _lib, find_packet_instances, validate_packet_timing


def markers(name, start, period, count, shift=0):
    return [(start + k * period, shift, name, "x", "C0") for k in range(count)]


def score(text):
    assert text.startswith("Timing Validation: ")
    return float(text.split()[2].rstrip("%")), text.split("% ", 1)[1]


def cfg(name="p", period=0.010, start=0.001, **kw):
    return dict(name=name, period=period, start_time=start, **kw)


def test_no_packets():
    assert validate_packet_timing([], []) == ("No packets to validate", [])
    # markers of a name no config carries
    assert validate_packet_timing(markers("other", 0.0, 0.01, 3), [cfg()]) == ("No packets to validate", [])


def test_prints_nothing(capsys):
    validate_packet_timing(markers("p", 0.001, 0.010, 4), [cfg()])
    assert capsys.readouterr().out == ""


def test_exact_plan_is_perfect_and_details_layout():
    text, det = validate_packet_timing(markers("p", 0.001, 0.010, 2, shift=2e6), [cfg(freq_shift=2e6)])
    assert text == "Timing Validation: 100.0% ✅ PERFECT"
    assert len(det) == 1
    d = det[0]
    assert set(d) == {"packet_name", "instances", "start_time_error_ms", "period_error_percent",
                      "freq_shift_mhz", "explanations"}
    assert d["packet_name"] == "p" and d["instances"] == 2 and d["freq_shift_mhz"] == 2.0
    assert d["start_time_error_ms"] == pytest.approx(0.0, abs=1e-12)
    assert d["period_error_percent"] == pytest.approx(0.0, abs=1e-9)
    assert set(d["explanations"]) == {"start", "period", "freq", "consistency"}


def test_name_comes_from_file_then_name_then_index():
    m = markers("packet_2", 0.0, 0.01, 2) + markers("cap", 0.0, 0.01, 2)
    cfgs = [dict(file="/x/y/cap.mat", period=0.01, start_time=0.0),
            dict(period=0.01, start_time=0.0)]
    _, det = validate_packet_timing(m, cfgs)
    assert [d["packet_name"] for d in det] == ["cap", "packet_2"]


def test_markers_are_sorted_by_time():
    m = markers("p", 0.001, 0.010, 4)
    a = validate_packet_timing(m, [cfg()])
    b = validate_packet_timing(m[::-1], [cfg()])
    assert a == b


@pytest.mark.parametrize("count, err_ms, want_start", [
    (2, 8.0, 100.0),                      # inside the 10 ms tolerance of <= 2 instances
    (2, 14.0, 100 - 14.0 / 10.0 * 50),    # outside it: 30
    (3, 4.0, 100.0),                      # inside the 5 ms tolerance of 3+ instances
    (3, 8.0, 100 - 8.0 / 5.0 * 50),       # outside: 20 (inside for 2 instances)
    (4, 12.0, 0.0),                       # clamped at 0
])
def test_start_tolerance(count, err_ms, want_start):
    text, det = validate_packet_timing(markers("p", 0.001 + err_ms / 1000, 0.010, count), [cfg()])
    want = 0.4 * 100 + 0.3 * want_start + 0.2 * 100 + 0.1 * 100
    if count > 2:
        want = min(100.0, want + min(5.0, count - 2))
    assert score(text)[0] == pytest.approx(want, abs=0.051)
    assert det[0]["start_time_error_ms"] == pytest.approx(err_ms, rel=1e-9)


@pytest.mark.parametrize("err_pct, want_period", [
    (0.5, 100.0),
    (3.0, 100 - (3.0 - 1.0) * 5),         # 90
    (10.0, 80 - (10.0 - 5.0) * 2),        # 70
    (60.0, 0.0),                          # clamped at 0
])
def test_period_error(err_pct, want_period):
    period = 0.010 * (1 + err_pct / 100)
    text, det = validate_packet_timing(markers("p", 0.001, period, 2), [cfg()])
    want = 0.4 * want_period + 0.3 * 100 + 0.2 * 100 + 0.1 * 100
    assert score(text)[0] == pytest.approx(want, abs=0.051)
    assert det[0]["period_error_percent"] == pytest.approx(err_pct, rel=1e-6)


def test_single_instance():
    text, det = validate_packet_timing(markers("p", 0.001, 0.010, 1), [cfg()])
    # period 100 (nothing to check), consistency 80: 40 + 30 + 20 + 8
    assert score(text) == (98.0, "⚠️ GOOD")
    assert det[0]["instances"] == 1 and det[0]["period_error_percent"] == 0


@pytest.mark.parametrize("count, bonus", [(2, 0.0), (3, 1.0), (5, 3.0), (7, 5.0), (12, 5.0)])
def test_bonus_and_its_cap(count, bonus):
    # a 10 % period error costs 0.4 * 30 = 12 points: base 88
    text, _ = validate_packet_timing(markers("p", 0.001, 0.011, count), [cfg()])
    assert score(text)[0] == pytest.approx(88.0 + bonus, abs=0.051)


def test_bonus_is_capped_at_100():
    text, _ = validate_packet_timing(markers("p", 0.001, 0.010, 9), [cfg()])
    assert text == "Timing Validation: 100.0% ✅ PERFECT"


@pytest.mark.parametrize("period_err, status", [
    (0.0, "✅ PERFECT"),        # 100
    (1.4, "✅ EXCELLENT"),      # 100 - 0.4 * 2 = 99.2
    (3.0, "⚠️ GOOD"),           # 96
    (5.0, "⚠️ FAIR"),           # 92
    (10.0, "❌ POOR"),          # 88
])
def test_status_words(period_err, status):
    text, _ = validate_packet_timing(markers("p", 0.001, 0.010 * (1 + period_err / 100), 2), [cfg()])
    assert score(text)[1] == status


def test_overall_is_the_mean_over_packets():
    m = markers("a", 0.001, 0.010, 2) + markers("b", 0.001, 0.011, 2)
    text, det = validate_packet_timing(m, [cfg("a"), cfg("b")])
    assert score(text)[0] == pytest.approx((100.0 + 88.0) / 2, abs=0.051)
    assert [d["packet_name"] for d in det] == ["a", "b"]


def test_abi_names_and_struct_sizes():
    for name in ("vsig_peaks_tile", "vsig_peaks_dev", "vsig_peaks"):
        assert name in _lib.SIGNATURES
    assert C.sizeof(_lib.Instance) == 16
    assert C.sizeof(_lib.PeaksInfo) == 32
    lib = _lib.load_library()
    tile = lib.vsig_peaks_tile()
    assert tile >= 256 and tile & (tile - 1) == 0
    # arguments are refused before a context is needed: a null context is VSIG_E_INVALID
    info = _lib.PeaksInfo(count=-7)
    a = np.ones(4, np.float32)
    rc = lib.vsig_peaks(None, _lib.DTYPES["f32"], a.ctypes.data_as(C.c_void_p), 4, 0.5, 0, 0, None, 0,
                        C.byref(info))
    assert rc == -1 and info.count == -7


def test_find_packet_instances_argument_errors():
    x = np.ones(16, np.complex64)
    with pytest.raises(ValueError, match="shorter than the packet"):
        find_packet_instances(x[:4], x)
    with pytest.raises(ValueError, match="a cannot be empty"):
        find_packet_instances(x[:0], x)
    with pytest.raises(ValueError, match="v cannot be empty"):
        find_packet_instances(x, x[:0])
    with pytest.raises(ValueError, match="min_distance"):
        find_packet_instances(x, x[:4], min_distance=-1)
    with pytest.raises(ValueError, match="NaN"):
        find_packet_instances(x, x[:4], threshold_ratio=float("nan"))
    with pytest.raises(ValueError, match="max_peaks"):
        find_packet_instances(x, x[:4], max_instances=-1)
