"""CPU checks of the transplant workflow's outer steps and of the numpy
restatement the GPU test (test_gpu_transplant.py) compares against.

tests/golden/transplant_quality.npz holds what the reference itself returned
(make_golden_transplant.py).  ``ref_validate`` / ``ref_timing`` below restate
utils.py:1504-1591 and :827-846 on the oracle's correlation functions; they
must reproduce every golden -- ints and bools exactly, floats to 1e-12 -- so
that the GPU test may use them for inputs that have no golden."""
import numpy as np
import pytest

from conftest import golden
from oracle import ref

CASES = ["ok", "clipped", "identical", "zero_orig", "no_ref", "flat", "mid"]
EXACT = ["transplant_length_samples", "vector_location", "success"]
FLOATS = ["reference_correlation", "reference_confidence", "power_ratio", "snr_improvement_db",
          "transplant_length_us", "time_precision_us"]
CRITERIA = ["confidence_ok", "power_ok", "snr_ok", "confidence_threshold", "power_ratio_threshold",
            "min_snr_threshold"]


def ref_validate(original_vector, transplanted_vector, packet_signal, vector_location,
                 reference_segment, sample_rate):
    """utils.py:1504-1591 in numpy."""
    transplant_end = min(vector_location + len(packet_signal), len(transplanted_vector))
    transplant_length = transplant_end - vector_location
    transplanted_region = transplanted_vector[vector_location:transplant_end]
    original_region = original_vector[vector_location:transplant_end]
    if len(reference_segment) > 0:
        c, lags = ref.cross_correlate_signals(reference_segment, transplanted_region)
        _, ref_peak_val, ref_confidence = ref.find_correlation_peak(c, lags)
    else:
        ref_confidence = 0.0
        ref_peak_val = 0.0
    original_power = np.mean(np.abs(original_region) ** 2)
    transplanted_power = np.mean(np.abs(transplanted_region) ** 2)
    power_ratio = transplanted_power / original_power if original_power > 0 else 0.0
    noise_power = np.mean(np.abs(original_region - transplanted_region) ** 2)
    signal_power = np.mean(np.abs(transplanted_region) ** 2)
    snr_improvement = 10 * np.log10(signal_power / noise_power) if noise_power > 0 else np.inf
    confidence_ok = ref_confidence > 0.3
    power_ok = power_ratio > 0.01
    snr_ok = snr_improvement > -30
    return {
        "reference_correlation": ref_peak_val,
        "reference_confidence": ref_confidence,
        "power_ratio": power_ratio,
        "snr_improvement_db": snr_improvement,
        "transplant_length_samples": transplant_length,
        "transplant_length_us": transplant_length * 1e6 / sample_rate,
        "time_precision_us": 1e6 / sample_rate,
        "vector_location": vector_location,
        "success": confidence_ok and power_ok and snr_ok,
        "criteria": {
            "confidence_ok": confidence_ok,
            "power_ok": power_ok,
            "snr_ok": snr_ok,
            "confidence_threshold": 0.3,
            "power_ratio_threshold": 0.01,
            "min_snr_threshold": -30,
        },
    }


def ref_timing(signal, template=None):
    """utils.py:827-846 in numpy."""
    packet_start = ref.find_packet_start(signal, template)
    post = len(signal) - packet_start - len(template) if template is not None else 0
    return packet_start, post, packet_start


def case_inputs(g, case):
    """(original, transplanted, packet, location, reference segment, sample
    rate) of a golden case, rebuilt from the shared arrays and the case's patch."""
    vector, packet = g["vector"], g["packet"]
    original, transplanted = vector, vector
    if case == "no_ref":
        transplanted = case_inputs(g, "ok")[1]
    elif f"{case}_patch" in g.files:
        at, p = int(g[f"{case}_patch_at"]), g[f"{case}_patch"]
        transplanted = vector.copy()
        transplanted[at:at + len(p)] = p
    if case == "zero_orig":
        original = vector.copy()
        original[5003:5003 + len(packet)] = 0
    return (original, transplanted, packet, int(g[f"{case}_vector_location"]), g[f"{case}_ref"],
            float(g["sample_rate"]))


def golden_dict(g, case):
    d = {k: g[f"{case}_{k}"][()] for k in EXACT + FLOATS}
    d["criteria"] = {k: g[f"{case}_criteria_{k}"][()] for k in CRITERIA}
    return d


@pytest.fixture(scope="module")
def G():
    return golden("transplant_quality.npz")


def test_extract_reference_segment_golden(G):
    import vector_amd as va
    packet = G["packet"]
    for j, (lo, hi) in enumerate(G["segment_args"].tolist()):
        got = va.extract_reference_segment(packet, lo, hi)
        assert np.array_equal(got, G[f"segment_{j}"])
        assert got.dtype == packet.dtype and np.shares_memory(got, packet)      # a view


def test_extract_reference_segment_errors(G):
    import vector_amd as va
    packet = G["packet"]
    for lo, hi in [(10, 10), (20, 10), (len(packet), len(packet) + 5), (-9, 0)]:
        with pytest.raises(ValueError, match="Invalid sample range: start_sample >= end_sample"):
            va.extract_reference_segment(packet, lo, hi)


def test_golden_fixture_is_decisive(G):
    """No comparison tolerance can flip a criterion of a stored case."""
    assert G["cases"].tolist() == CASES
    for case in CASES:
        assert abs(float(G[f"{case}_reference_confidence"]) - 0.3) > 0.05
        p = float(G[f"{case}_power_ratio"])
        assert p > 0.1 or p < 0.001
        s = float(G[f"{case}_snr_improvement_db"])
        assert not np.isfinite(s) or abs(s + 30) > 1


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden(G, case):
    want = golden_dict(G, case)
    with np.errstate(divide="ignore"):
        got = ref_validate(*case_inputs(G, case))
    assert set(got) == set(want) and set(got["criteria"]) == set(CRITERIA)
    for k in EXACT:
        assert got[k] == want[k], k
    for k in CRITERIA:
        assert got["criteria"][k] == want["criteria"][k], k
    for k in FLOATS:
        w = float(want[k])
        if np.isfinite(w) and w != 0.0:
            assert abs(float(got[k]) - w) <= 1e-12 * max(1.0, abs(w)), k
        else:
            assert float(got[k]) == w, k
    for k in ("power_ratio", "snr_improvement_db"):        # the reference's float32 results
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, k


def test_restatement_timing_reproduces_golden(G):
    vector, packet = G["vector"], G["packet"]
    assert list(ref_timing(vector, packet[:256])) == G["timing_tmpl"].tolist()
    assert list(ref_timing(vector)) == G["timing_energy"].tolist()


def test_validate_needs_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    import vector_amd as va
    with pytest.raises(va.VsigUnavailable):
        va.validate_transplant_quality(*case_inputs(G, "ok"))
