"""CPU-only checks of the vector assembly's host side against
tests/golden/vector_build.npz (made by the reference's own loader and mixer,
tests/golden/make_golden_vector_build.py): vector_plan reproduces the
placement arithmetic of generate_vector (unified_gui.py:1711, 1748-1769)
exactly, rejects what the GUI rejects, and compute_freq_ranges matches
utils.py:129-159."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden


def _configs(g, how):
    """The golden's six packets as build_vector / vector_plan configs."""
    cfgs = []
    for i in range(len(g["files"])):
        cfg = dict(freq_shift=float(g["freq_shift"][i]), period=float(g["period"][i]),
                   start_time=float(g["start_time"][i]), name=str(g["files"][i])[:-4])
        if how == "length":
            cfg.update(length=len(g[f"packet{i}"]), pre_samples=int(g["pre_samples"][i]))
        else:
            cfg.update(signal=g[f"packet{i}"], pre_samples=int(g["pre_samples"][i]))
        cfgs.append(cfg)
    return cfgs


@pytest.mark.parametrize("how", ["length", "signal"])
@pytest.mark.parametrize("scenario", ["a", "b"])
def test_vector_plan_matches_reference(scenario, how):
    from vector_amd import vector_plan
    g = golden("vector_build.npz")
    sr = float(g["sample_rate"])
    plan = vector_plan(_configs(g, how), float(g[f"{scenario}_vector_length"]), sr)
    places, total, markers = plan                        # unpacks like a tuple
    assert total == plan.total_samples == int(g[f"{scenario}_total_samples"])
    assert [p[0] for p in places] == g[f"{scenario}_starts"].tolist()
    assert [p[1] for p in places] == g[f"{scenario}_periods"].tolist()
    assert [p[2] for p in places] == g[f"{scenario}_counts"].tolist()
    assert [m[0] for m in markers] == g[f"{scenario}_marker_times"].tolist()   # exact, in order
    # the cases the fixture is there for
    pre, starts, counts = g["pre_samples"], g[f"{scenario}_starts"], g[f"{scenario}_counts"]
    clamped = [i for i in range(len(pre)) if round(float(g["start_time"][i]) * sr) < pre[i]]
    assert clamped and all(starts[i] == 0 for i in clamped)
    lens = np.array([len(g[f"packet{i}"]) for i in range(len(pre))])
    if scenario == "b":
        assert (lens > total).any() and (counts[lens > total] == 0).all()
    else:       # a next instance would start inside the vector but end past it: left out
        nxt = starts + counts * g["a_periods"]
        assert ((nxt < total) & (nxt + lens > total)).any()
    # markers carry the config's shift and name; one style per name
    shifts = [m[1] for m in markers]
    assert shifts == np.repeat(g["freq_shift"], counts).tolist()
    styles = {}
    for m in markers:
        assert styles.setdefault(m[2], m[3:]) == m[3:]


def test_vector_plan_reads_packet_files_on_the_host():
    from vector_amd import vector_plan
    cfg = dict(file=os.path.join(GOLDEN, "mat", "packet_1_5MHz.mat"), freq_shift=0, period=2e-3,
               start_time=1e-3)
    plan = vector_plan([cfg], 5e-3, 56e6)               # 56100 samples, pre_samples 100
    assert plan.places == [(56000 - 100, 112000, 2)]
    assert [m[0] for m in plan.markers] == [56000 / 56e6, 168000 / 56e6]
    assert plan.markers[0][2] == "packet_1_5MHz"


def test_vector_plan_rejects_what_the_gui_rejects():
    from vector_amd import vector_plan
    ok = dict(length=100, freq_shift=0, period=1e-3, start_time=0)
    with pytest.raises(ValueError):
        vector_plan([], 1e-3, 56e6)
    with pytest.raises(ValueError):
        vector_plan([ok], 0, 56e6)
    with pytest.raises(ValueError):
        vector_plan([ok], -1e-3, 56e6)
    with pytest.raises(ValueError):
        vector_plan([dict(ok, period=1e-9)], 1e-3, 56e6)     # int(period * sr) == 0
    with pytest.raises(ValueError):
        vector_plan([dict(ok, period=-1e-3)], 1e-3, 56e6)


def test_compute_freq_ranges_matches_reference():
    from vector_amd import compute_freq_ranges
    g = golden("vector_build.npz")
    cases = json.loads(str(g["fr_cases"]))
    assert len(cases) >= 6
    for j, (shifts, margin) in enumerate(cases):
        want = g[f"fr{j}"]
        got = compute_freq_ranges(shifts, margin)
        if want.shape[0] == 0:
            assert got is None, (shifts, got)
        else:
            assert got == [tuple(want[0])], (shifts, got)
    assert compute_freq_ranges([2e6, -1e6]) == [(-2e6, 3e6)]      # default margin 1e6


def test_header_declares_the_vector_build_calls():
    from vector_amd import _lib
    assert {"vsig_vector_build_dev", "vsig_normalize_c64_dev"} <= set(_lib.SIGNATURES)
    lib = _lib.load_library()
    assert lib.vsig_vector_build_dev.argtypes[1]._type_ is _lib.PacketPlace
    import ctypes as C
    assert C.sizeof(_lib.PacketPlace) == 40
