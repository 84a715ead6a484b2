"""Host side of the all-pairs burst similarity: the float64 reference against a
double loop, grouping, timing, carrier clustering and every argument error of
the front ends, with no device."""
import numpy as np
import pytest
import torch

import match_ref as mr
from vector_amd import _lib
from vector_amd import match as mt


def _rand(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def test_reference_against_the_double_loop():
    rng = np.random.default_rng(1)
    for la, lb in ((1, 1), (1, 5), (5, 1), (7, 4), (4, 7), (9, 9)):
        pa, pb = _rand(rng, la), _rand(rng, lb)
        peak, lag, _ = mr.pair(pa, pb)
        want, at = mr.brute(pa, pb)
        assert lag == at and abs(peak - want) <= 1e-12 * want
        assert -(lb - 1) <= lag <= la - 1


def test_reference_finds_a_shift_and_takes_the_first_maximum():
    rng = np.random.default_rng(2)
    base = _rand(rng, 40)
    # p_b is p_a cut 3 samples late: p_b's first sample lines up with p_a[3]
    assert mr.pair(base, base[3:])[1] == 3 and mr.pair(base[3:], base)[1] == -3
    # a tie between two lags goes to the smaller one
    assert mr.pair(np.ones(1), np.ones(4))[1] == -3
    assert mr.pair(np.ones(4), np.ones(1))[1] == 0


def test_reference_mirror_and_special_values():
    rng = np.random.default_rng(3)
    pk = [_rand(rng, n) for n in (5, 9, 1, 6)]
    pk.append(np.zeros(4, np.complex64))
    bad = _rand(rng, 7)
    bad[2] = np.nan
    pk.append(bad)
    r = mr.match(pk)
    assert np.array_equal(r.peak, r.peak.T, equal_nan=True) and np.array_equal(r.lag, -r.lag.T)
    assert np.all(np.diag(r.lag) == 0) and np.allclose(np.diag(r.peak)[:5], r.energy[:5])
    assert np.all(r.peak[4, :4] == 0) and np.all(r.rho[4, :5] == 0) and np.all(r.lag[4] == 0)
    assert np.isnan(r.peak[5]).all() and np.all(r.lag[5] == 0) and np.isnan(r.rho[5]).all()
    assert np.all((r.rho[:4, :4] >= 0) & (r.rho[:4, :4] <= 1 + 1e-12))
    assert np.allclose(mt.rho_from(r.peak, r.energy), r.rho, equal_nan=True)


def test_emitter_inputs_are_separable():
    """The GPU tests' inputs: every same-emitter pair is above the lag filter
    (rho >= 0.5, margin >= 1e-3) in the reference itself."""
    pk, who = mr.emitters(64)
    assert len(pk) == 15 and max(p.size for p in pk) == 64 and sorted(p.size for p in pk)[:2] == [1, 2]
    r = mr.match(pk)
    same = (who[:, None] == who[None, :]) & (who[:, None] >= 0) & ~np.eye(15, dtype=bool)
    assert np.count_nonzero(np.triu(same)) == 18
    assert np.all(r.rho[same] >= 0.5) and np.all(r.margin[same] >= 1e-3)
    other = (who[:, None] != who[None, :]) & (who[:, None] >= 0) & (who[None, :] >= 0)
    assert np.all(r.rho[other] < 0.7)


# ---------------------------------------------------------------------------
# group_packets
# ---------------------------------------------------------------------------
def test_groups_chain_nan_numbering_representative():
    rho = np.eye(6)

    def link(a, b, v=0.9):
        rho[a, b] = rho[b, a] = v
    link(1, 3)
    link(3, 5)                                      # 1-3-5 is a chain: 1 and 5 are not linked directly
    link(0, 4, 0.7)                                 # exactly the threshold links
    link(2, 0, np.nan)                              # NaN never links
    link(2, 4, 0.69)
    g = mt.group_packets(rho, 0.7)
    assert g.labels.tolist() == [0, 1, 2, 1, 0, 1]  # numbered by first member
    assert [m.tolist() for m in g.groups] == [[0, 4], [1, 3, 5], [2]]
    assert g.representative.tolist() == [0, 1, 2]   # no energy: the first member
    g = mt.group_packets(rho, 0.7, energy=[1.0, 2.0, 1.0, 5.0, 1.0, 5.0])
    assert g.representative.tolist() == [0, 3, 2]   # the largest energy, the first on ties
    g = mt.group_packets(rho, 0.7, energy=[np.nan, 1, 1, 1, 2, 1])
    assert g.representative.tolist() == [4, 1, 2]
    # a one-sided entry links too; a tensor is taken as well
    one = np.eye(2)
    one[0, 1] = 0.8
    assert mt.group_packets(torch.from_numpy(one)).labels.tolist() == [0, 0]
    assert mt.group_packets(np.eye(3), 2.0).labels.tolist() == [0, 1, 2]


def test_group_packets_errors():
    with pytest.raises(ValueError):
        mt.group_packets(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        mt.group_packets(np.eye(2), np.nan)
    with pytest.raises(ValueError):
        mt.group_packets(np.eye(2), energy=[1.0])


# ---------------------------------------------------------------------------
# group_timing
# ---------------------------------------------------------------------------
def test_timing_exact_period_missing_instance_and_count_one():
    K = 9
    starts = np.array([100, 1100, 2100, 3100, 50, 5100, 777, 4100, 0])
    lag = np.zeros((K, K), np.int64)
    groups = mt.PacketGroups(None, [np.array([0, 1, 2, 3, 7]), np.array([4, 5]), np.array([6])], np.array([0, 4, 6]))
    t = mt.group_timing(groups, starts, lag, 1e6)
    assert t.count.tolist() == [5, 2, 1]
    assert t.start[0] == 100 and t.period[0] == 1000 and t.jitter[0] == 0
    assert t.arrivals[0].tolist() == [100, 1100, 2100, 3100, 4100]
    assert t.period[1] == 5050 and t.start[1] == 50
    assert np.isnan(t.period[2]) and t.start[2] == 777 and t.jitter[2] == 0
    s = t.seconds
    assert s.period[0] == 1e-3 and s.start[0] == 1e-4 and s.count.tolist() == [5, 2, 1]
    # instance 2 of 6 missing: n = 0, 1, 3, 4, 5 and the same line
    st = 40 + 250 * np.array([0, 1, 3, 4, 5])
    t = mt.group_timing([np.arange(5)], st, np.zeros((5, 5), np.int64), 1.0)
    assert abs(t.period[0] - 250) < 1e-9 and abs(t.start[0] - 40) < 1e-9 and t.jitter[0] < 1e-9
    # jitter: one arrival 2 samples off the line
    st = np.array([0, 100, 202, 300, 400])
    t = mt.group_timing([np.arange(5)], st, np.zeros((5, 5), np.int64), 1.0)
    assert 1.0 < t.jitter[0] < 2.0 and abs(t.period[0] - 100) < 1.0


def test_timing_lag_sign_convention():
    """lag[k, rep] = l: the representative's first sample lines up with packet
    k's sample l, so a burst cut 3 samples early (its slice starts 3 before the
    content) has lag +3 and arrives where the others do."""
    rng = np.random.default_rng(5)
    base = _rand(rng, 50)
    capture = np.zeros(1000, np.complex64)
    for at in (100, 400, 700):
        capture[at:at + 50] = base
    cuts = np.array([100, 397, 702])                # exact, 3 early, 2 late
    pk = [capture[c:c + 50] for c in cuts]
    r = mr.match(pk)
    assert r.lag[:, 0].tolist() == [0, 3, -2]
    t = mt.group_timing(mt.PacketGroups(None, [np.arange(3)], np.array([0])), cuts, r.lag, 1.0)
    assert t.arrivals[0].tolist() == [100, 400, 700] and t.period[0] == 300 and t.jitter[0] == 0


def test_group_timing_errors():
    with pytest.raises(ValueError):
        mt.group_timing([np.arange(2)], [0, 1], np.zeros((2, 2), np.int64), 0.0)
    with pytest.raises(ValueError):
        mt.group_timing([np.arange(2)], [0, 1], np.zeros((3, 3), np.int64), 1.0)
    with pytest.raises(ValueError):
        mt.group_timing([np.array([0, 2])], [0, 1], np.zeros((2, 2), np.int64), 1.0)


# ---------------------------------------------------------------------------
# carriers
# ---------------------------------------------------------------------------
def test_carrier_clustering():
    c = np.array([8.02e6, -6.0e6, 7.99e6, 8.05e6, -5.96e6, np.nan, 1.0e6])
    bw = np.array([2e6, 2e6, 2e6, 2e6, 2e6, 1e6, 0.1e6])
    of, carriers = mt.cluster_carriers(c, bw)
    assert of.tolist() == [2, 0, 2, 2, 0, 3, 1]
    assert carriers[0] == np.median([-6.0e6, -5.96e6]) and carriers[1] == 1.0e6 and carriers[2] == 8.02e6
    assert np.isnan(carriers[3])
    # single linkage: a chain of small gaps is one carrier; an explicit tolerance splits it
    c = np.array([0.0, 0.9e6, 1.8e6, 2.7e6])
    assert mt.cluster_carriers(c, np.full(4, 2e6))[0].tolist() == [0, 0, 0, 0]
    assert mt.cluster_carriers(c, np.full(4, 2e6), freq_tol=0.5e6)[0].tolist() == [0, 1, 2, 3]
    # the smaller bandwidth of the two neighbours sets the gap
    assert mt.cluster_carriers(np.array([0.0, 0.4e6]), np.array([2e6, 0.5e6]))[0].tolist() == [0, 1]
    with pytest.raises(ValueError):
        mt.cluster_carriers([0.0], [1.0, 2.0])
    with pytest.raises(ValueError):
        mt.cluster_carriers([0.0], [1.0], freq_tol=-1)


def test_seconds_round_trip_through_vector_plan():
    from vector_amd.vectors import vector_plan
    for sr in (56e6, 1e6, 3.3e6):
        for n in (1, 999, 12345, 700001):
            cfg = {"length": 10, "start_time": mt._seconds_for(float(n), sr, False),
                   "period": mt._seconds_for(n + 1e-9, sr, True)}
            start, period, _ = vector_plan([cfg], 1.0, sr).places[0]
            assert (start, period) == (n, n)


# ---------------------------------------------------------------------------
# argument errors, no device
# ---------------------------------------------------------------------------
def test_packet_similarity_argument_errors():
    ok = np.ones(8, np.complex64)
    bad = [
        [],                                         # no packet
        np.ones((2, 8), np.complex64),              # an array, not a list
        [ok, np.ones((2, 4), np.complex64)],        # not 1-D
        [ok, np.ones(8, np.complex128)],            # dtype
        [ok, np.ones(8, np.float32)],
        [ok, np.zeros(0, np.complex64)],            # empty
        [ok, torch.ones(8, dtype=torch.complex64)],  # mixed host / tensor
        [torch.ones(8, dtype=torch.complex64)],     # a CPU tensor
        [ok] * 4097,                                # too many
    ]
    for p in bad:
        with pytest.raises(ValueError):
            mt.packet_similarity(p)
    with pytest.raises(ValueError, match="max_samples"):
        mt.packet_similarity([ok, np.ones(8193, np.complex64)])
    for ms in (0, -1, 8193):
        with pytest.raises(ValueError):
            mt.packet_similarity([ok], max_samples=ms)


def test_match_packets_argument_errors():
    x = np.ones(1000, np.complex64)
    pk = ([10], [500])
    with pytest.raises(NotImplementedError):
        mt.match_packets(x.astype(np.complex128), pk, 1e6)
    cases = [
        dict(packets=([10], [1000])), dict(packets=([], [])), dict(sample_rate=0.0), dict(sample_rate=np.inf),
        dict(center_freq=np.nan), dict(threshold=np.nan), dict(freq_tol=-1.0), dict(ntaps=254), dict(max_samples=0),
        dict(max_samples=8193), dict(pre_samples=-1), dict(post_samples=-1),
    ]
    for kw in cases:
        args = dict(packets=pk, sample_rate=1e6)
        args.update(kw)
        with pytest.raises(ValueError):
            mt.match_packets(x, args.pop("packets"), args.pop("sample_rate"), **args)
    with pytest.raises(NotImplementedError):
        mt.match_packets(x, pk, 1e6, ntaps=513)
    with pytest.raises(ValueError):
        mt.match_packets(np.ones((2, 4), np.complex64), pk, 1e6)
    from vector_amd.packets import PacketMeasurements
    m = PacketMeasurements(np.zeros(2), None, None, None, np.zeros(2), None, None, None)
    with pytest.raises(ValueError):
        mt.match_packets(x, pk, 1e6, measurements=m)


def test_symbols_and_exports():
    for name in ("vsig_match_create", "vsig_match_info", "vsig_match_run", "vsig_match_free"):
        assert name in _lib.SIGNATURES and not name.endswith("_dev")
    import vector_amd as va
    for name in ("packet_similarity", "group_packets", "group_timing", "match_packets", "Similarity", "PacketGroups",
                 "GroupTiming", "PacketMatches", "cluster_carriers"):
        assert hasattr(va, name)
    assert mt.match_size(512) == 1024 and mt.match_size(513) == 4096 and mt.match_size(2048) == 4096
    assert mt.match_size(2049) == 8192 and mt.match_size(4096) == 8192 and mt.match_size(4097) == 16384
    assert mt.match_size(8192) == 16384
