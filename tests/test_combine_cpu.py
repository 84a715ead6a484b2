"""CPU-only checks of combine_packets: the float64 reference (combine_ref.py)
against a plain double loop, the planted scene on the reference alone, and the
host side of the front ends (every argument error with no device, the ABI
names)."""
import cmath
import math

import numpy as np
import pytest

import combine_ref as cr


# ---------------------------------------------------------------------------
# the reference against a plain double loop
# ---------------------------------------------------------------------------
def loop_estimate(p, v, d, f0):
    """(a, freq, rho, Ep, Ev, res, n) by scalar loops; None without overlap."""
    Lg, Lk = len(v), len(p)
    lo, hi = max(0, -d), min(Lg, Lk - d)
    n = hi - lo
    if n <= 0:
        return None
    h, m = n // 2, lo + (n - 1) / 2
    A, Ep, Ev = [0j, 0j], [0.0, 0.0], [0.0, 0.0]
    for j in range(lo, hi):
        half = 0 if j - lo < h else 1
        x, r = complex(p[j + d]), complex(v[j])
        A[half] += x * cmath.exp(-2j * math.pi * f0 * (j - m)) * r.conjugate()
        Ep[half] += abs(x) ** 2
        Ev[half] += abs(r) ** 2
    phi = cmath.phase(A[1] * A[0].conjugate()) if A[0] != 0 and A[1] != 0 else 0.0
    B = A[0] * cmath.exp(0.5j * phi) + A[1] * cmath.exp(-0.5j * phi)
    res = sum(Ep) - sum(abs(A[i]) ** 2 / Ev[i] for i in range(2) if Ev[i] > 0)
    return B / sum(Ev), f0 + phi / (math.pi * n), abs(B) / math.sqrt(sum(Ep) * sum(Ev)), sum(Ep), sum(Ev), res, n


def loop_sum(packets, members, lag, Lg, rec):
    y = np.zeros(Lg, np.complex128)
    for j in range(Lg):
        num, den = 0j, 0.0
        for k in members:
            i = j + int(lag[k])
            if rec.used[k] and 0 <= i < len(packets[k]):
                num += (rec.a[k].conjugate() * cmath.exp(-2j * math.pi * rec.freq[k] * (j - rec.m[k]))
                        * complex(packets[k][i]))
                den += abs(rec.a[k]) ** 2
        y[j] = num / den if den > 0 else 0
    return y


def tiny_list():
    """Group 0: a representative of 9 samples with members of overlap 0, 1, 2,
    3 (odd), 8, lags of both signs, one longer and one shorter than it; group
    1: a representative alone; one packet in no group."""
    rng = np.random.default_rng(5)

    def noise(n):
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    rep = noise(9)
    packets = [rep,
               noise(4),                          # d = 9: starts past the frame, n = 0
               noise(5),                          # d = -8: its sample 0 under j = 8, n = 1
               noise(6),                          # d = 4: n = 2
               (rep[2:5] * (0.5 - 0.2j)).astype(np.complex64),          # shorter, d = -2: n = 3
               np.concatenate([noise(3), 2 * rep, noise(2)]).astype(np.complex64),   # longer, d = 3: n = 9
               (rep[1:] * np.exp(2j * np.pi * 0.01 * np.arange(8))).astype(np.complex64),   # d = -1: n = 8
               noise(7),                          # group 1 alone
               noise(5)]                          # in no group
    group = np.array([0, 0, 0, 0, 0, 0, 0, 1, -1], np.int32)
    lag = np.array([0, 9, -8, 4, -2, 3, -1, 0, 2], np.int64)
    return packets, group, lag, np.array([0, 7], np.int32)


def test_reference_against_a_plain_double_loop():
    packets, group, lag, rep = tiny_list()
    K = len(packets)
    f0 = np.array([0.0, 0.02, -0.03, 0.011, 0.0, -0.004, 0.007, 0.0, 0.01])
    assert [cr.overlap(9, p.size, d)[1] for p, d in zip(packets[:7], lag[:7])] == [9, 0, 1, 2, 3, 9, 8]
    for ref_is_rep in (True, False):
        ref = None if ref_is_rep else [np.conj(packets[0][::-1]).copy(), packets[7] * 2]
        pri = None if ref_is_rep else f0
        rec = cr.estimate(packets, group, lag, rep, ref, pri, 0.0)
        for k in range(K):
            fk = 0.0 if pri is None else pri[k]
            if group[k] < 0:
                assert not rec.used[k] and rec.n[k] == 0 and rec.a[k] == 0 and rec.freq[k] == fk
                continue
            v = packets[rep[group[k]]] if ref is None else ref[group[k]]
            want = loop_estimate(packets[k], v, int(lag[k]), fk)
            if want is None:
                assert not rec.used[k] and rec.n[k] == 0 and rec.a[k] == 0 and rec.freq[k] == fk and rec.rho[k] == 0
                continue
            if ref is None and k == rep[group[k]]:
                assert (rec.a[k], rec.freq[k], rec.rho[k], rec.res[k], rec.used[k]) == (1, 0, 1, 0, True)
                assert rec.n[k] == packets[k].size and rec.Ep[k] == rec.Ev[k] == pytest.approx(want[3], rel=1e-14)
                continue
            got = (rec.a[k], rec.freq[k], rec.rho[k], rec.Ep[k], rec.Ev[k], rec.res[k])
            for g_, w_ in zip(got, want[:6]):
                assert abs(g_ - w_) <= 1e-12 * max(1.0, abs(w_)), (k, got, want)
            assert rec.n[k] == want[6] and rec.used[k]
        assert rec.m[4] == 2 + (3 - 1) / 2 and rec.m[2] == 8.0
        for g, Lg in enumerate((9, 7)):
            y = cr.combine_sum(packets, group, lag, rep, rec)[g]
            np.testing.assert_allclose(y, loop_sum(packets, np.flatnonzero(group == g), lag, Lg, rec), rtol=0, atol=1e-12)
    # min_rho drops the uncorrelated members and they are skipped, not added as zero
    first = cr.estimate(packets, group, lag, rep, None, None, 0.9)
    assert first.used.tolist() == [True, False, True, True, True, True, True, True, False]
    assert np.all(first.a[~first.used] == 0) and np.all(first.rho[~first.used] == 0)
    # a group of one member returns its packet, first pass and refined
    for refine in (False, True):
        out = cr.combine(packets, group, lag, rep, refine=refine)
        assert np.array_equal(out.y[1], packets[7].astype(np.complex128)) and out.gain[1] == 1
    # a NaN member is not used; neither is an all-zero one
    bad = [p.copy() for p in packets]
    bad[5][6] = np.nan
    bad[6][:] = 0
    rec = cr.estimate(bad, group, lag, rep)
    assert not rec.used[5] and np.isnan(rec.rho[5]) and not rec.used[6] and rec.rho[6] == 0
    keep = [0, 1, 2, 3, 4, 7, 8]
    sub = cr.combine([packets[k] for k in keep], group[keep], lag[keep], np.array([0, 5], np.int32))
    full = cr.combine(bad, group, lag, rep)
    assert np.array_equal(full.y[0], sub.y[0])
    snr = full.snr
    assert np.isnan(snr[8]) and np.isnan(snr[1]) and np.isnan(snr[5]) and np.all(snr[[0, 2, 3, 4]] >= 0)


# ---------------------------------------------------------------------------
# the planted scene
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [False, True])
def test_planted_scene_on_the_reference(refine):
    """One emitter, 8 instances, noise 0.3 (combine_ref.planted_scene), seeds
    101 - 103.  Measured here on the float64 reference:
      measured error-power gain / gain_g   1.063, 1.094, 1.029 (refined: 1.063,
                                           1.096, 1.029); bar [0.9, 1.2]
      max |freq_k - planted| L             6.6e-3, 8.6e-3, 3.8e-3; bar 2e-2
      worst factor between the corrected snr_k and the planted amp^2 / sigma^2
                                           1.028, 1.034, 1.041
    so SNR_FACTOR_MEASURED = 1.041 and the bar is 1.25 times that (1.30), the
    estimate being itself noisy at sigma = 0.3."""
    worst = 0.0
    for seed in cr.SCENE_SEEDS:
        sc = cr.planted_scene(seed)
        out = cr.combine(sc.packets, sc.group, sc.lag, sc.rep, refine=refine)
        ratio, ferr, factor = cr.scene_figures(sc, out.y[0], out.gain[0], out.first.freq, out.snr)
        print(f"seed {seed} refine {refine}: gain_g {out.gain[0]:.3f}, measured / gain_g {ratio:.3f}, "
              f"max |freq - planted| L {ferr:.2e}, snr factor {factor:.3f}")
        assert out.first.used.all() and out.second.used.all()
        assert 0.9 <= ratio <= 1.2
        assert ferr <= 2e-2
        assert factor <= cr.SNR_FACTOR_BAR
        worst = max(worst, factor)
    print(f"worst snr factor {worst:.3f} (recorded {cr.SNR_FACTOR_MEASURED})")


# ---------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------
def test_abi_names():
    from vector_amd import _lib
    names = [n for n in _lib.SIGNATURES if n.startswith("vsig_combine_")]
    assert sorted(names) == ["vsig_combine_create", "vsig_combine_estimate", "vsig_combine_free", "vsig_combine_info",
                             "vsig_combine_offsets", "vsig_combine_sum"]
    assert not any(n.endswith("_dev") for n in names)
    lib = _lib.load_library()
    assert all(hasattr(lib, n) for n in names)
    import ctypes as C
    assert C.sizeof(_lib.CombineMember) == _lib.COMBINE_MEMBER.itemsize == 80
    for name, _ in _lib.CombineMember._fields_:
        assert getattr(_lib.CombineMember, name).offset == _lib.COMBINE_MEMBER.fields[name][1]


def test_argument_errors_need_no_device():
    import torch
    import vector_amd as va
    from vector_amd import match as mt
    rng = np.random.default_rng(0)
    pk = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) for n in (20, 18, 22, 9)]
    lag = np.zeros((4, 4), np.int64)
    groups = [np.array([0, 1]), np.array([2])]
    bad = [
        (dict(packets=np.concatenate(pk)), "list"),
        (dict(packets=[]), "1 to 4096"),
        (dict(packets=[pk[0], pk[1].astype(np.complex128), pk[2], pk[3]]), "complex64"),
        (dict(packets=[pk[0], pk[1].reshape(2, 9), pk[2], pk[3]]), "1-D"),
        (dict(packets=[pk[0], pk[1][:0], pk[2], pk[3]]), "empty"),
        (dict(packets=[pk[0], torch.zeros(4, dtype=torch.complex64), pk[2], pk[3]]), "all numpy arrays or all CUDA"),
        (dict(groups=[]), "at least one group"),
        (dict(groups=np.array([[0, 1]])), "list of member index arrays"),
        (dict(groups=[np.array([0, 1]), np.array([], np.int64)]), "empty"),
        (dict(groups=[np.array([0, 4])]), "outside"),
        (dict(groups=[np.array([0, -1])]), "outside"),
        (dict(groups=[np.array([0, 1]), np.array([1, 2])]), "twice"),
        (dict(groups=[np.array([0, 0])]), "twice"),
        (dict(groups=mt.PacketGroups(np.array([0, 0, 1, 1]), [np.array([0, 1]), np.array([2, 3])], np.array([0, 1]))),
         "not one of its members"),
        (dict(lag=np.zeros((4, 3), np.int64)), "K x K"),
        (dict(lag=np.zeros(4, np.int64)), "K x K"),
        (dict(lag=np.eye(4, dtype=np.int64)), "lag to itself"),
        (dict(min_rho=float("nan")), "min_rho"),
        (dict(min_rho=1.5), "min_rho"),
    ]
    for kw, text in bad:
        args = dict(packets=pk, groups=groups, lag=lag)
        opts = {k: kw.pop(k) for k in list(kw) if k == "min_rho"}
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            va.combine_packets(args["packets"], args["groups"], args["lag"], **opts)
    assert len(mt._check_packets([np.ones(20000, np.complex64)], None, cap=None, who="combine_packets")[0]) == 1
    with pytest.raises(ValueError, match="packet_similarity compares at most"):
        mt._check_packets([np.ones(20000, np.complex64)], None)
    x = np.ones(4096, np.complex64)
    seg = (np.array([10]), np.array([500]))
    with pytest.raises(ValueError, match="min_rho"):
        va.match_packets(x, seg, 1e6, combine=True, min_rho=float("nan"))
    with pytest.raises(ValueError, match="min_rho"):
        va.match_packets(x, seg, 1e6, min_rho=2.0)
    with pytest.raises(ValueError, match="combine must be"):
        va.match_packets(x, seg, 1e6, combine="yes")
    m = mt.PacketMatches(*range(8))
    assert m.combined is None and len(m) == 8 and m._fields[-1] == "configs"
    m.combined = 1
    assert mt.PacketMatches(*range(8)).combined is None
    if not torch.cuda.is_available():
        with pytest.raises(va.VsigUnavailable):
            va.combine_packets(pk, groups, lag)
        with pytest.raises(va.VsigUnavailable):
            va.match_packets(x, seg, 1e6, combine=True)
