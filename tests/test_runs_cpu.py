"""CPU-only checks of the run-list feature's host side: the reference against
the per-index rule, the new C-ABI names and struct sizes, the arguments the
library refuses before it needs a context, and the argument errors find_runs /
detect_packets / extract_packets raise before they touch the library."""
import ctypes as C

import numpy as np
import pytest

from runs_ref import runs_by_rule, runs_ref
from vector_amd import _lib, detect_packets, extract_packets, find_runs


def test_reference_matches_the_per_index_rule():
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(1, 60))
        mask = rng.random(n) < rng.choice([0.05, 0.3, 0.6, 0.95])
        gap = int(rng.choice([0, 1, 2, 5, n, 10 ** 6]))
        s, e = runs_ref(mask.astype(np.float64), 0.5, gap)
        rs, re = runs_by_rule(mask, gap)
        assert np.array_equal(s, rs) and np.array_equal(e, re)
        assert len(s) == len(e) and (s <= e).all()
        if mask.any():
            idx = np.flatnonzero(mask)
            assert s[0] == idx[0] and e[-1] == idx[-1]      # whatever the gap
            if gap >= n:
                assert len(s) == 1
        else:
            assert len(s) == 0


def test_reference_consequences():
    m = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1], np.float64)
    assert [list(x) for x in runs_ref(m, 1.0, 0)] == [[1, 4, 7, 11], [2, 4, 7, 11]]
    assert [list(x) for x in runs_ref(m, 1.0, 1)] == [[1, 7, 11], [4, 7, 11]]
    assert [list(x) for x in runs_ref(m, 1.0, 2)] == [[1, 11], [7, 11]]
    assert [list(x) for x in runs_ref(m, 1.0, 3)] == [[1], [11]]
    assert [list(x) for x in runs_ref(np.ones(5), 1.0, 0)] == [[0], [4]]
    assert [len(x) for x in runs_ref(np.zeros(5), 1.0, 0)] == [0, 0]


def test_abi_names_and_struct_sizes():
    for name in ("vsig_runs_tile", "vsig_runs_dev", "vsig_runs"):
        assert name in _lib.SIGNATURES
    assert C.sizeof(_lib.Run) == 40
    assert C.sizeof(_lib.RunsInfo) == 40
    lib = _lib.load_library()
    tile = lib.vsig_runs_tile()
    assert tile >= 256 and tile & (tile - 1) == 0


def test_bad_arguments_are_refused_before_a_context_is_needed():
    lib = _lib.load_library()
    a = np.ones(4, np.float32)
    ap = a.ctypes.data_as(C.c_void_p)
    f32 = _lib.DTYPES["f32"]
    out = (_lib.Run * 2)()
    op = C.cast(out, C.c_void_p)
    for fn in (lib.vsig_runs, lib.vsig_runs_dev):
        info = _lib.RunsInfo(count=-7)
        ip = C.cast(C.pointer(info), C.c_void_p)
        calls = [
            (None, f32, ap, 4, 0.5, 0, 0, None, 0, ip),                   # the null context alone
            (None, f32, ap, 0, 0.5, 0, 0, None, 0, ip),                   # n < 1
            (None, f32, ap, (1 << 40) + 1, 0.5, 0, 0, None, 0, ip),       # n > 2^40
            (None, f32, ap, 4, 0.5, 0, 0, op, -1, ip),                    # cap < 0
            (None, f32, ap, 4, 0.5, 0, -1, None, 0, ip),                  # max_gap < 0
            (None, f32, None, 4, 0.5, 0, 0, None, 0, ip),                 # NULL a
            (None, f32, ap, 4, 0.5, 0, 0, None, 2, ip),                   # NULL out with cap > 0
            (None, 4, ap, 4, 0.5, 0, 0, None, 0, ip),                     # unknown dtype
            (None, f32, ap, 4, float("nan"), 0, 0, None, 0, ip),          # NaN thr
        ]
        for args in calls:
            assert fn(*args) == -1, args
            assert info.count == -7
        assert fn(None, f32, ap, 4, 0.5, 0, 0, None, 0, None) == -1       # NULL info


def test_find_runs_argument_errors():
    x = np.ones(16, np.float32)
    with pytest.raises(ValueError, match="NaN"):
        find_runs(x, float("nan"))
    with pytest.raises(ValueError, match="max_gap"):
        find_runs(x, 0.5, max_gap=-1)
    with pytest.raises(ValueError, match="min_length"):
        find_runs(x, 0.5, min_length=0)
    with pytest.raises(ValueError, match="max_runs"):
        find_runs(x, 0.5, max_runs=-1)
    with pytest.raises(ValueError, match="empty"):
        find_runs(x[:0], 0.5)


def test_detect_packets_argument_errors():
    x = np.ones(64, np.complex64)
    with pytest.raises(ValueError, match="max_gap"):
        detect_packets(x, 56e6, max_gap=-1)
    with pytest.raises(ValueError, match="min_length"):
        detect_packets(x, 56e6, min_length=0)
    with pytest.raises(ValueError, match="max_packets"):
        detect_packets(x, 56e6, max_packets=-1)
    with pytest.raises(ValueError, match="empty"):
        detect_packets(x[:0], 56e6)


def test_extract_packets_on_the_host():
    x = np.arange(100, dtype=np.complex64)
    got = extract_packets(x, [(3, 9), (50, 50), (90, 99)], pre_samples=5, post_samples=4)
    assert [p for _, p in got] == [3, 5, 5]                               # clipped at the array start
    assert np.array_equal(got[0][0], x[0:14])
    assert np.array_equal(got[1][0], x[45:55])
    assert np.array_equal(got[2][0], x[85:100])                           # clipped at the end
    assert np.shares_memory(got[1][0], x)
    assert extract_packets(x, []) == []
    with pytest.raises(ValueError, match="pre_samples"):
        extract_packets(x, [(3, 9)], pre_samples=-1)
    with pytest.raises(ValueError, match="pre_samples"):
        extract_packets(x, [(3, 9)], post_samples=-1)
    with pytest.raises(ValueError, match="not inside"):
        extract_packets(x, [(3, 100)])
    with pytest.raises(ValueError, match="not inside"):
        extract_packets(x, [(9, 3)])
