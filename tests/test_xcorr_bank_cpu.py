"""CPU-only checks of the template bank: the numpy reference of the GPU tests
(tests/xcorr_bank_ref.py) finds what it plants, the C ABI declares and binds
the five entry points, and the front end's argument errors are raised before
any device or library is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import xcorr_bank_ref as xb
from vector_amd import CorrelatorBank, _lib, frequency_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["vsig_xcorr_bank_create", "vsig_xcorr_bank_create_dev", "vsig_xcorr_bank_free",
                "vsig_xcorr_bank_exec_dev", "vsig_xcorr_bank_plan"]
SR = 56e6


@pytest.mark.parametrize("mode", ["valid", "full"])
def test_reference_finds_the_planted_offset_and_position(mode):
    L, n, pos, k0 = 256, 3000, 1234, 6
    offs = xb.offset_grid(4 * xb.default_step(SR, L), xb.default_step(SR, L))
    assert len(offs) == 9
    s, p = xb.planted(L, n, offs, k0, pos, seed=3)
    f, lag, peak, lags, peaks = xb.frequency_search_ref(s, p, SR, offs, mode)
    assert f == offs[k0] and lag == pos
    assert int(np.argmax(peaks)) == k0 and lags[k0] == pos
    # |c| of the winner is about L; its neighbours sit half a cycle off
    # (sinc(1/2) = 0.64), the others a whole number of half cycles further
    assert abs(peak / L - 1) < 0.05
    assert np.all(np.abs(peaks[[k0 - 1, k0 + 1]] / L - 0.64) < 0.05)
    assert np.delete(peaks, [k0 - 1, k0, k0 + 1]).max() < 0.3 * L


def test_reference_between_two_grid_points_keeps_sinc_quarter():
    L, n, pos = 256, 2000, 700
    step = xb.default_step(SR, L)
    offs = xb.offset_grid(2 * step, step)
    s, p = xb.planted(L, n, [0.5 * step], 0, pos, seed=4)
    f, lag, peak, _, _ = xb.frequency_search_ref(s, p, SR, offs)
    assert f in (0.0, step) and lag == pos
    assert abs(peak / L - 0.90) < 0.05


def test_reference_only_correlates_max_template_samples():
    s, p = xb.planted(300, 1500, [0.0], 0, 400, seed=5)
    T = xb.hypotheses(p, [0.0, 1e4], SR, max_template=128)
    assert T.shape == (2, 128) and T.dtype == np.complex64
    assert np.array_equal(T[0], p[:128])
    _, lag, peak, _, _ = xb.frequency_search_ref(s, p, SR, [0.0], max_template=128)
    assert lag == 400 and abs(peak / 128 - 1) < 0.1


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "vsig.h")).read()
    assert "typedef struct vsig_xcorr_bank vsig_xcorr_bank;" in text
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|void)\s+" + name + r"\(", text), name


def test_lib_binds_the_entry_points():
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    sig = _lib.SIGNATURES
    assert sig["vsig_xcorr_bank_create"] == (C.c_int, [P, P, I32, I64, C.POINTER(P)])
    assert sig["vsig_xcorr_bank_create_dev"] == (C.c_int, [P, P, I32, I64, C.POINTER(P)])
    assert sig["vsig_xcorr_bank_free"] == (None, [P])
    assert sig["vsig_xcorr_bank_exec_dev"] == (C.c_int, [P, P, I64, I32, P, P])
    assert sig["vsig_xcorr_bank_plan"] == (C.c_int, [P, I64, I32, C.POINTER(I32), C.POINTER(I64),
                                                     C.POINTER(I64), C.POINTER(I64)])


def test_library_exports_the_entry_points():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libvsig.so is not built")
    lib = _lib.load_library()
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


VEC = np.zeros(64, np.complex64)
REF = np.ones(16, np.complex64)


@pytest.mark.parametrize("kw", [
    dict(),                                                  # neither
    dict(offsets=[0.0], max_offset=1e3),                     # both
    dict(offsets=[]),                                        # an empty grid
    dict(offsets=[0.0, np.nan]),                             # a NaN in the grid
    dict(offsets=[0.0, np.inf]),
    dict(offsets=np.zeros(4097)),                            # more than 4096 entries
    dict(offsets=np.zeros((2, 2))),
    dict(max_offset=1e10),                                   # 2 m + 1 > 4096 at the default step
    dict(max_offset=np.nan),
    dict(max_offset=-1.0),
    dict(max_offset=1e3, step=0.0),
    dict(offsets=[0.0], step=10.0),
    dict(offsets=[0.0], mode="same"),
    dict(offsets=[0.0], max_template=4097),
    dict(offsets=[0.0], max_template=0),
])
def test_frequency_search_argument_errors(kw):
    with pytest.raises(ValueError):
        frequency_search(VEC, REF, SR, **kw)


def test_frequency_search_shape_errors():
    with pytest.raises(ValueError):
        frequency_search(VEC, REF[:0], SR, offsets=[0.0])
    with pytest.raises(ValueError):
        frequency_search(VEC[:8], REF, SR, offsets=[0.0])          # valid: vector shorter
    with pytest.raises(ValueError):
        frequency_search(VEC.reshape(8, 8), REF, SR, offsets=[0.0])
    with pytest.raises(ValueError):
        frequency_search(VEC, REF, 0.0, offsets=[0.0])


@pytest.mark.parametrize("shape", [(0,), (16,), (0, 16), (3, 0), (2, 3, 4)])
def test_bank_rejects_empty_and_one_dimensional_input(shape):
    with pytest.raises(ValueError):
        CorrelatorBank(np.zeros(shape, np.complex64))


def test_bank_rejects_long_templates_and_large_banks():
    with pytest.raises(NotImplementedError, match="4096"):
        CorrelatorBank(np.zeros((1, 4097), np.complex64))
    with pytest.raises(ValueError, match="4096"):
        CorrelatorBank(np.zeros((4097, 1), np.complex64))
