"""Inputs and comparisons shared by the non-finite / extreme-value tests
(test_special_values_cpu.py, test_gpu_special_values.py).  A plain helper
module: no fixtures, no collection hooks."""
import numpy as np

_REAL = {np.dtype(np.float32): np.float32, np.dtype(np.float64): np.float64,
         np.dtype(np.complex64): np.float32, np.dtype(np.complex128): np.float64}
_CPLX = {np.float32: np.complex64, np.float64: np.complex128}
_BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64,
         np.dtype(np.complex64): np.uint32, np.dtype(np.complex128): np.uint64,
         np.dtype(np.int16): np.uint16}


def real_of(dtype):
    """The real scalar type behind a real or complex floating dtype."""
    return _REAL[np.dtype(dtype)]


def specials(dtype):
    """The 13 special values of a real floating dtype: +-0, the smallest and
    largest subnormal, the smallest normal, +-1, sqrt(max), +-max, +-inf, NaN."""
    rt = real_of(dtype)
    fi = np.finfo(rt)
    sub_max = np.nextafter(rt(fi.smallest_normal), rt(0))
    return np.array([0.0, -0.0, fi.smallest_subnormal, sub_max, fi.smallest_normal, 1.0, -1.0,
                     np.sqrt(rt(fi.max)), fi.max, -fi.max, np.inf, -np.inf, np.nan], dtype=rt)


def grid(dtype):
    """The cross product of specials as complex values (169 points); real and
    imaginary parts are assigned separately, so signed zeros and NaN survive."""
    rt = real_of(dtype)
    s = specials(rt)
    g = np.zeros(len(s) * len(s), dtype=_CPLX[rt])
    g.real = np.repeat(s, len(s))
    g.imag = np.tile(s, len(s))
    return g


def wide(n, dtype, seed):
    """n complex samples whose real and imaginary parts are scaled
    independently and log-uniformly over the whole exponent range of the dtype
    (smallest subnormal .. max), with random signs.  So that every class of
    result is present at any n >= 128: every 64th sample has both parts in the
    top decade (|z| overflows), every 61st both parts subnormal, and a sparse
    set holds NaN / inf in one part (an inf beside a NaN included)."""
    rt = real_of(dtype)
    fi = np.finfo(rt)
    rng = np.random.default_rng(seed)
    lo, hi = np.log10(float(fi.smallest_subnormal)), np.log10(float(fi.max))
    sn = np.log10(float(fi.smallest_normal))

    def part(lo_, hi_, m):
        with np.errstate(over="ignore", under="ignore"):
            mag = np.minimum(10.0 ** rng.uniform(lo_, hi_, m), float(fi.max)).astype(rt)
        return mag * rng.choice(np.array([-1, 1], rt), m)

    z = np.zeros(n, dtype=_CPLX[rt])
    z.real, z.imag = part(lo, hi, n), part(lo, hi, n)
    i = np.arange(n)
    top, sub = i % 64 == 1, i % 61 == 2
    z.real[top], z.imag[top] = part(hi - 1, hi, top.sum()), part(hi - 0.1, hi, top.sum())
    z.real[sub], z.imag[sub] = part(lo, sn, sub.sum()), part(lo, sn, sub.sum())
    z.real[i % 101 == 3] = np.nan
    z.imag[i % 103 == 4] = np.nan
    z.real[i % 107 == 5] = np.inf
    z.imag[i % 109 == 6] = -np.inf
    z.imag[i % (101 * 2) == 3] = np.inf          # inf beside a NaN: inf wins
    return z


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(_BITS[a.dtype])


def same_bits(got, want):
    """Elementwise: equal bit patterns, or both NaN.  dtypes and shapes must
    agree (a result of another type is a mismatch, not something to cast)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.dtype.kind == "c":
        rt = real_of(got.dtype)
        got, want = np.ascontiguousarray(got).view(rt), np.ascontiguousarray(want).view(rt)
    if got.dtype.kind != "f":
        return got == want
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def same_scalar(got, want):
    """same_bits for two scalars compared as float64."""
    return bool(same_bits(np.array([got], np.float64), np.array([want], np.float64))[0])


def poison(x, at, value):
    """A copy of x with the sample(s) at index / indices `at` replaced."""
    y = np.array(x, copy=True)
    y[at] = value
    return y


def first_diff(mask, *arrays):
    """A short report of the first mismatches (for assertion messages)."""
    bad = np.flatnonzero(~np.asarray(mask).ravel())[:5]
    return [(int(i), *[np.asarray(a).ravel()[i] for a in arrays]) for i in bad]


# ---------------------------------------------------------------------------
# Section B: one clean base vector and the poisoned cases every reduction /
# detector test runs, with numpy's own answers (the GPU tests compare with
# these; test_special_values_cpu.py proves each poisoned answer differs from
# the clean one, so a kernel that ignores the poison cannot pass).
# ---------------------------------------------------------------------------
N_BASE = 2 * 4096 + 5          # two scan tiles and a tail; 8197 % 256 == 5
DTYPES = [np.complex64, np.complex128, np.float32, np.float64]


def base_signal(dtype, n=N_BASE, seed=1234):
    """Noise at 0.02 with a burst of amplitude 0.8 over [n // 3, 2 n // 3)
    (at most [3000, 5200)); the real dtypes take the real part."""
    rng = np.random.default_rng(seed)
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    a, b = min(3000, n // 3), min(5200, 2 * n // 3)
    x[a:b] += 0.8 * np.exp(2j * np.pi * 0.013 * np.arange(b - a))
    if np.dtype(dtype).kind != "c":
        x = x.real
    return x.astype(dtype)


def poison_cases(n=N_BASE, energy=False, cplx=False):
    """[(name, index or indices, value)]: NaN and +inf (and 1e20 for the
    energy-based functions: its float32 energy overflows to inf) at index 0,
    on either side of the 4096 boundary and at n - 1; two NaNs in different
    blocks; all NaN.  cplx adds a NaN in the imaginary part alone."""
    vals = [("nan", np.nan), ("inf", np.inf)] + ([("1e20", 1e20)] if energy else [])
    spots = sorted({0, min(4095, n // 2), min(4096, n // 2 + 1), n - 1})
    cases = [(f"{nm}@{at}", at, v) for nm, v in vals for at in spots]
    if n > 4:
        cases.append(("nan@two_blocks", [n // 4 + 1, n - 2], np.nan))
    if cplx:
        cases.append((f"nanj@{n // 2}", n // 2, complex(0.0, np.nan)))
    cases.append(("all_nan", slice(None), np.nan))
    return cases


def differs(a, b):
    """Do two answers (scalars, arrays, or tuples / lists of them) differ,
    with NaN equal to NaN?"""
    if isinstance(a, (tuple, list)):
        return len(a) != len(b) or any(differs(p, q) for p, q in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return True
    if a.dtype.kind in "fc" or b.dtype.kind in "fc":
        a, b = a.astype(np.complex128), b.astype(np.complex128)
        return not np.all((a == b) | (np.isnan(a) & np.isnan(b)))
    return not np.array_equal(a, b)


def np_threshold_stats(a, thr):
    """(count, first, last, max) of |a| >= thr: first = n, last = -1 when
    nothing passes; max is np.max (NaN when any element is)."""
    m = np.abs(a)
    idx = np.flatnonzero(m >= thr)
    return (len(idx), int(idx[0]) if len(idx) else len(a), int(idx[-1]) if len(idx) else -1,
            float(np.max(m)))


def np_boxcar(x, w):
    with np.errstate(all="ignore"):
        return np.convolve(np.abs(x) ** 2, np.ones(w) / w, mode="same")


def np_peak(c):
    """(argmax, max, mean, std) of |c| as numpy gives them."""
    with np.errstate(all="ignore"):
        a = np.abs(c)
        return int(np.argmax(a)), a[np.argmax(a)], np.mean(a), np.std(a)


def np_normalized_vector(packet, period, total, start=0):
    """ref.periodic_vector followed by generate_vector's peak normalise."""
    from oracle import ref
    with np.errstate(all="ignore"):
        v = ref.periodic_vector(packet, period, total, start)
        m = np.max(np.abs(v))
        return v / m if m > 0 else v


def nan_to_minus_one(m):
    """The magnitudes peaks.hip's rule amounts to: a NaN is never an instance,
    never beats a neighbour and never becomes a maximum -- as if it were -1."""
    return np.where(np.isnan(m), -1.0, m)
