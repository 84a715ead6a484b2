"""Guard arenas: does a device entry point stay inside its operands?

Every device pointer of a call sits in an arena, one uint8 tensor of
GUARD + skew + payload + GUARD bytes whose payload starts at GUARD + skew, so
the operand's 16-byte alignment is the case's choice and both sides of it are
memory this module owns.

An input arena's guards, and the payload elements the contract says are not
used (holes: samples between strided samples, between frames, past the last
whole frame, a row's ld - extent pad, outside a trace's [lo, hi)), are filled
with one byte value that works for every element type:
  0xFF  NaN as float32 / float64, -1 as any integer;
  0x00  zero;
  0x7F  a huge finite value (float32 3.4e38, float64 1.4e306).
An output arena is filled with 0xA5 throughout before every call.

run(case) makes the same call four times on the same addresses (so the launch
path is the same) under the fills 0xFF, 0x00, 0x00, 0x7F and checks
  status      every call returns VSIG_OK;
  write       every output arena's two guards are still 0xA5 after each call;
  const       every input arena (payload, holes, guards) is byte-identical
              before and after, except an operand declared in-place;
  stable      the two 0x00 calls give the same bytes;
  read        the three fills give the same bytes: an FFT frame, a reduction
              or a window that takes in one stray element changes with it
              (tests/test_gpu_special_values.py pins that a NaN poisons the
              whole frame that holds it);
  value       the 0x00 payloads pass the case's check against its reference.
A case with stable=False (an entry point shown not to be bit-stable) replaces
`stable` and `read` by: no NaN or inf in any output and `value` under all
three fills.

One limit: a stray load whose value is discarded cannot be seen this way.

A violation raises GuardViolation naming the entry point, the case, the bound,
the operand and the first offending byte offset relative to the payload
(negative: in the guard before it).  The arenas may be CPU tensors, which is
how the harness's own logic is tested without a device.
"""
import numpy as np
import torch

GUARD = 256 * 1024          # > one 16384-point complex64 segment (128 KiB)
FILLS = (0xFF, 0x00, 0x7F)
OUT_FILL = 0xA5


class GuardViolation(AssertionError):
    def __init__(self, entry, label, bound, operand=None, offset=None, detail=""):
        self.entry, self.label, self.bound, self.operand, self.offset = entry, label, bound, operand, offset
        where = "" if operand is None else f" operand {operand!r}"
        at = "" if offset is None else f" first offending byte {offset:+d} relative to the payload"
        super().__init__(f"{entry} [{label}]: {bound} bound violated:{where}{at} {detail}".rstrip())


class In:
    """An input operand: data (any numpy array; its bytes are the payload),
    skew in bytes, holes: a boolean mask over data's elements that the entry
    point must not use.  inplace: the entry point writes its result over the
    payload (returned as an output of dtype data.dtype)."""

    def __init__(self, data, skew=0, holes=None, inplace=False):
        data = np.ascontiguousarray(data)
        self.dtype = data.dtype
        self.bytes = data.reshape(-1).view(np.uint8).copy()
        self.skew, self.inplace = int(skew), bool(inplace)
        self.hole = None
        if holes is not None:
            holes = np.asarray(holes, bool).reshape(-1)
            assert holes.size == data.size
            self.hole = np.repeat(holes, data.dtype.itemsize)
        self.nbytes = self.bytes.size


class Out:
    """An output operand of n elements of dtype."""

    def __init__(self, n, dtype, skew=0):
        self.dtype = np.dtype(dtype)
        self.nbytes = int(n) * self.dtype.itemsize
        self.skew = int(skew)


class Case:
    """entry: the entry point's name; label: the case; ins / outs: name -> In /
    Out; call(p): makes the call with p[name] the payload's address (an int)
    and returns the status, or (status, {name: numpy array}) for results the
    entry point returns to the host; check(o): raises AssertionError unless
    o[name], the output payloads as arrays of their dtype (in-place inputs and
    host results included), agree with the reference."""

    def __init__(self, entry, label, ins, outs, call, check, stable=True):
        self.entry, self.label, self.ins, self.outs = entry, label, ins, outs
        self.call, self.check, self.stable = call, check, stable


def _arena(op, device):
    t = torch.empty(GUARD + op.skew + op.nbytes + GUARD, dtype=torch.uint8, device=device)
    if t.is_cuda:
        assert t.data_ptr() % 256 == 0, "an arena's base must be a multiple of 256"
    return t


def _image(op, fill):
    """The bytes of an input arena under one fill."""
    img = np.full(GUARD + op.skew + op.nbytes + GUARD, fill, np.uint8)
    pay = img[GUARD + op.skew:GUARD + op.skew + op.nbytes]
    pay[:] = op.bytes
    if op.hole is not None:
        pay[op.hole] = fill
    return img


def _first_diff(a, b):
    d = np.flatnonzero(a != b)
    return int(d[0]) if d.size else None


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _one_call(case, arenas, fill, device):
    """One call under one fill: {name: output payload bytes} (host results as
    arrays), after the write and const bounds."""
    images = {}
    for name, op in case.ins.items():
        images[name] = _image(op, fill)
        arenas[name].copy_(torch.from_numpy(images[name]))
    for name in case.outs:
        arenas[name].fill_(OUT_FILL)
    _sync(device)
    ptrs = {name: arenas[name].data_ptr() + GUARD + op.skew
            for name, op in list(case.ins.items()) + list(case.outs.items())}
    rc = case.call(ptrs)
    host = {}
    if isinstance(rc, tuple):
        rc, host = rc
    _sync(device)
    if rc != 0:
        raise GuardViolation(case.entry, case.label, "status", detail=f"the call returned {rc} (fill {fill:#04x})")
    got = {}
    for name, op in case.outs.items():
        back = arenas[name].cpu().numpy()
        lo, hi = GUARD + op.skew, GUARD + op.skew + op.nbytes
        bad = np.flatnonzero(back[:lo] != OUT_FILL)
        if bad.size:                      # the byte nearest the payload
            raise GuardViolation(case.entry, case.label, "write", name, int(bad[-1]) - lo, f"(fill {fill:#04x})")
        bad = np.flatnonzero(back[hi:] != OUT_FILL)
        if bad.size:
            raise GuardViolation(case.entry, case.label, "write", name, op.nbytes + int(bad[0]),
                                 f"(fill {fill:#04x})")
        got[name] = back[lo:hi].copy()
    for name, op in case.ins.items():
        back = arenas[name].cpu().numpy()
        lo, hi = GUARD + op.skew, GUARD + op.skew + op.nbytes
        if op.inplace:
            got[name] = back[lo:hi].copy()
            back[lo:hi] = images[name][lo:hi]
        d = _first_diff(back, images[name])
        if d is not None:
            raise GuardViolation(case.entry, case.label, "const", name, d - lo,
                                 f"an input was written (fill {fill:#04x})")
    for name, a in host.items():
        got[name] = np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()
        case.host_dtypes[name] = np.asarray(a).dtype
    return got


def _typed(case, got):
    out = {}
    for name, b in got.items():
        if name in case.outs:
            dt = case.outs[name].dtype
        elif name in case.ins:
            dt = case.ins[name].dtype
        else:
            dt = case.host_dtypes[name]
        out[name] = b.view(dt)
    return out


def _same(case, bound, a, b, what):
    for name in a:
        d = _first_diff(a[name], b[name])
        if d is not None:
            raise GuardViolation(case.entry, case.label, bound, name, d, what)


def _finite(case, typed, fill):
    for name, a in typed.items():
        if a.dtype.kind in "fc":
            bad = np.flatnonzero(~np.isfinite(a))
            if bad.size:
                raise GuardViolation(case.entry, case.label, "read", name, int(bad[0]) * a.dtype.itemsize,
                                     f"a non-finite output under fill {fill:#04x}")


def _value(case, typed, fill):
    try:
        case.check(typed)
    except GuardViolation:
        raise
    except AssertionError as e:
        raise GuardViolation(case.entry, case.label, "value", detail=f"(fill {fill:#04x}) {e}") from e


def run(case, device="cuda"):
    """The four calls and every bound; returns the 0x00 call's outputs."""
    case.host_dtypes = {}
    arenas = {name: _arena(op, device) for name, op in list(case.ins.items()) + list(case.outs.items())}
    nan = _one_call(case, arenas, 0xFF, device)
    zero = _one_call(case, arenas, 0x00, device)
    again = _one_call(case, arenas, 0x00, device)
    huge = _one_call(case, arenas, 0x7F, device)
    if case.stable:
        _same(case, "stable", zero, again, "two calls on identical bytes differ")
        _same(case, "read", zero, nan, "the output changes with the 0xff (NaN) fill outside the operands")
        _same(case, "read", zero, huge, "the output changes with the 0x7f (huge) fill outside the operands")
        _value(case, _typed(case, zero), 0x00)
    else:
        for fill, got in ((0xFF, nan), (0x00, zero), (0x7F, huge)):
            typed = _typed(case, got)
            _finite(case, typed, fill)
            _value(case, typed, fill)
    return _typed(case, zero)
