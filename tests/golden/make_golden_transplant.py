"""Generate tests/golden/transplant_quality.npz from the REFERENCE itself.

Like make_golden_vector_build.py, it needs a checkout of the reference named
by VECTOR_REFERENCE and imports its ``utils`` module (CPU only):

    VECTOR_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python tests/golden/make_golden_transplant.py

The transplant tab's four steps (unified_gui.py:1087-1233) -- utils.py's
extract_reference_segment, find_packet_location_in_vector,
transplant_packet_in_vector, validate_transplant_quality -- and
measure_packet_timing run on seeded inputs: one 16 384-sample complex64
vector (noise of sigma 0.1 with the packet at half amplitude added at 5003)
and one 3 001-sample QPSK packet, shared by every case.  Only data is stored:
the two shared arrays, each case's reference segment, the samples a case
writes over the shared vector (``<case>_patch`` at ``<case>_patch_at``) and
the reference's results, every dict flattened to ``<case>_<key>`` /
``<case>_criteria_<key>`` arrays.

  ok            locate -> transplant -> validate with packet[200:712]
  clipped       transplant and validate at len(vector) - 1000
  identical     transplanted is original (snr inf)
  zero_orig     the original region zeroed before the transplant (power_ratio 0.0)
  no_ref        an empty reference segment
  flat          a 512-sample tone reference (f/fs 0.05) against a tone region:
                a flat |c|
  mid           an unrelated 2048-sample noise reference against noise
  timing_tmpl / timing_energy   measure_packet_timing with / without a template
  segment       extract_reference_segment clamped at either end

The script refuses to write a fixture in which a tolerance could flip a
criterion: every confidence is more than 0.05 away from 0.3, every power_ratio
more than 10x away from 0.01, every finite snr more than 1 dB away from -30.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["VECTOR_REFERENCE"]
sys.path.insert(0, REF)

import utils as refutils  # noqa: E402  (the reference)

SR = 56e6
NV, NP, AT = 16384, 3001, 5003
CASES = ["ok", "clipped", "identical", "zero_orig", "no_ref", "flat", "mid"]


def cnoise(rng, n, sigma):
    """Complex noise of standard deviation sigma (sigma / sqrt(2) a component)."""
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return (sigma * np.sqrt(0.5) * w).astype(np.complex64)


def flatten(out, case, res):
    for k, v in res.items():
        if k == "criteria":
            for ck, cv in v.items():
                out[f"{case}_criteria_{ck}"] = np.asarray(cv)
        else:
            out[f"{case}_{k}"] = np.asarray(v)


def quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def main():
    rng = np.random.default_rng(20251019)
    bits = rng.integers(0, 2, size=(2, NP))
    packet = (((2 * bits[0] - 1) + 1j * (2 * bits[1] - 1)) / np.sqrt(2)).astype(np.complex64)
    vector = cnoise(rng, NV, 0.1)
    vector[AT:AT + NP] += np.complex64(0.5) * packet
    out = {"sample_rate": np.float64(SR), "vector": vector, "packet": packet}
    results = {}

    def validate(case, original, transplanted, location, ref):
        res = refutils.validate_transplant_quality(original, transplanted, packet, location, ref, SR)
        results[case] = res
        flatten(out, case, res)
        out[f"{case}_ref"] = np.asarray(ref, np.complex64)

    def patch(case, new, at):
        end = min(at + NP, NV)
        out[f"{case}_patch"] = new[at:end].copy()
        out[f"{case}_patch_at"] = np.int64(at)
        chk = vector.copy()
        chk[at:end] = new[at:end]
        assert np.array_equal(chk, new), case

    # ok: the tab's sequence
    ref = refutils.extract_reference_segment(packet, 200, 712)
    vloc, ploc, conf = refutils.find_packet_location_in_vector(vector, packet, ref)
    out["ok_location"] = np.array([vloc, ploc], np.int64)
    out["ok_location_confidence"] = np.float64(conf)
    new = quiet(refutils.transplant_packet_in_vector, vector, packet, vloc, ploc, normalize_power=True)
    patch("ok", new, int(vloc))
    validate("ok", vector, new, vloc, ref)
    ok_new = new

    # clipped: the region runs off the end of the vector
    at = NV - 1000
    new = quiet(refutils.transplant_packet_in_vector, vector, packet, at, 0, normalize_power=True)
    patch("clipped", new, at)
    validate("clipped", vector, new, at, ref)

    validate("identical", vector, vector, AT, ref)

    # zero_orig: nothing to normalise to
    zeroed = vector.copy()
    zeroed[AT:AT + NP] = 0
    new = quiet(refutils.transplant_packet_in_vector, zeroed, packet, AT, 0, normalize_power=True)
    patch("zero_orig", new, AT)
    validate("zero_orig", zeroed, new, AT, ref)

    validate("no_ref", vector, ok_new, AT, np.zeros(0, np.complex64))

    # flat: tone against tone
    tone = np.exp(2j * np.pi * 0.05 * np.arange(NP)).astype(np.complex64)
    new = vector.copy()
    new[AT:AT + NP] = tone
    patch("flat", new, AT)
    validate("flat", vector, new, AT, tone[:512].copy())

    # mid: noise against unrelated noise
    new = vector.copy()
    new[AT:AT + NP] = cnoise(rng, NP, 0.3)
    patch("mid", new, AT)
    validate("mid", vector, new, AT, cnoise(rng, 2048, 0.3))

    out["timing_tmpl"] = np.array(refutils.measure_packet_timing(vector, packet[:256]), np.int64)
    out["timing_energy"] = np.array(refutils.measure_packet_timing(vector), np.int64)
    out["segment_args"] = np.array([[-5, 100], [2900, 5000]], np.int64)
    out["segment_0"] = refutils.extract_reference_segment(packet, -5, 100)
    out["segment_1"] = refutils.extract_reference_segment(packet, 2900, 5000)

    for case, res in results.items():
        c, p, s = (float(res[k]) for k in ("reference_confidence", "power_ratio", "snr_improvement_db"))
        assert abs(c - 0.3) > 0.05, (case, c)
        assert p > 0.1 or p < 0.001, (case, p)
        assert not np.isfinite(s) or abs(s + 30) > 1, (case, s)

    out["cases"] = np.array(CASES)
    out["meta_numpy"] = np.array(np.__version__)
    out["meta_scipy"] = np.array(scipy.__version__)
    out["meta_reference"] = np.array("ramiyako/vector@2025-07-18 utils.py")
    path = os.path.join(HERE, "transplant_quality.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("location", vloc, ploc, conf)
    for case, res in results.items():
        print(case, {k: v for k, v in res.items() if k != "criteria"})
    print("timing", out["timing_tmpl"], out["timing_energy"])


if __name__ == "__main__":
    main()
