"""Generate tests/golden/vector_build.npz from the REFERENCE itself.

Like make_golden.py, it needs a checkout of the reference named by
VECTOR_REFERENCE and imports its ``utils`` module:

    VECTOR_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg \
        python tests/golden/make_golden_vector_build.py

generate_vector (unified_gui.py:1692-1791) lives in a GUI class, so its loop
is run here in plain numpy on what the reference's own load_packet_info and
apply_frequency_shift return: packets from tests/golden/mat/ (truncated to a
few thousand samples), added into a zeroed complex64 vector every period from
start_time, then divided by the peak.  Only data is stored.

  scenario a   ~10^5-sample vector at 56 MS/s, six packets: three overlap at
               their first instances, one has pre_samples above its start
               (clamped to 0), last instances that would be cut off are left out
  scenario b   the same packets in a 2500-sample vector: the longer packets
               get zero instances
  fr*          compute_freq_ranges (utils.py:129-159) on a few shift lists
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["VECTOR_REFERENCE"]
sys.path.insert(0, REF)

import utils as refutils  # noqa: E402  (the reference)

SR = 56e6
#          file                 keep  freq_shift  period     start_time
PACKETS = [("packet_1.mat",       4101, 5e6,      0.7143e-3, 100e-6),
           ("packet_1_5MHz.mat",  3000, 0,        0.4100e-3, 110e-6),
           ("packet_2_chirp.mat", 2047, -7.5e6,   0.7200e-3, 120e-6),
           ("packet_3.mat",       1500, 1e6,      0.8929e-3, 300e-6),
           ("sample_vector.mat",   777, 0,        0.3571e-3, 52.3e-6),
           ("packet_2_chirp.mat", 1000, -2e6,     0.8036e-3, 1e-6)]
SCENARIOS = {"a": 1.7858e-3, "b": 2500.5 / SR}
FR_CASES = [([5e6, 0, -7.5e6], 1e6), ([0, 0], 1e6), ([], 1e6), ([True, 2e6], 1e6),
            (["a", 3e6, -1e6], 1e6), ([True, False], 1e6), ([1, 2.5], 5e5), ([0, 4e6], 1e6)]


def assemble(packets, vector_length):
    """The reference's loop (unified_gui.py:1711-1781) on loaded packets."""
    total_samples = int(vector_length * SR)
    vector = np.zeros(total_samples, dtype=np.complex64)
    starts, periods, counts, times = [], [], [], []
    for (y, pre), (_, _, shift, period, start_time) in zip(packets, PACKETS):
        if shift != 0:
            y = refutils.apply_frequency_shift(y, shift, SR)
        period_samples = int(period * SR)
        start_offset = max(0, int(round(start_time * SR)) - pre)
        pos, count = start_offset, 0
        while pos + len(y) <= total_samples:
            vector[pos:pos + len(y)] += y
            times.append((pos + pre) / SR)
            count += 1
            pos += period_samples
        starts.append(start_offset)
        periods.append(period_samples)
        counts.append(count)
    max_val = np.max(np.abs(vector))
    normalised = vector / max_val if max_val > 0 else vector
    return dict(total_samples=np.int64(total_samples), starts=np.array(starts, np.int64),
                periods=np.array(periods, np.int64), counts=np.array(counts, np.int64),
                marker_times=np.array(times, np.float64), vector=vector,
                max_val=np.float32(max_val), normalised=normalised.astype(np.complex64))


def main():
    out = {"sample_rate": np.float64(SR),
           "files": np.array([p[0] for p in PACKETS]),
           "freq_shift": np.array([p[2] for p in PACKETS], np.float64),
           "period": np.array([p[3] for p in PACKETS], np.float64),
           "start_time": np.array([p[4] for p in PACKETS], np.float64)}
    packets = []
    for i, (name, keep, *_) in enumerate(PACKETS):
        y, pre = refutils.load_packet_info(os.path.join(HERE, "mat", name))
        packets.append((y[:keep], pre))
        out[f"packet{i}"] = y[:keep]
    out["pre_samples"] = np.array([p[1] for p in packets], np.int64)
    for key, vector_length in SCENARIOS.items():
        out[f"{key}_vector_length"] = np.float64(vector_length)
        for k, v in assemble(packets, vector_length).items():
            out[f"{key}_{k}"] = v
    out["fr_cases"] = np.array(json.dumps(FR_CASES))
    for j, (shifts, margin) in enumerate(FR_CASES):
        r = refutils.compute_freq_ranges(shifts, margin)
        out[f"fr{j}"] = np.zeros((0, 2)) if r is None else np.array(r, np.float64)
    out["meta_numpy"] = np.array(np.__version__)
    out["meta_scipy"] = np.array(scipy.__version__)
    out["meta_reference"] = np.array("ramiyako/vector@2025-07-18 utils.py")
    path = os.path.join(HERE, "vector_build.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for key in SCENARIOS:
        print(key, int(out[f"{key}_total_samples"]), out[f"{key}_starts"], out[f"{key}_counts"],
              float(out[f"{key}_max_val"]))


if __name__ == "__main__":
    main()
