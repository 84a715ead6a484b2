"""Which bursts of a capture are the same packet sent again, and with what
period: the analysis path's last step, capture -> plan -> build_vector.

  packet_similarity  every pair of K packets against each other in one pass:
                     the normalised correlation peak rho, its lag and the
                     energies (vsig_match_run)
  group_packets      emitters: the connected components of rho >= threshold
  group_timing       each emitter's first arrival, period, count and jitter
  cluster_carriers   bursts' measured centres merged into carriers
  combine_packets    every emitter's bursts averaged coherently into one clean
                     packet, with a gain, a frequency and an SNR per instance
                     (vsig_combine_estimate / vsig_combine_sum)
  match_packets      the whole path from a capture and its burst list to the
                     ``configs`` that vector_plan / build_vector accept

group_packets, group_timing and cluster_carriers are host only.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .dsp import _is_dev, _ptr
from .packets import _check_ntaps, _check_segments, _per_burst, _signal_length, isolate_packets, measure_packets

__all__ = ["Similarity", "PacketGroups", "GroupTiming", "PacketMatches", "CombinedPackets", "CombineMembers",
           "packet_similarity", "group_packets", "group_timing", "cluster_carriers", "combine_packets", "match_packets"]

Similarity = namedtuple("Similarity", "rho lag energy")
PacketGroups = namedtuple("PacketGroups", "labels groups representative")
CombinedPackets = namedtuple("CombinedPackets", "packets gain members")
CombineMembers = namedtuple("CombineMembers", "a freq rho snr overlap used")


class PacketMatches(namedtuple("PacketMatches",
                               "similarity groups timing carriers carrier_of measurements isolated configs")):
    """match_packets' result; ``combined`` is the CombinedPackets of
    match_packets(..., combine=True), else None."""
    combined = None


MATCH_MAX_K = 4096
MATCH_MAX_L = 8192


class GroupTiming(namedtuple("GroupTiming", "start period count jitter arrivals")):
    """group_timing's result, one entry per group, in samples; ``seconds`` is
    the same record divided by the sample rate (count unchanged)."""
    sample_rate = 1.0

    @property
    def seconds(self):
        sr = self.sample_rate
        return GroupTiming(self.start / sr, self.period / sr, self.count, self.jitter / sr,
                           [a / sr for a in self.arrivals])


def match_size(lmax):
    """The transform length vsig_match_create takes for a longest packet of
    ``lmax`` samples: the smallest of 1024 / 4096 / 8192 / 16384 with
    N >= 2 lmax - 1."""
    for n in (1024, 4096, 8192):
        if n >= 2 * int(lmax) - 1:
            return n
    return 16384


def _check_packets(packets, max_samples, cap=MATCH_MAX_L, who="packet_similarity"):
    """(list of 1-D complex64 prefixes, lengths, all-device flag), with no
    device.  cap: the longest packet taken (None: any length)."""
    if hasattr(packets, "packets") and hasattr(packets, "cutoff"):      # IsolatedPackets
        packets = packets.packets
    if isinstance(packets, (np.ndarray, torch.Tensor)):
        raise ValueError("packets must be a list of 1-D complex64 arrays (or an IsolatedPackets)")
    packets = list(packets)
    if max_samples is not None:
        max_samples = int(max_samples)
        if max_samples < 1:
            raise ValueError("max_samples must be >= 1")
        if max_samples > MATCH_MAX_L:
            raise ValueError(f"max_samples must be at most {MATCH_MAX_L}")
    K = len(packets)
    if K < 1 or K > MATCH_MAX_K:
        raise ValueError(f"{who} takes 1 to {MATCH_MAX_K} packets ({K} given)")
    dev = [_is_dev(p) for p in packets]
    if any(dev) and not all(dev):
        raise ValueError("packets must be all numpy arrays or all CUDA tensors")
    out = []
    for k, p in enumerate(packets):
        if not dev[k]:
            p = np.asarray(p)
        if (p.dim() if dev[k] else p.ndim) != 1:
            raise ValueError(f"packet {k} is not 1-D")
        if p.dtype != (torch.complex64 if dev[k] else np.complex64):
            raise ValueError(f"packet {k} is {p.dtype}: complex64 packets only")
        if dev[k] and not p.is_cuda:
            raise ValueError(f"packet {k} is a CPU tensor: numpy arrays or CUDA tensors")
        if p.shape[0] < 1:
            raise ValueError(f"packet {k} is empty")
        if max_samples is not None:
            p = p[:max_samples]
        if cap is not None and p.shape[0] > cap:
            raise ValueError(f"packet {k} has {p.shape[0]} samples: packet_similarity compares at most "
                             f"{MATCH_MAX_L}; pass max_samples to compare prefixes")
        out.append(p)
    return out, np.array([int(p.shape[0]) for p in out], np.int64), all(dev)


def _packed_in_place(pk, lens):
    """The packets as one device buffer if they already are views of one,
    back to back and in order (isolate_packets' output); else None."""
    p0 = pk[0]
    base = p0.untyped_storage().data_ptr()
    pos = p0.storage_offset()
    for p, n in zip(pk, lens):
        if (p.untyped_storage().data_ptr() != base or p.storage_offset() != pos or p.device != p0.device
                or (n > 1 and p.stride(0) != 1)):
            return None
        pos += int(n)
    return torch.as_strided(p0, (int(lens.sum()),), (1,))


def _match_dev(ctx, packed, lens):
    """(peak float32 K x K, lag int32 K x K, energy float64 K) device tensors:
    one plan, one run."""
    K = int(lens.size)
    dev = packed.device
    peak = torch.empty((K, K), dtype=torch.float32, device=dev)
    lag = torch.empty((K, K), dtype=torch.int32, device=dev)
    energy = torch.empty(K, dtype=torch.float64, device=dev)
    plan = _lib.P()
    lens = np.ascontiguousarray(lens, np.int64)
    ctx.check(ctx.lib.vsig_match_create(ctx.h, lens.ctypes.data_as(C.POINTER(C.c_int64)), K, C.byref(plan)),
              "packet_similarity")
    try:
        ctx.check(ctx.lib.vsig_match_run(plan, _ptr(packed), _ptr(peak), _ptr(lag), _ptr(energy)),
                  "packet_similarity")
    finally:
        ctx.lib.vsig_match_free(plan)              # waits for the run: the plan owns its workspace
    return peak, lag, energy


def rho_from(peak, energy):
    """rho = peak / sqrt(E_a E_b) in float64; 0 where either energy is 0 (host)."""
    peak, energy = np.asarray(peak, np.float64), np.asarray(energy, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = np.sqrt(energy[:, None]) * np.sqrt(energy[None, :])
        rho = peak / den
    fin = np.isfinite(energy)
    rho[((energy[:, None] == 0) | (energy[None, :] == 0)) & fin[:, None] & fin[None, :]] = 0.0
    return rho


def packet_similarity(packets, max_samples=None):
    """Every packet against every other -> Similarity(rho, lag, energy).

    With c_ab[l] = sum_j p_a[j + l] conj(p_b[j]) (np.correlate(p_a, p_b,
    'full'), l = index - (len(p_b) - 1)):

      rho     float64 (K, K): max_l |c_ab[l]| / sqrt(E_a E_b), in [0, 1]; 1 for
              two packets that differ by a delay, a gain and a constant phase
      lag     int64 (K, K): the smallest l that attains the maximum --
              p_b's first sample lines up with p_a[l]; lag[b, a] = -lag[a, b]
      energy  float64 (K,): sum |p_k|^2

    packets: a list of 1-D complex64 arrays or CUDA tensors, or an
    IsolatedPackets; views of one packed device buffer (isolate_packets'
    output) are used in place, anything else is packed once.  1 to 4096
    packets of 1 to 8192 samples; max_samples compares the prefixes
    ``p[:max_samples]`` (as frequency_search's max_template) -- a longer
    packet without it is a ValueError.  All pairs run in one launch
    (vsig_match_run); rho is formed on the host from the device's fp32 peak
    and double energies.  A packet with a NaN or Inf sample has rho NaN and lag
    0 against every packet; an all-zero one rho 0 and lag 0.
    numpy in -> numpy out; CUDA tensors in -> tensors on their device.  Every
    argument error is raised before the device is touched."""
    pk, lens, dev_in = _check_packets(packets, max_samples)
    ctx = _lib.get_context()
    if dev_in:
        packed = _packed_in_place(pk, lens)
        if packed is None:
            packed = torch.cat([p.to(f"cuda:{ctx.device}") for p in pk])
    else:
        packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(pk))).to(f"cuda:{ctx.device}")
    peak, lag, energy = _match_dev(ctx, packed, lens)
    energy_h = energy.cpu().numpy()
    rho = rho_from(peak.cpu().numpy(), energy_h)
    lag_h = lag.cpu().numpy().astype(np.int64)
    if dev_in:
        d = packed.device
        return Similarity(torch.from_numpy(rho).to(d), torch.from_numpy(lag_h).to(d), energy)
    return Similarity(rho, lag_h, energy_h)


def _host(a, dtype):
    if _is_dev(a):
        a = a.cpu().numpy()
    return np.asarray(a, dtype)


def group_packets(rho, threshold=0.7, energy=None):
    """Emitters from a similarity matrix -> PacketGroups(labels, groups,
    representative).  Groups are the connected components of the graph that
    links a and b where rho[a, b] >= threshold or rho[b, a] >= threshold (so
    a chain a-b, b-c makes one group); NaN never links.  labels[k] is packet
    k's group, groups numbered by their first member; groups[g] the members in
    ascending order; representative[g] the member with the largest energy,
    the first on ties (the first member when energy is None).  Host only."""
    rho = _host(rho, np.float64)
    if rho.ndim != 2 or rho.shape[0] != rho.shape[1]:
        raise ValueError("rho must be a square matrix")
    threshold = float(threshold)
    if np.isnan(threshold):
        raise ValueError("threshold is NaN")
    K = rho.shape[0]
    if energy is not None:
        energy = _host(energy, np.float64)
        if energy.shape != (K,):
            raise ValueError(f"energy must have one entry per packet ({K})")
    with np.errstate(invalid="ignore"):
        link = rho >= threshold
    link = link | link.T
    labels = np.full(K, -1, np.int64)
    groups = []
    for k in range(K):
        if labels[k] >= 0:
            continue
        g = len(groups)
        labels[k] = g
        stack, members = [k], []
        while stack:
            i = stack.pop()
            members.append(i)
            for j in np.flatnonzero(link[i] & (labels < 0)):
                labels[j] = g
                stack.append(int(j))
        groups.append(np.array(sorted(members), np.int64))
    rep = np.zeros(len(groups), np.int64)
    for g, m in enumerate(groups):
        if energy is None:
            rep[g] = m[0]
        else:
            e = np.where(np.isnan(energy[m]), -np.inf, energy[m])
            rep[g] = m[int(np.argmax(e))]
    return PacketGroups(labels, groups, rep)


def group_timing(groups, starts, lag, sample_rate):
    """When each emitter sends -> GroupTiming(start, period, count, jitter,
    arrivals), one entry per group, in samples (``.seconds``: the same in
    seconds).

    groups: group_packets' PacketGroups (or a list of member index arrays: the
    representative is then the first member).  starts[k]: the capture index of
    packet k's first sample; lag: packet_similarity's.  Member k's arrival is
    ``t_k = starts[k] + lag[k, rep]`` -- where the representative's first
    sample lies in the capture when laid over packet k -- so a burst cut a few
    samples early or late arrives where the others do.  With the arrivals
    sorted, ``n_k = round((t_k - t_0) / min diff)`` counts periods, and period
    and start are the slope and the intercept of the least-squares line of t_k
    on n_k: a missed instance leaves a gap in n_k and biases neither.
    jitter = max |t_k - (start + period n_k)|.  A group of one member (or whose
    arrivals all coincide) has period NaN, start t_0, jitter 0.  Host only."""
    sample_rate = float(sample_rate)
    if not (sample_rate > 0 and np.isfinite(sample_rate)):
        raise ValueError("sample_rate must be finite and > 0")
    if hasattr(groups, "representative"):
        members, reps = list(groups.groups), np.asarray(groups.representative, np.int64)
    else:
        members = [np.asarray(m, np.int64) for m in groups]
        reps = np.array([int(m[0]) for m in members], np.int64)
    starts = _host(starts, np.float64)
    lag = _host(lag, np.int64)
    K = starts.size
    if starts.ndim != 1 or lag.shape != (K, K):
        raise ValueError("starts must be 1-D with one entry per packet and lag K x K")
    G = len(members)
    start, period, jitter = np.zeros(G), np.full(G, np.nan), np.zeros(G)
    count = np.zeros(G, np.int64)
    arrivals = []
    for g, (m, r) in enumerate(zip(members, reps)):
        if m.size < 1 or m.min() < 0 or m.max() >= K:
            raise ValueError(f"group {g} is empty or names a packet outside [0, {K})")
        t = np.sort(starts[m] + lag[m, r])
        arrivals.append(t)
        count[g] = t.size
        start[g] = t[0]
        d = np.diff(t)
        d = d[d > 0]
        if d.size == 0:
            continue
        n = np.round((t - t[0]) / d.min())
        nm, tm = n.mean(), t.mean()
        period[g] = np.sum((n - nm) * (t - tm)) / np.sum((n - nm) ** 2)
        start[g] = tm - period[g] * nm
        jitter[g] = np.max(np.abs(t - (start[g] + period[g] * n)))
    out = GroupTiming(start, period, count, jitter, arrivals)
    out.sample_rate = sample_rate
    return out


def cluster_carriers(centers, bandwidths, freq_tol=None):
    """Bursts' centre frequencies merged into carriers -> (carrier_of,
    carriers): the carrier index of every burst and the carriers' frequencies.
    Single linkage on the sorted centres: two neighbours share a carrier where
    their gap is below ``freq_tol`` (default: half the smaller of the two
    bursts' bandwidths); a carrier is the median centre of its cluster.
    Carriers are numbered in ascending frequency; a burst whose centre or
    bandwidth is NaN is a carrier of its own, frequency NaN, after the others.
    Host only."""
    centers, bandwidths = np.asarray(centers, np.float64), np.asarray(bandwidths, np.float64)
    if centers.ndim != 1 or centers.shape != bandwidths.shape:
        raise ValueError("centers and bandwidths must be 1-D arrays of one length")
    if freq_tol is not None:
        freq_tol = float(freq_tol)
        if not freq_tol >= 0:
            raise ValueError("freq_tol must be >= 0")
    ok = ~(np.isnan(centers) | np.isnan(bandwidths))
    order = np.flatnonzero(ok)[np.argsort(centers[ok], kind="stable")]
    carrier_of = np.full(centers.size, -1, np.int64)
    carriers = []
    cluster = []

    def close():
        if cluster:
            carrier_of[cluster] = len(carriers)
            carriers.append(float(np.median(centers[cluster])))
    for i, k in enumerate(order):
        if cluster:
            j = order[i - 1]
            tol = 0.5 * min(bandwidths[j], bandwidths[k]) if freq_tol is None else freq_tol
            if not centers[k] - centers[j] < tol:
                close()
                cluster = []
        cluster.append(int(k))
    close()
    for k in np.flatnonzero(~ok):
        carrier_of[k] = len(carriers)
        carriers.append(np.nan)
    return carrier_of, np.array(carriers, np.float64)


COMBINE_MAX_TOTAL = 1 << 31


def _check_min_rho(min_rho):
    min_rho = float(min_rho)
    if np.isnan(min_rho) or min_rho > 1:
        raise ValueError("min_rho must be a number no larger than 1")
    return min_rho


def _check_groups(groups, lag, K):
    """(group int32 K, lag-to-representative int64 K, representative int32 G)
    of a PacketGroups or a list of member index arrays, with no device."""
    if hasattr(groups, "representative"):
        members, reps = list(groups.groups), [int(r) for r in np.asarray(groups.representative)]
    else:
        if isinstance(groups, (np.ndarray, torch.Tensor)):
            raise ValueError("groups must be a PacketGroups or a list of member index arrays")
        members = list(groups)
        reps = None
    members = [np.asarray(_host(m, np.int64)).reshape(-1) for m in members]
    G = len(members)
    if G < 1:
        raise ValueError("combine_packets needs at least one group")
    if reps is None:
        if any(m.size < 1 for m in members):
            raise ValueError("a group is empty")
        reps = [int(m[0]) for m in members]
    lag = _host(lag, np.int64)
    if lag.shape != (K, K):
        raise ValueError(f"lag must be the K x K matrix of packet_similarity ({K} x {K})")
    group = np.full(K, -1, np.int32)
    for g, m in enumerate(members):
        if m.size < 1 or m.min() < 0 or m.max() >= K:
            raise ValueError(f"group {g} is empty or names a packet outside [0, {K})")
        if np.unique(m).size != m.size or np.any(group[m] >= 0):
            raise ValueError(f"group {g} names a packet twice or one that another group holds")
        group[m] = g
        if reps[g] not in m:
            raise ValueError(f"group {g}'s representative {reps[g]} is not one of its members")
        if lag[reps[g], reps[g]] != 0:
            raise ValueError(f"group {g}'s representative {reps[g]} has a lag to itself")
    reps = np.asarray(reps, np.int32)
    ok = group >= 0
    d = np.zeros(K, np.int64)
    d[ok] = lag[np.flatnonzero(ok), reps[group[ok]]]
    return group, d, reps


def _records_host(rec):
    return rec.cpu().numpy().view(_lib.COMBINE_MEMBER).reshape(-1)


def combine_packets(packets, groups, lag, *, min_rho=0.0, refine=False):
    """Each group's bursts averaged coherently into one packet ->
    CombinedPackets(packets, gain, members).

    packets: the K bursts (a list of 1-D complex64 arrays or CUDA tensors, or
    an IsolatedPackets: the full isolated bursts, of any length -- lags found
    on prefixes still hold); groups: group_packets' PacketGroups, or a list of
    member index arrays whose first entry is the representative (a packet no
    group names is left out); lag: packet_similarity's K x K matrix.

    Group g's packet lives in its representative's sample frame and has its
    length.  Every other member is first measured against the representative
    over their overlap -- a complex gain a_k, a residual frequency freq_k
    (cycles per sample, from the phase between the two halves of the overlap)
    and the normalised correlation rho_k -- then

      y_g[j] = sum_k conj(a_k) exp(-2j pi freq_k (j - m_k)) p_k[j + d_k] / sum_k |a_k|^2

    over the members that cover j (maximum-ratio combining; m_k the overlap's
    centre, d_k = lag[k, representative]).  A member with rho_k < min_rho, with
    a NaN or Inf sample, all zero or without overlap is not used (it is
    skipped, not added as zero); a group of one returns its packet's bytes.
    A second measurement against y_g, with freq_k as the prior, gives the
    per-instance SNR; refine=True sums once more with that second
    measurement's gains and frequencies.

      packets  G views of one packed complex64 buffer
      gain     float64 (G,): sum |a_k|^2 over the used members -- the predicted
               SNR of y_g over the representative alone
      members  CombineMembers(a complex128, freq, rho, snr, overlap, used), each
               (K,): the first measurement (the representative's own: a = 1,
               freq = 0, rho = 1), the overlap in samples, and snr_k = (Ep -
               res) / res (1 - |a_k|^2 / gain_g) from the second: signal over
               residual power against y_g, less the member's own noise inside
               y_g (inf where nothing is left over; NaN for a packet in no
               group, without overlap or with a non-finite sample)

    Three launches a pass on tables built once (vsig_combine_estimate, _sum,
    _estimate), whatever K and G are.  numpy in -> numpy out; CUDA tensors in
    -> tensors on their device, packed views used in place.  Every argument
    error is raised before the device is touched."""
    pk, lens, dev_in = _check_packets(packets, None, cap=None, who="combine_packets")
    K = int(lens.size)
    if int(lens.sum()) >= COMBINE_MAX_TOTAL:
        raise NotImplementedError("combine_packets: the packets hold 2^31 samples or more")
    group, d, reps = _check_groups(groups, lag, K)
    min_rho = _check_min_rho(min_rho)
    refine = bool(refine)
    G = int(reps.size)
    ctx = _lib.get_context()
    if dev_in:
        packed = _packed_in_place(pk, lens)
        if packed is None:
            packed = torch.cat([p.to(f"cuda:{ctx.device}") for p in pk])
    else:
        packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(pk))).to(f"cuda:{ctx.device}")
    dev = packed.device
    plan = _lib.P()
    I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    ctx.check(ctx.lib.vsig_combine_create(ctx.h, lens.ctypes.data_as(I64P), group.ctypes.data_as(I32P),
                                          d.ctypes.data_as(I64P), K, reps.ctypes.data_as(I32P), G, C.byref(plan)),
              "combine_packets")
    try:
        offsets = np.zeros(G + 1, np.int64)
        ctx.check(ctx.lib.vsig_combine_offsets(plan, offsets.ctypes.data_as(I64P)), "combine_packets")
        nrec = _lib.COMBINE_MEMBER.itemsize
        rec1 = torch.empty(K * nrec, dtype=torch.uint8, device=dev)
        rec2 = torch.empty(K * nrec, dtype=torch.uint8, device=dev)
        y = torch.empty(int(offsets[G]), dtype=torch.complex64, device=dev)
        ctx.check(ctx.lib.vsig_combine_estimate(plan, _ptr(packed), None, None, min_rho, _ptr(rec1)), "combine_packets")
        ctx.check(ctx.lib.vsig_combine_sum(plan, _ptr(packed), _ptr(rec1), _ptr(y)), "combine_packets")
        f0 = rec1.view(torch.float64).view(K, nrec // 8)[:, 2].contiguous()
        ctx.check(ctx.lib.vsig_combine_estimate(plan, _ptr(packed), _ptr(y), _ptr(f0), min_rho, _ptr(rec2)),
                  "combine_packets")
        if refine:
            ctx.check(ctx.lib.vsig_combine_sum(plan, _ptr(packed), _ptr(rec2), _ptr(y)), "combine_packets")
    finally:
        ctx.lib.vsig_combine_free(plan)            # waits for the launches: the plan owns their tables
    first, second = _records_host(rec1), _records_host(rec2)
    used = first["used"] != 0
    a = first["a_re"] + 1j * first["a_im"]
    power = np.where(used, np.abs(a) ** 2, 0.0)
    gain = np.array([power[group == g].sum() for g in range(G)])
    snr = np.full(K, np.nan)
    with np.errstate(all="ignore"):
        ok = (group >= 0) & (second["n"] > 0) & np.isfinite(second["Ep"]) & np.isfinite(second["res"])
        share = np.where(used & ok, power / np.where(ok, gain[np.maximum(group, 0)], 1.0), 0.0)
        share = np.where(np.isfinite(share), share, 0.0)
        res = second["res"]
        snr[ok] = np.where(res[ok] <= 0, np.inf, (second["Ep"][ok] - res[ok]) / res[ok] * (1 - share[ok]))
    members = CombineMembers(a, first["freq"].copy(), first["rho"].copy(), snr, first["n"].copy(), used)
    if dev_in:
        out = [y[int(offsets[g]):int(offsets[g + 1])] for g in range(G)]
        return CombinedPackets(out, torch.from_numpy(gain).to(dev),
                               CombineMembers(*(torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in members)))
    yh = y.cpu().numpy()
    return CombinedPackets([yh[int(offsets[g]):int(offsets[g + 1])] for g in range(G)], gain, members)


def _seconds_for(samples, sample_rate, trunc):
    """A time t with int(t * sample_rate) (trunc) or int(round(t * sample_rate))
    equal to ``samples`` where that is a whole number within 1e-6; else
    samples / sample_rate."""
    n = np.round(samples)
    if not np.isfinite(samples) or abs(samples - n) > 1e-6:
        return float(samples / sample_rate)
    t = n / sample_rate
    if trunc:
        while int(t * sample_rate) < n:
            t = np.nextafter(t, np.inf)
    return float(t)


def match_packets(signal, packets, sample_rate, center_freq=0.0, *, threshold=0.7, freq_tol=None, ntaps=255,
                  max_samples=4096, pre_samples=0, post_samples=0, measurements=None, combine=False, min_rho=0.0):
    """From a capture and its burst list to emitters and their timing ->
    PacketMatches(similarity, groups, timing, carriers, carrier_of,
    measurements, isolated, configs).

    1. centres and bandwidths: ``measurements`` (a PacketMeasurements of these
       bursts) or measure_packets(signal, packets, sample_rate, center_freq);
    2. cluster_carriers(centres, bandwidths, freq_tol): bursts on one carrier;
    3. isolate_packets with every burst's *carrier* as its centre and the
       widest bandwidth of its carrier: bursts of one emitter then differ by a
       constant phase only (their own measured centres differ by up to a bin,
       a residual rotation that decorrelates them);
    4. packet_similarity(isolated, max_samples), group_packets(rho, threshold,
       energy), group_timing with every slice's first capture index.

    configs: one dict per group, in group order, that vector_plan /
    build_vector accept: ``signal`` the representative's isolated packet,
    ``start_time`` and ``period`` the group's timing in seconds (chosen so that
    vector_plan's int() / round() give back the recovered whole samples),
    ``freq_shift`` = carrier - center_freq.  A group of one burst has the
    capture's duration as its period (one instance).
    combine=True: combine_packets(isolated, groups, lag, min_rho=min_rho) --
    every group's bursts averaged coherently -- is returned as ``.combined``
    and its packets are the configs' ``signal`` in place of one noisy instance.
    packets: detect_packets' Packets or a (starts, ends) pair, inclusive ends;
    complex64 signals only; numpy in -> numpy out.  Every argument error is
    raised before the device is touched."""
    starts, ends = (packets.starts, packets.ends) if hasattr(packets, "starts") else packets
    dev_in = _is_dev(signal)
    if not dev_in:
        signal = np.asarray(signal)
    n = _signal_length(signal)
    if signal.dtype != (torch.complex64 if dev_in else np.complex64):
        raise NotImplementedError("match_packets: complex64 signals only")
    if n < 1:
        raise ValueError("match_packets of an empty signal")
    starts, ends = _check_segments(n, starts, ends)
    K = int(starts.size)
    if K < 1 or K > MATCH_MAX_K:
        raise ValueError(f"match_packets takes 1 to {MATCH_MAX_K} bursts ({K} given)")
    sample_rate, center_freq, threshold = float(sample_rate), float(center_freq), float(threshold)
    if not (sample_rate > 0 and np.isfinite(sample_rate)):
        raise ValueError("sample_rate must be finite and > 0")
    if not np.isfinite(center_freq):
        raise ValueError("center_freq must be finite")
    if np.isnan(threshold):
        raise ValueError("threshold is NaN")
    if freq_tol is not None and not float(freq_tol) >= 0:
        raise ValueError("freq_tol must be >= 0")
    ntaps = _check_ntaps(ntaps)
    max_samples = int(max_samples)
    if max_samples < 1 or max_samples > MATCH_MAX_L:
        raise ValueError(f"max_samples must be in [1, {MATCH_MAX_L}]")
    pre_samples, post_samples = int(pre_samples), int(post_samples)
    if pre_samples < 0 or post_samples < 0:
        raise ValueError("pre_samples and post_samples must be >= 0")
    if not isinstance(combine, (bool, np.bool_)):
        raise ValueError("combine must be True or False")
    min_rho = _check_min_rho(min_rho)
    if measurements is not None:
        for name in ("center_freq", "bandwidth"):
            _per_burst(f"measurements.{name}", getattr(measurements, name), K)
    else:
        measurements = measure_packets(signal, (starts, ends), sample_rate, center_freq)
    centers = np.asarray(measurements.center_freq, np.float64)
    bws = np.asarray(measurements.bandwidth, np.float64)
    carrier_of, carriers = cluster_carriers(centers, bws, freq_tol)
    wide = np.array([np.max(bws[carrier_of == c]) for c in range(carriers.size)])
    iso = isolate_packets(signal, (starts, ends), sample_rate, center_freq, freqs=carriers[carrier_of],
                          bandwidths=wide[carrier_of], pre_samples=pre_samples, post_samples=post_samples,
                          ntaps=ntaps)
    sim = packet_similarity(iso, max_samples)
    # bursts on different carriers never link, whatever their envelopes share
    rho = _host(sim.rho, np.float64).copy()
    rho[carrier_of[:, None] != carrier_of[None, :]] = 0.0
    groups = group_packets(rho, threshold, sim.energy)
    timing = group_timing(groups, starts - np.asarray(iso.pre, np.int64), sim.lag, sample_rate)
    configs = []
    for g, r in enumerate(groups.representative):
        period = timing.period[g] if timing.count[g] > 1 and np.isfinite(timing.period[g]) else float(n)
        shift = carriers[carrier_of[r]] - center_freq
        configs.append({"signal": iso.packets[int(r)], "pre_samples": 0,
                        "start_time": _seconds_for(max(0.0, timing.start[g]), sample_rate, False),
                        "period": _seconds_for(period, sample_rate, True),
                        "freq_shift": 0.0 if np.isnan(shift) else float(shift)})
    out = PacketMatches(sim, groups, timing, carriers, carrier_of, measurements, iso, configs)
    if combine:
        out.combined = combine_packets(iso, groups, sim.lag, min_rho=min_rho)
        for cfg, y in zip(configs, out.combined.packets):
            cfg["signal"] = y
    return out
