// C-ABI layer: what finds and measures things in |a|: the peak, the peak and
// run lists, region powers, the line-trace envelope, numpy-order statistics,
// rank selection, thresholds, the boxcar energy, dB and |a| transforms.
#include <cstring>

#include "vsig_ctx.hpp"

// Partials of a reduction over a whole array: one per 256 elements, 2048 at most.
static long long reduce_parts(long long n) { return n > 2048 * 256 ? 2048 : (n + 255) / 256; }

// What the two record lists (peaks, runs) refuse; `reach`: the name of the
// list's distance argument.
static int list_check(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int64_t reach_value,
                      const char* reach, const void* out, int64_t cap, const void* info) {
  if (int rc = check_array(c, c && a && info, n)) return rc;
  if (n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n above 2^40");
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  if (cap < 0 || reach_value < 0)
    return fail(c, VSIG_E_INVALID, std::string("need cap >= 0 and ") + reach + " >= 0");
  if (cap > 0 && !out) return fail(c, VSIG_E_INVALID, "null out with cap > 0");
  if (thr != thr) return fail(c, VSIG_E_INVALID, "thr is NaN");
  return VSIG_OK;
}

// Host-pointer entry of a record list: the operand into stage[0]; stage[1]
// holds the info record, then `cap` records; dev(a_dev, out_dev, info_dev) is
// the device entry; the info comes back, then the min(count, cap) records.
template <class Rec, class Info, class Dev>
static int list_host(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, Rec* out, int64_t cap, Info* info,
                     Dev dev) {
  int rc;
  const size_t ib = sizeof(Info);
  if ((rc = stage_in(c, 0, a, (size_t)n * dtype_bytes(dtype))) ||
      (rc = c->stage[1].reserve(c, ib + (size_t)cap * sizeof(Rec))))
    return rc;
  char* sb = c->stage[1].as<char>();
  Rec* od = cap > 0 ? reinterpret_cast<Rec*>(sb + ib) : nullptr;
  if ((rc = dev(c->stage[0].data(), od, reinterpret_cast<Info*>(sb)))) return rc;
  Info h;
  HIPCHK(c, hipMemcpyAsync(&h, sb, ib, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t k = h.count < cap ? h.count : cap;
  if (k > 0) {
    HIPCHK(c, hipMemcpyAsync(out, od, (size_t)k * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *info = h;
  return VSIG_OK;
}

// ---------------------------------------------------------------- peak
int vsig_peak_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, vsig_peak_t* peak_dev) {
  if (int rc = check_array(c, c && a, n)) return rc;  // np.argmax of empty raises
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  const long long nparts = reduce_parts(n);
  int rc;
  if ((rc = ensure_partials(c, nparts))) return rc;
  {
    Timed t(c, "peak");
    HIPCHK(c, vsig::launch_peak_reduce(dtype, a, n, c->parts(), (int)nparts, c->stream));
  }
  if ((rc = finalize_peak(c, nparts, 0, peak_dev))) return rc;
  // numpy's answer when the array holds a NaN (a no-op on any other record)
  return HIPRC(c, vsig::launch_peak_first_nan(dtype, a, n, peak_record(c, peak_dev), c->stream));
}

int vsig_peak(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, vsig_peak_t* peak) {
  if (int rc = check_array(c, c && a && peak, n)) return rc;
  int rc;
  if ((rc = stage_in(c, 0, a, (size_t)n * dtype_bytes(dtype))) ||
      (rc = vsig_peak_dev(c, dtype, c->stage[0].data(), n, nullptr)) ||
      (rc = stage_out(c, peak, c->result, sizeof(vsig_peak_t))))
    return rc;
  return HIPRC(c, hipStreamSynchronize(c->stream));
}

// ---------------------------------------------------------------- peak list
static_assert(sizeof(vsig_instance_t) == sizeof(vsig::PeakInst) && sizeof(vsig_instance_t) == 16,
              "vsig_instance_t layout");
static_assert(sizeof(vsig_peaks_info_t) == sizeof(vsig::PeaksInfo) && sizeof(vsig_peaks_info_t) == 32,
              "vsig_peaks_info_t layout");

int vsig_peaks_tile(void) { return vsig::kPeaksTile; }

int vsig_peaks_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
                   int64_t min_distance, vsig_instance_t* out_dev, int64_t cap,
                   vsig_peaks_info_t* info_dev) {
  int rc = list_check(c, dtype, a, n, thr, min_distance, "min_distance", out_dev, cap, info_dev);
  if (rc || (rc = c->pscratch.reserve(c, vsig::peaks_scratch_bytes(n)))) return rc;
  Timed t(c, "peaks");
  return HIPRC(c, vsig::launch_peaks(dtype, a, n, thr, relative != 0, min_distance,
                                     reinterpret_cast<vsig::PeakInst*>(out_dev), cap,
                                     reinterpret_cast<vsig::PeaksInfo*>(info_dev), c->pscratch.data(), c->stream));
}

int vsig_peaks(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
               int64_t min_distance, vsig_instance_t* out, int64_t cap, vsig_peaks_info_t* info) {
  if (const int rc = list_check(c, dtype, a, n, thr, min_distance, "min_distance", out, cap, info)) return rc;
  return list_host(c, dtype, a, n, out, cap, info,
                   [&](const void* a_dev, vsig_instance_t* out_dev, vsig_peaks_info_t* info_dev) {
                     return vsig_peaks_dev(c, dtype, a_dev, n, thr, relative, min_distance, out_dev, cap, info_dev);
                   });
}

// ---------------------------------------------------------------- run list
static_assert(sizeof(vsig_run_t) == sizeof(vsig::RunRec) && sizeof(vsig_run_t) == 40, "vsig_run_t layout");
static_assert(sizeof(vsig_runs_info_t) == sizeof(vsig::RunsInfo) && sizeof(vsig_runs_info_t) == 40,
              "vsig_runs_info_t layout");

int vsig_runs_tile(void) { return vsig::kRunsTile; }

int vsig_runs_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
                  int64_t max_gap, vsig_run_t* out_dev, int64_t cap, vsig_runs_info_t* info_dev) {
  int rc = list_check(c, dtype, a, n, thr, max_gap, "max_gap", out_dev, cap, info_dev);
  if (rc || (rc = c->rnscratch.reserve(c, vsig::runs_scratch_bytes(n)))) return rc;
  Timed t(c, "runs");
  return HIPRC(c, vsig::launch_runs(dtype, a, n, thr, relative != 0, max_gap,
                                    reinterpret_cast<vsig::RunRec*>(out_dev), cap,
                                    reinterpret_cast<vsig::RunsInfo*>(info_dev), c->rnscratch.data(), c->stream));
}

int vsig_runs(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
              int64_t max_gap, vsig_run_t* out, int64_t cap, vsig_runs_info_t* info) {
  if (const int rc = list_check(c, dtype, a, n, thr, max_gap, "max_gap", out, cap, info)) return rc;
  return list_host(c, dtype, a, n, out, cap, info,
                   [&](const void* a_dev, vsig_run_t* out_dev, vsig_runs_info_t* info_dev) {
                     return vsig_runs_dev(c, dtype, a_dev, n, thr, relative, max_gap, out_dev, cap, info_dev);
                   });
}

// ---------------------------------------------------------------- region powers
int vsig_region_power_dev(vsig_ctx* c, const void* a, const void* b, int64_t n, double* sums_dev) {
  if (int rc = check_array(c, c && a && b && sums_dev, n)) return rc;  // the mean of an empty region
  if (!aligned8(a, b)) return fail(c, VSIG_E_INVALID, "region power: operands must be 8-byte aligned");
  if (int rc = c->gscratch.reserve(c, vsig::region_scratch_bytes())) return rc;
  Timed t(c, "region_power");
  return HIPRC(c, vsig::launch_region_power(static_cast<const float2*>(a), static_cast<const float2*>(b), n,
                                            sums_dev, c->gscratch.data(), c->stream));
}

// ---------------------------------------------------------------- line traces
static_assert(sizeof(vsig_trace_info_t) == sizeof(vsig::TraceInfo) && sizeof(vsig_trace_info_t) == 32,
              "vsig_trace_info_t layout");
static_assert(VSIG_TRACE_ABS == vsig::kTraceAbs && VSIG_TRACE_DB20 == vsig::kTraceDb20, "VSIG_TRACE_*");

int vsig_trace_envelope_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, int32_t shift, int64_t lo,
                            int64_t hi, int64_t bin, int32_t kind, double eps, void* env_min_dev,
                            void* env_max_dev, vsig_trace_info_t* info_dev) {
  if (int rc = check_array(c, c && a && env_max_dev, n)) return rc;
  if (n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n above 2^40");
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  if (kind != VSIG_TRACE_ABS && kind != VSIG_TRACE_DB20) return fail(c, VSIG_E_INVALID, "kind");
  if (lo < 0 || hi > n || lo >= hi) return fail(c, VSIG_E_INVALID, "need 0 <= lo < hi <= n");
  if (bin < 1) return fail(c, VSIG_E_INVALID, "need bin >= 1");
  if (!(eps >= 0.0) || std::isinf(eps)) return fail(c, VSIG_E_INVALID, "need a finite eps >= 0");
  if (int rc = c->tscratch.reserve(c, vsig::trace_scratch_bytes(lo, hi, bin))) return rc;
  Timed t(c, "trace");
  return HIPRC(c, vsig::launch_trace_envelope(dtype, a, n, shift != 0, lo, hi, bin, kind, eps, env_min_dev,
                                              env_max_dev, reinterpret_cast<vsig::TraceInfo*>(info_dev),
                                              c->tscratch.data(), c->stream));
}

// numpy's np.mean / np.std of |a| (find_correlation_peak's mean_corr /
// std_corr, utils.py:1329-1330) in numpy's own summation order.
int vsig_abs_stats_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double* stats_dev) {
  if (int rc = check_array(c, c && a && stats_dev, n)) return rc;
  if (dtype != VSIG_DTYPE_C128 && dtype != VSIG_DTYPE_F64)
    return fail(c, VSIG_E_UNSUPPORTED, "abs stats: dtype must be VSIG_DTYPE_C128 or VSIG_DTYPE_F64");
  if (int rc = c->sscratch.reserve(c, vsig::np_stats_scratch_bytes(n))) return rc;
  Timed t(c, "stats");
  return HIPRC(c, vsig::launch_np_stats(dtype, a, n, stats_dev, c->sscratch.data(), c->stream));
}

// ---------------------------------------------------------------- analysis
// k-th smallest of |a| (0-based ranks) by MSB-first 8-bit radix select:
// ceil(bits/8) histogram passes over the data, all ranks at once.
int vsig_select_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, const int64_t* ranks,
                    int32_t nranks, double* values) {
  if (!c || !a || !ranks || !values) return fail(c, VSIG_E_INVALID, "null pointer");
  if (dtype != VSIG_DTYPE_F32 && dtype != VSIG_DTYPE_F64) return fail(c, VSIG_E_INVALID, "dtype");
  if (nranks < 1 || nranks > 4 || n < 1) return fail(c, VSIG_E_INVALID, "1..4 ranks, n >= 1");
  for (int q = 0; q < nranks; ++q)
    if (ranks[q] < 0 || ranks[q] >= n) return fail(c, VSIG_E_INVALID, "rank out of range");
  const int bits = dtype == VSIG_DTYPE_F32 ? 32 : 64;
  unsigned long long pf[4] = {0, 0, 0, 0}, mk[4] = {0, 0, 0, 0};
  long long k[4];
  for (int q = 0; q < nranks; ++q) k[q] = ranks[q];
  if (int rc = c->stage[2].reserve(c, 4096 * 8 + 64)) return rc;
  unsigned long long* dhist = c->stage[2].as<unsigned long long>();
  unsigned long long* dpf = dhist + 4 * 256;
  unsigned long long* dmk = dpf + 4;
  std::vector<unsigned long long> h(4 * 256);
  for (int shift = bits - 8; shift >= 0; shift -= 8) {
    HIPCHK(c, hipMemsetAsync(dhist, 0, 4 * 256 * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(dpf, pf, sizeof(pf), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dmk, mk, sizeof(mk), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, vsig::launch_radix_hist(dtype, a, n, dpf, dmk, nranks, shift, dhist, c->stream));
    HIPCHK(c, hipMemcpyAsync(h.data(), dhist, 4 * 256 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < nranks; ++q) {
      long long acc = 0;
      int d = 0;
      for (; d < 255; ++d) {
        const long long cnt = (long long)h[q * 256 + d];
        if (k[q] < acc + cnt) break;
        acc += cnt;
      }
      k[q] -= acc;
      pf[q] |= (unsigned long long)d << shift;
      mk[q] |= 0xffull << shift;
    }
  }
  for (int q = 0; q < nranks; ++q) {
    // invert the order-preserving key (|a| >= 0: sign bit set, no flip)
    if (bits == 32) {
      const unsigned int u = (unsigned int)pf[q] & 0x7fffffffu;
      float f;
      memcpy(&f, &u, 4);
      values[q] = (double)f;
    } else {
      const unsigned long long u = pf[q] & 0x7fffffffffffffffull;
      double d;
      memcpy(&d, &u, 8);
      values[q] = d;
    }
  }
  return VSIG_OK;
}

int vsig_threshold_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr,
                       int64_t* count, int64_t* first, int64_t* last, double* maxval) {
  if (!c || !a || !count || !first || !last || !maxval) return fail(c, VSIG_E_INVALID, "null pointer");
  if (dtype != VSIG_DTYPE_F32 && dtype != VSIG_DTYPE_F64) return fail(c, VSIG_E_INVALID, "dtype");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  const long long nparts = reduce_parts(n);
  if (int rc = c->stage[2].reserve(c, (size_t)nparts * sizeof(vsig::ThreshPartialH))) return rc;
  HIPCHK(c, vsig::launch_thresh_reduce(dtype, a, n, thr, c->stage[2].data(), (int)nparts, c->stream));
  std::vector<vsig::ThreshPartialH> h(nparts);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->stage[2].data(), nparts * sizeof(vsig::ThreshPartialH),
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  long long cnt = 0, f = n, l = -1;
  double mx = -INFINITY;
  for (auto& p : h) {
    cnt += p.count;
    f = p.first < f ? p.first : f;
    l = p.last > l ? p.last : l;
    mx = vsig::np_max(mx, p.max);
  }
  *count = cnt;
  *first = f;
  *last = l;
  *maxval = mx;
  return VSIG_OK;
}

int vsig_boxcar_energy_dev(vsig_ctx* c, int32_t dtype, const void* x, int64_t n, int64_t w,
                           double* sm) {
  if (!c || !x || !sm) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  if (n < 1 || w < 1) return fail(c, VSIG_E_INVALID, "need n >= 1, w >= 1");
  const long long nt = vsig::energy_scan_tiles(n);
  int rc;
  if ((rc = c->stage[1].reserve(c, (size_t)nt * 8)) || (rc = c->stage[2].reserve(c, (size_t)n * 8))) return rc;
  double* P = c->stage[2].as<double>();
  HIPCHK(c, vsig::launch_energy_prefix(dtype, x, n, c->stage[1].as<double>(), P, c->stream));
  HIPCHK(c, vsig::launch_boxcar_same(P, n, w, sm, c->stream));
  double last = 0.0;
  HIPCHK(c, hipMemcpyAsync(&last, P + (n - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // stage buffers are reused by the next call
  if (!std::isfinite(last)) {
    // a non-finite energy poisons every prefix sum after it: np.convolve is
    // non-finite inside the window alone, so the outputs are summed directly
    HIPCHK(c, vsig::launch_boxcar_direct(dtype, x, n, w, sm, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VSIG_OK;
}

int vsig_db_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double floor_, void* out) {
  if (int rc = check_array(c, c && a && out, n)) return rc;
  return HIPRC(c, vsig::launch_db_transform(dtype, a, n, floor_, out, c->stream));
}

int vsig_abs_c64_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, void* out) {
  if (int rc = check_array(c, c && a && out, n)) return rc;
  return HIPRC(c, vsig::launch_abs_c64(dtype, a, n, (float2*)out, c->stream));
}

int vsig_abs_c128_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, void* out) {
  if (int rc = check_array(c, c && a && out, n)) return rc;
  return HIPRC(c, vsig::launch_abs_c128(dtype, a, n, (double2*)out, c->stream));
}
