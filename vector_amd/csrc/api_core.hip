// C-ABI layer of libvsig.so (declared in include/vsig.h), the part every
// feature uses: contexts, streams, options, the twiddle-table cache, partials,
// host staging, timing and clock sinks, the build id.
#include "vsig_ctx.hpp"

namespace vsig {
thread_local unsigned long long* g_clock_sink = nullptr;
}

namespace vsig::api {

void join_refine(vsig_ctx* c) {
  vsig_ctx::RefineAsync& ra = c->ra;
  if (!ra.pending) return;
  if (ra.joined && ra.joined_on == c->stream) return;
  (void)hipStreamWaitEvent(c->stream, ra.ev_ref, 0);
  ra.joined = true;
  ra.joined_on = c->stream;
}

static float2 cis(double a) { return make_float2((float)std::cos(a), (float)std::sin(a)); }

// tw[off_p + (r-1)*Ns + k] = exp(-2 pi i r k / (Ns R)), passes p >= 1.
int get_twiddles(vsig_ctx* c, int N, const float2** out) {
  return cached_table(c, {TableKind::Pass, N}, out, [&](std::vector<float2>& h) {
    int R[16], np = 0;
    if (vsig::plan_info(N, R, &np) != hipSuccess)
      return fail(c, VSIG_E_UNSUPPORTED, "FFT size " + std::to_string(N) + " not supported");
    int Ns = R[0];
    for (int p = 1; p < np; ++p) {
      for (int r = 1; r < R[p]; ++r)
        for (int k = 0; k < Ns; ++k)
          h.push_back(cis(-2.0 * M_PI * (double)r * (double)k / ((double)Ns * R[p])));
      Ns *= R[p];
    }
    if (h.empty()) h.push_back(make_float2(1.f, 0.f));
    return VSIG_OK;
  });
}

int get_tw2(vsig_ctx* c, int N, const float2** out) {
  return cached_table(c, {TableKind::TwoLevel, N}, out, [&](std::vector<float2>& h) {
    int S = 0, hi = 0;
    if (vsig::tw2_info(N, &S, &hi) != hipSuccess)
      return fail(c, VSIG_E_UNSUPPORTED, "FFT size " + std::to_string(N) + " not supported");
    const int n = N < 0 ? -N : N;
    for (int i = 0; i < hi; ++i) h.push_back(cis(-2.0 * M_PI * (double)i * (double)(1 << S) / (double)n));
    for (int i = 0; i < (1 << S); ++i) h.push_back(cis(-2.0 * M_PI * (double)i / (double)n));
    return VSIG_OK;
  });
}

int get_half_tw(vsig_ctx* c, int M, int T, const float2** out) {
  return cached_table(c, {TableKind::HalfFrame, M}, out, [&](std::vector<float2>& h) {
    for (int t = 0; t < T; ++t) h.push_back(cis(-2.0 * M_PI * (double)t / (double)M));
    return VSIG_OK;
  });
}

// Built in double.
int get_tw_big(vsig_ctx* c, long long M, const float2** out, int* S, int* hiA) {
  int lg = 0;
  while ((1LL << lg) < M) ++lg;
  *S = (lg + 1) / 2;
  *hiA = (int)(M >> *S);
  // keyed by log2 M (every caller's M is a power of two)
  return cached_table(c, {TableKind::FourStep, lg}, out, [&](std::vector<float2>& h) {
    for (long long i = 0; i < *hiA; ++i) h.push_back(cis(-2.0 * M_PI * (double)(i << *S) / (double)M));
    for (long long j = 0; j < (1LL << *S); ++j) h.push_back(cis(-2.0 * M_PI * (double)j / (double)M));
    return VSIG_OK;
  });
}

int ensure_partials(vsig_ctx* c, long long n) {
  join_refine(c);
  if (n <= c->npartials) return VSIG_OK;
  c->npartials = 0;
  long long cap = n < 4096 ? 4096 : n + n / 4;
  // + finalize_tmp() and counters() (see vsig_ctx)
  HIPCHK(c, c->partials.alloc((cap + vsig::kFinalizeTmp + vsig::kCounterRecs) * sizeof(PeakPartial)));
  HIPCHK(c, hipMemset(c->parts() + cap + vsig::kFinalizeTmp, 0, vsig::kCounterRecs * sizeof(PeakPartial)));
  c->npartials = cap;
  return VSIG_OK;
}

int stage_in(vsig_ctx* c, int i, const void* host, size_t bytes) {
  if (const int rc = c->stage[i].reserve(c, bytes)) return rc;
  return HIPRC(c, hipMemcpyAsync(c->stage[i].data(), host, bytes, hipMemcpyHostToDevice, c->stream));
}

int stage_out(vsig_ctx* c, void* host, const DevBuf& src, size_t bytes) {
  return HIPRC(c, hipMemcpyAsync(host, src.data(), bytes, hipMemcpyDeviceToHost, c->stream));
}

int check_segment_table(vsig_ctx* c, const void* segs, long long nseg, long long n) {
  if (nseg < 0 || nseg > (1LL << 24)) return fail(c, VSIG_E_INVALID, "nseg must be in [0, 2^24]");
  if (nseg > 0 && !segs) return fail(c, VSIG_E_INVALID, "null segment table");
  if (n < 1 || n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n must be in [1, 2^40]");
  return VSIG_OK;
}

int check_blocks(vsig_ctx* c, long long nblocks) {
  if (nblocks > 0x7fffffffLL) return fail(c, VSIG_E_UNSUPPORTED, "more than 2^31 - 1 blocks");
  return VSIG_OK;
}

PeakPartial* peak_record(vsig_ctx* c, vsig_peak_t* peak_dev) {
  return peak_dev ? reinterpret_cast<PeakPartial*>(peak_dev) : c->result.as<PeakPartial>();
}

int finalize_peak(vsig_ctx* c, long long nparts, int sqrt_max, vsig_peak_t* peak_dev) {
  return HIPRC(c, vsig::launch_partial_finalize(c->parts(), nparts, sqrt_max, peak_record(c, peak_dev),
                                                c->finalize_tmp(), c->stream));
}

int read_refine_keys(vsig_ctx* c, vsig::RefineKeys* keys) {
  HIPCHK(c, hipMemcpyAsync(keys, c->rscratch.data(), sizeof(*keys), hipMemcpyDeviceToHost, c->stream));
  return HIPRC(c, hipStreamSynchronize(c->stream));
}

int clear_refine_fault(vsig_ctx* c, unsigned long long fault) {
  char* keys = c->rscratch.as<char>();
  HIPCHK(c, hipMemsetAsync(keys, 0, sizeof(vsig::RefineKeys), c->stream));
  if (fault)
    HIPCHK(c, hipMemcpyAsync(keys + offsetof(vsig::RefineKeys, fault), &fault, sizeof(fault),
                             hipMemcpyHostToDevice, c->stream));
  if (c->parts())
    HIPCHK(c, hipMemsetAsync(c->counters(), 0, vsig::kCounterRecs * sizeof(PeakPartial), c->stream));
  return HIPRC(c, hipStreamSynchronize(c->stream));     // also: fault is a host local
}

}  // namespace vsig::api

int DevBuf::reserve(vsig_ctx* c, size_t bytes) {
  join_refine(c);
  if (bytes <= n_) return VSIG_OK;
  return HIPRC(c, alloc(bytes));
}

#ifndef VSIG_SRC_HASH
#define VSIG_SRC_HASH "unknown"
#endif
int vsig_version(void) { return 2; }
const char* vsig_build_id(void) { return VSIG_SRC_HASH; }

const char* vsig_errstr(int s) {
  switch (s) {
    case VSIG_OK: return "ok";
    case VSIG_E_INVALID: return "invalid argument";
    case VSIG_E_HIP: return "HIP runtime error";
    case VSIG_E_NOMEM: return "device out of memory";
    case VSIG_E_UNSUPPORTED: return "unsupported size";
    case VSIG_E_NODEVICE: return "no HIP device";
    case VSIG_E_REFINE: return "exact-argmax refine faulted (watchdog); peak record invalid";
    default: return "unknown status";
  }
}

int vsig_init(int device, vsig_ctx** out) {
  if (!out) return VSIG_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VSIG_E_NODEVICE;
  if (device < 0 || device >= ndev) return VSIG_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return VSIG_E_HIP;
  vsig_ctx* c = new vsig_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) { delete c; return VSIG_E_HIP; }
  c->stream = c->own;
  if (c->result.alloc(sizeof(PeakPartial)) != hipSuccess) { vsig_free(c); return VSIG_E_NOMEM; }
  *out = c;
  return VSIG_OK;
}

int vsig_timing_reset(vsig_ctx* c) {
  if (!c) return VSIG_E_INVALID;
  for (auto& kv : c->timers)
    for (auto& p : kv.second) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  c->timers.clear();
  return VSIG_OK;
}

void vsig_free(vsig_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  vsig_timing_reset(c);
  // the device is idle: every DevBuf of the context is freed with it, then
  // the streams and events
  const vsig_ctx::RefineAsync ra = c->ra;
  const hipStream_t own = c->own;
  delete c;
  if (ra.stream) (void)hipStreamDestroy(ra.stream);
  if (ra.ev_corr) (void)hipEventDestroy(ra.ev_corr);
  if (ra.ev_ref) (void)hipEventDestroy(ra.ev_ref);
  if (own) (void)hipStreamDestroy(own);
}

const char* vsig_last_error(const vsig_ctx* c) { return c ? c->err.c_str() : "null context"; }

void* vsig_get_stream(vsig_ctx* c) { return c ? (void*)c->stream : nullptr; }

int vsig_set_stream(vsig_ctx* c, void* s) {
  if (!c) return VSIG_E_INVALID;
  c->stream = (hipStream_t)s;  // NULL is the device's default (null) stream
  return VSIG_OK;
}

int vsig_set_option(vsig_ctx* c, const char* key, int value) {
  if (!c || !key) return VSIG_E_INVALID;
  const std::string k(key);
  if (k == "refine") {
    c->refine = value != 0;
  } else if (k == "refine_eps_ppm") {
    if (value < 1 || value > 500000) return fail(c, VSIG_E_INVALID, "refine_eps_ppm must be in [1, 500000]");
    c->refine_eps_ppm = value;
  } else if (k == "refine_cap") {
    if (value != 0 && value < 4096) return fail(c, VSIG_E_INVALID, "refine_cap must be 0 or >= 4096");
    c->refine_cap = value;
  } else if (k == "refine_watchdog_us") {
    if (value < 1) return fail(c, VSIG_E_INVALID, "refine_watchdog_us must be >= 1");
    c->refine_wd_us = value;
  } else if (k == "blas_threads") {
    if (value < 1 || value > 1024) return fail(c, VSIG_E_INVALID, "blas_threads must be in [1, 1024]");
    c->blas_threads = value;
  } else if (k == "psd_traces_batch") {
    if (value < 0) return fail(c, VSIG_E_INVALID, "psd_traces_batch must be >= 0");
    c->psd_traces_batch = value;
  } else if (k == "xcorr_bank_m") {
    if (value != 0 && value != 4096 && value != 8192 && value != 16384)
      return fail(c, VSIG_E_INVALID, "xcorr_bank_m must be 0, 4096, 8192 or 16384");
    c->xcorr_bank_m = value;
  } else if (k == "match_grid") {
    if (value < 0) return fail(c, VSIG_E_INVALID, "match_grid must be >= 0");
    c->match_grid = value;
  } else if (k == "refine_async") {
    vsig_ctx::RefineAsync& ra = c->ra;
    if (value && !ra.stream) {
      // the highest stream priority: the refine's few blocks are dispatched
      // ahead of the next step's FIR blocks queued beside them (at the default
      // priority they waited for CU slots behind the FIR and spun for ~3 ms)
      int lo = 0, hi = 0;
      if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
      HIPCHK(c, hipStreamCreateWithPriority(&ra.stream, hipStreamNonBlocking, hi));
      HIPCHK(c, hipEventCreateWithFlags(&ra.ev_corr, hipEventDisableTiming));
      HIPCHK(c, hipEventCreateWithFlags(&ra.ev_ref, hipEventDisableTiming));
    }
    if (!value) join_refine(c);
    c->refine_async = value != 0;
  } else {
    return fail(c, VSIG_E_INVALID, "unknown option " + k);
  }
  return VSIG_OK;
}

int vsig_get_option(const vsig_ctx* c, const char* key, int* value) {
  if (!c || !key || !value) return VSIG_E_INVALID;
  const std::string k(key);
  if (k == "refine") *value = c->refine;
  else if (k == "refine_eps_ppm") *value = c->refine_eps_ppm;
  else if (k == "refine_cap") *value = (int)c->refine_cap;
  else if (k == "refine_watchdog_us") *value = (int)c->refine_wd_us;
  else if (k == "blas_threads") *value = c->blas_threads;
  else if (k == "refine_async") *value = c->refine_async;
  else if (k == "psd_traces_batch") *value = (int)c->psd_traces_batch;
  else if (k == "xcorr_bank_m") *value = c->xcorr_bank_m;
  else if (k == "match_grid") *value = c->match_grid;
  else return VSIG_E_INVALID;
  return VSIG_OK;
}

void* vsig_refine_stream(vsig_ctx* c) {
  if (!c) return nullptr;
  return (void*)(c->refine_async && c->ra.stream ? c->ra.stream : c->stream);
}

int vsig_refine_join(vsig_ctx* c) {
  if (!c) return VSIG_E_INVALID;
  join_refine(c);
  return VSIG_OK;
}

int vsig_refine_status(vsig_ctx* c, int32_t* status, int64_t* candidates) {
  if (!c || !status || !candidates) return VSIG_E_INVALID;
  *status = 2;
  *candidates = 0;
  join_refine(c);
  if (!c->refine_ran || !c->rscratch.data()) return VSIG_OK;
  vsig::RefineKeys keys;
  int rc;
  if ((rc = read_refine_keys(c, &keys))) return rc;
  *candidates = (int64_t)keys.count;
  if (keys.fault) {
    // a watchdog fired in some refine since the last report: status 3 once,
    // then the fused launch's counters and the keys (fault word included) are
    // cleared, and the record is not to be trusted until then
    *status = 3;
    if ((rc = clear_refine_fault(c))) return rc;
    c->refine_ran = false;
    return VSIG_OK;
  }
  *status = keys.status ? 1 : 0;
  return VSIG_OK;
}

#ifdef VSIG_TUNING      // the tools' probes: not in include/vsig.h, so they name their linkage
extern "C" int vsig_fft_bench(vsig_ctx* c, int key, void* io, int frames, int iters, int twl) {
  if (!c || !io || frames < 1 || iters < 1) return fail(c, VSIG_E_INVALID, "bad arguments");
  const float2* tw;
  if (int rc = twl == 1 ? get_tw2(c, key, &tw) : get_twiddles(c, key, &tw)) return rc;
  Timed t(c, "fft_bench");
  return HIPRC(c, vsig::launch_fft_bench(key, (float2*)io, frames, iters, tw, twl, c->stream));
}

extern "C" int vsig_copy_bench(vsig_ctx* c, const void* x, int64_t n, void* y, int variant, int grid) {
  if (!c || !x || !y || n < 0) return fail(c, VSIG_E_INVALID, "bad arguments");
  Timed t(c, "copy_bench");
  return HIPRC(c, vsig::launch_copy_probe((const float2*)x, n, (float2*)y, variant, grid, c->stream));
}
#endif

int vsig_copy_dev(vsig_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c || !dst || !src || bytes < 0) return fail(c, VSIG_E_INVALID, "bad copy");
  if (bytes) HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDefault, c->stream));
  return VSIG_OK;
}

int vsig_synchronize(vsig_ctx* c) {
  if (!c) return VSIG_E_INVALID;
  join_refine(c);
  return HIPRC(c, hipStreamSynchronize(c->stream));
}

int vsig_clock_enable(vsig_ctx* c, int on) {
  if (!c) return VSIG_E_INVALID;
  if (on) {
    if (!c->clkbuf.data()) HIPCHK(c, c->clkbuf.alloc(2 * kClockSlots * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->clkbuf.data(), 0, c->clkbuf.bytes(), c->stream));
  }
  c->clock = on != 0;
  return VSIG_OK;
}

int vsig_clock_read(vsig_ctx* c, const char* kernel, double* ghz, int64_t* ticks) {
  if (!c || !kernel || !ghz) return VSIG_E_INVALID;
  *ghz = 0.0;
  if (ticks) *ticks = 0;
  auto it = c->clkslot.find(kernel);
  if (!c->clkbuf.data() || it == c->clkslot.end()) return VSIG_OK;
  unsigned long long h[2] = {0, 0};
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(h, c->clkbuf.as<unsigned long long>() + 2 * it->second, sizeof(h),
                      hipMemcpyDeviceToHost));
  if (h[1]) *ghz = (double)h[0] / (double)h[1] * 0.1;      // s_memrealtime runs at 100 MHz
  if (ticks) *ticks = (int64_t)h[1];
  return VSIG_OK;
}

int vsig_timing_enable(vsig_ctx* c, int on) {
  if (!c) return VSIG_E_INVALID;
  c->timing = on != 0;
  return VSIG_OK;
}

int vsig_timing_read(vsig_ctx* c, const char* kernel, double* total_ms, int64_t* launches) {
  if (!c || !kernel || !total_ms || !launches) return VSIG_E_INVALID;
  *total_ms = 0.0;
  *launches = 0;
  auto it = c->timers.find(kernel);
  if (it == c->timers.end()) return VSIG_OK;
  for (auto& p : it->second) {
    HIPCHK(c, hipEventSynchronize(p.second));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, p.first, p.second));
    *total_ms += ms;
    *launches += 1;
  }
  return VSIG_OK;
}
