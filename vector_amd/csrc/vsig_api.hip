// C-ABI layer of libvsig.so (declared in include/vsig.h): contexts, plans
// (twiddle tables, filter / template spectra), launch geometry, host staging.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vsig.h"
#include "dtype.hpp"

using vsig::PeakPartial;
using vsig::dtype_bytes;
using vsig::dtype_ok;
static_assert(VSIG_DTYPE_C128 == vsig::VSIG_C128 && VSIG_DTYPE_C64 == vsig::VSIG_C64 &&
              VSIG_DTYPE_F64 == vsig::VSIG_F64 && VSIG_DTYPE_F32 == vsig::VSIG_F32, "VSIG_DTYPE_*");

struct TimingRec {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};

constexpr int kClockSlots = 32;            // per-stage clock sinks (vsig_clock_*)

namespace vsig {
thread_local unsigned long long* g_clock_sink = nullptr;
}

// Owner of one device allocation (move-only; the destructor frees it).  Every
// device pointer the contexts and handles below own is one of these.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void* data() const { return p_; }
  size_t bytes() const { return n_; }
  template <class T> T* as() const { return static_cast<T*>(p_); }
  // A fresh allocation of exactly `bytes` (what it held is freed first; empty
  // on failure).  Plans, tables and handle members, which nothing reuses.
  hipError_t alloc(size_t bytes) {
    release();
    const hipError_t e = hipMalloc(&p_, bytes);
    if (e != hipSuccess) p_ = nullptr; else n_ = bytes;
    return e;
  }
  // Context scratch: at least `bytes`, grow-only, joined with a pending
  // asynchronous refine first (join_refine) because the caller is about to
  // reuse the buffer; VSIG_E_NOMEM / VSIG_E_HIP and empty on failure.
  int reserve(vsig_ctx* c, size_t bytes);

 private:
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  void* p_ = nullptr;
  size_t n_ = 0;
};

// Twiddle tables are cached per context by what they are and the transform
// they serve: its length (n < 0: an alternative plan of |n| points, the
// convention of plan_info / tw2_info), for FourStep log2 of it.
enum class TableKind { Pass, TwoLevel, HalfFrame, FourStep };
struct TableKey {
  TableKind kind;
  long long n;
  bool operator<(const TableKey& o) const { return kind != o.kind ? kind < o.kind : n < o.n; }
};

struct vsig_ctx {
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  std::map<TableKey, DevBuf> tables;     // device twiddle tables (cached_table)
  DevBuf partials;                       // per-block partials (ensure_partials)
  long long npartials = 0;
  DevBuf result;                         // scratch device result
  DevBuf stage[3];                       // host-API device staging
  DevBuf conv[3];                        // complex128 path: c64 operands / output
  DevBuf rscratch;                       // refine.hip scratch (keys first)
  DevBuf lkeys;                          // correlator lane keys (refine column candidates)
  DevBuf vscratch;                       // numpy-order |c| of every output (exact stats)
  DevBuf sscratch;                       // np_stats buffer sums
  DevBuf pscratch;                       // peaks.hip tile table, counts, offsets
  DevBuf rnscratch;                      // runs.hip tile table, mask words, per-group records
  DevBuf gscratch;                       // region.hip per-block partials
  DevBuf tscratch;                       // trace.hip per-block / per-chunk / per-column records
  DevBuf ptscratch;                      // psd_traces.hip record rows (+ the fold route's frame batch)
  long long psd_traces_batch = 0;        // fold route: frames per batch at most (0: the 256 MB rule)
  int xcorr_bank_m = 0;                  // template bank block size (0: by template length)
  PeakPartial* parts() const { return partials.as<PeakPartial>(); }
  // the first-level buffer of a two-level finalize, right after the partials,
  // then the fused finalize's block counters (zero between launches)
  PeakPartial* finalize_tmp() const { return parts() + npartials; }
  PeakPartial* counters() const { return finalize_tmp() + vsig::kFinalizeTmp; }
  int refine = 1;                        // exact re-rank of the correlators' peak
  int refine_eps_ppm = 1000;             // fp32 candidate band (relative, ppm of max |c|)
  long long refine_cap = 0;              // opt-in limit on candidate outputs (0: none)
  long long refine_wd_us = 2000000;      // refine_fused watchdog (option "refine_watchdog_us")
  int blas_threads = 1;                  // numpy's OpenBLAS threads (its zdotu splits > 10000 terms)
  bool refine_ran = false;
  struct Chirp { long long M; DevBuf c, B; };
  std::map<long long, Chirp> chirps;     // Bluestein plans by length (bigfft.hip)
  DevBuf bigtmp;                         // four-step scratch
  DevBuf spec[2];                        // resample / channel spectra
  std::string err;
  bool timing = false;
  std::map<std::string, TimingRec> timers;
  // "refine_async": the xcorr handle's refine on its own stream behind ev_corr,
  // ev_ref recorded after it; joined (the context stream waits on ev_ref) before
  // any reuse of its scratch -- see join_refine
  int refine_async = 0;
  struct RefineAsync {
    hipStream_t stream = nullptr;
    hipEvent_t ev_corr = nullptr, ev_ref = nullptr;
    bool pending = false;                // an async refine was enqueued
    bool joined = false;                 // ... and joined on joined_on
    hipStream_t joined_on = nullptr;
  } ra;
  bool clock = false;                    // per-stage clock sinks on (vsig_clock_enable)
  DevBuf clkbuf;                         // kClockSlots x {shader ticks, 100 MHz ticks}
  std::map<std::string, int> clkslot;
};

constexpr int kFirPartTaps = 8192;
struct vsig_fir {
  vsig_ctx* ctx;
  int ntaps, decim, M;
  long long hop;
  DevBuf Hs;
  DevBuf G;              // D = 4 polyphase component filters (M = 1024)
  // more than kFirPartTaps taps: undecimated parts of kFirPartTaps taps each,
  // summed with their delays (fir_part_accum); z: one part's output
  std::vector<vsig_fir*> parts;
  DevBuf z;
  // the stream may still use the buffers: wait, then the members free them
  ~vsig_fir() {
    (void)hipStreamSynchronize(ctx->stream);
    for (vsig_fir* p : parts) delete p;
  }
};

// A correlation template: L <= 8192 one spectrum of M points; longer
// templates a spectrum per 8192-sample chunk (M = 16384), applied as a sum of
// passes accumulated in c (a scratch kept with the handle when the caller
// passes none).  tmpl: the template on the device (refine pass).
struct vsig_xcorr {
  vsig_ctx* ctx;
  long long L = 0;
  int M = 0;
  std::vector<DevBuf> Ps;
  DevBuf SD;        // M = 16384, one spectrum: its parity-split table (xcorr.hip)
  DevBuf tmpl;
  DevBuf cbuf;
  explicit vsig_xcorr(vsig_ctx* c) : ctx(c) {}
  // the stream may still use the spectra: wait, then the members free them
  ~vsig_xcorr() { (void)hipStreamSynchronize(ctx->stream); }
};

// The tables and record rows of one segment table (vsig_psd_segments_create).
struct vsig_psd_segments {
  vsig_ctx* ctx;
  long long nseg = 0, n = 0, hop = 0;
  int nperseg = 0, nfft = 0;
  long long frames_total = 0, nblocks = 0, step = 0, run = 0, max_rows = 0;
  const float2* tw = nullptr;      // the context's cached table
  DevBuf blocks, segs, rows;
  explicit vsig_psd_segments(vsig_ctx* c) : ctx(c) {}
  // the stream may still use the tables: wait, then the members free them
  ~vsig_psd_segments() { (void)hipStreamSynchronize(ctx->stream); }
};

// The frame table and filter spectra of one burst table (vsig_isolate_create).
constexpr int kIsoMaxTaps = 511, kIsoMaxFilters = 4096;
struct vsig_isolate {
  vsig_ctx* ctx;
  long long nseg = 0, n = 0, nframes = 0, hop = 0;
  int lo = 0;                      // circular index of a frame's first output (ntaps - 1)
  std::vector<long long> offsets;  // nseg + 1 prefix sums of the packed output
  const float2* tw = nullptr;      // the context's cached table
  DevBuf frames, Hs;
  explicit vsig_isolate(vsig_ctx* c) : ctx(c) {}
  // the stream may still use the tables: wait, then the members free them
  ~vsig_isolate() { (void)hipStreamSynchronize(ctx->stream); }
};

// A bank of K templates of one length L <= kBankMaxL: the K spectra of M
// points in one table (row k at Ps + k M).
constexpr long long kBankMaxL = 4096;
constexpr int kBankMaxK = 4096;
struct vsig_xcorr_bank {
  vsig_ctx* ctx;
  int K = 0;
  long long L = 0;
  int M = 0;
  DevBuf Ps;
  explicit vsig_xcorr_bank(vsig_ctx* c) : ctx(c) {}
  // the stream may still use the spectra: wait, then the member frees them
  ~vsig_xcorr_bank() { (void)hipStreamSynchronize(ctx->stream); }
};

namespace {

int fail(vsig_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

// The context stream waits for the last asynchronous refine (once per stream
// after each refine): called before anything reuses the refine's scratch or
// operands -- every scratch / partials / staging allocation and use below goes
// through DevBuf::reserve / ensure_partials -- and by vsig_refine_join.
void join_refine(vsig_ctx* c) {
  vsig_ctx::RefineAsync& ra = c->ra;
  if (!ra.pending) return;
  if (ra.joined && ra.joined_on == c->stream) return;
  (void)hipStreamWaitEvent(c->stream, ra.ev_ref, 0);
  ra.joined = true;
  ra.joined_on = c->stream;
}

#define HIPCHK(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(ctx, e_ == hipErrorOutOfMemory ? VSIG_E_NOMEM : VSIG_E_HIP,          \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)

// The device table for `key`, built on first use: fill(h) appends its entries
// to a host vector (or returns a status), which is uploaded and kept for the
// context's lifetime.  A failed upload caches nothing.
template <class Fill>
int cached_table(vsig_ctx* c, TableKey key, const float2** out, Fill fill) {
  auto it = c->tables.find(key);
  if (it != c->tables.end()) { *out = it->second.as<float2>(); return VSIG_OK; }
  std::vector<float2> h;
  const int rc = fill(h);
  if (rc) return rc;
  DevBuf d;
  HIPCHK(c, d.alloc(h.size() * sizeof(float2)));
  HIPCHK(c, hipMemcpy(d.data(), h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
  *out = d.as<float2>();
  c->tables.emplace(key, std::move(d));
  return VSIG_OK;
}

float2 cis(double a) { return make_float2((float)std::cos(a), (float)std::sin(a)); }

// Twiddle table of the plan for N (see fft_engine.hpp):
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

// Two-level table for plan key N.
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

// W_M^t for t < T (the per-thread twiddle of the half-frame correlator; T is
// a function of M).
int get_half_tw(vsig_ctx* c, int M, int T, const float2** out) {
  return cached_table(c, {TableKind::HalfFrame, M}, out, [&](std::vector<float2>& h) {
    for (int t = 0; t < T; ++t) h.push_back(cis(-2.0 * M_PI * (double)t / (double)M));
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

// Host-pointer entry points: the operand into staging buffer i ...
int stage_in(vsig_ctx* c, int i, const void* host, size_t bytes) {
  const int rc = c->stage[i].reserve(c, bytes);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->stage[i].data(), host, bytes, hipMemcpyHostToDevice, c->stream));
  return VSIG_OK;
}
// ... and a result back from the device (the caller synchronises once).
int stage_out(vsig_ctx* c, void* host, const DevBuf& src, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(host, src.data(), bytes, hipMemcpyDeviceToHost, c->stream));
  return VSIG_OK;
}

// Event pair around one kernel launch (only when timing is on); with the
// clock option on, the stage's clock sink for the launches in its scope.
struct Timed {
  vsig_ctx* c;
  hipEvent_t b = nullptr, e = nullptr;
  const char* name;
  unsigned long long* prev_sink;
  hipStream_t st;
  Timed(vsig_ctx* c_, const char* n, hipStream_t s = nullptr)
      : c(c_), name(n), prev_sink(vsig::g_clock_sink), st(s ? s : c_->stream) {
    if (c->clock && c->clkbuf.data()) {
      auto it = c->clkslot.find(name);
      int slot = -1;
      if (it != c->clkslot.end()) slot = it->second;
      else if ((int)c->clkslot.size() < kClockSlots) slot = c->clkslot[name] = (int)c->clkslot.size();
      if (slot >= 0) vsig::g_clock_sink = c->clkbuf.as<unsigned long long>() + 2 * slot;
    }
    if (!c->timing) return;
    if (hipEventCreate(&b) != hipSuccess || hipEventCreate(&e) != hipSuccess) { b = e = nullptr; return; }
    (void)hipEventRecord(b, st);
  }
  ~Timed() {
    vsig::g_clock_sink = prev_sink;
    if (!b) return;
    (void)hipEventRecord(e, st);
    c->timers[name].ev.emplace_back(b, e);
  }
};

bool pow2_in(long long v, long long lo, long long hi) {
  return v >= lo && v <= hi && (v & (v - 1)) == 0;
}

// Overlap-save block sizes (measured best on MI355X for the chain's sizes).
int os_size_fir(int ntaps) {
  if (ntaps <= 256) return 1024;      // one-wave blocks; hop >= 769 (measured best at 255 taps)
  if (ntaps <= 512) return 4096;
  if (ntaps <= 2048) return 8192;
  if (ntaps <= 8192) return 16384;
  return 0;
}
// templates of 8193 .. 16384 samples use M = 32768 (measured slower than
// M = 16384 for shorter ones, xcorr.hip PlanX32k)
int os_size_xcorr(long long L) {
  if (L <= 1024) return 4096;
  if (L <= 2048) return 8192;
  if (L <= 8192) return 16384;
  if (L <= 16384) return 32768;
  return 0;
}

// FFT_M(zero-padded u[0..len)) / M into a new device buffer (natural order;
// M > 16384 by the four-step passes of bigfft.hip).
int big_plan_fwd(vsig_ctx* c, long long M, const float2* u, long long len, float2* S);
int make_spectrum(vsig_ctx* c, const float2* u_dev, int len, int M, DevBuf* out) {
  DevBuf S;
  HIPCHK(c, S.alloc((size_t)M * sizeof(float2)));
  if (M > 16384) {
    const int rc = big_plan_fwd(c, M, u_dev, len, S.as<float2>());
    if (rc) return rc;
  } else {
    const float2* tw;
    const int rc = get_twiddles(c, M, &tw);
    if (rc) return rc;
    hipError_t e = vsig::launch_spectrum_prep(M, u_dev, len, 1.0f / (float)M, S.as<float2>(), tw, c->stream);
    if (e != hipSuccess) return fail(c, VSIG_E_HIP, hipGetErrorString(e));
  }
  *out = std::move(S);
  return VSIG_OK;
}

// Where a peak record goes: the caller's device record, or the context's.
PeakPartial* peak_record(vsig_ctx* c, vsig_peak_t* peak_dev) {
  return peak_dev ? reinterpret_cast<PeakPartial*>(peak_dev) : c->result.as<PeakPartial>();
}

int finalize_peak(vsig_ctx* c, long long nparts, int sqrt_max, vsig_peak_t* peak_dev) {
  HIPCHK(c, vsig::launch_partial_finalize(c->parts(), nparts, sqrt_max, peak_record(c, peak_dev),
                                          c->finalize_tmp(), c->stream));
  return VSIG_OK;
}

// The refine scratch's header (vsig::RefineKeys), read back once the stream
// has drained.
int read_refine_keys(vsig_ctx* c, vsig::RefineKeys* keys) {
  HIPCHK(c, hipMemcpyAsync(keys, c->rscratch.data(), sizeof(*keys), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VSIG_OK;
}

// After a watchdog fire: zero the keys and the fused launch's counters (a fire
// can leave them inconsistent, and the next launch must start from zero),
// leave `fault` in the sticky fault word, and wait for the stream.
int clear_refine_fault(vsig_ctx* c, unsigned long long fault = 0) {
  char* keys = c->rscratch.as<char>();
  HIPCHK(c, hipMemsetAsync(keys, 0, sizeof(vsig::RefineKeys), c->stream));
  if (fault)
    HIPCHK(c, hipMemcpyAsync(keys + offsetof(vsig::RefineKeys, fault), &fault, sizeof(fault),
                             hipMemcpyHostToDevice, c->stream));
  if (c->parts())
    HIPCHK(c, hipMemsetAsync(c->counters(), 0, vsig::kCounterRecs * sizeof(PeakPartial), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));     // also: fault is a host local
  return VSIG_OK;
}

// np.correlate(a, v, mode): F, the start index into the 'full' correlation,
// and the output length (numeric.py); false for an unknown mode.
bool corr_span(int mode, long long na, long long nv, long long* F, long long* nout) {
  const long long nmin = na < nv ? na : nv, nmax = na < nv ? nv : na;
  if (mode == VSIG_MODE_FULL) { *F = 0; *nout = na + nv - 1; }
  else if (mode == VSIG_MODE_VALID) { *F = nmin - 1; *nout = nmax - nmin + 1; }
  else if (mode == VSIG_MODE_SAME) { *F = na >= nv ? nmin - 1 - nmin / 2 : nmin / 2; *nout = nmax; }
  else return false;
  return true;
}

bool is_complex_dtype(int dtype) { return dtype == VSIG_DTYPE_C64 || dtype == VSIG_DTYPE_C128; }

// Operands of the refine pass: np.correlate(a, v) in the final output
// space (o <-> full index F + o), complex128 or complex64 on the device.
struct RefineOperands {
  const void* a; long long na;
  const void* v; long long nv;
  int c128;
  long long F;
};

// Re-rank the peak record rec (finalized, max |c|) over the outputs within the
// fp32 band; src: the correlator's wave partials (geometry of an M-point
// launch with raw->final reversal rev) or, if c64 != null, a stored c64 array.
// fused: the correlator's partials are not finalized yet -- the refine's first
// launch finalizes them into rec and selects (thread columns when lkeys).
int run_refine(vsig_ctx* c, const RefineOperands& op, long long nout, int M, long long hop,
               long long nparts, int rev, const float2* c64, PeakPartial* rec, void* out128,
               bool fused = false, const unsigned* lkeys = nullptr, bool async = false,
               bool parity = false) {
  c->refine_ran = false;
  if (!c->refine) return fused ? fail(c, VSIG_E_INVALID, "refine: fused finalize with refine off")
                             : VSIG_OK;
  vsig::RefineArgs r{};
  r.a = op.a; r.na = op.na; r.v = op.v; r.nv = op.nv; r.c128 = op.c128;
  r.nout = nout; r.F = op.F; r.rev = rev;
  if (c64) {
    r.from_array = 1; r.c64 = c64; r.Q = 1; r.stride = 0; r.waves = 1; r.hop = 64;
    r.wstep = 64; r.rsub = 1;
  } else {
    vsig::XcorrGeom g;
    if (vsig::xcorr_geom(M, parity, &g) != hipSuccess)
      return fail(c, VSIG_E_INVALID, "refine: no correlator geometry for M");
    const int Q = g.Q;
    r.parts = c->parts(); r.nparts = nparts; r.hop = hop;
    r.waves = g.waves; r.Q = g.Q; r.stride = g.stride; r.wstep = g.wstep; r.rsub = g.rsub;
    r.lstep = g.lstep; r.rstep = g.rstep;
    if (fused) {
      r.finalize = 1;
      r.tmp = c->finalize_tmp();
      r.done = reinterpret_cast<unsigned long long*>(c->counters());
    }
    if (lkeys) {                 // items = thread columns of Q rows, one unit each
      r.cols = Q; r.lkeys = lkeys; r.Q = 1;
    }
  }
  r.eps = c->refine_eps_ppm * 1e-6;
  r.blas_threads = c->blas_threads;
  r.cap = c->refine_cap;
  r.wd_ticks = (unsigned long long)c->refine_wd_us * 100ull;   // s_memrealtime: 100 MHz
  const size_t need = vsig::refine_scratch_bytes(r);
  const bool fresh = need > c->rscratch.bytes();
  // a watchdog fire of an earlier pass whose status nobody read (device-tensor
  // callers) lives in the old scratch's sticky fault word: carry it into the
  // new one, so vsig_refine_status still reports 3 ("fired in some pass since
  // the last call"), and clear the fused launch's counters as that report
  // does (a fire can leave them inconsistent)
  unsigned long long pending_fault = 0;
  if (fresh && c->rscratch.data()) {
    vsig::RefineKeys keys;
    int rc = read_refine_keys(c, &keys);
    if (rc) return rc;
    pending_fault = keys.fault;
  }
  int rc = c->rscratch.reserve(c, need);
  if (rc) return rc;
  // a new scratch starts with zero keys (the sticky fault word is read by
  // vsig_refine_status; the finalize resets only the per-launch words)
  if (pending_fault) {
    if ((rc = clear_refine_fault(c, pending_fault))) return rc;
  } else if (fresh) {
    HIPCHK(c, hipMemsetAsync(c->rscratch.data(), 0, sizeof(vsig::RefineKeys), c->stream));
  }
  r.scratch = c->rscratch.data();
  r.rec = rec;
  r.out128 = out128;
  if (async && c->refine_async) {
    // on the refine stream behind the correlator; ev_ref marks its end
    vsig_ctx::RefineAsync& ra = c->ra;
    HIPCHK(c, hipEventRecord(ra.ev_corr, c->stream));
    HIPCHK(c, hipStreamWaitEvent(ra.stream, ra.ev_corr, 0));
    {
      Timed t(c, "refine", ra.stream);
      HIPCHK(c, vsig::launch_refine(r, ra.stream));
    }
    HIPCHK(c, hipEventRecord(ra.ev_ref, ra.stream));
    ra.pending = true;
    ra.joined = false;
    c->refine_ran = true;
    return VSIG_OK;
  }
  Timed t(c, "refine");
  HIPCHK(c, vsig::launch_refine(r, c->stream));
  c->refine_ran = true;
  return VSIG_OK;
}

// W_M^m for the four-step twiddles (bigfft.hip): two-level table
// A[i] = W_M^(i 2^S), B[j] = W_M^j, S = ceil(log2 M / 2), built in double.
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

constexpr long long kBigMax = 1LL << 28;    // largest four-step transform

// split_channels.py's frequency axis, as numpy forms it: fftfreq(n, 1/sr)[k]
// * sr + CENTER_FREQ (k >= 0 here, or -1), no contraction into FMAs.
#pragma clang fp contract(off)
double channel_freq(long long k, long long n, double sr, double center) {
  const double d = 1.0 / sr;
  const double val = 1.0 / ((double)n * d);
  const double f = (double)k * val;
  const double g = f * sr;
  return g + center;
}
#pragma clang fp contract(on)

// Twiddles of a (four-step) transform of M points.
struct BigPlan {
  long long M;
  int N1, N2, S, hiA;
  const float2 *tw1, *tw2, *t2;
};
int big_plan(vsig_ctx* c, long long M, BigPlan* p) {
  p->M = M;
  vsig::bigfft_split(M, &p->N1, &p->N2);
  int rc;
  p->tw1 = p->t2 = nullptr;
  p->S = p->hiA = 0;
  if ((rc = get_twiddles(c, p->N2, &p->tw2))) return rc;
  if (p->N1 > 1) {
    if ((rc = get_twiddles(c, p->N1, &p->tw1))) return rc;
    if ((rc = get_tw_big(c, M, &p->t2, &p->S, &p->hiA))) return rc;
  }
  return VSIG_OK;
}

// S = FFT_M(zero-padded u[0..len)) / M in natural order (four-step, M > 16384).
int big_plan_fwd(vsig_ctx* c, long long M, const float2* u, long long len, float2* S) {
  BigPlan bp;
  int rc = big_plan(c, M, &bp);
  if (rc) return rc;
  if ((rc = c->bigtmp.reserve(c, (size_t)M * sizeof(float2)))) return rc;
  float2* tmp = c->bigtmp.as<float2>();
  vsig::BigIn in{u, 0, 0, 1, len, nullptr, nullptr, 0, 1.0f / (float)M};
  HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, 1, in, tmp, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
  const vsig::BigOut o{S, 0, M, M, nullptr, 0, 1.0f};
  HIPCHK(c, vsig::launch_bf_row(3, bp.N1, bp.N2, 1, tmp, nullptr, bp.tw2, 1.0f, nullptr, 0, c->stream, &o));
  return VSIG_OK;
}

// Bluestein plan for length N: chirp c[N] and B = FFT_M(b) / M (permuted order
// for the four-step sizes), M = the power of two >= max(256, 2N - 1).
int chirp_plan(vsig_ctx* c, long long N, vsig_ctx::Chirp** out) {
  auto it = c->chirps.find(N);
  if (it != c->chirps.end()) { *out = &it->second; return VSIG_OK; }
  long long M = 256;
  while (M < 2 * N - 1) M *= 2;
  if (M > kBigMax) return fail(c, VSIG_E_UNSUPPORTED, "transform length above 2^27");
  BigPlan bp;
  int rc = big_plan(c, M, &bp);
  if (rc) return rc;
  DevBuf cv, Bk, b;      // b: the chirp filter before its transform, dropped on return
  if (cv.alloc(N * sizeof(float2)) != hipSuccess || Bk.alloc(M * sizeof(float2)) != hipSuccess ||
      b.alloc(M * sizeof(float2)) != hipSuccess)
    return fail(c, VSIG_E_NOMEM, "Bluestein plan allocation");
  float2* B = Bk.as<float2>();
  hipError_t e = vsig::launch_bf_chirp(N, M, cv.as<float2>(), b.as<float2>(), c->stream);
  vsig::BigIn in{b.data(), 0, 0, 1, M, nullptr, nullptr, 0, 1.0f / (float)M};
  if (e == hipSuccess) {
    if (bp.N1 == 1) {
      vsig::BigOut o{B, 0, 0, M, nullptr, 0, 1.0f};
      e = vsig::launch_bf_small(1, (int)M, 1, in, o, nullptr, bp.tw2, c->stream);
    } else {
      e = vsig::launch_bf_col(bp.N1, bp.N2, 1, in, B, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream);
      if (e == hipSuccess)
        e = vsig::launch_bf_row(1, bp.N1, bp.N2, 1, B, nullptr, bp.tw2, 1.0f, nullptr, 0, c->stream);
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, VSIG_E_HIP, hipGetErrorString(e));
  auto& ch = c->chirps[N];
  ch = vsig_ctx::Chirp{M, std::move(cv), std::move(Bk)};
  *out = &ch;
  return VSIG_OK;
}

// DFT of any length N (batch frames): X[k] = sum_n x[n] W_N^(nk), or the
// inverse (conj) form; in / out describe the operands (their chirp / conj
// fields are set here), out.scale includes any 1/N.
int dft_any(vsig_ctx* c, long long N, long long batch, vsig::BigIn in, vsig::BigOut out, bool inverse) {
  int rc;
  // a power of two with an in-LDS plan is its own transform: one N-point FFT
  // (inverse by conj) instead of two chirp products around a 2N-point
  // convolution, whose three transforms cost ~2.7e-7 of accuracy against ~1.3e-7
  if (N >= 256 && N <= 16384 && (N & (N - 1)) == 0) {
    const float2* tw;
    if ((rc = get_twiddles(c, (int)N, &tw))) return rc;
    in.conj = out.conj = inverse ? 1 : 0;
    in.nvalid = in.nvalid < N ? in.nvalid : N;
    HIPCHK(c, vsig::launch_bf_small(1, (int)N, batch, in, out, nullptr, tw, c->stream));
    return VSIG_OK;
  }
  // every other length up to 512 points (256 and 512 have gone above): the sum
  // itself, in double, one block per frame -- exact to the store's rounding,
  // where a chirp-z of M = 256 .. 1024 points put the engine's error in the
  // result three times (bigfft.hip: bf_direct_kernel)
  if (N <= vsig::kDirectMax) {
    in.conj = out.conj = inverse ? 1 : 0;
    in.nvalid = in.nvalid < N ? in.nvalid : N;
    HIPCHK(c, vsig::launch_bf_direct((int)N, batch, in, out, c->stream));
    return VSIG_OK;
  }
  // a longer power of two (up to 2^28) is one four-step transform of N points:
  // column pass, then the row pass storing natural order through `out` (inverse
  // by conj at the loads and the stores).  As a chirp-z it was three transforms
  // of 2N points: max-norm error 2.2 .. 6.9 x complex64 scipy's at 2^15 .. 2^21
  // against 0.6 .. 2.5 x for the single transform.
  if (N > 16384 && N <= kBigMax && (N & (N - 1)) == 0) {
    BigPlan bp;
    if ((rc = big_plan(c, N, &bp))) return rc;
    if ((rc = c->bigtmp.reserve(c, (size_t)(batch * N) * sizeof(float2)))) return rc;
    float2* tmp = c->bigtmp.as<float2>();
    in.conj = out.conj = inverse ? 1 : 0;
    in.nvalid = in.nvalid < N ? in.nvalid : N;
    HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, batch, in, tmp, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
    HIPCHK(c, vsig::launch_bf_row(3, bp.N1, bp.N2, batch, tmp, nullptr, bp.tw2, 1.0f, nullptr, 0, c->stream,
                                  &out));
    return VSIG_OK;
  }
  vsig_ctx::Chirp* ch;
  if ((rc = chirp_plan(c, N, &ch))) return rc;
  BigPlan bp;
  if ((rc = big_plan(c, ch->M, &bp))) return rc;
  const float2* B = ch->B.as<float2>();
  in.chirp = ch->c.as<float2>();
  in.conj = inverse ? 1 : 0;
  in.nvalid = in.nvalid < N ? in.nvalid : N;
  out.chirp = ch->c.as<float2>();
  out.conj = inverse ? 1 : 0;
  if (bp.N1 == 1) {
    HIPCHK(c, vsig::launch_bf_small(0, (int)ch->M, batch, in, out, B, bp.tw2, c->stream));
    return VSIG_OK;
  }
  if ((rc = c->bigtmp.reserve(c, (size_t)(batch * ch->M) * sizeof(float2)))) return rc;
  float2* tmp = c->bigtmp.as<float2>();
  HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, batch, in, tmp, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
  HIPCHK(c, vsig::launch_bf_row(0, bp.N1, bp.N2, batch, tmp, B, bp.tw2, 1.0f, nullptr, 0, c->stream));
  HIPCHK(c, vsig::launch_bf_icol(bp.N1, bp.N2, batch, tmp, out, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
  return VSIG_OK;
}

}  // namespace

int DevBuf::reserve(vsig_ctx* c, size_t bytes) {
  join_refine(c);
  if (bytes <= n_) return VSIG_OK;
  HIPCHK(c, alloc(bytes));
  return VSIG_OK;
}

extern "C" {

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
    for (auto& p : kv.second.ev) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
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
  int rc = read_refine_keys(c, &keys);
  if (rc) return rc;
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

#ifdef VSIG_TUNING
int vsig_fft_bench(vsig_ctx* c, int key, void* io, int frames, int iters, int twl) {
  if (!c || !io || frames < 1 || iters < 1) return fail(c, VSIG_E_INVALID, "bad arguments");
  const float2* tw;
  int rc = twl == 1 ? get_tw2(c, key, &tw) : get_twiddles(c, key, &tw);
  if (rc) return rc;
  Timed t(c, "fft_bench");
  HIPCHK(c, vsig::launch_fft_bench(key, (float2*)io, frames, iters, tw, twl, c->stream));
  return VSIG_OK;
}

int vsig_copy_bench(vsig_ctx* c, const void* x, int64_t n, void* y, int variant, int grid) {
  if (!c || !x || !y || n < 0) return fail(c, VSIG_E_INVALID, "bad arguments");
  Timed t(c, "copy_bench");
  HIPCHK(c, vsig::launch_copy_probe((const float2*)x, n, (float2*)y, variant, grid, c->stream));
  return VSIG_OK;
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
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VSIG_OK;
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
  for (auto& p : it->second.ev) {
    HIPCHK(c, hipEventSynchronize(p.second));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, p.first, p.second));
    *total_ms += ms;
    *launches += 1;
  }
  return VSIG_OK;
}

// ---------------------------------------------------------------- spectrum
int vsig_psd_c64_dev(vsig_ctx* c, const void* x, int64_t n, int64_t stride, const float* win,
                     int32_t nperseg, int64_t hop, int32_t nfft, float scale, int32_t shift,
                     float* sxx, int64_t nframes) {
  if (!c || !x || !win || !sxx) return fail(c, VSIG_E_INVALID, "null pointer");
  if (stride < 1) return fail(c, VSIG_E_INVALID, "stride must be >= 1");
  if (nperseg < 1 || nperseg > nfft || hop < 1 || n < nperseg)
    return fail(c, VSIG_E_INVALID, "need 1 <= nperseg <= nfft, hop >= 1, n >= nperseg");
  if (nframes != (n - nperseg) / hop + 1) return fail(c, VSIG_E_INVALID, "nframes mismatch");
  if (!pow2_in(nfft, 64, kBigMax)) {
    // any other length: a direct sum (<= 512 points) or Bluestein per frame
    // (bigfft.hip), |X|^2 stored by the transform's output stage; frames in
    // batches of <= 256 MB of scratch
    if (2LL * nfft - 1 > kBigMax) return fail(c, VSIG_E_UNSUPPORTED, "nfft above 2^27");
    int rc;
    long long fb = nframes;
    if (nfft > vsig::kDirectMax) {
      vsig_ctx::Chirp* ch;
      if ((rc = chirp_plan(c, nfft, &ch))) return rc;
      if (ch->M > 16384) fb = (256LL << 20) / (ch->M * 8);
    }
    if (fb < 1) fb = 1;
    Timed t(c, "psd");
    for (long long f0 = 0; f0 < nframes; f0 += fb) {
      const long long nb = nframes - f0 < fb ? nframes - f0 : fb;
      vsig::BigIn in{(const float2*)x + f0 * hop * stride, 0, hop * stride, stride, nperseg, nullptr,
                     win, 0, 1.0f};
      vsig::BigOut out{sxx + f0 * (long long)nfft, 4, nfft, nfft, nullptr, 0, scale, shift ? 1 : 0};
      if ((rc = dft_any(c, nfft, nb, in, out, false))) return rc;
    }
    return VSIG_OK;
  }
  if (nfft > 16384) {          // long frames: four-step FFT per frame (bigfft.hip)
    BigPlan bp;
    int rc = big_plan(c, nfft, &bp);
    if (rc) return rc;
    long long fb = (256LL << 20) / ((long long)nfft * 8);   // frames per 256 MB of scratch
    if (fb < 1) fb = 1;
    if (fb > nframes) fb = nframes;
    if ((rc = c->bigtmp.reserve(c, (size_t)(fb * nfft) * sizeof(float2)))) return rc;
    float2* tmp = c->bigtmp.as<float2>();
    Timed t(c, "psd");
    for (long long f0 = 0; f0 < nframes; f0 += fb) {
      const long long nb = nframes - f0 < fb ? nframes - f0 : fb;
      vsig::BigIn in{(const float2*)x + f0 * hop * stride, 0, hop * stride, stride, nperseg, nullptr,
                     win, 0, 1.0f};
      HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, nb, in, tmp, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
      HIPCHK(c, vsig::launch_bf_row(2, bp.N1, bp.N2, nb, tmp, nullptr, bp.tw2, scale, sxx + f0 * nfft,
                                    shift, c->stream));
    }
    return VSIG_OK;
  }
  const float2* tw;
  // pair kernel (>= 256 threads per frame): per-pass table; smaller plans: two-level table
  const bool pair = vsig::psd_plan_threads(nfft) >= 256;
  int rc = pair ? get_twiddles(c, nfft, &tw) : get_tw2(c, nfft, &tw);
  if (rc) return rc;
  Timed t(c, "psd");
  HIPCHK(c, vsig::launch_psd(nfft, (const float2*)x, stride, win, nperseg, hop, scale, sxx, nframes,
                             shift, tw, c->stream));
  return VSIG_OK;
}

int vsig_psd_c64(vsig_ctx* c, const void* x, int64_t n, const float* win, int32_t nperseg,
                 int64_t hop, int32_t nfft, float scale, int32_t shift, float* sxx,
                 int64_t nframes) {
  if (!c || !x || !win || !sxx) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < nperseg || nperseg < 1 || hop < 1) return fail(c, VSIG_E_INVALID, "bad sizes");
  const size_t bx = (size_t)n * 8, bw = (size_t)nperseg * 4, bo = (size_t)nframes * nfft * 4;
  int rc;
  if ((rc = stage_in(c, 0, x, bx)) || (rc = stage_in(c, 1, win, bw)) || (rc = c->stage[2].reserve(c, bo)))
    return rc;
  rc = vsig_psd_c64_dev(c, c->stage[0].data(), n, 1, c->stage[1].as<float>(), nperseg, hop, nfft, scale,
                        shift, c->stage[2].as<float>(), nframes);
  if (rc || (rc = stage_out(c, sxx, c->stage[2], bo))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- spectrum traces
int vsig_psd_traces_plan(int32_t nfft, int64_t nframes, int64_t* blocks, int64_t* frames_per_block_step,
                         int64_t* frames_per_block) {
  if (nfft < 1 || nframes < 1 || !blocks || !frames_per_block_step || !frames_per_block) return VSIG_E_INVALID;
  const vsig::PsdTracesPlan p = vsig::psd_traces_plan(nfft, nframes);
  if (p.blocks < 1) return VSIG_E_INVALID;
  *blocks = p.blocks;
  *frames_per_block_step = p.step;
  *frames_per_block = p.fpb;
  return VSIG_OK;
}

int vsig_psd_traces_c64_dev(vsig_ctx* c, const void* x, int64_t n, int64_t stride, const float* win,
                            int32_t nperseg, int64_t hop, int32_t nfft, float scale, int32_t shift,
                            int64_t nframes, double* mean_dev, float* max_dev, float* min_dev) {
  if (!c || !x || !win) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!mean_dev && !max_dev && !min_dev) return fail(c, VSIG_E_INVALID, "no output asked for");
  if (stride < 1) return fail(c, VSIG_E_INVALID, "stride must be >= 1");
  if (nperseg < 1 || nperseg > nfft || hop < 1 || n < nperseg)
    return fail(c, VSIG_E_INVALID, "need 1 <= nperseg <= nfft, hop >= 1, n >= nperseg");
  if (nframes != (n - nperseg) / hop + 1) return fail(c, VSIG_E_INVALID, "nframes mismatch");
  int rc;
  if (vsig::psd_traces_in_lds(nfft)) {
    // the transform kernels' epilogue reduces over the frames: one record row per block
    const vsig::PsdTracesPlan p = vsig::psd_traces_plan(nfft, nframes);
    if (p.blocks < 1) return fail(c, VSIG_E_INVALID, "no plan");
    if ((rc = c->ptscratch.reserve(c, (size_t)(p.blocks * nfft) * sizeof(vsig::PsdRec)))) return rc;
    const float2* tw;
    bool two_level;
    const int key = vsig::psd_traces_table(nfft, &two_level);
    if ((rc = two_level ? get_tw2(c, key, &tw) : get_twiddles(c, key, &tw))) return rc;
    vsig::PsdRec* rows = c->ptscratch.as<vsig::PsdRec>();
    Timed t(c, "psd_traces");
    HIPCHK(c, vsig::launch_psd_traces(nfft, (const float2*)x, stride, win, nperseg, hop, scale, nframes,
                                      shift, tw, rows, c->stream));
    HIPCHK(c, vsig::launch_psd_traces_merge(rows, p.blocks, nfft, nframes, mean_dev, max_dev, min_dev,
                                            c->stream));
    return VSIG_OK;
  }
  // every other length: vsig_psd_c64_dev's own route into a bounded batch of
  // stored frames (256 MB, or the "psd_traces_batch" option), each batch's
  // columns folded into the same record rows, then the same merge
  if (!pow2_in(nfft, 64, kBigMax) && 2LL * nfft - 1 > kBigMax)
    return fail(c, VSIG_E_UNSUPPORTED, "nfft above 2^27");
  long long fb = (256LL << 20) / ((long long)nfft * 4);
  if (c->psd_traces_batch > 0 && fb > c->psd_traces_batch) fb = c->psd_traces_batch;
  if (fb < 1) fb = 1;
  if (fb > nframes) fb = nframes;
  const size_t rb = ((size_t)vsig::kPsdFoldRows * nfft * sizeof(vsig::PsdRec) + 255) & ~(size_t)255;
  if ((rc = c->ptscratch.reserve(c, rb + (size_t)(fb * nfft) * sizeof(float)))) return rc;
  vsig::PsdRec* rows = c->ptscratch.as<vsig::PsdRec>();
  float* batch = reinterpret_cast<float*>(c->ptscratch.as<char>() + rb);
  for (long long f0 = 0; f0 < nframes; f0 += fb) {
    const long long nb = nframes - f0 < fb ? nframes - f0 : fb;
    if ((rc = vsig_psd_c64_dev(c, (const float2*)x + f0 * hop * stride, (nb - 1) * hop + nperseg, stride, win,
                               nperseg, hop, nfft, scale, shift, batch, nb)))
      return rc;
    HIPCHK(c, vsig::launch_psd_traces_fold(batch, nb, nfft, f0 == 0, rows, c->stream));
  }
  HIPCHK(c, vsig::launch_psd_traces_merge(rows, vsig::kPsdFoldRows, nfft, nframes, mean_dev, max_dev, min_dev,
                                          c->stream));
  return VSIG_OK;
}

int vsig_psd_traces_c64(vsig_ctx* c, const void* x, int64_t n, const float* win, int32_t nperseg,
                        int64_t hop, int32_t nfft, float scale, int32_t shift, int64_t nframes,
                        double* mean, float* max, float* min) {
  if (!c || !x || !win) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!mean && !max && !min) return fail(c, VSIG_E_INVALID, "no output asked for");
  if (n < nperseg || nperseg < 1 || hop < 1 || nfft < nperseg) return fail(c, VSIG_E_INVALID, "bad sizes");
  const size_t bx = (size_t)n * 8, bw = (size_t)nperseg * 4, bm = (size_t)nfft * 8, bf = (size_t)nfft * 4;
  int rc;
  if ((rc = stage_in(c, 0, x, bx)) || (rc = stage_in(c, 1, win, bw)) || (rc = c->stage[2].reserve(c, bm + 2 * bf)))
    return rc;
  char* o = c->stage[2].as<char>();
  double* dm = reinterpret_cast<double*>(o);
  float* dx = reinterpret_cast<float*>(o + bm);
  float* dn = reinterpret_cast<float*>(o + bm + bf);
  rc = vsig_psd_traces_c64_dev(c, c->stage[0].data(), n, 1, c->stage[1].as<float>(), nperseg, hop, nfft, scale,
                               shift, nframes, mean ? dm : nullptr, max ? dx : nullptr, min ? dn : nullptr);
  if (rc) return rc;
  if (mean) HIPCHK(c, hipMemcpyAsync(mean, dm, bm, hipMemcpyDeviceToHost, c->stream));
  if (max) HIPCHK(c, hipMemcpyAsync(max, dx, bf, hipMemcpyDeviceToHost, c->stream));
  if (min) HIPCHK(c, hipMemcpyAsync(min, dn, bf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- segmented spectrum traces
int vsig_psd_segments_create(vsig_ctx* c, const vsig_segment_t* segs, int64_t nseg, int64_t n, int32_t nperseg,
                             int64_t hop, int32_t nfft, vsig_psd_segments** out) {
  if (!c || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  if (nseg < 0 || nseg > (1LL << 24)) return fail(c, VSIG_E_INVALID, "nseg must be in [0, 2^24]");
  if (nseg > 0 && !segs) return fail(c, VSIG_E_INVALID, "null segment table");
  if (n < 1 || n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n must be in [1, 2^40]");
  if (nperseg < 1 || hop < 1) return fail(c, VSIG_E_INVALID, "need nperseg >= 1 and hop >= 1");
  if (nfft < nperseg) return fail(c, VSIG_E_INVALID, "nfft must be >= nperseg");
  for (long long s = 0; s < nseg; ++s) {
    const long long st = segs[s].start, ln = segs[s].len;
    if (st < 0 || ln < 0 || st > n || ln > n - st)
      return fail(c, VSIG_E_INVALID, "segment " + std::to_string(s) + " {start " + std::to_string(st) + ", len " +
                                         std::to_string(ln) + "} is outside [0, " + std::to_string(n) + "]");
  }
  if (!vsig::psd_traces_in_lds(nfft))
    return fail(c, VSIG_E_UNSUPPORTED, "segmented traces: nfft " + std::to_string(nfft) +
                                           " is not a power of two in [64, 8192]");
  int step = 0;
  long long maxb = 0;
  if (vsig::psd_segments_geom(nfft, &step, &maxb) != hipSuccess) return fail(c, VSIG_E_UNSUPPORTED, "no plan");
  std::unique_ptr<vsig_psd_segments> p(new vsig_psd_segments(c));
  p->nseg = nseg; p->n = n; p->nperseg = nperseg; p->hop = hop; p->nfft = nfft; p->step = step;
  // runs of `run` frames: enough steps per block that the blocks fill the
  // device once, and kTracesMinUnits at least; a segment's blocks (its record
  // rows) are consecutive
  std::vector<vsig::PsdSegRows> rows((size_t)nseg);
  long long units = 0;
  for (long long s = 0; s < nseg; ++s) {
    const long long nf = segs[s].len >= nperseg ? (segs[s].len - nperseg) / hop + 1 : 0;
    rows[s].nframes = nf;
    p->frames_total += nf;
    units += (nf + step - 1) / step;
  }
  long long upb = (units + maxb - 1) / maxb;
  if (upb < vsig::kTracesMinUnits) upb = vsig::kTracesMinUnits;
  p->run = upb * step;
  std::vector<vsig::PsdSegBlock> blocks;
  for (long long s = 0; s < nseg; ++s) {
    rows[s].r0 = (long long)blocks.size();
    for (long long f0 = 0; f0 < rows[s].nframes; f0 += p->run) {
      const long long left = rows[s].nframes - f0;
      blocks.push_back({segs[s].start + f0 * hop, left < p->run ? left : p->run});
    }
    rows[s].r1 = (long long)blocks.size();
    if (rows[s].r1 - rows[s].r0 > p->max_rows) p->max_rows = rows[s].r1 - rows[s].r0;
  }
  p->nblocks = (long long)blocks.size();
  if (p->nblocks > 0x7fffffffLL) return fail(c, VSIG_E_UNSUPPORTED, "more than 2^31 - 1 blocks");
  if (nseg > 0) {
    bool two_level;
    const int key = vsig::psd_traces_table(nfft, &two_level);
    int rc;
    if ((rc = two_level ? get_tw2(c, key, &p->tw) : get_twiddles(c, key, &p->tw))) return rc;
    HIPCHK(c, p->segs.alloc(rows.size() * sizeof(vsig::PsdSegRows)));
    HIPCHK(c, hipMemcpyAsync(p->segs.data(), rows.data(), rows.size() * sizeof(vsig::PsdSegRows),
                             hipMemcpyHostToDevice, c->stream));
    if (p->nblocks > 0) {
      HIPCHK(c, p->blocks.alloc(blocks.size() * sizeof(vsig::PsdSegBlock)));
      HIPCHK(c, hipMemcpyAsync(p->blocks.data(), blocks.data(), blocks.size() * sizeof(vsig::PsdSegBlock),
                               hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, p->rows.alloc((size_t)p->nblocks * (size_t)nfft * sizeof(vsig::PsdRec)));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the host tables go out of scope
  }
  *out = p.release();
  return VSIG_OK;
}

void vsig_psd_segments_free(vsig_psd_segments* p) { delete p; }

int vsig_psd_segments_info(const vsig_psd_segments* p, int64_t* frames_total, int64_t* blocks,
                           int64_t* frames_per_step, int64_t* max_run_frames) {
  if (!p) return VSIG_E_INVALID;
  if (!frames_total || !blocks || !frames_per_step || !max_run_frames)
    return fail(p->ctx, VSIG_E_INVALID, "null pointer");
  *frames_total = p->frames_total; *blocks = p->nblocks; *frames_per_step = p->step; *max_run_frames = p->run;
  return VSIG_OK;
}

int vsig_psd_segments_run(vsig_psd_segments* p, const void* x, const float* win, float scale, int32_t shift,
                          double* mean, float* max, float* min) {
  if (!p) return VSIG_E_INVALID;
  vsig_ctx* c = p->ctx;
  if (!x || !win) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!mean && !max && !min) return fail(c, VSIG_E_INVALID, "no output asked for");
  if (reinterpret_cast<uintptr_t>(x) & 7) return fail(c, VSIG_E_INVALID, "x must be 8-byte aligned");
  if (p->nseg == 0) return VSIG_OK;
  Timed t(c, "psd_segments");
  if (p->nblocks > 0)
    HIPCHK(c, vsig::launch_psd_segments(p->nfft, (const float2*)x, win, p->nperseg, p->hop, scale, shift ? 1 : 0,
                                        p->tw, p->blocks.as<vsig::PsdSegBlock>(), p->nblocks,
                                        p->rows.as<vsig::PsdRec>(), c->stream));
  HIPCHK(c, vsig::launch_psd_segments_merge(p->rows.as<vsig::PsdRec>(), p->segs.as<vsig::PsdSegRows>(), p->nseg,
                                            p->nfft, p->max_rows, mean, max, min, c->stream));
  return VSIG_OK;
}

int vsig_band_measure_run(vsig_ctx* c, const double* rows, int64_t nrows, int32_t nbins, int64_t ld, double tail,
                          vsig_band_t* out) {
  static_assert(sizeof(vsig_band_t) == sizeof(vsig::BandRec) && sizeof(vsig_band_t) == 40, "vsig_band_t");
  if (!c) return VSIG_E_INVALID;
  if (nrows < 0 || nrows > 0x7fffffffLL) return fail(c, VSIG_E_INVALID, "nrows must be in [0, 2^31)");
  if (nbins < 1 || ld < nbins) return fail(c, VSIG_E_INVALID, "need nbins >= 1 and ld >= nbins");
  if (!(tail > 0.0 && tail < 0.5)) return fail(c, VSIG_E_INVALID, "tail must be inside (0, 0.5)");
  if (!rows || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  if ((reinterpret_cast<uintptr_t>(rows) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
    return fail(c, VSIG_E_INVALID, "rows and out must be 8-byte aligned");
  if (nrows == 0) return VSIG_OK;
  Timed t(c, "band_measure");
  HIPCHK(c, vsig::launch_band_measure(rows, nrows, nbins, ld, tail, reinterpret_cast<vsig::BandRec*>(out),
                                      c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- burst isolation
int vsig_isolate_create(vsig_ctx* c, const vsig_isolate_seg_t* segs, int64_t nseg, int64_t n, const float* taps,
                        int32_t nfilters, int32_t ntaps, double sr, vsig_isolate** out) {
  static_assert(sizeof(vsig_isolate_seg_t) == 32 && sizeof(vsig::IsoFrame) == 32, "table records");
  constexpr int M = vsig::kIsoM;
  if (!c || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  if (nseg < 0 || nseg > (1LL << 24)) return fail(c, VSIG_E_INVALID, "nseg must be in [0, 2^24]");
  if (nseg > 0 && !segs) return fail(c, VSIG_E_INVALID, "null segment table");
  if (n < 1 || n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n must be in [1, 2^40]");
  if (!taps) return fail(c, VSIG_E_INVALID, "null taps");
  if (nfilters < 1 || nfilters > kIsoMaxFilters)
    return fail(c, VSIG_E_INVALID, "nfilters must be in [1, " + std::to_string(kIsoMaxFilters) + "]");
  if (ntaps < 3 || ntaps % 2 == 0) return fail(c, VSIG_E_INVALID, "ntaps must be odd and >= 3");
  if (ntaps > kIsoMaxTaps)
    return fail(c, VSIG_E_UNSUPPORTED, "isolate: ntaps " + std::to_string(ntaps) + " is above " +
                                           std::to_string(kIsoMaxTaps));
  if (!(sr > 0.0) || !std::isfinite(sr)) return fail(c, VSIG_E_INVALID, "sr must be finite and > 0");
  for (long long i = 0; i < (long long)nfilters * ntaps; ++i)
    if (!std::isfinite(taps[i])) return fail(c, VSIG_E_INVALID, "tap " + std::to_string(i) + " is not finite");
  for (long long s = 0; s < nseg; ++s) {
    const long long st = segs[s].start, ln = segs[s].len;
    if (st < 0 || ln < 1 || st >= n || ln > n - st)
      return fail(c, VSIG_E_INVALID, "segment " + std::to_string(s) + " {start " + std::to_string(st) + ", len " +
                                         std::to_string(ln) + "} is empty or outside [0, " + std::to_string(n) + ")");
    if (segs[s].filter < 0 || segs[s].filter >= nfilters)
      return fail(c, VSIG_E_INVALID, "segment " + std::to_string(s) + ": filter " + std::to_string(segs[s].filter) +
                                         " is outside [0, " + std::to_string(nfilters) + ")");
    if (!std::isfinite(segs[s].freq))
      return fail(c, VSIG_E_INVALID, "segment " + std::to_string(s) + ": freq is not finite");
  }
  std::unique_ptr<vsig_isolate> p(new vsig_isolate(c));
  p->nseg = nseg; p->n = n; p->lo = ntaps - 1; p->hop = M - p->lo;
  const long long d = (ntaps - 1) / 2;
  // segment s: frames k < ceil(len / hop), frame k owns the outputs [k hop, k hop + keep)
  p->offsets.assign((size_t)nseg + 1, 0);
  std::vector<vsig::IsoFrame> frames;
  for (long long s = 0; s < nseg; ++s) {
    const double wsr = (2.0 * M_PI) * -segs[s].freq / sr;       // vsig_fir_exec_mix_dev's w / sr
    for (long long o = 0; o < segs[s].len; o += p->hop) {
      const long long left = segs[s].len - o;
      frames.push_back({segs[s].start + o + d - p->lo, p->offsets[s] + o, wsr,
                        (int)(left < p->hop ? left : p->hop), segs[s].filter});
    }
    p->offsets[s + 1] = p->offsets[s] + segs[s].len;
  }
  p->nframes = (long long)frames.size();
  if ((p->nframes + 1) / 2 > 0x7fffffffLL) return fail(c, VSIG_E_UNSUPPORTED, "more than 2^31 - 1 blocks");
  if (nseg > 0) {
    int rc;
    const float2* twp;
    if ((rc = get_twiddles(c, -M, &p->tw)) || (rc = get_twiddles(c, M, &twp))) return rc;
    // Hs row f = FFT_M(h_f) / M, as vsig_fir_create builds its one
    std::vector<float2> hc((size_t)nfilters * ntaps);
    for (size_t i = 0; i < hc.size(); ++i) hc[i] = make_float2(taps[i], 0.f);
    DevBuf hd;                     // the taps on the device, dropped on return
    HIPCHK(c, hd.alloc(hc.size() * sizeof(float2)));
    HIPCHK(c, p->Hs.alloc((size_t)nfilters * M * sizeof(float2)));
    HIPCHK(c, p->frames.alloc(frames.size() * sizeof(vsig::IsoFrame)));
    HIPCHK(c, hipMemcpyAsync(hd.data(), hc.data(), hc.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p->frames.data(), frames.data(), frames.size() * sizeof(vsig::IsoFrame),
                             hipMemcpyHostToDevice, c->stream));
    hipError_t e = hipSuccess;
    for (int f = 0; f < nfilters && e == hipSuccess; ++f)
      e = vsig::launch_spectrum_prep(M, hd.as<float2>() + (size_t)f * ntaps, ntaps, 1.0f / (float)M,
                                     p->Hs.as<float2>() + (size_t)f * M, twp, c->stream);
    (void)hipStreamSynchronize(c->stream);           // hd and the host tables go out of scope
    if (e != hipSuccess) return fail(c, VSIG_E_HIP, hipGetErrorString(e));
  }
  *out = p.release();
  return VSIG_OK;
}

void vsig_isolate_free(vsig_isolate* p) { delete p; }

int vsig_isolate_info(const vsig_isolate* p, int64_t* out_total, int64_t* frames, int64_t* blocks, int64_t* hop) {
  if (!p) return VSIG_E_INVALID;
  if (!out_total || !frames || !blocks || !hop) return fail(p->ctx, VSIG_E_INVALID, "null pointer");
  *out_total = p->offsets.back(); *frames = p->nframes; *blocks = (p->nframes + 1) / 2; *hop = p->hop;
  return VSIG_OK;
}

int vsig_isolate_offsets(const vsig_isolate* p, int64_t* offsets) {
  if (!p) return VSIG_E_INVALID;
  if (!offsets) return fail(p->ctx, VSIG_E_INVALID, "null pointer");
  for (size_t s = 0; s < p->offsets.size(); ++s) offsets[s] = p->offsets[s];
  return VSIG_OK;
}

int vsig_isolate_run(vsig_isolate* p, const void* x, void* y) {
  if (!p) return VSIG_E_INVALID;
  vsig_ctx* c = p->ctx;
  if (!x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if ((reinterpret_cast<uintptr_t>(x) & 7) || (reinterpret_cast<uintptr_t>(y) & 7))
    return fail(c, VSIG_E_INVALID, "x and y must be 8-byte aligned");
  if (p->nseg == 0) return VSIG_OK;
  Timed t(c, "isolate");
  HIPCHK(c, vsig::launch_isolate((const float2*)x, p->n, p->Hs.as<float2>(), p->lo, (float2*)y,
                                 p->frames.as<vsig::IsoFrame>(), p->nframes, p->tw, c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- FIR
int vsig_fir_create(vsig_ctx* c, const void* taps, int32_t ntaps, int32_t decim, vsig_fir** out) {
  if (!c || !taps || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  if (ntaps < 1 || decim < 1) return fail(c, VSIG_E_INVALID, "ntaps and decim must be >= 1");
  if (ntaps > kFirPartTaps) {        // np.convolve has no length limit: parts
    std::unique_ptr<vsig_fir> f(new vsig_fir{c, ntaps, decim, 0, 0});
    for (int j = 0; j * kFirPartTaps < ntaps; ++j) {
      const int nt = ntaps - j * kFirPartTaps < kFirPartTaps ? ntaps - j * kFirPartTaps : kFirPartTaps;
      vsig_fir* p = nullptr;
      const int rc = vsig_fir_create(c, static_cast<const float2*>(taps) + (size_t)j * kFirPartTaps, nt, 1, &p);
      if (rc) return rc;
      f->parts.push_back(p);
    }
    f->M = f->parts[0]->M;
    *out = f.release();
    return VSIG_OK;
  }
  const int M = os_size_fir(ntaps);
  if (!M) return fail(c, VSIG_E_UNSUPPORTED, "no block size for ntaps");
  long long hop = ((long long)M - (ntaps - 1)) / decim * decim;
  if (hop < 1) return fail(c, VSIG_E_UNSUPPORTED, "decim too large for the block size");
  // 1024-point pairs at hop 768 (ntaps 225..257): the second segment's first
  // quarter comes from the first one's registers (load_pair_x4), 14 loads per
  // pair instead of 16 for <= 4 % more segments (0.84 -> 0.80 ms at config 2,
  // profiles/r03_pl1_ab.txt)
  if (M == 1024 && decim == 1 && hop > 768 && hop < 800) hop = 768;
  DevBuf hd, Hs, G;      // hd: the taps on the device, dropped on return
  HIPCHK(c, hd.alloc((size_t)ntaps * sizeof(float2)));
  hipError_t e = hipMemcpyAsync(hd.data(), taps, (size_t)ntaps * sizeof(float2), hipMemcpyHostToDevice,
                                c->stream);
  if (e != hipSuccess) return fail(c, VSIG_E_HIP, hipGetErrorString(e));
  int rc = make_spectrum(c, hd.as<float2>(), ntaps, M, &Hs);
  if (!rc && M == 1024 && decim == 4) {
    hipError_t ge = G.alloc(1024 * sizeof(float2));
    if (ge == hipSuccess) ge = vsig::launch_fir_poly_gtable(Hs.as<float2>(), G.as<float2>(), c->stream);
    if (ge != hipSuccess) rc = fail(c, VSIG_E_HIP, hipGetErrorString(ge));
  }
  (void)hipStreamSynchronize(c->stream);     // hd and the caller's taps are free to go
  if (rc) return rc;
  *out = new vsig_fir{c, ntaps, decim, M, hop, std::move(Hs), std::move(G)};
  return VSIG_OK;
}

void vsig_fir_free(vsig_fir* f) { delete f; }

static int fir_exec(vsig_fir* f, const void* x, int64_t nhist, int64_t n, void* y, int64_t ny,
                    const vsig::MixArgs* mix) {
  if (!f) return VSIG_E_INVALID;
  vsig_ctx* c = f->ctx;
  if (!x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1 || nhist < 0) return fail(c, VSIG_E_INVALID, "need n >= 1 and nhist >= 0");
  if (ny != (n + f->decim - 1) / f->decim) return fail(c, VSIG_E_INVALID, "ny != ceil(n/decim)");
  const float2* tw;
  int rc;
  if (!f->parts.empty()) {
    if (mix) return fail(c, VSIG_E_UNSUPPORTED, "fused mixer needs ntaps <= 256 (mix first)");
    const long long nz = nhist + n;
    if ((rc = f->z.reserve(c, (size_t)nz * sizeof(float2)))) return rc;
    float2* z = f->z.as<float2>();
    for (size_t j = 0; j < f->parts.size(); ++j) {
      if ((rc = fir_exec(f->parts[j], x, 0, nz, z, nz, nullptr))) return rc;
      Timed t(c, "fir");
      HIPCHK(c, vsig::launch_fir_part_accum(z, nz, nhist - (long long)j * kFirPartTaps, f->decim, ny,
                                            j == 0, (float2*)y, c->stream));
    }
    return VSIG_OK;
  }
  if (f->M == 1024 && (f->decim == 2 || f->decim == 4)) {
    // decimation in the frequency domain: M/D-point inverse transforms
    const float2* twd;
    const int D = f->decim;
    int lo2 = (f->ntaps - 1 + D - 1) / D * D;
    // a multiple of 16 when the block allows (as fir_os_kernel's lo): the
    // decimated output runs (64 per store instruction) then start on 128-byte
    // lines, and so do the segments of a 16-multiple history (the chain's)
    if (((lo2 + 15) & ~15) + 768 <= f->M) lo2 = (lo2 + 15) & ~15;
    const long long hop = (long long)(f->M - lo2) / D * D;
    if (hop < D) return fail(c, VSIG_E_UNSUPPORTED, "decim too large for the block size");
    if (f->G.data()) {      // D = 4: polyphase form (fir_poly_kernel)
      if ((rc = get_twiddles(c, 256, &tw)) || (rc = get_twiddles(c, -256, &twd))) return rc;
      Timed t(c, "fir");
      HIPCHK(c, vsig::launch_fir_poly((const float2*)x, nhist + n, nhist, f->G.as<float2>(), lo2, hop,
                                      (float2*)y, tw, twd, c->stream, mix));
      return VSIG_OK;
    }
    if ((rc = get_twiddles(c, -1024, &tw)) || (rc = get_twiddles(c, -1024 / f->decim, &twd))) return rc;
    Timed t(c, "fir");
    HIPCHK(c, vsig::launch_fir_dec(D, (const float2*)x, nhist + n, nhist, f->Hs.as<float2>(), lo2, hop,
                                   (float2*)y, tw, twd, c->stream, mix));
    return VSIG_OK;
  }
  if (mix && f->M != 1024)
    return fail(c, VSIG_E_UNSUPPORTED, "fused mixer needs the 1024-point block (ntaps <= 256)");
  rc = get_twiddles(c, f->M == 1024 ? -1024 : f->M, &tw);
  if (rc) return rc;
  Timed t(c, "fir");
  HIPCHK(c, vsig::launch_fir_os(f->M, (const float2*)x, nhist + n, nhist, f->Hs.as<float2>(), f->ntaps,
                                f->hop, f->decim, (float2*)y, tw, c->stream, mix));
  return VSIG_OK;
}

int vsig_fir_block(const vsig_fir* f) { return f ? f->M : 0; }

int vsig_fir_exec_hist_dev(vsig_fir* f, const void* x, int64_t nhist, int64_t n, void* y,
                           int64_t ny) {
  return fir_exec(f, x, nhist, n, y, ny, nullptr);
}

int vsig_fir_exec_mix_dev(vsig_fir* f, const void* x, int64_t nhist, int64_t n, void* y, int64_t ny,
                          double freq_shift, double sample_rate, int64_t i0) {
  if (!f) return VSIG_E_INVALID;
  if (freq_shift == 0.0) return fir_exec(f, x, nhist, n, y, ny, nullptr);   // utils.py:122-123
  if (!(sample_rate != 0.0)) return fail(f->ctx, VSIG_E_INVALID, "sample_rate must be non-zero");
  const double w = (2.0 * M_PI) * freq_shift;
  vsig::MixArgs m{};
  m.w = w;
  m.sr = sample_rate;
  m.i0 = (long long)i0;
  m.wsr = w / sample_rate;
  for (int e = 0; e < 16; ++e) {       // exp(j wsr 64 e), reduced mod 2 pi in double
    const double a = std::remainder(m.wsr * 64.0 * e, 2.0 * M_PI);
    m.rot[2 * e] = (float)std::cos(a);
    m.rot[2 * e + 1] = (float)std::sin(a);
  }
  return fir_exec(f, x, nhist, n, y, ny, &m);
}

int vsig_fir_exec_dev(vsig_fir* f, const void* x, int64_t n, void* y, int64_t ny) {
  return vsig_fir_exec_hist_dev(f, x, 0, n, y, ny);
}

int vsig_fir_c64(vsig_ctx* c, const void* x, int64_t n, const float* taps, int32_t ntaps,
                 int32_t decim, void* y, int64_t ny) {
  if (!c || !x || !taps || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (ntaps < 1) return fail(c, VSIG_E_INVALID, "ntaps must be >= 1");
  std::vector<float2> tc(ntaps);
  for (int i = 0; i < ntaps; ++i) tc[i] = make_float2(taps[i], 0.f);
  vsig_fir* f = nullptr;
  int rc = vsig_fir_create(c, tc.data(), ntaps, decim, &f);
  if (rc) return rc;
  const std::unique_ptr<vsig_fir> owner(f);     // freed on every path below
  const size_t bx = (size_t)n * 8, by = (size_t)ny * 8;
  if ((rc = stage_in(c, 0, x, bx)) || (rc = c->stage[1].reserve(c, by)) ||
      (rc = vsig_fir_exec_dev(f, c->stage[0].data(), n, c->stage[1].data(), ny)) ||
      (rc = stage_out(c, y, c->stage[1], by)))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- correlation
// Template spectra from a device c64 template of L samples: L <= 8192 one
// M-point spectrum; longer templates one M = 16384 spectrum per 8192-sample
// chunk (sum of passes, see xcorr_run).
static int xcorr_build(vsig_ctx* c, const float2* td, long long L, vsig_xcorr* x) {
  constexpr long long B = 8192;
  x->L = L;
  x->M = os_size_xcorr(L) ? os_size_xcorr(L) : 16384;
  const long long Bc = x->M == 32768 ? 16384 : B;    // one pass up to 16384 at M = 32768
  for (long long p = 0; p * Bc < L || p == 0; ++p) {
    const long long Lp = L <= Bc ? L : ((L - p * Bc) < B ? (L - p * Bc) : B);
    DevBuf P;
    const int rc = make_spectrum(c, td + p * B, (int)Lp, x->M, &P);
    if (rc) return rc;
    x->Ps.push_back(std::move(P));
    if (L <= Bc) break;
  }
  if (x->M == 16384 && x->Ps.size() == 1) {     // the parity split's (S, D) table
    HIPCHK(c, x->SD.alloc((size_t)(x->M / 2) * sizeof(float4)));
    HIPCHK(c, vsig::launch_xcorr_parity_table(x->M, x->Ps[0].as<float2>(), x->SD.as<float4>(), c->stream));
  }
  return VSIG_OK;
}

// The correlation c[o] = sum_k s[o - off + k] conj(p[k]) of the handle's
// template over the c64 stream s, o < nout, stored per store_mode bits 0-2
// into cout (c64, may be null), the peak record into rec, then refined with
// op (see run_refine; out128: complex128 c to patch).  Templates longer than
// 8192: the chunks' passes accumulate in c (store bit 8; a scratch kept with
// the handle when cout is null), then one fp64 peak reduction over c and the
// refine from the stored array.
static int xcorr_run(vsig_xcorr* x, const float2* s, long long n, long long off, long long nout,
                     int store_mode, float2* cout, vsig_peak_t* peak_dev,
                     const RefineOperands* op, void* out128, bool async = false) {
  vsig_ctx* c = x->ctx;
  PeakPartial* rec = peak_record(c, peak_dev);
  if (x->Ps.size() == 1 && x->L <= (x->M == 32768 ? 16384 : 8192)) {
    // outputs per block: M - L + 1, rounded down to even at M = 16384 (every
    // segment start then has one parity: the correlator's 16-byte loads)
    long long hop = (long long)x->M - x->L + 1;
    if (x->M == 16384 && hop > 1) hop &= ~1LL;
    const long long nblocks = (nout + hop - 1) / hop;
    // the parity split wherever the segments start 16-byte aligned (else the
    // split by halves, on the natural-order spectrum)
    const bool parity = x->M == 16384 && x->SD.data() && !(hop & 1) && vsig::xcorr_parity_aligned(s, off);
    vsig::XcorrGeom g;
    if (vsig::xcorr_geom(x->M, parity, &g) != hipSuccess)
      return fail(c, VSIG_E_UNSUPPORTED, "correlator block size");
    const int waves = g.waves, Q = g.Q, plan = g.plan;
    const long long nparts = nblocks * waves;   // one partial per wave
    int rc = ensure_partials(c, nparts);
    if (rc) return rc;
    // with the refine on, the partials' finalize and the candidate select run
    // as the refine's first launch, on thread columns where the kernel writes
    // lane keys (64x fewer outputs re-ranked than whole waves)
    const bool fused = op && c->refine && !(store_mode & 8);
    unsigned* lk = nullptr;
    if (fused && Q <= 64 && vsig::xcorr_lane_keys(x->M) == Q) {
      if ((rc = c->lkeys.reserve(c, (size_t)nparts * 64 * sizeof(unsigned)))) return rc;
      lk = c->lkeys.as<unsigned>();
    }
    const float2* tw;
    const float2* wt = nullptr;
    if ((rc = get_twiddles(c, plan, &tw))) return rc;
    if (x->M >= 16384 && (rc = get_half_tw(c, x->M, x->M == 16384 ? 512 : 1024, &wt))) return rc;
    {
      Timed t(c, "xcorr");
      HIPCHK(c, vsig::launch_xcorr_os(x->M, s, n, x->Ps[0].as<float2>(), off, nout, hop, cout, store_mode,
                                      c->parts(), tw, wt, c->stream, lk,
                                      parity ? x->SD.as<float4>() : nullptr));
    }
    if (!fused) {
      if ((rc = finalize_peak(c, nparts, 1, peak_dev))) return rc;
      if (!op) return VSIG_OK;
    }
    if (out128 && cout) HIPCHK(c, vsig::launch_convert_c(1, cout, nout, out128, c->stream));
    return run_refine(c, *op, nout, x->M, hop, nparts, (store_mode & 4) ? 1 : 0, nullptr, rec, out128,
                      fused, lk, async && peak_dev != nullptr, parity);
  }
  constexpr long long B = 8192;
  constexpr int M = 16384;
  float2* cbuf = cout;
  int rc;
  if (!cbuf) {
    if ((rc = x->cbuf.reserve(c, (size_t)nout * sizeof(float2)))) return rc;
    cbuf = x->cbuf.as<float2>();
  }
  const float2 *tw, *wt;
  vsig::XcorrGeom g;
  if (vsig::xcorr_geom(M, false, &g) != hipSuccess)
    return fail(c, VSIG_E_UNSUPPORTED, "correlator block size");
  if ((rc = get_twiddles(c, g.plan, &tw)) || (rc = get_half_tw(c, M, 512, &wt))) return rc;
  {
    Timed t(c, "xcorr");            // the whole chunked correlation + its peak pass
    for (size_t p = 0; p < x->Ps.size(); ++p) {
      const long long Lp = (x->L - (long long)p * B) < B ? (x->L - (long long)p * B) : B;
      const int mode = (store_mode & 4 ? 2 | 4 : 1) | (p ? 8 : 0);
      HIPCHK(c, vsig::launch_xcorr_os(M, s, n, x->Ps[p].as<float2>(), off - (long long)p * B, nout,
                                      (long long)M - Lp + 1, cbuf, mode, nullptr, tw, wt,
                                      c->stream));
    }
    if ((rc = vsig_peak_dev(c, VSIG_DTYPE_C64, cbuf, nout, peak_dev))) return rc;
  }
  if (!op) return VSIG_OK;
  if (out128 && cout) HIPCHK(c, vsig::launch_convert_c(1, cout, nout, out128, c->stream));
  return run_refine(c, *op, nout, M, 0, 0, 0, cbuf, rec, out128);
}

int vsig_xcorr_create(vsig_ctx* c, const void* tmpl, int64_t L, vsig_xcorr** out) {
  if (!c || !tmpl || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  if (L < 1) return fail(c, VSIG_E_INVALID, "template length must be >= 1");
  std::unique_ptr<vsig_xcorr> x(new vsig_xcorr(c));
  hipError_t e = x->tmpl.alloc((size_t)L * sizeof(float2));
  if (e == hipSuccess)
    e = hipMemcpyAsync(x->tmpl.data(), tmpl, (size_t)L * sizeof(float2), hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess)
    return fail(c, e == hipErrorOutOfMemory ? VSIG_E_NOMEM : VSIG_E_HIP, hipGetErrorString(e));
  const int rc = xcorr_build(c, x->tmpl.as<float2>(), L, x.get());
  (void)hipStreamSynchronize(c->stream);     // the caller's template is free to go
  if (rc) return rc;
  *out = x.release();
  return VSIG_OK;
}

void vsig_xcorr_free(vsig_xcorr* x) { delete x; }

int vsig_xcorr_exec_dev(vsig_xcorr* x, const void* s, int64_t n, int32_t mode, void* cout,
                        vsig_peak_t* peak_dev) {
  if (!x) return VSIG_E_INVALID;
  vsig_ctx* c = x->ctx;
  if (!s) return fail(c, VSIG_E_INVALID, "null pointer");
  long long off, nout;
  if (mode == VSIG_MODE_VALID) { off = 0; nout = n - x->L + 1; }
  else if (mode == VSIG_MODE_FULL) { off = x->L - 1; nout = n + x->L - 1; }
  else return fail(c, VSIG_E_INVALID, "streaming correlation supports VALID and FULL");
  if (nout < 1) return fail(c, VSIG_E_INVALID, "stream shorter than the template");
  // np.correlate(s, p): output o is full index (L - 1 - off) + o
  const RefineOperands op{s, n, x->tmpl.data(), x->L, 0, (x->L - 1) - off};
  return xcorr_run(x, (const float2*)s, n, off, nout, cout ? 1 : 0, (float2*)cout, peak_dev, &op,
                   nullptr, true);
}

// ---------------------------------------------------------------- template bank
// Block size of a bank of templates of L samples: 4096 up to L = 1024, 8192
// above (hop 4097 at L = 4096; measured against M = 16384).
static int os_size_bank(long long L) { return L <= 1024 ? 4096 : 8192; }

// The partials of one launch are held to this many records (256 MB): a bank
// whose K groups need more runs as several launches over runs of templates.
constexpr long long kBankPartialsCap = 1LL << 23;

struct BankGeom {
  long long off, nout, hop, nblocks, grid, npk;   // npk: partials per template
  int waves;
};

static int bank_geom(const vsig_xcorr_bank* x, long long n, int mode, BankGeom* g) {
  vsig_ctx* c = x->ctx;
  if (mode == VSIG_MODE_VALID) { g->off = 0; g->nout = n - x->L + 1; }
  else if (mode == VSIG_MODE_FULL) { g->off = x->L - 1; g->nout = n + x->L - 1; }
  else return fail(c, VSIG_E_INVALID, "the template bank supports VALID and FULL");
  if (n < 1 || g->nout < 1) return fail(c, VSIG_E_INVALID, "stream shorter than the templates");
  g->hop = (long long)x->M - x->L + 1;
  g->nblocks = (g->nout + g->hop - 1) / g->hop;
  if (vsig::xcorr_bank_geom(x->M, g->nblocks, &g->waves, &g->grid) != hipSuccess)
    return fail(c, VSIG_E_UNSUPPORTED, "template bank block size");
  g->npk = g->nblocks * g->waves;
  return VSIG_OK;
}

// td: DEVICE complex64[K][L]
static int bank_create(vsig_ctx* c, const float2* td, int K, long long L, vsig_xcorr_bank** out) {
  std::unique_ptr<vsig_xcorr_bank> x(new vsig_xcorr_bank(c));
  x->K = K;
  x->L = L;
  x->M = os_size_bank(L);
  if (c->xcorr_bank_m) {
    if (2 * L > c->xcorr_bank_m)
      return fail(c, VSIG_E_INVALID, "xcorr_bank_m: the templates are longer than half the block");
    x->M = c->xcorr_bank_m;
  }
  const float2* tw;
  int rc = get_twiddles(c, x->M, &tw);
  if (rc) return rc;
  HIPCHK(c, x->Ps.alloc((size_t)K * x->M * sizeof(float2)));
  for (int k = 0; k < K; ++k)      // make_spectrum's launch, row k into the table
    HIPCHK(c, vsig::launch_spectrum_prep(x->M, td + (long long)k * L, (int)L, 1.0f / (float)x->M,
                                         x->Ps.as<float2>() + (long long)k * x->M, tw, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));     // the caller's templates are free to go
  *out = x.release();
  return VSIG_OK;
}

static int bank_check(vsig_ctx* c, const void* tmpls, int32_t K, int64_t L, vsig_xcorr_bank** out) {
  if (!c || !tmpls || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  if (K < 1 || K > kBankMaxK)
    return fail(c, VSIG_E_INVALID, "template bank: K must be in [1, " + std::to_string(kBankMaxK) + "]");
  if (L < 1) return fail(c, VSIG_E_INVALID, "template length must be >= 1");
  if (L > kBankMaxL)
    return fail(c, VSIG_E_UNSUPPORTED,
                "template bank: templates of at most " + std::to_string(kBankMaxL) + " samples");
  return VSIG_OK;
}

int vsig_xcorr_bank_create(vsig_ctx* c, const void* tmpls, int32_t K, int64_t L, vsig_xcorr_bank** out) {
  int rc = bank_check(c, tmpls, K, L, out);
  if (rc) return rc;
  DevBuf td;      // freed after bank_create's synchronise
  const size_t bytes = (size_t)K * (size_t)L * sizeof(float2);
  HIPCHK(c, td.alloc(bytes));
  HIPCHK(c, hipMemcpyAsync(td.data(), tmpls, bytes, hipMemcpyHostToDevice, c->stream));
  rc = bank_create(c, td.as<float2>(), K, L, out);
  (void)hipStreamSynchronize(c->stream);
  return rc;
}

int vsig_xcorr_bank_create_dev(vsig_ctx* c, const void* tmpls_dev, int32_t K, int64_t L,
                               vsig_xcorr_bank** out) {
  const int rc = bank_check(c, tmpls_dev, K, L, out);
  if (rc) return rc;
  return bank_create(c, (const float2*)tmpls_dev, K, L, out);
}

void vsig_xcorr_bank_free(vsig_xcorr_bank* x) { delete x; }

int vsig_xcorr_bank_plan(const vsig_xcorr_bank* x, int64_t n, int32_t mode, int32_t* M, int64_t* hop,
                         int64_t* nblocks, int64_t* grid) {
  if (!x) return VSIG_E_INVALID;
  if (!M || !hop || !nblocks || !grid) return fail(x->ctx, VSIG_E_INVALID, "null pointer");
  BankGeom g;
  const int rc = bank_geom(x, n, mode, &g);
  if (rc) return rc;
  *M = x->M; *hop = g.hop; *nblocks = g.nblocks; *grid = g.grid;
  return VSIG_OK;
}

int vsig_xcorr_bank_exec_dev(vsig_xcorr_bank* x, const void* s, int64_t n, int32_t mode, void* cout,
                             vsig_peak_t* peaks_dev) {
  if (!x) return VSIG_E_INVALID;
  vsig_ctx* c = x->ctx;
  if (!s || !peaks_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  BankGeom g;
  int rc = bank_geom(x, n, mode, &g);
  if (rc) return rc;
  // templates per launch (the partials' cap); ensure_partials joins a pending
  // asynchronous refine of this context before its partials are overwritten
  long long kc = kBankPartialsCap / g.npk;
  kc = kc < 1 ? 1 : kc > x->K ? x->K : kc;
  if ((rc = ensure_partials(c, kc * g.npk))) return rc;
  const float2* tw;
  if ((rc = get_twiddles(c, x->M, &tw))) return rc;
  Timed t(c, "xcorr_bank");
  for (long long k0 = 0; k0 < x->K; k0 += kc) {
    const int kn = (int)(x->K - k0 < kc ? x->K - k0 : kc);
    float2* ck = cout ? (float2*)cout + k0 * g.nout : nullptr;
    HIPCHK(c, vsig::launch_xcorr_bank(x->M, (const float2*)s, n, x->Ps.as<float2>() + k0 * x->M, kn,
                                      g.off, g.nout, g.hop, ck, c->parts(), tw, c->stream));
    HIPCHK(c, vsig::launch_bank_finalize(c->parts(), kn, g.npk,
                                         reinterpret_cast<PeakPartial*>(peaks_dev) + k0, c->stream));
  }
  return VSIG_OK;
}

// np.correlate(a, v, mode): the shorter operand is the template; with
// nv > na the correlation of v by a is computed and stored conj() reversed.
static int correlate_impl(vsig_ctx* c, int in128, const void* a, long long na, const void* v,
                          long long nv, int32_t mode, int out128, void* cout,
                          vsig_peak_t* peak_dev) {
  if (!c || !a || !v) return fail(c, VSIG_E_INVALID, "null pointer");
  if (na < 1 || nv < 1) return fail(c, VSIG_E_INVALID, "empty input");  // numeric.py:865-868
  const long long nmin = na < nv ? na : nv, nmax = na < nv ? nv : na;
  long long F, nout;
  if (!corr_span(mode, na, nv, &F, &nout)) return fail(c, VSIG_E_INVALID, "mode must be VALID, FULL or SAME");
  int rc;
  // complex64 operands of the FFT pass (complex128 callers: converted copies)
  const float2 *a64 = (const float2*)a, *v64 = (const float2*)v;
  if (in128) {
    if ((rc = c->conv[0].reserve(c, (size_t)na * 8)) || (rc = c->conv[1].reserve(c, (size_t)nv * 8)))
      return rc;
    HIPCHK(c, vsig::launch_convert_c(0, a, na, c->conv[0].data(), c->stream));
    HIPCHK(c, vsig::launch_convert_c(0, v, nv, c->conv[1].data(), c->stream));
    a64 = c->conv[0].as<float2>();
    v64 = c->conv[1].as<float2>();
  }
  float2* c64 = (float2*)cout;
  if (out128 && cout) {
    if ((rc = c->conv[2].reserve(c, (size_t)nout * 8))) return rc;
    c64 = c->conv[2].as<float2>();
  }
  const bool swap = nv > na;  // template must be the shorter operand
  const float2* tmpl = swap ? a64 : v64;
  const float2* strm = swap ? v64 : a64;
  // c[o] = full[F + o]; full[i] = sum_k a[i-(nv-1)+k] conj(v[k]).
  // Not swapped: kernel offset off = (L-1) - F.  Swapped: compute the
  // correlation of v by a and store conj() reversed, off' = F + nout - nv.
  const long long off = swap ? F + nout - nv : (nmin - 1) - F;
  vsig_xcorr x(c);       // its destructor synchronises before the template spectra are freed
  if ((rc = xcorr_build(c, tmpl, nmin, &x))) return rc;
  const RefineOperands op{a, na, v, nv, in128, F};
  const int store = (cout ? (swap ? 2 : 1) : 0) | (swap ? 4 : 0);
  return xcorr_run(&x, strm, nmax, off, nout, store, c64, peak_dev, &op, out128 ? cout : nullptr);
}

int vsig_correlate_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t na, const void* v,
                       int64_t nv, int32_t mode, int32_t out_dtype, void* cout,
                       vsig_peak_t* peak_dev) {
  if (!is_complex_dtype(dtype) || !is_complex_dtype(out_dtype))
    return fail(c, VSIG_E_INVALID, "dtype must be VSIG_DTYPE_C64 or VSIG_DTYPE_C128");
  return correlate_impl(c, dtype == VSIG_DTYPE_C128, a, na, v, nv, mode,
                        out_dtype == VSIG_DTYPE_C128, cout, peak_dev);
}

int vsig_correlate_c64_dev(vsig_ctx* c, const void* a, int64_t na, const void* v, int64_t nv,
                           int32_t mode, void* cout, vsig_peak_t* peak_dev) {
  return correlate_impl(c, 0, a, na, v, nv, mode, 0, cout, peak_dev);
}

int vsig_correlate(vsig_ctx* c, int32_t dtype, const void* a, int64_t na, const void* v,
                   int64_t nv, int32_t mode, int32_t out_dtype, void* cout, vsig_peak_t* peak) {
  if (!c || !a || !v) return fail(c, VSIG_E_INVALID, "null pointer");
  if (na < 1 || nv < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (!is_complex_dtype(dtype) || !is_complex_dtype(out_dtype))
    return fail(c, VSIG_E_INVALID, "dtype must be VSIG_DTYPE_C64 or VSIG_DTYPE_C128");
  const size_t es = dtype_bytes(dtype), eo = dtype_bytes(out_dtype);
  long long F, nout;
  if (!corr_span(mode, na, nv, &F, &nout)) return fail(c, VSIG_E_INVALID, "mode must be VALID, FULL or SAME");
  int rc;
  if ((rc = stage_in(c, 0, a, (size_t)na * es)) || (rc = stage_in(c, 1, v, (size_t)nv * es)) ||
      (cout && (rc = c->stage[2].reserve(c, (size_t)nout * eo))))
    return rc;
  rc = vsig_correlate_dev(c, dtype, c->stage[0].data(), na, c->stage[1].data(), nv, mode, out_dtype,
                          cout ? c->stage[2].data() : nullptr, nullptr);
  if (rc || (cout && (rc = stage_out(c, cout, c->stage[2], (size_t)nout * eo))) ||
      (peak && (rc = stage_out(c, peak, c->result, sizeof(vsig_peak_t)))))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VSIG_OK;
}

int vsig_correlate_c64(vsig_ctx* c, const void* a, int64_t na, const void* v, int64_t nv,
                       int32_t mode, void* cout, vsig_peak_t* peak) {
  return vsig_correlate(c, VSIG_DTYPE_C64, a, na, v, nv, mode, VSIG_DTYPE_C64, cout, peak);
}

// ---------------------------------------------------------------- any-length transforms
int vsig_dft_dev(vsig_ctx* c, int32_t dtype, const void* x, int64_t n, int64_t batch, int32_t inverse,
                 int32_t out_dtype, void* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1 || batch < 1) return fail(c, VSIG_E_INVALID, "need n >= 1 and batch >= 1");
  if (!is_complex_dtype(dtype) || !is_complex_dtype(out_dtype))
    return fail(c, VSIG_E_INVALID, "dtype must be VSIG_DTYPE_C64 or VSIG_DTYPE_C128");
  vsig::BigIn in{x, dtype == VSIG_DTYPE_C128 ? 1 : 0, n, 1, n, nullptr, nullptr, 0, 1.0f};
  vsig::BigOut out{y, out_dtype == VSIG_DTYPE_C128 ? 1 : 0, n, n, nullptr, 0,
                   inverse ? (float)(1.0 / (double)n) : 1.0f};
  Timed t(c, "dft");
  return dft_any(c, n, batch, in, out, inverse != 0);
}

int vsig_resample_dev(vsig_ctx* c, int32_t dtype, const void* x, int64_t n, int64_t num,
                      int32_t real_input, void* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1 || num < 1) return fail(c, VSIG_E_INVALID, "need n >= 1 and num >= 1");
  if (!is_complex_dtype(dtype))
    return fail(c, VSIG_E_INVALID, "dtype must be VSIG_DTYPE_C64 or VSIG_DTYPE_C128");
  int rc;
  if ((rc = c->spec[0].reserve(c, (size_t)n * 8)) || (rc = c->spec[1].reserve(c, (size_t)num * 8)))
    return rc;
  float2* X = c->spec[0].as<float2>();
  float2* Y = c->spec[1].as<float2>();
  Timed t(c, "resample");
  vsig::BigIn in{x, dtype == VSIG_DTYPE_C128 ? 1 : 0, n, 1, n, nullptr, nullptr, 0, 1.0f};
  vsig::BigOut ox{X, 0, n, n, nullptr, 0, 1.0f};
  if ((rc = dft_any(c, n, 1, in, ox, false))) return rc;
  HIPCHK(c, vsig::launch_resample_spectrum(X, n, num, Y, c->stream));
  // y = ifft(Y) * num / n  ->  the inverse DFT's 1/num and num/n leave 1/n
  vsig::BigIn iy{Y, 0, num, 1, num, nullptr, nullptr, 0, 1.0f};
  vsig::BigOut oy{y, real_input ? 3 : 0, num, num, nullptr, 0, (float)(1.0 / (double)n)};
  return dft_any(c, num, 1, iy, oy, true);
}

int vsig_filter_channel_dev(vsig_ctx* c, int32_t dtype, const void* x, int64_t n,
                            double center_freq, double sample_rate, double bandwidth,
                            double* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (n > 1 && (n & 1))
    return fail(c, VSIG_E_INVALID, "odd length: the conjugate mirror's halves differ (numpy "
                                   "raises on the shape mismatch)");
  if (!is_complex_dtype(dtype))
    return fail(c, VSIG_E_INVALID, "dtype must be VSIG_DTYPE_C64 or VSIG_DTYPE_C128");
  const double center = 5230e6;                  // split_channels.py:7 CENTER_FREQ
  const double lo = center_freq - bandwidth / 2, hi = center_freq + bandwidth / 2;
  if (n > 1) {   // the mirror's halves are the natural ones unless f(-1) rounds onto CENTER
    if (!(channel_freq(-1, n, sample_rate, center) < center))
      return fail(c, VSIG_E_UNSUPPORTED, "frequency spacing below the rounding of CENTER_FREQ");
  }
  // kept non-negative bins: f(k) rises with k, so the mask is one range [ka, kb]
  const long long h = n == 1 ? 1 : n / 2;
  auto keep = [&](long long k) { const double f = channel_freq(k, n, sample_rate, center); return f >= lo && f <= hi; };
  auto first_at_least = [&](double bound) {      // smallest k in [0, h] with f(k) >= bound
    long long a = 0, b = h;
    while (a < b) { const long long m = (a + b) / 2; if (channel_freq(m, n, sample_rate, center) >= bound) b = m; else a = m + 1; }
    return a;
  };
  long long ka = first_at_least(lo), kb = ka - 1;
  if (ka < h && keep(ka)) {
    long long a = ka, b = h - 1;                 // largest kept k
    while (a < b) { const long long m = (a + b + 1) / 2; if (keep(m)) a = m; else b = m - 1; }
    kb = a;
  }
  const long long nk = kb >= ka ? kb - ka + 1 : 0;
  int rc;
  if (nk * n <= (1LL << 32)) {                   // direct double-precision path
    if ((rc = c->spec[0].reserve(c, (size_t)(nk > 0 ? nk : 1) * 256 * 16)) ||
        (rc = c->spec[1].reserve(c, (size_t)(nk > 0 ? nk : 1) * 16)))
      return rc;
    Timed t(c, "channel");
    HIPCHK(c, vsig::launch_channel_direct(dtype == VSIG_DTYPE_C128, x, n, ka, kb, c->spec[0].as<double2>(),
                                          c->spec[1].as<double2>(), y, c->stream));
    return VSIG_OK;
  }
  if ((rc = c->spec[0].reserve(c, (size_t)n * 8)) || (rc = c->spec[1].reserve(c, (size_t)n * 8)))
    return rc;
  float2* X = c->spec[0].as<float2>();
  float2* F = c->spec[1].as<float2>();
  Timed t(c, "channel");
  vsig::BigIn in{x, dtype == VSIG_DTYPE_C128 ? 1 : 0, n, 1, n, nullptr, nullptr, 0, 1.0f};
  vsig::BigOut ox{X, 0, n, n, nullptr, 0, 1.0f};
  if ((rc = dft_any(c, n, 1, in, ox, false))) return rc;
  HIPCHK(c, vsig::launch_channel_mask(X, n, sample_rate, center, center_freq - bandwidth / 2,
                                      center_freq + bandwidth / 2, F, c->stream));
  vsig::BigIn iF{F, 0, n, 1, n, nullptr, nullptr, 0, 1.0f};
  vsig::BigOut oy{y, 2, n, n, nullptr, 0, (float)(1.0 / (double)n)};
  return dft_any(c, n, 1, iF, oy, true);
}

// ---------------------------------------------------------------- peak
int vsig_peak_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, vsig_peak_t* peak_dev) {
  if (!c || !a) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");  // np.argmax of empty raises
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  long long nparts = (n + 255) / 256;
  if (nparts > 2048) nparts = 2048;
  int rc = ensure_partials(c, nparts);
  if (rc) return rc;
  {
    Timed t(c, "peak");
    HIPCHK(c, vsig::launch_peak_reduce(dtype, a, n, c->parts(), (int)nparts, c->stream));
  }
  if ((rc = finalize_peak(c, nparts, 0, peak_dev))) return rc;
  // numpy's answer when the array holds a NaN (a no-op on any other record)
  HIPCHK(c, vsig::launch_peak_first_nan(dtype, a, n, peak_record(c, peak_dev), c->stream));
  return VSIG_OK;
}

int vsig_peak(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, vsig_peak_t* peak) {
  if (!c || !a || !peak) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  int rc;
  if ((rc = stage_in(c, 0, a, (size_t)n * dtype_bytes(dtype))) ||
      (rc = vsig_peak_dev(c, dtype, c->stage[0].data(), n, nullptr)) ||
      (rc = stage_out(c, peak, c->result, sizeof(vsig_peak_t))))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- peak list
static_assert(sizeof(vsig_instance_t) == sizeof(vsig::PeakInst) && sizeof(vsig_instance_t) == 16,
              "vsig_instance_t layout");
static_assert(sizeof(vsig_peaks_info_t) == sizeof(vsig::PeaksInfo) && sizeof(vsig_peaks_info_t) == 32,
              "vsig_peaks_info_t layout");

int vsig_peaks_tile(void) { return vsig::kPeaksTile; }

static int peaks_check(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr,
                       int64_t min_distance, const void* out, int64_t cap, const void* info) {
  if (!c || !a || !info) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n above 2^40");
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  if (cap < 0 || min_distance < 0) return fail(c, VSIG_E_INVALID, "need cap >= 0 and min_distance >= 0");
  if (cap > 0 && !out) return fail(c, VSIG_E_INVALID, "null out with cap > 0");
  if (thr != thr) return fail(c, VSIG_E_INVALID, "thr is NaN");
  return VSIG_OK;
}

int vsig_peaks_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
                   int64_t min_distance, vsig_instance_t* out_dev, int64_t cap,
                   vsig_peaks_info_t* info_dev) {
  int rc = peaks_check(c, dtype, a, n, thr, min_distance, out_dev, cap, info_dev);
  if (rc || (rc = c->pscratch.reserve(c, vsig::peaks_scratch_bytes(n)))) return rc;
  Timed t(c, "peaks");
  HIPCHK(c, vsig::launch_peaks(dtype, a, n, thr, relative != 0, min_distance,
                               reinterpret_cast<vsig::PeakInst*>(out_dev), cap,
                               reinterpret_cast<vsig::PeaksInfo*>(info_dev), c->pscratch.data(), c->stream));
  return VSIG_OK;
}

int vsig_peaks(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
               int64_t min_distance, vsig_instance_t* out, int64_t cap, vsig_peaks_info_t* info) {
  int rc = peaks_check(c, dtype, a, n, thr, min_distance, out, cap, info);
  if (rc) return rc;
  // stage[1]: the info record, then the instance records
  const size_t ib = sizeof(vsig_peaks_info_t);
  if ((rc = stage_in(c, 0, a, (size_t)n * dtype_bytes(dtype))) ||
      (rc = c->stage[1].reserve(c, ib + (size_t)cap * sizeof(vsig_instance_t))))
    return rc;
  char* sb = c->stage[1].as<char>();
  vsig_instance_t* od = cap > 0 ? reinterpret_cast<vsig_instance_t*>(sb + ib) : nullptr;
  if ((rc = vsig_peaks_dev(c, dtype, c->stage[0].data(), n, thr, relative, min_distance, od, cap,
                           reinterpret_cast<vsig_peaks_info_t*>(sb))))
    return rc;
  vsig_peaks_info_t h;
  HIPCHK(c, hipMemcpyAsync(&h, sb, ib, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t k = h.count < cap ? h.count : cap;
  if (k > 0) {
    HIPCHK(c, hipMemcpyAsync(out, od, (size_t)k * sizeof(vsig_instance_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *info = h;
  return VSIG_OK;
}

// ---------------------------------------------------------------- run list
static_assert(sizeof(vsig_run_t) == sizeof(vsig::RunRec) && sizeof(vsig_run_t) == 40, "vsig_run_t layout");
static_assert(sizeof(vsig_runs_info_t) == sizeof(vsig::RunsInfo) && sizeof(vsig_runs_info_t) == 40,
              "vsig_runs_info_t layout");

int vsig_runs_tile(void) { return vsig::kRunsTile; }

static int runs_check(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int64_t max_gap,
                      const void* out, int64_t cap, const void* info) {
  if (!c || !a || !info) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n above 2^40");
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  if (cap < 0 || max_gap < 0) return fail(c, VSIG_E_INVALID, "need cap >= 0 and max_gap >= 0");
  if (cap > 0 && !out) return fail(c, VSIG_E_INVALID, "null out with cap > 0");
  if (thr != thr) return fail(c, VSIG_E_INVALID, "thr is NaN");
  return VSIG_OK;
}

int vsig_runs_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
                  int64_t max_gap, vsig_run_t* out_dev, int64_t cap, vsig_runs_info_t* info_dev) {
  int rc = runs_check(c, dtype, a, n, thr, max_gap, out_dev, cap, info_dev);
  if (rc || (rc = c->rnscratch.reserve(c, vsig::runs_scratch_bytes(n)))) return rc;
  Timed t(c, "runs");
  HIPCHK(c, vsig::launch_runs(dtype, a, n, thr, relative != 0, max_gap,
                              reinterpret_cast<vsig::RunRec*>(out_dev), cap,
                              reinterpret_cast<vsig::RunsInfo*>(info_dev), c->rnscratch.data(), c->stream));
  return VSIG_OK;
}

int vsig_runs(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
              int64_t max_gap, vsig_run_t* out, int64_t cap, vsig_runs_info_t* info) {
  int rc = runs_check(c, dtype, a, n, thr, max_gap, out, cap, info);
  if (rc) return rc;
  // stage[1]: the info record, then the run records
  const size_t ib = sizeof(vsig_runs_info_t);
  if ((rc = stage_in(c, 0, a, (size_t)n * dtype_bytes(dtype))) ||
      (rc = c->stage[1].reserve(c, ib + (size_t)cap * sizeof(vsig_run_t))))
    return rc;
  char* sb = c->stage[1].as<char>();
  vsig_run_t* od = cap > 0 ? reinterpret_cast<vsig_run_t*>(sb + ib) : nullptr;
  if ((rc = vsig_runs_dev(c, dtype, c->stage[0].data(), n, thr, relative, max_gap, od, cap,
                          reinterpret_cast<vsig_runs_info_t*>(sb))))
    return rc;
  vsig_runs_info_t h;
  HIPCHK(c, hipMemcpyAsync(&h, sb, ib, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t k = h.count < cap ? h.count : cap;
  if (k > 0) {
    HIPCHK(c, hipMemcpyAsync(out, od, (size_t)k * sizeof(vsig_run_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *info = h;
  return VSIG_OK;
}

// ---------------------------------------------------------------- region powers
int vsig_region_power_dev(vsig_ctx* c, const void* a, const void* b, int64_t n, double* sums_dev) {
  if (!c || !a || !b || !sums_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");  // the mean of an empty region
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7)
    return fail(c, VSIG_E_INVALID, "region power: operands must be 8-byte aligned");
  int rc = c->gscratch.reserve(c, vsig::region_scratch_bytes());
  if (rc) return rc;
  Timed t(c, "region_power");
  HIPCHK(c, vsig::launch_region_power(static_cast<const float2*>(a), static_cast<const float2*>(b), n,
                                      sums_dev, c->gscratch.data(), c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- line traces
static_assert(sizeof(vsig_trace_info_t) == sizeof(vsig::TraceInfo) && sizeof(vsig_trace_info_t) == 32,
              "vsig_trace_info_t layout");
static_assert(VSIG_TRACE_ABS == vsig::kTraceAbs && VSIG_TRACE_DB20 == vsig::kTraceDb20, "VSIG_TRACE_*");

int vsig_trace_envelope_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, int32_t shift, int64_t lo,
                            int64_t hi, int64_t bin, int32_t kind, double eps, void* env_min_dev,
                            void* env_max_dev, vsig_trace_info_t* info_dev) {
  if (!c || !a || !env_max_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n above 2^40");
  if (!dtype_ok(dtype)) return fail(c, VSIG_E_INVALID, "dtype");
  if (kind != VSIG_TRACE_ABS && kind != VSIG_TRACE_DB20) return fail(c, VSIG_E_INVALID, "kind");
  if (lo < 0 || hi > n || lo >= hi) return fail(c, VSIG_E_INVALID, "need 0 <= lo < hi <= n");
  if (bin < 1) return fail(c, VSIG_E_INVALID, "need bin >= 1");
  if (!(eps >= 0.0) || std::isinf(eps)) return fail(c, VSIG_E_INVALID, "need a finite eps >= 0");
  int rc = c->tscratch.reserve(c, vsig::trace_scratch_bytes(lo, hi, bin));
  if (rc) return rc;
  Timed t(c, "trace");
  HIPCHK(c, vsig::launch_trace_envelope(dtype, a, n, shift != 0, lo, hi, bin, kind, eps, env_min_dev,
                                        env_max_dev, reinterpret_cast<vsig::TraceInfo*>(info_dev),
                                        c->tscratch.data(), c->stream));
  return VSIG_OK;
}

// numpy's np.mean / np.std of |a| (find_correlation_peak's mean_corr /
// std_corr, utils.py:1329-1330) in numpy's own summation order.
int vsig_abs_stats_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, double* stats_dev) {
  if (!c || !a || !stats_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (dtype != VSIG_DTYPE_C128 && dtype != VSIG_DTYPE_F64)
    return fail(c, VSIG_E_UNSUPPORTED, "abs stats: dtype must be VSIG_DTYPE_C128 or VSIG_DTYPE_F64");
  int rc = c->sscratch.reserve(c, vsig::np_stats_scratch_bytes(n));
  if (rc) return rc;
  Timed t(c, "stats");
  HIPCHK(c, vsig::launch_np_stats(dtype, a, n, stats_dev, c->sscratch.data(), c->stream));
  return VSIG_OK;
}

// np.correlate(a, v, mode)'s |c| for every output in numpy's operation order
// (refine.hip, values mode), then its mean / std as above.
int vsig_correlate_stats_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t na, const void* v,
                             int64_t nv, int32_t mode, double* stats_dev) {
  if (!c || !a || !v || !stats_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (na < 1 || nv < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (!is_complex_dtype(dtype))
    return fail(c, VSIG_E_INVALID, "dtype must be VSIG_DTYPE_C64 or VSIG_DTYPE_C128");
  long long F, nout;
  if (!corr_span(mode, na, nv, &F, &nout)) return fail(c, VSIG_E_INVALID, "mode must be VALID, FULL or SAME");
  const size_t vb = ((size_t)nout * 8 + 255) & ~(size_t)255;
  const size_t kb = (vsig::refine_values_scratch_bytes() + 255) & ~(size_t)255;
  int rc;
  if ((rc = c->vscratch.reserve(c, vb + kb)) || (rc = c->sscratch.reserve(c, vsig::np_stats_scratch_bytes(nout))))
    return rc;
  double* vals = c->vscratch.as<double>();
  vsig::RefineArgs r{};
  r.a = a; r.na = na; r.v = v; r.nv = nv; r.c128 = dtype == VSIG_DTYPE_C128;
  r.nout = nout; r.F = F; r.waves = 1; r.Q = 1; r.rsub = 1;
  r.blas_threads = c->blas_threads;
  r.scratch = c->vscratch.as<char>() + vb;
  Timed t(c, "stats");
  HIPCHK(c, vsig::launch_refine_values(r, 0, nout - 1, vals, c->stream));
  HIPCHK(c, vsig::launch_np_stats(VSIG_DTYPE_F64, vals, nout, stats_dev, c->sscratch.data(), c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- stream ops
int vsig_mix_c64_dev(vsig_ctx* c, const void* x, int64_t n, double w, double sr, int64_t i0,
                     void* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0 || !(sr != 0.0)) return fail(c, VSIG_E_INVALID, "need n >= 0 and sample_rate != 0");
  if (n == 0) return VSIG_OK;
  HIPCHK(c, vsig::launch_mix_c64((const float2*)x, n, w, sr, i0, (float2*)y, c->stream));
  return VSIG_OK;
}

int vsig_scale_c64_dev(vsig_ctx* c, const void* x, int64_t n, float s, void* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0) return fail(c, VSIG_E_INVALID, "n < 0");
  if (n == 0) return VSIG_OK;
  HIPCHK(c, vsig::launch_scale_c64((const float2*)x, n, s, (float2*)y, c->stream));
  return VSIG_OK;
}

int vsig_wv_quantize_dev(vsig_ctx* c, const void* x, int64_t n, float norm, int16_t* out) {
  if (!c || !x || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0) return fail(c, VSIG_E_INVALID, "n < 0");
  if (n == 0) return VSIG_OK;
  HIPCHK(c, vsig::launch_wv_quantize((const float2*)x, n, norm, (short*)out, c->stream));
  return VSIG_OK;
}

int vsig_planar_to_c64_dev(vsig_ctx* c, int32_t mi_type, const void* re, const void* im, int64_t n,
                           void* y) {
  if (!c || !re || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0) return fail(c, VSIG_E_INVALID, "n < 0");
  if (n == 0) return VSIG_OK;
  const hipError_t e = vsig::launch_planar_to_c64(mi_type, re, im, n, (float2*)y, c->stream);
  if (e == hipErrorInvalidValue) return fail(c, VSIG_E_UNSUPPORTED, "MAT storage type");
  HIPCHK(c, e);
  return VSIG_OK;
}

int vsig_c64_to_planar_dev(vsig_ctx* c, const void* x, int64_t n, float* re, float* im) {
  if (!c || !x || !re || !im) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0) return fail(c, VSIG_E_INVALID, "n < 0");
  if (n == 0) return VSIG_OK;
  HIPCHK(c, vsig::launch_c64_to_planar((const float2*)x, n, re, im, c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- vector assembly
int vsig_vector_build_dev(vsig_ctx* c, const vsig_packet_place* places, int32_t nplaces, void* out,
                          int64_t n, float* maxabs_dev) {
  if (!c || !out || (nplaces > 0 && !places)) return fail(c, VSIG_E_INVALID, "null pointer");
  if (nplaces < 0 || n < 0) return fail(c, VSIG_E_INVALID, "need nplaces >= 0 and n >= 0");
  if (n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n above 2^40");
  if (reinterpret_cast<uintptr_t>(out) & 7) return fail(c, VSIG_E_INVALID, "out must be 8-byte aligned");
  for (int32_t i = 0; i < nplaces; ++i) {
    const vsig_packet_place& p = places[i];
    const std::string who = "place " + std::to_string(i) + ": ";
    if (!p.y) return fail(c, VSIG_E_INVALID, who + "null packet pointer");
    if (reinterpret_cast<uintptr_t>(p.y) & 7) return fail(c, VSIG_E_INVALID, who + "packet must be 8-byte aligned");
    if (p.len < 1) return fail(c, VSIG_E_INVALID, who + "len must be >= 1");
    if (p.period < 1) return fail(c, VSIG_E_INVALID, who + "period must be >= 1");
    if (p.count < 0) return fail(c, VSIG_E_INVALID, who + "count must be >= 0");
    if (p.start < 0) return fail(c, VSIG_E_INVALID, who + "start must be >= 0");
    // start + (count-1) period + len <= n without overflow
    if (p.count >= 1 && (p.start > n || p.len > n - p.start ||
                         p.count - 1 > (n - p.start - p.len) / p.period))
      return fail(c, VSIG_E_INVALID, who + "an instance ends past the vector");
  }
  if (maxabs_dev) HIPCHK(c, hipMemsetAsync(maxabs_dev, 0, sizeof(float), c->stream));
  if (n == 0) return VSIG_OK;
  // successive launches of kPlacesPerLaunch descriptors keep the add order:
  // each later one starts from what the earlier ones wrote
  vsig::PlaceBatch pb{};
  int launches = 0;
  for (int32_t i = 0; i < nplaces; ++i) {
    const vsig_packet_place& p = places[i];
    if (p.count == 0) continue;
    if (pb.nd == vsig::kPlacesPerLaunch) {
      HIPCHK(c, vsig::launch_vector_build(pb, (float2*)out, n, launches > 0, nullptr, c->stream));
      ++launches;
      pb.nd = 0;
    }
    pb.d[pb.nd++] = vsig::PlaceDesc{(const float2*)p.y, p.len, p.start, p.period, p.count};
  }
  HIPCHK(c, vsig::launch_vector_build(pb, (float2*)out, n, launches > 0, maxabs_dev, c->stream));
  return VSIG_OK;
}

int vsig_normalize_c64_dev(vsig_ctx* c, const void* x, int64_t n, const float* maxabs_dev, void* y) {
  if (!c || !x || !y || !maxabs_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0) return fail(c, VSIG_E_INVALID, "n < 0");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 7)
    return fail(c, VSIG_E_INVALID, "x and y must be 8-byte aligned");
  if (n == 0) return VSIG_OK;
  HIPCHK(c, vsig::launch_normalize_c64((const float2*)x, n, maxabs_dev, (float2*)y, c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- PFB
int vsig_pfb_c64_dev(vsig_ctx* c, const void* x, int64_t n, const float* h, int32_t ntaps,
                     int32_t nchan, void* y, int64_t nframes) {
  if (!c || !x || !h || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (nchan != 64 && nchan != 128 && nchan != 256)
    return fail(c, VSIG_E_UNSUPPORTED, "nchan must be 64, 128 or 256");
  const int pt = ntaps / nchan;
  if (ntaps % nchan || (pt != 4 && pt != 8 && pt != 16))
    return fail(c, VSIG_E_UNSUPPORTED, "ntaps must be 4, 8 or 16 times nchan");
  if (n < ntaps) return fail(c, VSIG_E_INVALID, "signal shorter than the prototype filter");
  if (nframes != (n - ntaps) / nchan + 1) return fail(c, VSIG_E_INVALID, "nframes mismatch");
  const float2* tw;
  int rc = get_twiddles(c, nchan, &tw);
  if (rc) return rc;
  Timed t(c, "pfb");
  HIPCHK(c, vsig::launch_pfb(nchan, pt, (const float2*)x, n, h, nframes, (float2*)y, tw, c->stream));
  return VSIG_OK;
}

int vsig_pfb_plan(int32_t nchan, int32_t ntaps, int64_t nframes, int64_t* frames_per_group,
                  int64_t* groups_per_block, int64_t* blocks) {
  if (!frames_per_group || !groups_per_block || !blocks || nframes < 1 || nchan < 1 || ntaps % nchan)
    return VSIG_E_INVALID;
  long long fpg = 0, gpb = 0, nb = 0;
  if (vsig::pfb_plan(nchan, ntaps / nchan, nframes, &fpg, &gpb, &nb) != hipSuccess) return VSIG_E_UNSUPPORTED;
  *frames_per_group = fpg; *groups_per_block = gpb; *blocks = nb;
  return VSIG_OK;
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
  int rc = c->stage[2].reserve(c, 4096 * 8 + 64);
  if (rc) return rc;
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
  long long nparts = (n + 255) / 256;
  if (nparts > 2048) nparts = 2048;
  int rc = c->stage[2].reserve(c, (size_t)nparts * sizeof(vsig::ThreshPartialH));
  if (rc) return rc;
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
  if (!c || !a || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  HIPCHK(c, vsig::launch_db_transform(dtype, a, n, floor_, out, c->stream));
  return VSIG_OK;
}

int vsig_abs_c64_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, void* out) {
  if (!c || !a || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  HIPCHK(c, vsig::launch_abs_c64(dtype, a, n, (float2*)out, c->stream));
  return VSIG_OK;
}

int vsig_abs_c128_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t n, void* out) {
  if (!c || !a || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1) return fail(c, VSIG_E_INVALID, "empty input");
  HIPCHK(c, vsig::launch_abs_c128(dtype, a, n, (double2*)out, c->stream));
  return VSIG_OK;
}

// ---------------------------------------------------------------- display image
int vsig_spectrogram_image_dev(vsig_ctx* c, int32_t dtype, const void* sxx, int64_t n_freq,
                               int64_t n_time, int32_t freq_fast, int64_t ld, double floor_,
                               double vmin, double vmax, int32_t median, int32_t flip_freq,
                               int32_t pool_f, int32_t pool_t, const uint8_t* lut_dev,
                               uint8_t* rgba_dev) {
  if (!c || !sxx || !lut_dev || !rgba_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (dtype != VSIG_DTYPE_F32 && dtype != VSIG_DTYPE_F64)
    return fail(c, VSIG_E_INVALID, "spectrogram image: dtype must be VSIG_DTYPE_F32 or VSIG_DTYPE_F64");
  if (n_freq < 1 || n_time < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (pool_f < 1 || pool_t < 1) return fail(c, VSIG_E_INVALID, "spectrogram image: pool factors must be >= 1");
  if (ld < (freq_fast ? n_freq : n_time))
    return fail(c, VSIG_E_INVALID, "spectrogram image: ld is below the fast extent");
  if ((reinterpret_cast<uintptr_t>(lut_dev) | reinterpret_cast<uintptr_t>(rgba_dev)) & 3)
    return fail(c, VSIG_E_INVALID, "spectrogram image: table and image must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(sxx) & (dtype == VSIG_DTYPE_F32 ? 3 : 7))
    return fail(c, VSIG_E_INVALID, "spectrogram image: sxx is not aligned to its dtype");
  if (!std::isfinite(vmin) || !std::isfinite(vmax) || !(vmax > vmin) ||
      (dtype == VSIG_DTYPE_F32 && !((float)vmax > (float)vmin && std::isfinite((float)vmax) &&
                                    std::isfinite((float)vmin))))
    return fail(c, VSIG_E_INVALID, "spectrogram image: need finite levels with vmax > vmin");
  Timed t(c, "spectrogram_image");
  HIPCHK(c, vsig::launch_spectrogram_image(dtype, sxx, n_freq, n_time, freq_fast != 0, ld, floor_, vmin,
                                           vmax, median != 0, flip_freq != 0, pool_f, pool_t, lut_dev,
                                           rgba_dev, c->stream));
  return VSIG_OK;
}

}  // extern "C"
