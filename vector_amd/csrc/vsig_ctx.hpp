// What the C-ABI sources (api_*.hip) share: the context, the handles, the
// owner of a device allocation, and the host helpers more than one of them
// uses.  Included by those sources only; nothing here is extern "C", so the
// exported vsig_* symbols are the ones include/vsig.h declares: each is defined
// once in a source, and takes its C linkage from that declaration.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vsig.h"
#include "dtype.hpp"

using vsig::PeakPartial;
using vsig::dtype_bytes;
using vsig::dtype_ok;
static_assert(VSIG_DTYPE_C128 == vsig::VSIG_C128 && VSIG_DTYPE_C64 == vsig::VSIG_C64 &&
              VSIG_DTYPE_F64 == vsig::VSIG_F64 && VSIG_DTYPE_F32 == vsig::VSIG_F32, "VSIG_DTYPE_*");

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
  int match_grid = 0;                    // all-pairs match: cap on the launched grid (0: the resident blocks)
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
  std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> timers;   // event pairs by stage
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

// The tables and the K x N spectra of one packet list (vsig_match_create).
struct vsig_match {
  vsig_ctx* ctx;
  int K = 0, N = 0, tile = 0;
  long long total = 0, pairs = 0, nunits = 0, grid = 0;
  const float2* tw = nullptr;      // the context's cached table
  DevBuf offsets, units, W;
  explicit vsig_match(vsig_ctx* c) : ctx(c) {}
  // the stream may still use the tables: wait, then the members free them
  ~vsig_match() { (void)hipStreamSynchronize(ctx->stream); }
};

// The tables and the estimate partials of one grouped packet list (vsig_combine_create).
struct vsig_combine {
  vsig_ctx* ctx;
  int K = 0, G = 0;
  long long total = 0, out_total = 0, est_items = 0, sum_items = 0;
  std::vector<long long> offsets;  // G + 1 prefix sums of the packed output
  DevBuf mem, grp, csr, est, sum, parts;
  explicit vsig_combine(vsig_ctx* c) : ctx(c) {}
  // the stream may still use the tables: wait, then the members free them
  ~vsig_combine() { (void)hipStreamSynchronize(ctx->stream); }
};

// A bank of K templates of one length L <= kBankMaxL: the K spectra of M
// points in one table (row k at Ps + k M).
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

namespace vsig::api {

constexpr int kClockSlots = 32;            // per-stage clock sinks (vsig_clock_*)

inline int fail(vsig_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
inline int hip_status(vsig_ctx* c, hipError_t e, const char* what) {
  if (e == hipSuccess) return VSIG_OK;
  return fail(c, e == hipErrorOutOfMemory ? VSIG_E_NOMEM : VSIG_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// The status of a HIP call or launch (its text with the runtime's message on
// failure); HIPCHK returns it from the enclosing function unless it is VSIG_OK.
#define HIPRC(ctx, expr) ::vsig::api::hip_status(ctx, (expr), #expr)
#define HIPCHK(ctx, expr)                        \
  do {                                           \
    if (const int s_ = HIPRC(ctx, expr)) return s_; \
  } while (0)

// What many entry points refuse alike, each a status with its message.
inline int check_array(vsig_ctx* c, bool operands, long long n) {
  if (!operands) return fail(c, VSIG_E_INVALID, "null pointer");
  return n < 1 ? fail(c, VSIG_E_INVALID, "empty input") : VSIG_OK;
}
inline bool is_complex_dtype(int dtype) { return dtype == VSIG_DTYPE_C64 || dtype == VSIG_DTYPE_C128; }
inline int check_complex(vsig_ctx* c, int dtype, int out_dtype = VSIG_DTYPE_C64) {
  if (is_complex_dtype(dtype) && is_complex_dtype(out_dtype)) return VSIG_OK;
  return fail(c, VSIG_E_INVALID, "dtype must be VSIG_DTYPE_C64 or VSIG_DTYPE_C128");
}
inline bool pow2_in(long long v, long long lo, long long hi) {
  return v >= lo && v <= hi && (v & (v - 1)) == 0;
}
// Device operands read or written as 8-byte elements.
inline bool aligned8(const void* a, const void* b = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0;
}
// The two segment tables (psd segments, isolate): segment s lies in [0, n]
// (allow_empty: len 0 and start n pass) or is a non-empty part of [0, n); how
// their messages name it.  Each caller words its own refusal.
inline bool segment_inside(long long start, long long len, long long n, bool allow_empty) {
  return start >= 0 && len <= n - start && (allow_empty ? len >= 0 && start <= n : len >= 1 && start < n);
}
inline std::string segment_name(long long s, long long start, long long len) {
  return "segment " + std::to_string(s) + " {start " + std::to_string(start) + ", len " + std::to_string(len) + "}";
}

// ---- api_core.hip
// The context stream waits for the last asynchronous refine (once per stream
// after each refine): called before anything reuses the refine's scratch or
// operands -- every scratch / partials / staging allocation and use goes
// through DevBuf::reserve / ensure_partials -- and by vsig_refine_join.
void join_refine(vsig_ctx* c);
// Cached twiddle tables (fft_engine.hpp): the per-pass table of the plan for
// N; the two-level table for plan key N; W_M^t for t < T (the half-frame
// correlator's per-thread twiddle, T a function of M); the four-step table
// A[i] = W_M^(i 2^S), B[j] = W_M^j with S = ceil(log2 M / 2) (bigfft.hip).
int get_twiddles(vsig_ctx* c, int N, const float2** out);
int get_tw2(vsig_ctx* c, int N, const float2** out);
int get_half_tw(vsig_ctx* c, int M, int T, const float2** out);
int get_tw_big(vsig_ctx* c, long long M, const float2** out, int* S, int* hiA);
int ensure_partials(vsig_ctx* c, long long n);
// Host-pointer entry points: the operand into staging buffer i, and a result
// back from the device (the caller synchronises once).
int stage_in(vsig_ctx* c, int i, const void* host, size_t bytes);
int stage_out(vsig_ctx* c, void* host, const DevBuf& src, size_t bytes);
// The sizes both segment tables refuse; more blocks than a grid holds.
int check_segment_table(vsig_ctx* c, const void* segs, long long nseg, long long n);
int check_blocks(vsig_ctx* c, long long nblocks);
// Where a peak record goes: the caller's device record, or the context's.
PeakPartial* peak_record(vsig_ctx* c, vsig_peak_t* peak_dev);
int finalize_peak(vsig_ctx* c, long long nparts, int sqrt_max, vsig_peak_t* peak_dev);
// The refine scratch's header (vsig::RefineKeys), read back once the stream
// has drained.  After a watchdog fire: zero the keys and the fused launch's
// counters (a fire can leave them inconsistent, and the next launch must
// start from zero), leave `fault` in the sticky fault word, and wait.
int read_refine_keys(vsig_ctx* c, vsig::RefineKeys* keys);
int clear_refine_fault(vsig_ctx* c, unsigned long long fault = 0);

// `count` host elements into a fresh allocation of d, on the context stream.
// The caller owns the synchronise that lets the host memory go.
template <class T>
int upload(vsig_ctx* c, DevBuf& d, const T* src, size_t count) {
  HIPCHK(c, d.alloc(count * sizeof(T)));
  return HIPRC(c, hipMemcpyAsync(d.data(), src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
}

// The device table for `key`, built on first use: fill(h) appends its entries
// to a host vector (or returns a status), which is uploaded and kept for the
// context's lifetime.  A failed upload caches nothing.  The copy is a blocking
// one that leaves the context stream alone (it may be the caller's, and busy).
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
    c->timers[name].emplace_back(b, e);
  }
};

// ---- api_transform.hip
constexpr long long kBigMax = 1LL << 28;    // largest four-step transform
// Twiddles of a (four-step) transform of M points.
struct BigPlan {
  long long M;
  int N1, N2, S, hiA;
  const float2 *tw1, *tw2, *t2;
};
int big_plan(vsig_ctx* c, long long M, BigPlan* p);
// Bluestein plan for length N: chirp c[N] and B = FFT_M(b) / M (permuted order
// for the four-step sizes), M = the power of two >= max(256, 2N - 1).
int chirp_plan(vsig_ctx* c, long long N, vsig_ctx::Chirp** out);
// DFT of any length N (batch frames): X[k] = sum_n x[n] W_N^(nk), or the
// inverse (conj) form; in / out describe the operands (their chirp / conj
// fields are set there), out.scale includes any 1/N.
int dft_any(vsig_ctx* c, long long N, long long batch, vsig::BigIn in, vsig::BigOut out, bool inverse);
// Row r of dst (M <= 16384 points) = FFT_M(zero-padded row r of src, len
// points) / M in natural order: the filter / template spectra of every plan.
int spectrum_rows(vsig_ctx* c, const float2* src_dev, long long rows, int len, int M, float2* dst_dev);
// One such spectrum in a new device buffer (M > 16384 by the four-step passes).
int make_spectrum(vsig_ctx* c, const float2* u_dev, int len, int M, DevBuf* out);

}  // namespace vsig::api

using namespace vsig::api;      // the C-ABI sources (and only they include this) name the helpers plainly
