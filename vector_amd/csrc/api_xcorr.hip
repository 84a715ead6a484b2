// C-ABI layer: overlap-save correlation against one template (vsig_xcorr_*,
// vsig_correlate*) or a bank of them (vsig_xcorr_bank_*), and the exact
// re-rank of the peak (refine.hip) behind them.
#include "vsig_ctx.hpp"

constexpr long long kBankMaxL = 4096;
constexpr int kBankMaxK = 4096;

// np.correlate(a, v, mode): F, the start index into the 'full' correlation,
// and the output length (numeric.py); an unknown mode is refused.
static int corr_span(vsig_ctx* c, int mode, long long na, long long nv, long long* F, long long* nout) {
  const long long nmin = na < nv ? na : nv, nmax = na < nv ? nv : na;
  if (mode == VSIG_MODE_FULL) { *F = 0; *nout = na + nv - 1; }
  else if (mode == VSIG_MODE_VALID) { *F = nmin - 1; *nout = nmax - nmin + 1; }
  else if (mode == VSIG_MODE_SAME) { *F = na >= nv ? nmin - 1 - nmin / 2 : nmin / 2; *nout = nmax; }
  else return fail(c, VSIG_E_INVALID, "mode must be VALID, FULL or SAME");
  return VSIG_OK;
}

// A template of L samples against a stream of n: the kernels' offset of the
// first output and the output count, VALID or FULL; false for another mode.
static bool stream_span(int mode, long long n, long long L, long long* off, long long* nout) {
  if (mode == VSIG_MODE_VALID) { *off = 0; *nout = n - L + 1; }
  else if (mode == VSIG_MODE_FULL) { *off = L - 1; *nout = n + L - 1; }
  else return false;
  return true;
}

// templates of 8193 .. 16384 samples use M = 32768 (measured slower than
// M = 16384 for shorter ones, xcorr.hip PlanX32k)
static int os_size_xcorr(long long L) {
  if (L <= 1024) return 4096;
  if (L <= 2048) return 8192;
  if (L <= 8192) return 16384;
  if (L <= 16384) return 32768;
  return 0;
}

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
static int run_refine(vsig_ctx* c, const RefineOperands& op, long long nout, int M, long long hop,
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
    if (int rc = read_refine_keys(c, &keys)) return rc;
    pending_fault = keys.fault;
  }
  int rc;
  if ((rc = c->rscratch.reserve(c, need))) return rc;
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
    if (const int rc = make_spectrum(c, td + p * B, (int)Lp, x->M, &P)) return rc;
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
    int rc;
    if ((rc = ensure_partials(c, nparts))) return rc;
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
  if (!stream_span(mode, n, x->L, &g->off, &g->nout))
    return fail(c, VSIG_E_INVALID, "the template bank supports VALID and FULL");
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
  HIPCHK(c, x->Ps.alloc((size_t)K * x->M * sizeof(float2)));
  if (const int rc = spectrum_rows(c, td, K, (int)L, x->M, x->Ps.as<float2>())) return rc;
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

// np.correlate(a, v, mode): the shorter operand is the template; with
// nv > na the correlation of v by a is computed and stored conj() reversed.
static int correlate_impl(vsig_ctx* c, int in128, const void* a, long long na, const void* v,
                          long long nv, int32_t mode, int out128, void* cout,
                          vsig_peak_t* peak_dev) {
  if (!c || !a || !v) return fail(c, VSIG_E_INVALID, "null pointer");
  if (na < 1 || nv < 1) return fail(c, VSIG_E_INVALID, "empty input");  // numeric.py:865-868
  const long long nmin = na < nv ? na : nv, nmax = na < nv ? nv : na;
  long long F, nout;
  if (int rc = corr_span(c, mode, na, nv, &F, &nout)) return rc;
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

int vsig_xcorr_create(vsig_ctx* c, const void* tmpl, int64_t L, vsig_xcorr** out) {
  if (!c || !tmpl || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  if (L < 1) return fail(c, VSIG_E_INVALID, "template length must be >= 1");
  std::unique_ptr<vsig_xcorr> x(new vsig_xcorr(c));
  int rc;
  if ((rc = upload(c, x->tmpl, static_cast<const float2*>(tmpl), (size_t)L))) return rc;
  rc = xcorr_build(c, x->tmpl.as<float2>(), L, x.get());
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
  if (!stream_span(mode, n, x->L, &off, &nout))
    return fail(c, VSIG_E_INVALID, "streaming correlation supports VALID and FULL");
  if (nout < 1) return fail(c, VSIG_E_INVALID, "stream shorter than the template");
  // np.correlate(s, p): output o is full index (L - 1 - off) + o
  const RefineOperands op{s, n, x->tmpl.data(), x->L, 0, (x->L - 1) - off};
  return xcorr_run(x, (const float2*)s, n, off, nout, cout ? 1 : 0, (float2*)cout, peak_dev, &op,
                   nullptr, true);
}

int vsig_xcorr_bank_create(vsig_ctx* c, const void* tmpls, int32_t K, int64_t L, vsig_xcorr_bank** out) {
  int rc;
  if ((rc = bank_check(c, tmpls, K, L, out))) return rc;
  DevBuf td;      // freed after bank_create's synchronise
  if ((rc = upload(c, td, static_cast<const float2*>(tmpls), (size_t)K * (size_t)L))) return rc;
  rc = bank_create(c, td.as<float2>(), K, L, out);
  (void)hipStreamSynchronize(c->stream);
  return rc;
}

int vsig_xcorr_bank_create_dev(vsig_ctx* c, const void* tmpls_dev, int32_t K, int64_t L,
                               vsig_xcorr_bank** out) {
  if (const int rc = bank_check(c, tmpls_dev, K, L, out)) return rc;
  return bank_create(c, (const float2*)tmpls_dev, K, L, out);
}

void vsig_xcorr_bank_free(vsig_xcorr_bank* x) { delete x; }

int vsig_xcorr_bank_plan(const vsig_xcorr_bank* x, int64_t n, int32_t mode, int32_t* M, int64_t* hop,
                         int64_t* nblocks, int64_t* grid) {
  if (!x) return VSIG_E_INVALID;
  if (!M || !hop || !nblocks || !grid) return fail(x->ctx, VSIG_E_INVALID, "null pointer");
  BankGeom g;
  if (const int rc = bank_geom(x, n, mode, &g)) return rc;
  *M = x->M; *hop = g.hop; *nblocks = g.nblocks; *grid = g.grid;
  return VSIG_OK;
}

int vsig_xcorr_bank_exec_dev(vsig_xcorr_bank* x, const void* s, int64_t n, int32_t mode, void* cout,
                             vsig_peak_t* peaks_dev) {
  if (!x) return VSIG_E_INVALID;
  vsig_ctx* c = x->ctx;
  if (!s || !peaks_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  BankGeom g;
  int rc;
  if ((rc = bank_geom(x, n, mode, &g))) return rc;
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

int vsig_correlate_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t na, const void* v,
                       int64_t nv, int32_t mode, int32_t out_dtype, void* cout,
                       vsig_peak_t* peak_dev) {
  if (int rc = check_complex(c, dtype, out_dtype)) return rc;
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
  if (int rc = check_complex(c, dtype, out_dtype)) return rc;
  const size_t es = dtype_bytes(dtype), eo = dtype_bytes(out_dtype);
  long long F, nout;
  if (int rc = corr_span(c, mode, na, nv, &F, &nout)) return rc;
  int rc;
  if ((rc = stage_in(c, 0, a, (size_t)na * es)) || (rc = stage_in(c, 1, v, (size_t)nv * es)) ||
      (cout && (rc = c->stage[2].reserve(c, (size_t)nout * eo))))
    return rc;
  rc = vsig_correlate_dev(c, dtype, c->stage[0].data(), na, c->stage[1].data(), nv, mode, out_dtype,
                          cout ? c->stage[2].data() : nullptr, nullptr);
  if (rc || (cout && (rc = stage_out(c, cout, c->stage[2], (size_t)nout * eo))) ||
      (peak && (rc = stage_out(c, peak, c->result, sizeof(vsig_peak_t)))))
    return rc;
  return HIPRC(c, hipStreamSynchronize(c->stream));
}

int vsig_correlate_c64(vsig_ctx* c, const void* a, int64_t na, const void* v, int64_t nv,
                       int32_t mode, void* cout, vsig_peak_t* peak) {
  return vsig_correlate(c, VSIG_DTYPE_C64, a, na, v, nv, mode, VSIG_DTYPE_C64, cout, peak);
}

// np.correlate(a, v, mode)'s |c| for every output in numpy's operation order
// (refine.hip, values mode), then np.mean / np.std of it as vsig_abs_stats_dev.
int vsig_correlate_stats_dev(vsig_ctx* c, int32_t dtype, const void* a, int64_t na, const void* v,
                             int64_t nv, int32_t mode, double* stats_dev) {
  if (!c || !a || !v || !stats_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (na < 1 || nv < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (int rc = check_complex(c, dtype)) return rc;
  long long F, nout;
  if (int rc = corr_span(c, mode, na, nv, &F, &nout)) return rc;
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
  return HIPRC(c, vsig::launch_np_stats(VSIG_DTYPE_F64, vals, nout, stats_dev, c->sscratch.data(), c->stream));
}
