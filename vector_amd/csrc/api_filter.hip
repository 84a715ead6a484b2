// C-ABI layer: overlap-save FIR filters (vsig_fir_*), with the fused mixer,
// and the per-burst mix-down and band filter of a burst table (vsig_isolate_*).
#include "vsig_ctx.hpp"

constexpr int kFirPartTaps = 8192;
constexpr int kIsoMaxTaps = 511, kIsoMaxFilters = 4096;

// Overlap-save block sizes (measured best on MI355X for the chain's sizes).
static int os_size_fir(int ntaps) {
  if (ntaps <= 256) return 1024;      // one-wave blocks; hop >= 769 (measured best at 255 taps)
  if (ntaps <= 512) return 4096;
  if (ntaps <= 2048) return 8192;
  if (ntaps <= 8192) return 16384;
  return 0;
}

// Real taps as the complex64 taps the spectra are built from.
static std::vector<float2> widen_taps(const float* taps, size_t n) {
  std::vector<float2> tc(n);
  for (size_t i = 0; i < n; ++i) tc[i] = make_float2(taps[i], 0.f);
  return tc;
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
  int rc;
  if ((rc = upload(c, hd, static_cast<const float2*>(taps), (size_t)ntaps))) return rc;
  rc = make_spectrum(c, hd.as<float2>(), ntaps, M, &Hs);
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
      return HIPRC(c, vsig::launch_fir_poly((const float2*)x, nhist + n, nhist, f->G.as<float2>(), lo2, hop,
                                            (float2*)y, tw, twd, c->stream, mix));
    }
    if ((rc = get_twiddles(c, -1024, &tw)) || (rc = get_twiddles(c, -1024 / f->decim, &twd))) return rc;
    Timed t(c, "fir");
    return HIPRC(c, vsig::launch_fir_dec(D, (const float2*)x, nhist + n, nhist, f->Hs.as<float2>(), lo2, hop,
                                         (float2*)y, tw, twd, c->stream, mix));
  }
  if (mix && f->M != 1024)
    return fail(c, VSIG_E_UNSUPPORTED, "fused mixer needs the 1024-point block (ntaps <= 256)");
  rc = get_twiddles(c, f->M == 1024 ? -1024 : f->M, &tw);
  if (rc) return rc;
  Timed t(c, "fir");
  return HIPRC(c, vsig::launch_fir_os(f->M, (const float2*)x, nhist + n, nhist, f->Hs.as<float2>(), f->ntaps,
                                      f->hop, f->decim, (float2*)y, tw, c->stream, mix));
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
  const std::vector<float2> tc = widen_taps(taps, (size_t)ntaps);
  vsig_fir* f = nullptr;
  int rc;
  if ((rc = vsig_fir_create(c, tc.data(), ntaps, decim, &f))) return rc;
  const std::unique_ptr<vsig_fir> owner(f);     // freed on every path below
  const size_t bx = (size_t)n * 8, by = (size_t)ny * 8;
  if ((rc = stage_in(c, 0, x, bx)) || (rc = c->stage[1].reserve(c, by)) ||
      (rc = vsig_fir_exec_dev(f, c->stage[0].data(), n, c->stage[1].data(), ny)) ||
      (rc = stage_out(c, y, c->stage[1], by)))
    return rc;
  return HIPRC(c, hipStreamSynchronize(c->stream));
}

// ---------------------------------------------------------------- burst isolation
int vsig_isolate_create(vsig_ctx* c, const vsig_isolate_seg_t* segs, int64_t nseg, int64_t n, const float* taps,
                        int32_t nfilters, int32_t ntaps, double sr, vsig_isolate** out) {
  static_assert(sizeof(vsig_isolate_seg_t) == 32 && sizeof(vsig::IsoFrame) == 32, "table records");
  constexpr int M = vsig::kIsoM;
  if (!c || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  int rc;
  if ((rc = check_segment_table(c, segs, nseg, n))) return rc;
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
    if (!segment_inside(segs[s].start, segs[s].len, n, false))     // every segment owns output
      return fail(c, VSIG_E_INVALID, segment_name(s, segs[s].start, segs[s].len) + " is empty or outside [0, " +
                                         std::to_string(n) + ")");
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
  if ((rc = check_blocks(c, (p->nframes + 1) / 2))) return rc;
  if (nseg > 0) {
    if ((rc = get_twiddles(c, -M, &p->tw))) return rc;
    HIPCHK(c, p->Hs.alloc((size_t)nfilters * M * sizeof(float2)));
    // Hs row f = FFT_M(h_f) / M, as vsig_fir_create builds its one
    const std::vector<float2> hc = widen_taps(taps, (size_t)nfilters * ntaps);
    DevBuf hd;                     // the taps on the device, dropped on return
    if (!(rc = upload(c, hd, hc.data(), hc.size())) && !(rc = upload(c, p->frames, frames.data(), frames.size())))
      rc = spectrum_rows(c, hd.as<float2>(), nfilters, ntaps, M, p->Hs.as<float2>());
    (void)hipStreamSynchronize(c->stream);           // hd and the host tables go out of scope
    if (rc) return rc;
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
  if (!aligned8(x, y)) return fail(c, VSIG_E_INVALID, "x and y must be 8-byte aligned");
  if (p->nseg == 0) return VSIG_OK;
  Timed t(c, "isolate");
  return HIPRC(c, vsig::launch_isolate((const float2*)x, p->n, p->Hs.as<float2>(), p->lo, (float2*)y,
                                       p->frames.as<vsig::IsoFrame>(), p->nframes, p->tw, c->stream));
}
