// C-ABI layer: power spectra (vsig_psd_*), their mean / max / min traces over
// a capture or a segment table, per-row band measures, and the polyphase
// filter bank.
#include "vsig_ctx.hpp"

// Frames per batch when one frame takes frame_bytes of scratch: 256 MB worth,
// at least 1, at most nframes.
static long long frames_per_batch(long long frame_bytes, long long nframes) {
  const long long fb = (256LL << 20) / frame_bytes;
  return fb < 1 ? 1 : fb > nframes ? nframes : fb;
}

// body(f0, nb) for the frames [f0, f0 + nb) of each batch of at most fb, up to
// the first status that is not VSIG_OK.
template <class Body>
static int for_frame_batches(long long nframes, long long fb, Body body) {
  for (long long f0 = 0; f0 < nframes; f0 += fb) {
    if (const int rc = body(f0, nframes - f0 < fb ? nframes - f0 : fb)) return rc;
  }
  return VSIG_OK;
}

// The frames of a capture as the per-frame spectrum entries take them.
static int check_frames(vsig_ctx* c, int64_t n, int64_t stride, int32_t nperseg, int64_t hop, int32_t nfft,
                        int64_t nframes) {
  if (stride < 1) return fail(c, VSIG_E_INVALID, "stride must be >= 1");
  if (nperseg < 1 || nperseg > nfft || hop < 1 || n < nperseg)
    return fail(c, VSIG_E_INVALID, "need 1 <= nperseg <= nfft, hop >= 1, n >= nperseg");
  return nframes != (n - nperseg) / hop + 1 ? fail(c, VSIG_E_INVALID, "nframes mismatch") : VSIG_OK;
}

// The table of the trace kernels' plan for nfft (psd_traces.hip).
static int traces_table(vsig_ctx* c, int nfft, const float2** tw) {
  bool two_level;
  const int key = vsig::psd_traces_table(nfft, &two_level);
  return two_level ? get_tw2(c, key, tw) : get_twiddles(c, key, tw);
}

// ---------------------------------------------------------------- spectrum
int vsig_psd_c64_dev(vsig_ctx* c, const void* x, int64_t n, int64_t stride, const float* win,
                     int32_t nperseg, int64_t hop, int32_t nfft, float scale, int32_t shift,
                     float* sxx, int64_t nframes) {
  if (!c || !x || !win || !sxx) return fail(c, VSIG_E_INVALID, "null pointer");
  if (int rc = check_frames(c, n, stride, nperseg, hop, nfft, nframes)) return rc;
  // frames [f0, f0 + nb) as a transform's operand
  auto frames_in = [&](long long f0) {
    return vsig::BigIn{(const float2*)x + f0 * hop * stride, 0, hop * stride, stride, nperseg, nullptr,
                       win, 0, 1.0f};
  };
  if (!pow2_in(nfft, 64, kBigMax)) {
    // any other length: a direct sum (<= 512 points) or Bluestein per frame
    // (bigfft.hip), |X|^2 stored by the transform's output stage; frames in
    // batches of <= 256 MB of scratch
    if (2LL * nfft - 1 > kBigMax) return fail(c, VSIG_E_UNSUPPORTED, "nfft above 2^27");
    long long fb = nframes;
    if (nfft > vsig::kDirectMax) {
      vsig_ctx::Chirp* ch;
      if (const int rc = chirp_plan(c, nfft, &ch)) return rc;
      if (ch->M > 16384) fb = frames_per_batch(ch->M * 8, nframes);
    }
    Timed t(c, "psd");
    return for_frame_batches(nframes, fb, [&](long long f0, long long nb) {
      vsig::BigOut out{sxx + f0 * (long long)nfft, 4, nfft, nfft, nullptr, 0, scale, shift ? 1 : 0};
      return dft_any(c, nfft, nb, frames_in(f0), out, false);
    });
  }
  if (nfft > 16384) {          // long frames: four-step FFT per frame (bigfft.hip)
    BigPlan bp;
    int rc;
    if ((rc = big_plan(c, nfft, &bp))) return rc;
    const long long fb = frames_per_batch((long long)nfft * 8, nframes);
    if ((rc = c->bigtmp.reserve(c, (size_t)(fb * nfft) * sizeof(float2)))) return rc;
    float2* tmp = c->bigtmp.as<float2>();
    Timed t(c, "psd");
    return for_frame_batches(nframes, fb, [&](long long f0, long long nb) {
      HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, nb, frames_in(f0), tmp, bp.tw1, bp.t2, bp.S, bp.hiA,
                                    c->stream));
      return HIPRC(c, vsig::launch_bf_row(2, bp.N1, bp.N2, nb, tmp, nullptr, bp.tw2, scale, sxx + f0 * nfft,
                                          shift, c->stream));
    });
  }
  const float2* tw;
  // pair kernel (>= 256 threads per frame): per-pass table; smaller plans: two-level table
  const bool pair = vsig::psd_plan_threads(nfft) >= 256;
  if (int rc = pair ? get_twiddles(c, nfft, &tw) : get_tw2(c, nfft, &tw)) return rc;
  Timed t(c, "psd");
  return HIPRC(c, vsig::launch_psd(nfft, (const float2*)x, stride, win, nperseg, hop, scale, sxx, nframes,
                                   shift, tw, c->stream));
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
  return HIPRC(c, hipStreamSynchronize(c->stream));
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
  if (int rc = check_frames(c, n, stride, nperseg, hop, nfft, nframes)) return rc;
  int rc;
  if (vsig::psd_traces_in_lds(nfft)) {
    // the transform kernels' epilogue reduces over the frames: one record row per block
    const vsig::PsdTracesPlan p = vsig::psd_traces_plan(nfft, nframes);
    if (p.blocks < 1) return fail(c, VSIG_E_INVALID, "no plan");
    if ((rc = c->ptscratch.reserve(c, (size_t)(p.blocks * nfft) * sizeof(vsig::PsdRec)))) return rc;
    const float2* tw;
    if ((rc = traces_table(c, nfft, &tw))) return rc;
    vsig::PsdRec* rows = c->ptscratch.as<vsig::PsdRec>();
    Timed t(c, "psd_traces");
    HIPCHK(c, vsig::launch_psd_traces(nfft, (const float2*)x, stride, win, nperseg, hop, scale, nframes,
                                      shift, tw, rows, c->stream));
    return HIPRC(c, vsig::launch_psd_traces_merge(rows, p.blocks, nfft, nframes, mean_dev, max_dev, min_dev,
                                                  c->stream));
  }
  // every other length: vsig_psd_c64_dev's own route into a bounded batch of
  // stored frames (256 MB, or the "psd_traces_batch" option), each batch's
  // columns folded into the same record rows, then the same merge
  if (!pow2_in(nfft, 64, kBigMax) && 2LL * nfft - 1 > kBigMax)
    return fail(c, VSIG_E_UNSUPPORTED, "nfft above 2^27");
  long long fb = frames_per_batch((long long)nfft * 4, nframes);
  if (c->psd_traces_batch > 0 && fb > c->psd_traces_batch) fb = c->psd_traces_batch;
  const size_t rb = ((size_t)vsig::kPsdFoldRows * nfft * sizeof(vsig::PsdRec) + 255) & ~(size_t)255;
  if ((rc = c->ptscratch.reserve(c, rb + (size_t)(fb * nfft) * sizeof(float)))) return rc;
  vsig::PsdRec* rows = c->ptscratch.as<vsig::PsdRec>();
  float* batch = reinterpret_cast<float*>(c->ptscratch.as<char>() + rb);
  rc = for_frame_batches(nframes, fb, [&](long long f0, long long nb) {
    const int st = vsig_psd_c64_dev(c, (const float2*)x + f0 * hop * stride, (nb - 1) * hop + nperseg, stride,
                                    win, nperseg, hop, nfft, scale, shift, batch, nb);
    if (st) return st;
    return HIPRC(c, vsig::launch_psd_traces_fold(batch, nb, nfft, f0 == 0, rows, c->stream));
  });
  if (rc) return rc;
  return HIPRC(c, vsig::launch_psd_traces_merge(rows, vsig::kPsdFoldRows, nfft, nframes, mean_dev, max_dev, min_dev,
                                                c->stream));
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
  return HIPRC(c, hipStreamSynchronize(c->stream));
}

// ---------------------------------------------------------------- segmented spectrum traces
int vsig_psd_segments_create(vsig_ctx* c, const vsig_segment_t* segs, int64_t nseg, int64_t n, int32_t nperseg,
                             int64_t hop, int32_t nfft, vsig_psd_segments** out) {
  if (!c || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  int rc;
  if ((rc = check_segment_table(c, segs, nseg, n))) return rc;
  if (nperseg < 1 || hop < 1) return fail(c, VSIG_E_INVALID, "need nperseg >= 1 and hop >= 1");
  if (nfft < nperseg) return fail(c, VSIG_E_INVALID, "nfft must be >= nperseg");
  for (long long s = 0; s < nseg; ++s)      // an empty segment is a row of no frames
    if (!segment_inside(segs[s].start, segs[s].len, n, true))
      return fail(c, VSIG_E_INVALID, segment_name(s, segs[s].start, segs[s].len) + " is outside [0, " +
                                         std::to_string(n) + "]");
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
  if ((rc = check_blocks(c, p->nblocks))) return rc;
  if (nseg > 0) {
    if ((rc = traces_table(c, nfft, &p->tw))) return rc;
    if ((rc = upload(c, p->segs, rows.data(), rows.size()))) return rc;
    if (p->nblocks > 0) {
      if ((rc = upload(c, p->blocks, blocks.data(), blocks.size()))) return rc;
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
  if (!aligned8(x)) return fail(c, VSIG_E_INVALID, "x must be 8-byte aligned");
  if (p->nseg == 0) return VSIG_OK;
  Timed t(c, "psd_segments");
  if (p->nblocks > 0)
    HIPCHK(c, vsig::launch_psd_segments(p->nfft, (const float2*)x, win, p->nperseg, p->hop, scale, shift ? 1 : 0,
                                        p->tw, p->blocks.as<vsig::PsdSegBlock>(), p->nblocks,
                                        p->rows.as<vsig::PsdRec>(), c->stream));
  return HIPRC(c, vsig::launch_psd_segments_merge(p->rows.as<vsig::PsdRec>(), p->segs.as<vsig::PsdSegRows>(), p->nseg,
                                                  p->nfft, p->max_rows, mean, max, min, c->stream));
}

int vsig_band_measure_run(vsig_ctx* c, const double* rows, int64_t nrows, int32_t nbins, int64_t ld, double tail,
                          vsig_band_t* out) {
  static_assert(sizeof(vsig_band_t) == sizeof(vsig::BandRec) && sizeof(vsig_band_t) == 40, "vsig_band_t");
  if (!c) return VSIG_E_INVALID;
  if (nrows < 0 || nrows > 0x7fffffffLL) return fail(c, VSIG_E_INVALID, "nrows must be in [0, 2^31)");
  if (nbins < 1 || ld < nbins) return fail(c, VSIG_E_INVALID, "need nbins >= 1 and ld >= nbins");
  if (!(tail > 0.0 && tail < 0.5)) return fail(c, VSIG_E_INVALID, "tail must be inside (0, 0.5)");
  if (!rows || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!aligned8(rows, out)) return fail(c, VSIG_E_INVALID, "rows and out must be 8-byte aligned");
  if (nrows == 0) return VSIG_OK;
  Timed t(c, "band_measure");
  return HIPRC(c, vsig::launch_band_measure(rows, nrows, nbins, ld, tail, reinterpret_cast<vsig::BandRec*>(out),
                                            c->stream));
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
  if (int rc = get_twiddles(c, nchan, &tw)) return rc;
  Timed t(c, "pfb");
  return HIPRC(c, vsig::launch_pfb(nchan, pt, (const float2*)x, n, h, nframes, (float2*)y, tw, c->stream));
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
