// C-ABI layer: transforms of any length (four-step and Bluestein plans over
// bigfft.hip), the plans' spectra, and the entry points built on them
// (vsig_dft_dev, vsig_resample_dev, vsig_filter_channel_dev).
#include "vsig_ctx.hpp"

namespace vsig::api {

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
static int big_plan_fwd(vsig_ctx* c, long long M, const float2* u, long long len, float2* S) {
  BigPlan bp;
  int rc;
  if ((rc = big_plan(c, M, &bp))) return rc;
  if ((rc = c->bigtmp.reserve(c, (size_t)M * sizeof(float2)))) return rc;
  float2* tmp = c->bigtmp.as<float2>();
  vsig::BigIn in{u, 0, 0, 1, len, nullptr, nullptr, 0, 1.0f / (float)M};
  HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, 1, in, tmp, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
  const vsig::BigOut o{S, 0, M, M, nullptr, 0, 1.0f};
  return HIPRC(c, vsig::launch_bf_row(3, bp.N1, bp.N2, 1, tmp, nullptr, bp.tw2, 1.0f, nullptr, 0, c->stream, &o));
}

int spectrum_rows(vsig_ctx* c, const float2* src_dev, long long rows, int len, int M, float2* dst_dev) {
  const float2* tw;
  if (const int rc = get_twiddles(c, M, &tw)) return rc;
  for (long long r = 0; r < rows; ++r)
    HIPCHK(c, vsig::launch_spectrum_prep(M, src_dev + r * len, len, 1.0f / (float)M, dst_dev + r * M, tw,
                                         c->stream));
  return VSIG_OK;
}

int make_spectrum(vsig_ctx* c, const float2* u_dev, int len, int M, DevBuf* out) {
  DevBuf S;
  HIPCHK(c, S.alloc((size_t)M * sizeof(float2)));
  const int rc = M > 16384 ? big_plan_fwd(c, M, u_dev, len, S.as<float2>())
                           : spectrum_rows(c, u_dev, 1, len, M, S.as<float2>());
  if (rc) return rc;
  *out = std::move(S);
  return VSIG_OK;
}

int chirp_plan(vsig_ctx* c, long long N, vsig_ctx::Chirp** out) {
  auto it = c->chirps.find(N);
  if (it != c->chirps.end()) { *out = &it->second; return VSIG_OK; }
  long long M = 256;
  while (M < 2 * N - 1) M *= 2;
  if (M > kBigMax) return fail(c, VSIG_E_UNSUPPORTED, "transform length above 2^27");
  BigPlan bp;
  if (int rc = big_plan(c, M, &bp)) return rc;
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

int dft_any(vsig_ctx* c, long long N, long long batch, vsig::BigIn in, vsig::BigOut out, bool inverse) {
  int rc;
  in.conj = out.conj = inverse ? 1 : 0;
  in.nvalid = in.nvalid < N ? in.nvalid : N;
  // a power of two with an in-LDS plan is its own transform: one N-point FFT
  // (inverse by conj) instead of two chirp products around a 2N-point
  // convolution, whose three transforms cost ~2.7e-7 of accuracy against ~1.3e-7
  if (N >= 256 && N <= 16384 && (N & (N - 1)) == 0) {
    const float2* tw;
    if ((rc = get_twiddles(c, (int)N, &tw))) return rc;
    return HIPRC(c, vsig::launch_bf_small(1, (int)N, batch, in, out, nullptr, tw, c->stream));
  }
  // every other length up to 512 points (256 and 512 have gone above): the sum
  // itself, in double, one block per frame -- exact to the store's rounding,
  // where a chirp-z of M = 256 .. 1024 points put the engine's error in the
  // result three times (bigfft.hip: bf_direct_kernel)
  if (N <= vsig::kDirectMax) return HIPRC(c, vsig::launch_bf_direct((int)N, batch, in, out, c->stream));
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
    HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, batch, in, tmp, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
    return HIPRC(c, vsig::launch_bf_row(3, bp.N1, bp.N2, batch, tmp, nullptr, bp.tw2, 1.0f, nullptr, 0, c->stream,
                                        &out));
  }
  vsig_ctx::Chirp* ch;
  if ((rc = chirp_plan(c, N, &ch))) return rc;
  BigPlan bp;
  if ((rc = big_plan(c, ch->M, &bp))) return rc;
  const float2* B = ch->B.as<float2>();
  in.chirp = out.chirp = ch->c.as<float2>();
  if (bp.N1 == 1) return HIPRC(c, vsig::launch_bf_small(0, (int)ch->M, batch, in, out, B, bp.tw2, c->stream));
  if ((rc = c->bigtmp.reserve(c, (size_t)(batch * ch->M) * sizeof(float2)))) return rc;
  float2* tmp = c->bigtmp.as<float2>();
  HIPCHK(c, vsig::launch_bf_col(bp.N1, bp.N2, batch, in, tmp, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
  HIPCHK(c, vsig::launch_bf_row(0, bp.N1, bp.N2, batch, tmp, B, bp.tw2, 1.0f, nullptr, 0, c->stream));
  return HIPRC(c, vsig::launch_bf_icol(bp.N1, bp.N2, batch, tmp, out, bp.tw1, bp.t2, bp.S, bp.hiA, c->stream));
}

// One contiguous frame of n elements of `dtype` (complex64 or complex128).
static vsig::BigIn contiguous_in(const void* x, int dtype, long long n) {
  return vsig::BigIn{x, dtype == VSIG_DTYPE_C128 ? 1 : 0, n, 1, n, nullptr, nullptr, 0, 1.0f};
}

}  // namespace vsig::api

// split_channels.py's frequency axis, as numpy forms it: fftfreq(n, 1/sr)[k]
// * sr + CENTER_FREQ (k >= 0 here, or -1), no contraction into FMAs.
#pragma clang fp contract(off)
static double channel_freq(long long k, long long n, double sr, double center) {
  const double d = 1.0 / sr;
  const double val = 1.0 / ((double)n * d);
  const double f = (double)k * val;
  const double g = f * sr;
  return g + center;
}
#pragma clang fp contract(on)

int vsig_dft_dev(vsig_ctx* c, int32_t dtype, const void* x, int64_t n, int64_t batch, int32_t inverse,
                 int32_t out_dtype, void* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1 || batch < 1) return fail(c, VSIG_E_INVALID, "need n >= 1 and batch >= 1");
  if (int rc = check_complex(c, dtype, out_dtype)) return rc;
  vsig::BigOut out{y, out_dtype == VSIG_DTYPE_C128 ? 1 : 0, n, n, nullptr, 0,
                   inverse ? (float)(1.0 / (double)n) : 1.0f};
  Timed t(c, "dft");
  return dft_any(c, n, batch, contiguous_in(x, dtype, n), out, inverse != 0);
}

int vsig_resample_dev(vsig_ctx* c, int32_t dtype, const void* x, int64_t n, int64_t num,
                      int32_t real_input, void* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 1 || num < 1) return fail(c, VSIG_E_INVALID, "need n >= 1 and num >= 1");
  if (int rc = check_complex(c, dtype)) return rc;
  int rc;
  if ((rc = c->spec[0].reserve(c, (size_t)n * 8)) || (rc = c->spec[1].reserve(c, (size_t)num * 8)))
    return rc;
  float2* X = c->spec[0].as<float2>();
  float2* Y = c->spec[1].as<float2>();
  Timed t(c, "resample");
  vsig::BigOut ox{X, 0, n, n, nullptr, 0, 1.0f};
  if ((rc = dft_any(c, n, 1, contiguous_in(x, dtype, n), ox, false))) return rc;
  HIPCHK(c, vsig::launch_resample_spectrum(X, n, num, Y, c->stream));
  // y = ifft(Y) * num / n  ->  the inverse DFT's 1/num and num/n leave 1/n
  vsig::BigOut oy{y, real_input ? 3 : 0, num, num, nullptr, 0, (float)(1.0 / (double)n)};
  return dft_any(c, num, 1, contiguous_in(Y, VSIG_DTYPE_C64, num), oy, true);
}

int vsig_filter_channel_dev(vsig_ctx* c, int32_t dtype, const void* x, int64_t n,
                            double center_freq, double sample_rate, double bandwidth,
                            double* y) {
  if (int rc = check_array(c, c && x && y, n)) return rc;
  if (n > 1 && (n & 1))
    return fail(c, VSIG_E_INVALID, "odd length: the conjugate mirror's halves differ (numpy "
                                   "raises on the shape mismatch)");
  if (int rc = check_complex(c, dtype)) return rc;
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
    return HIPRC(c, vsig::launch_channel_direct(dtype == VSIG_DTYPE_C128, x, n, ka, kb, c->spec[0].as<double2>(),
                                                c->spec[1].as<double2>(), y, c->stream));
  }
  if ((rc = c->spec[0].reserve(c, (size_t)n * 8)) || (rc = c->spec[1].reserve(c, (size_t)n * 8)))
    return rc;
  float2* X = c->spec[0].as<float2>();
  float2* F = c->spec[1].as<float2>();
  Timed t(c, "channel");
  vsig::BigOut ox{X, 0, n, n, nullptr, 0, 1.0f};
  if ((rc = dft_any(c, n, 1, contiguous_in(x, dtype, n), ox, false))) return rc;
  HIPCHK(c, vsig::launch_channel_mask(X, n, sample_rate, center, center_freq - bandwidth / 2,
                                      center_freq + bandwidth / 2, F, c->stream));
  vsig::BigOut oy{y, 2, n, n, nullptr, 0, (float)(1.0 / (double)n)};
  return dft_any(c, n, 1, contiguous_in(F, VSIG_DTYPE_C64, n), oy, true);
}
