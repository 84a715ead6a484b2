// The one-frame correlators' epilogue (xcorr.hip xcorr_os_kernel, xcorr_bank.hip):
// optional store of c, per-wave |c| partials.
#pragma once
#include "os_common.hpp"

namespace vsig {

__device__ __forceinline__ void put_c(float2* p, float2 v, bool accum) {
  *p = accum ? cadd(*p, v) : v;
}

template <class P>
__device__ __forceinline__ void xcorr_epilogue(const float2* v, long long b, long long hop,
                                               long long nout, float2* __restrict__ c,
                                               int store_mode, PeakPartial* partials, int t) {
  const long long ob = b * hop;                         // block's first output
  const long long rem = nout - ob;
  const int lim = rem < hop ? (int)rem : (int)hop;
  const bool rev = store_mode & 4;
  const bool accum = store_mode & 8;
  const int smode = store_mode & 3;
  if (smode == 1) {
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      const int i = out_index<P>(t, e);
      if (i < lim) put_c(c + ob + (unsigned)i, cconj(v[e]), accum);
    }
  } else if (smode == 2) {
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      const int i = out_index<P>(t, e);
      if (i < lim) put_c(c + (nout - 1 - ob) - i, v[e], accum);
    }
  }
  if (!partials) return;
  // branch-free peak / sums.  A thread's output indices rise with e, so a
  // strict '>' keeps the first maximum; in the reversed index space (rev)
  // '>=' keeps the last raw index, i.e. the first reversed one.
  float m = -1.f, s1 = 0.f, s2 = 0.f;
  int mi = 0;
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int i = out_index<P>(t, e);
    const bool ok = i < lim;
    const float a2r = v[e].x * v[e].x + v[e].y * v[e].y;
    const float a2 = ok ? a2r : -1.f;
    const bool take = (a2 > m) | (rev & (a2 == m) & ok);
    m = take ? a2 : m;
    mi = take ? i : mi;
    s1 += ok ? __builtin_amdgcn_sqrtf(a2r) : 0.f;   // v_sqrt_f32 (1 ulp), not the IEEE expansion
    s2 += ok ? a2r : 0.f;
  }
  wave_partial_f(m, mi, s1, s2, rev, ob, nout, partials + b * (P::TF / 64) + (t >> 6));
}

}  // namespace vsig
