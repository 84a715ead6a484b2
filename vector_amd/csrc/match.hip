// All-pairs burst similarity (gfx950): K packets p_k of lengths L_k <= 8192,
// packed back to back, every pair's correlation peak in one pass.
//   E_k     = sum_j |p_k[j]|^2
//   c_ab[l] = sum_j p_a[j + l] conj(p_b[j]),  l in [-(L_b - 1), L_a - 1]
//   peak[a,b] = max_l |c_ab[l]|, lag[a,b] = the smallest l that attains it
// on one in-LDS plan of N >= 2 L_max - 1 points (1024 one-wave / 4096 / 8192 /
// 16384; palindromic, as the template bank's: a spectrum's register layout is
// the next transform's operand layout).
//   match_spectra_kernel  one block per packet: P_k = FFT_N(p_k zero-padded) in
//     natural order into row k of the plan's K x N workspace; E_k as a double
//     sum of the fp32 squares (per thread in element order, then block_fold,
//     block_ops.hpp); the diagonal record (a, a).
//   match_pairs_kernel    a unit is (a, b0, nb): packet a against b0 .. b0 + nb
//     - 1, all > a.  The block loads P_a / N into registers once per unit (it
//     transforms nothing for a) and for every b forms conj(P_a / N) P_b, runs
//     one transform -- result i is conj(c_ab[l]) with l = i for i < L_a and l =
//     i - N for i > N - L_b, nothing aliases because N >= L_a + L_b - 1 -- and
//     takes the first maximum of the fp32 |c|^2 over those positions only, ties
//     to the smaller l: per thread, per wave (DPP), then the waves in order;
//     thread 0 writes peak (v_sqrt) and lag for (a, b) and the mirror (b, a).
//     K + K (K - 1) / 2 transforms where a loop of single correlations runs
//     three a pair.  The grid is persistent (a block walks units u, u + grid,
//     ...); no atomics, every output element is written once, and a pair's
//     record is a function of its two packets and N alone.
// Special values are decided from the energies: a non-finite E_a or E_b gives
// peak NaN and lag 0, a zero one peak 0 and lag 0.
#include "os_common.hpp"

namespace vsig {

template <class P>
constexpr int match_waves_per_eu() { return P::E >= 32 ? 2 : 1; }   // the bank kernel's budget

template <class P>
__global__ __launch_bounds__(P::TF) void match_spectra_kernel(
    const float2* __restrict__ packed, const long long* __restrict__ offsets, int K,
    float2* __restrict__ W, double* __restrict__ energy, float* __restrict__ peak,
    int* __restrict__ lag, const float2* __restrict__ tw) {
  static_assert(P::R[0] == P::RL, "the pair kernel needs a palindromic plan");
  __shared__ __attribute__((aligned(16))) float2 lds[lds_size<P>()];
  __shared__ Sums<1> wsum[P::TF / 64];
  const int t = threadIdx.x;
  const int k = blockIdx.x;
  const long long o = offsets[k];
  const long long L = offsets[k + 1] - o;
  float2 wa[nanch_total<P>()];
  load_anchors<P>(wa, tw, t);
  float2 X[P::E];
  load_segment<P>(X, packed + o, 0, L, t);        // L < N: the bounds-tested path, zero fill
  Sums<1> s{{0.0}};
#pragma unroll
  for (int e = 0; e < P::E; ++e) s.s[0] += (double)(X[e].x * X[e].x + X[e].y * X[e].y);
  // before the transform: behind it the fold's value would stay live across
  // it and double the kernel's VGPRs (profiles/block_ops_ab.md)
  block_fold<P::TF / 64>(s, wsum);
  if (t == 0) {
    const double E = s.s[0];
    energy[k] = E;
    const long long d = (long long)k * K + k;
    peak[d] = isfinite(E) ? (float)E : __builtin_nanf("");
    lag[d] = 0;
  }
  fft_frame_anch<P>(X, lds, wa, t);
  float2* __restrict__ Wk = W + (long long)k * P::N;
#pragma unroll
  for (int e = 0; e < P::E; ++e) Wk[out_index<P>(t, e)] = X[e];
}

template <class P>
__global__ __launch_bounds__(P::TF, match_waves_per_eu<P>()) void match_pairs_kernel(
    const float2* __restrict__ W, const long long* __restrict__ offsets,
    const double* __restrict__ energy, const MatchUnit* __restrict__ units, long long nunits, int K,
    float* __restrict__ peak, int* __restrict__ lag, const float2* __restrict__ tw) {
  static_assert(P::R[0] == P::RL, "the spectrum's layout must be the transform's operand layout");
  constexpr int NW = P::TF / 64;
  __shared__ __attribute__((aligned(16))) float2 lds[lds_size<P>()];
  __shared__ float red_m[NW];
  __shared__ int red_l[NW];
  const int t = threadIdx.x;
  float2 wa[nanch_total<P>()];
  load_anchors<P>(wa, tw, t);
  constexpr float kInvN = 1.0f / (float)P::N;      // a power of two: exact
  for (long long u = blockIdx.x; u < nunits; u += gridDim.x) {
    const MatchUnit un = units[u];
    const int a = un.a;
    const int La = (int)(offsets[a + 1] - offsets[a]);
    const float2* __restrict__ Pa = W + (long long)a * P::N;
    float2 X[P::E];
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      const float2 p = Pa[out_index<P>(t, e)];
      X[e] = make_float2(p.x * kInvN, p.y * kInvN);
    }
    for (int q = 0; q < un.nb; ++q) {
      const int b = un.b0 + q;
      const int Lb = (int)(offsets[b + 1] - offsets[b]);
      const float2* __restrict__ Pb = W + (long long)b * P::N;
      float2 v[P::E];
#pragma unroll
      for (int e = 0; e < P::E; ++e) v[e] = cmul(cconj(X[e]), Pb[out_index<P>(t, e)]);
      fft_frame_anch<P>(v, lds, wa, t);
      // first maximum over the valid lags: i < La is l = i, i > N - Lb is l = i - N
      const int neg0 = P::N - (Lb - 1);
      float m = -1.f, s1 = 0.f, s2 = 0.f;
      int ml = 0;
#pragma unroll
      for (int e = 0; e < P::E; ++e) {
        const int i = out_index<P>(t, e);
        const bool pos = i < La;
        const bool ok = pos | (i >= neg0);
        const int l = pos ? i : i - P::N;
        const float a2 = ok ? v[e].x * v[e].x + v[e].y * v[e].y : -1.f;
        const bool take = (a2 > m) | ((a2 == m) & ok & (l < ml));
        m = take ? a2 : m;
        ml = take ? l : ml;
      }
      // lane 63 ends with the wave's (max, smallest lag on ties)
      wave_peak_dpp(m, ml, s1, s2, false);
      if ((t & 63) == 63) { red_m[t >> 6] = m; red_l[t >> 6] = ml; }
      __syncthreads();        // the next transform's barriers keep the next writes behind this read
      if (t == 0) {
        float bm = red_m[0];
        int bl = red_l[0];
        for (int w = 1; w < NW; ++w) {
          const float om = red_m[w];
          const int ol = red_l[w];
          const bool take = (om > bm) | ((om == bm) & (ol < bl));
          bm = take ? om : bm;
          bl = take ? ol : bl;
        }
        const double Ea = energy[a], Eb = energy[b];
        float pk = __builtin_amdgcn_sqrtf(bm);
        if (!isfinite(Ea) || !isfinite(Eb)) { pk = __builtin_nanf(""); bl = 0; }
        else if (Ea == 0.0 || Eb == 0.0) { pk = 0.f; bl = 0; }
        else if (!(bm >= 0.f)) bl = 0;             // every |c|^2 NaN (fp32 overflow): NaN, lag 0
        const long long ab = (long long)a * K + b, ba = (long long)b * K + a;
        peak[ab] = pk; lag[ab] = bl;
        peak[ba] = pk; lag[ba] = -bl;
      }
    }
  }
}

template <class F>
static hipError_t match_plan_switch(int N, F f) {
  if (N == 1024) f(Plan1024s{});
  else if (N == 4096) f(Plan4096{});
  else if (N == 8192) f(Plan8192{});
  else if (N == 16384) f(Plan16384{});
  else return hipErrorInvalidValue;
  return hipSuccess;
}

hipError_t match_geom(int N, int* table_key, long long* resident) {
  return match_plan_switch(N, [&](auto plan) {
    using PL = decltype(plan);
    *table_key = N == 1024 ? -1024 : N;
    *resident = persistent_grid(match_pairs_kernel<PL>, PL::TF, 0x7fffffffLL);
  });
}

hipError_t launch_match(int N, const float2* packed, const long long* offsets, int K, float2* W,
                        double* energy, const MatchUnit* units, long long nunits, long long grid,
                        float* peak, int* lag, const float2* tw, hipStream_t st) {
  if (K <= 0 || (nunits > 0 && grid <= 0)) return hipErrorInvalidValue;
  const hipError_t e = match_plan_switch(N, [&](auto plan) {
    using PL = decltype(plan);
    hipLaunchKernelGGL(match_spectra_kernel<PL>, dim3((unsigned)K), dim3(PL::TF), 0, st, packed, offsets,
                       K, W, energy, peak, lag, tw);
    if (nunits > 0)
      hipLaunchKernelGGL(match_pairs_kernel<PL>, dim3((unsigned)grid), dim3(PL::TF), 0, st,
                         (const float2*)W, offsets, (const double*)energy, units, nunits, K, peak, lag, tw);
  });
  return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace vsig
