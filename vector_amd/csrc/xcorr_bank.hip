// Template bank (gfx950): K templates of one length L against one stream in
// one pass -- the frequency search (one reference mixed at K offsets) and any
// "which of these K packets, and where" question.
//   c_k[o] = sum_{j<L} s[o - off + j] conj(p_k[j]),  k < K, o in [0, nout)
// by overlap-save on the in-LDS plans (M = 4096 / 8192 / 16384).  A block
// transforms a segment once, keeps its spectrum X in registers, and for every
// k forms conj(X) Ps[k], runs the second transform and the correlator's fused
// epilogue (xcorr_epilogue: optional store, first maximum of the fp32 |c|^2,
// v_sqrt sum of |c|, sum of |c|^2): K + 1 transforms per segment where K
// single-template passes run 2 K, and the stream is read once.
// The grid is persistent (a block walks segments b, b + grid, ...).  The next
// segment is not prefetched as in xcorr_os_kernel: its load is amortised over
// K inverse transforms, and X, the product and the anchors leave no room for a
// third frame at two blocks per CU (M = 8192: 64 values a thread already).
// Record k is the unrefined fp32 result -- no exact re-rank runs on a bank: the
// first maximum of the fp32 |c|^2, peak = sqrt of it, sums in double over the
// per-wave fp32 partials (what the option "refine" = 0 gives for M <= 8192).
// A NaN |c|^2 is never the maximum; the sums become NaN.
#include "xcorr_epilogue.hpp"

namespace vsig {

// Waves per SIMD the kernel is compiled for: the 32-value plan (M = 8192: X and
// the product are 128 VGPRs) is held to 256 registers so that two blocks share
// a CU and one's barriers and loads run under the other's butterflies.
template <class P>
constexpr int bank_waves_per_eu() { return P::E >= 32 ? 2 : 1; }

// partials[(k nblocks + b) waves + wave]; c (optional): c[k nout + o].
template <class P>
__global__ __launch_bounds__(P::TF, bank_waves_per_eu<P>()) void xcorr_bank_kernel(
    const float2* __restrict__ s, long long n, const float2* __restrict__ Ps, int K, long long off,
    long long nout, long long hop, float2* __restrict__ c, PeakPartial* __restrict__ partials,
    long long nblocks, const float2* __restrict__ tw) {
  static_assert(P::R[0] == P::RL, "overlap-save needs a palindromic plan");
  __shared__ __attribute__((aligned(16))) float2 lds[lds_size<P>()];
  const int t = threadIdx.x;
  long long b = blockIdx.x;
  if (b >= nblocks) return;
  float2 wa[nanch_total<P>()];
  load_anchors<P>(wa, tw, t);
  const long long kparts = nblocks * (P::TF / 64);
  for (; b < nblocks; b += gridDim.x) {
    float2 X[P::E];
    load_segment<P>(X, s, b * hop - off, n, t);
    fft_frame_anch<P>(X, lds, wa, t);
    for (int k = 0; k < K; ++k) {
      const float2* __restrict__ Pk = Ps + (long long)k * P::N;
      float2 v[P::E];
#pragma unroll
      for (int e = 0; e < P::E; ++e) v[e] = cmul(cconj(X[e]), Pk[out_index<P>(t, e)]);
      fft_frame_anch<P>(v, lds, wa, t);
      xcorr_epilogue<P>(v, b, hop, nout, c ? c + (long long)k * nout : nullptr, c ? 1 : 0,
                        partials + (long long)k * kparts, t);
    }
  }
}

// Record k from its group of nparts partials, one block per k, in the fixed
// order of partial_finalize (reduce.hip): the same call gives the same bits.
__global__ __launch_bounds__(1024) void bank_finalize(const PeakPartial* __restrict__ parts,
                                                      long long nparts, PeakPartial* __restrict__ out) {
  const PeakPartial* g = parts + (long long)blockIdx.x * nparts;
  double m = -1.0, s1 = 0.0, s2 = 0.0;
  long long mi = 0x7fffffffffffffffLL;
  for (long long i = threadIdx.x; i < nparts; i += 1024) {
    const PeakPartial p = g[i];
    betterd(m, mi, p.max2, p.idx);
    s1 += p.sum_abs;
    s2 += p.sum_abs2;
  }
  __shared__ PeakPartial tmp[1];
  block_partial<1024>(m, mi, s1, s2, tmp);
  __syncthreads();
  if (threadIdx.x == 0) {
    PeakPartial r = tmp[0];
    r.max2 = sqrt(r.max2);
    out[blockIdx.x] = r;
  }
}

template <class F>
static hipError_t bank_plan_switch(int M, F f) {
  if (M == 4096) f(Plan4096{});
  else if (M == 8192) f(Plan8192{});
  else if (M == 16384) f(Plan16384{});
  else return hipErrorInvalidValue;
  return hipSuccess;
}

hipError_t xcorr_bank_geom(int M, long long nblocks, int* waves, long long* grid) {
  return bank_plan_switch(M, [&](auto plan) {
    using PL = decltype(plan);
    *waves = PL::TF / 64;
    *grid = persistent_grid(xcorr_bank_kernel<PL>, PL::TF, nblocks);
  });
}

hipError_t launch_xcorr_bank(int M, const float2* s, long long n, const float2* Ps, int K,
                             long long off, long long nout, long long hop, float2* c,
                             PeakPartial* partials, const float2* tw, hipStream_t st) {
  if (nout <= 0 || K <= 0 || hop <= 0) return hipErrorInvalidValue;
  const long long nblocks = (nout + hop - 1) / hop;
  const hipError_t e = bank_plan_switch(M, [&](auto plan) {
    using PL = decltype(plan);
    auto k = xcorr_bank_kernel<PL>;
    const long long grid = persistent_grid(k, PL::TF, nblocks);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(PL::TF), 0, st, s, n, Ps, K, off, nout, hop, c,
                       partials, nblocks, tw);
  });
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_bank_finalize(const PeakPartial* parts, int K, long long nparts, PeakPartial* out,
                                hipStream_t st) {
  hipLaunchKernelGGL(bank_finalize, dim3((unsigned)K), dim3(1024), 0, st, parts, nparts, out);
  return hipGetLastError();
}

}  // namespace vsig
