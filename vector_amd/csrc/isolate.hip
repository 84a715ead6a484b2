// Segmented mix-down + band filter (gfx950): every burst of a host table taken
// out of a capture as a baseband packet, all bursts in one launch
// (vsig_isolate_run).  The definition is in include/vsig.h:
//   z_s[j] = sum_{m<T} h_s[m] u_s[lo_s + j + d - m],  u_s[i] = x[i] exp(j wsr_s i),
// d = (T - 1) / 2, x = 0 outside [0, n).
//
//   isolate_kernel   the D = 1 body of fir_os_kernel<Plan1024x, MIX> (fir.hip):
//                    two 1024-point overlap-save frames per one-wave workgroup
//                    through fft_pair.  What the FIR derives from its block
//                    index each FRAME reads from its own record of the table
//                    the host built (vsig_isolate_create): where its input
//                    window starts in the capture (x0, may be negative or run
//                    past n: zero fill), where its outputs go in the packed
//                    output (y0), how many it keeps (keep <= hop: circular
//                    indices [lo, lo + keep)), its filter's row of the F x 1024
//                    spectrum table and its segment's phase slope w / sr.  The
//                    two frames of a workgroup may belong to different
//                    segments and filters.  The odd last frame of the last
//                    pair takes an empty record (no sample inside [0, n), keep
//                    0): it reads and writes nothing.
//
// The mixer is load_segment_mix's with the per-launch table MixArgs::rot formed
// in the wave: lane l < 16 holds exp(j wsr 64 l) (one cis_rev on a phase reduced
// in double), read by the others through v_readlane; a lane then rotates by
// exp(j wsr (x0 + m(t))) -- global phase origin at capture index 0 -- once and by
// those per element, all in fp32 (about 2e-7 relative per sample).
//
// No atomics; the grid is ceil(frames / 2), a function of the table alone: the
// same input gives the same bytes on every run.  Output offsets are 8-byte
// aligned only, so the stores are fir_store's 8-byte streaming ones.
#include "os_common.hpp"

namespace vsig {

namespace {

template <class P>
__device__ __forceinline__ void load_frame_mix(float2* v, const float2* __restrict__ x, long long s0,
                                               long long n, int t, double wsr) {
  static_assert(P::TF == 64 && P::E == 16 && P::R[0] == 16,
                "the rotations assume in_index(t, e) = m(t) + 64 e");
  load_segment<P>(v, x, s0, n, t);
  if (wsr == 0.0) return;                              // uniform: a segment at 0 Hz is not rotated
  const float2 r0 = mix_rot_fast(s0 + in_index<P>(t, 0), wsr);
  const float2 re = mix_rot_fast(64 * (t & 15), wsr);  // lane e < 16: exp(j wsr 64 e)
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const float2 ro = make_float2(
        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(re.x), e)),
        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(re.y), e)));
    v[e] = cmul(v[e], cmul(r0, ro));
  }
}

// fir_store at decim = 1 with the frame's own base and count
template <class P>
__device__ __forceinline__ void frame_store(const float2* v, float2* __restrict__ yb, int lo, int keep,
                                            int t) {
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int i = out_index<P>(t, e) - lo;
    if (i >= 0 && i < keep) st_stream(yb + (unsigned)i, conj1(v[e]));
  }
}

template <class P>
__global__ __launch_bounds__(P::TF) void isolate_kernel(
    const float2* __restrict__ x, long long n, const float2* __restrict__ Hs, int lo,
    float2* __restrict__ y, const IsoFrame* __restrict__ frames, long long nframes,
    const float2* __restrict__ tw) {
  static_assert(P::R[0] == P::RL, "overlap-save needs a palindromic plan");
  __shared__ float2 lds[lds_size<P>()];
  const int t = threadIdx.x;
  const long long b = xcd_remap(blockIdx.x, gridDim.x);
  if (2 * b >= nframes) return;  // uniform per block
  const IsoFrame fa = frames[2 * b];
  // past the table's end: no sample inside [0, n), nothing kept
  const IsoFrame fd = 2 * b + 1 < nframes ? frames[2 * b + 1] : IsoFrame{n, 0, 0.0, 0, fa.filter};
  float2 wa[nanch_total<P>()];
  load_anchors<P>(wa, tw, t);
  float2 a[P::E], d[P::E];
  load_frame_mix<P>(a, x, fa.x0, n, t, fa.wsr);
  load_frame_mix<P>(d, x, fd.x0, n, t, fd.wsr);
  launder_anchors<P>(wa);
  fft_pair<P>(a, d, lds, TwAnchors{wa}, t);
  const float2* Ha = Hs + (long long)fa.filter * P::N;
  const float2* Hd = Hs + (long long)fd.filter * P::N;
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int k = out_index<P>(t, e);
    a[e] = cmul_conj(a[e], Ha[k]);
    d[e] = cmul_conj(d[e], Hd[k]);
  }
  launder_anchors<P>(wa);
  fft_pair<P>(a, d, lds, TwAnchors{wa}, t);
  frame_store<P>(a, y + fa.y0, lo, fa.keep, t);
  frame_store<P>(d, y + fd.y0, lo, fd.keep, t);
}

}  // namespace

hipError_t launch_isolate(const float2* x, long long n, const float2* Hs, int lo, float2* y,
                          const IsoFrame* frames, long long nframes, const float2* tw, hipStream_t st) {
  using PL = Plan1024x;
  static_assert(PL::N == kIsoM, "the frame length vsig_isolate_create plans for");
  const long long nblocks = (nframes + 1) / 2;
  if (nframes < 1 || nblocks > 0x7fffffffLL || lo < 0 || lo >= PL::N) return hipErrorInvalidValue;
  hipLaunchKernelGGL(isolate_kernel<PL>, dim3((unsigned)nblocks), dim3(PL::TF), 0, st, x, n, Hs, lo, y, frames,
                     nframes, tw);
  return hipGetLastError();
}

}  // namespace vsig
