// What psd_traces.hip (one slice) and psd_segments.hip (a table of slices)
// share: the per-bin accumulators and records of the spectrum traces, the frame
// load, and the body of the two in-LDS kernels -- a block's run of frames
// through the PSD's own engine calls into one record row.  The kernels differ
// only in which frames a block owns.
#pragma once
#include "os_common.hpp"

namespace vsig {

__device__ __forceinline__ PsdRec rec_identity() {
  PsdRec r;
  r.sum = 0.0; r.mx = -__builtin_inff(); r.mn = __builtin_inff();
  return r;
}
__device__ __forceinline__ void rec_fold(PsdRec& a, const PsdRec& b) {
  a.sum += b.sum;
  a.mx = np_max(a.mx, b.mx);
  a.mn = np_min(a.mn, b.mn);
}

// The accumulators of a thread's E bins (fully unrolled: registers).
template <int E>
struct Acc {
  double s[E];
  float mx[E], mn[E];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int e = 0; e < E; ++e) { s[e] = 0.0; mx[e] = -__builtin_inff(); mn[e] = __builtin_inff(); }
  }
  __device__ __forceinline__ void frame(const float2* v, float scale) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float p = (v[e].x * v[e].x + v[e].y * v[e].y) * scale;
      s[e] += (double)p;
      mx[e] = np_max(mx[e], p);
      mn[e] = np_min(mn[e], p);
    }
  }
  __device__ __forceinline__ PsdRec rec(int e) const {
    PsdRec r;
    r.sum = s[e]; r.mx = mx[e]; r.mn = mn[e];
    return r;
  }
};

// psd.hip's psd_load (frame `frame` of the strided input, zeros when inactive
// or past nperseg) and its window multiply.
template <class P>
__device__ __forceinline__ void load_windowed(float2* v, const float2* __restrict__ x, long long stride,
                                              const float* __restrict__ win, int nperseg, long long hop,
                                              long long frame, long long nframes, int t) {
  const bool active = frame < nframes;
  const float2* xf = x + (active ? frame * hop * stride : 0);
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int i = in_index<P>(t, e);
    v[e] = (active && i < nperseg) ? ld_stream<true>(xf + (long long)i * stride) : make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int i = in_index<P>(t, e);
    const float w = i < nperseg ? win[i] : 0.f;
    v[e] = make_float2(v[e].x * w, v[e].y * w);
  }
}

// A wave of a TF-thread block gets 512 / (TF / 256) registers.  Two frames of
// a pair and the accumulators are 8 E of them beside the engine's own (about
// 120); where that does not fit, one frame at a time (6 E).
template <class P>
constexpr bool pairs_fit() { return 8 * P::E + 120 <= 512 / ((P::TF + 255) / 256); }

// One block of P::TF >= 256 threads: the steps [u0, u1) of the frames
// [0, nframes) of x into `row`, a step being the frames 2u, 2u + 1 through
// fft_pair (PAIR), or the frame u alone through fft_frame_anch where two frames
// and the accumulators do not fit a wave's registers (pairs_fit; no plan in use
// needs it).  X4: psd_pair_kernel's 16-byte loads of the interleaved plan
// (Plan8192i), a launch-time property.  lds: lds_size<P>() float2.
template <class P, bool X4, bool PAIR>
__device__ __forceinline__ void traces_pair_run(
    const float2* __restrict__ x, long long stride, const float* __restrict__ win, int nperseg,
    long long hop, float scale, PsdRec* __restrict__ row, long long nframes, int shift,
    const float2* __restrict__ tw, long long u0, long long u1, float2* lds) {
  static_assert(P::TF >= 256, "one frame per block");
  constexpr int F = PAIR ? 2 : 1;
  const int t = threadIdx.x;
  float2 wa[nanch_total<P>()];
  load_anchors<P>(wa, tw, t);
  Acc<P::E> acc;
  acc.init();
  for (long long u = u0; u < u1; ++u) {
    float2 v[F][P::E];
    if constexpr (X4) {
      static_assert(map0_of<P>::value == kMapIlv && mapl_of<P>::value == kMapIlv && PAIR, "interleaved plan");
      static_assert(P::E == 2 * P::R[0] && P::E == 2 * P::RL, "two butterflies per thread");
      typedef float f4 __attribute__((ext_vector_type(4)));
      constexpr int R0 = P::R[0], S0 = P::N / R0;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const long long frame = u * 2 + f;
        const bool active = frame < nframes;
        const float2* xf = x + (active ? frame * hop : 0);
#pragma unroll
        for (int r = 0; r < R0; ++r) {
          const int i = 2 * t + S0 * r;
          const f4 q = active ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(xf + i))
                              : f4{0.f, 0.f, 0.f, 0.f};
          const f2v w2 = *reinterpret_cast<const f2v*>(win + i);
          v[f][r] = fromv((f2v){q.x, q.y} * w2.xx);
          v[f][R0 + r] = fromv((f2v){q.z, q.w} * w2.yy);
        }
      }
    } else {
#pragma unroll
      for (int f = 0; f < F; ++f) load_windowed<P>(v[f], x, stride, win, nperseg, hop, u * F + f, nframes, t);
    }
    if constexpr (PAIR) {
      launder_anchors<P>(wa);
      fft_pair<P>(v[0], v[1], lds, TwAnchors{wa}, t);
    } else {
      __syncthreads();                                 // the previous frame's LDS reads are done
      fft_frame_anch<P>(v[0], lds, wa, t);
    }
    acc.frame(v[0], scale);                            // frame F u < nframes: the step exists
    if constexpr (PAIR) {
      if (u * 2 + 1 < nframes) acc.frame(v[1], scale); // uniform over the block
    }
  }
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int i = out_index<P>(t, e);
    row[shift ? ((i + P::N / 2) & (P::N - 1)) : i] = acc.rec(e);
  }
}

// The split kernels' LDS (float2): psd_split_kernel's exchange buffer and
// two-level table, or the N records the lane groups are combined in.
template <class P>
constexpr int traces_split_lds() {
  constexpr int FPB = block_threads<P>() / P::TF;
  constexpr int FL = (lds_size<P>() + 1) / 2;
  constexpr int kExch = FPB * FL + tw2_size<P>();
  constexpr int kComb = 2 * P::N;                            // N records of 16 bytes
  return kExch > kComb ? kExch : kComb;
}

// One block of block_threads<P>() threads: the steps [u0, u1) of the frames
// [0, nframes) of x into `row`, a step being the FPB frames u * FPB + fl of
// its lane groups fl.  lds: traces_split_lds<P>() float2.
template <class P>
__device__ __forceinline__ void traces_split_run(
    const float2* __restrict__ x, long long stride, const float* __restrict__ win, int nperseg,
    long long hop, float scale, PsdRec* __restrict__ row, long long nframes, int shift,
    const float2* __restrict__ tw, long long u0, long long u1, float2* lds) {
  constexpr int BT = block_threads<P>();
  constexpr int FPB = BT / P::TF;
  constexpr int FL = (lds_size<P>() + 1) / 2;
  static_assert(sizeof(PsdRec) == 2 * sizeof(float2), "record size");
  const int fl = threadIdx.x / P::TF;
  const int t = threadIdx.x % P::TF;
  float2* t2 = lds + FPB * FL;
  load_tw2<P>(t2, tw, threadIdx.x, BT);
  Acc<P::E> acc;
  acc.init();
  for (long long u = u0; u < u1; ++u) {
    const long long frame = u * FPB + fl;
    float2 v[P::E];
    load_windowed<P>(v, x, stride, win, nperseg, hop, frame, nframes, t);
    fft_frame_split<P>(v, reinterpret_cast<float*>(lds + fl * FL), t2, t);
    if (frame < nframes) acc.frame(v, scale);
  }
  // the lane groups' accumulators, combined in group order in the exchange
  // buffer (every group is past its last LDS read)
  __syncthreads();
  PsdRec* cmb = reinterpret_cast<PsdRec*>(lds);
  for (int g = 0; g < FPB; ++g) {
    if (fl == g) {
#pragma unroll
      for (int e = 0; e < P::E; ++e) {
        const int i = out_index<P>(t, e);
        PsdRec r = acc.rec(e);
        if (g > 0) {
          PsdRec a = cmb[i];
          rec_fold(a, r);
          r = a;
        }
        cmb[i] = r;
      }
    }
    __syncthreads();
  }
  for (int k = threadIdx.x; k < P::N; k += BT) row[shift ? ((k + P::N / 2) & (P::N - 1)) : k] = cmb[k];
}

// The traces' plans: the PSD's own up to 8192 points.  16384 points are not
// among them: a bin's accumulators are 16 bytes, 256 KB for the frame, half a
// CU's register file, and the exchange buffer (136 KB) leaves no LDS for them.
// The PSD's 1024-thread plan gives a wave 128 registers (one frame at a time:
// 332 bytes of scratch per lane), the 512-thread plans 256 (radices 32 16 32:
// 596 bytes; 16 4 16 16: 576 bytes).  That length takes the fold route.
#define VSIG_TRACES_SWITCH(N, ...)                                  \
  switch (N) {                                                      \
    case 64: { using PL = Plan64; __VA_ARGS__; } break;             \
    case 128: { using PL = Plan128; __VA_ARGS__; } break;           \
    case 256: { using PL = Plan256; __VA_ARGS__; } break;           \
    case 512: { using PL = Plan512; __VA_ARGS__; } break;           \
    case 1024: { using PL = Plan1024; __VA_ARGS__; } break;         \
    case 2048: { using PL = Plan2048; __VA_ARGS__; } break;         \
    case 4096: { using PL = Plan4096; __VA_ARGS__; } break;         \
    case 8192: { using PL = Plan8192; __VA_ARGS__; } break;         \
    default: return hipErrorInvalidValue;                           \
  }

// Blocks of `kernel` a CU holds (occupancy API), asked once per instantiation:
// the launches themselves make no runtime query (graph capture).
template <class K>
inline int resident_blocks(K kernel, int block) {
  int per = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, block, 0) != hipSuccess || per < 1) per = 1;
  return per;
}

inline int cu_count() {
  static thread_local int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
  }
  return cus;
}

}  // namespace vsig
