// Spectrum traces (gfx950): per-bin mean / max-hold / min-hold of the block
// PSD over its frames, reduced in the transform kernel's epilogue instead of
// storing the (nframes, nfft) spectrogram (vsig_psd_traces_c64_dev; the
// definition is in include/vsig.h).
//
// P[m][k] is the float32 value psd.hip stores, by the same expression
// (re * re + im * im) * scale on the outputs of the same engine calls.  A
// block owns a contiguous run of frames, transforms them `step` at a time
// (psd_pair_kernel's two frames through fft_pair, psd_split_kernel's
// 256 / TF frames side by side) and folds every active frame into per-bin
// accumulators that stay in registers across the run: the sum in double, the
// maximum and the minimum in float under np.max / np.min's rule (a NaN stays).
// An inactive frame -- past nframes: the second of a pair, a lane group of a
// split block -- touches no accumulator.
//
//   psd_traces_pair   nfft 4096, 8192: a thread holds the E bins of its
//                     out_index for both frames of a pair; one record row per
//                     block straight from registers.
//   psd_traces_split  nfft 64 .. 2048: the block's 256 / TF lane groups hold
//                     the same bins; they are combined in group order through
//                     the (now idle) exchange buffer, then stored contiguously.
//   psd_traces_fold   every other nfft (16384 included, see VSIG_TRACES_SWITCH):
//                     the existing route stores a batch of
//                     frames (frame-major); a lane per bin folds the batch's
//                     columns into kPsdFoldRows rows kept across batches.
//   psd_traces_merge  a lane per bin folds the rows in a fixed order and
//                     stores mean = sum / nframes (double), max, min.
//
// A record is {sum, max, min}; the NaN flag is the record's max itself (a NaN
// P makes it NaN and it stays NaN through every later fold), and a flagged bin
// gets NaN in all three outputs.  Nothing crosses blocks through atomics and
// the grid is a function of (nfft, nframes) and the device's CU count alone:
// the same input gives the same bytes on every run.
#include "os_common.hpp"

namespace vsig {

namespace {

constexpr int kMinUnits = 4;                 // steps a block runs at least (when there are that many)
constexpr int kMergeT = 1024, kMergeG = kMergeT / 64;   // merge: 64 bins x 16 row groups
constexpr int kFoldT = 256, kFoldG = kFoldT / 64;       // fold: 64 bins x 4 frame groups

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

// Block b owns the steps [b * upb, min((b + 1) * upb, units)), a step being
// the frames 2u, 2u + 1 through fft_pair (PAIR), or the frame u alone through
// fft_frame_anch where two frames and the accumulators do not fit a wave's
// registers (pairs_fit; no plan in use needs it).  X4: psd_pair_kernel's
// 16-byte loads of the interleaved plan (Plan8192i), a launch-time property
// here too.
template <class P, bool X4, bool PAIR>
__global__ __launch_bounds__(P::TF) void psd_traces_pair(
    const float2* __restrict__ x, long long stride, const float* __restrict__ win, int nperseg,
    long long hop, float scale, PsdRec* __restrict__ rows, long long nframes, int shift,
    const float2* __restrict__ tw, long long upb) {
  static_assert(P::TF >= 256, "one frame per block");
  constexpr int F = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float2 lds[lds_size<P>()];
  const int t = threadIdx.x;
  const long long units = (nframes + F - 1) / F;
  const long long u0 = (long long)blockIdx.x * upb;
  const long long u1 = u0 + upb < units ? u0 + upb : units;
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
  PsdRec* row = rows + (long long)blockIdx.x * P::N;
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int i = out_index<P>(t, e);
    row[shift ? ((i + P::N / 2) & (P::N - 1)) : i] = acc.rec(e);
  }
}

// Block b owns the steps [b * upb, ...), a step being the FPB frames
// u * FPB + fl of its lane groups fl.
template <class P>
__global__ __launch_bounds__(block_threads<P>(), (P::E <= 16 ? 2 : 1)) void psd_traces_split(
    const float2* __restrict__ x, long long stride, const float* __restrict__ win, int nperseg,
    long long hop, float scale, PsdRec* __restrict__ rows, long long nframes, int shift,
    const float2* __restrict__ tw, long long upb) {
  constexpr int BT = block_threads<P>();
  constexpr int FPB = BT / P::TF;
  constexpr int FL = (lds_size<P>() + 1) / 2;
  constexpr int kExch = FPB * FL + tw2_size<P>();            // psd_split_kernel's buffer
  constexpr int kComb = 2 * P::N;                            // N records of 16 bytes
  __shared__ __attribute__((aligned(16))) float2 lds[kExch > kComb ? kExch : kComb];
  static_assert(sizeof(PsdRec) == 2 * sizeof(float2), "record size");
  const int fl = threadIdx.x / P::TF;
  const int t = threadIdx.x % P::TF;
  const long long units = (nframes + FPB - 1) / FPB;
  const long long u0 = (long long)blockIdx.x * upb;
  const long long u1 = u0 + upb < units ? u0 + upb : units;
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
  PsdRec* row = rows + (long long)blockIdx.x * P::N;
  for (int k = threadIdx.x; k < P::N; k += BT) row[shift ? ((k + P::N / 2) & (P::N - 1)) : k] = cmb[k];
}

// A batch of nb stored frames (frame-major, already shifted) into the rows:
// block (bx, by) folds the frames by * kFoldG + g + j * kPsdFoldRows * kFoldG
// of the bins 64 bx .. into row by (first: the row starts from the identity).
__global__ __launch_bounds__(kFoldT) void psd_traces_fold(const float* __restrict__ sxx, long long nb, int N,
                                                          int first, PsdRec* __restrict__ rows) {
  __shared__ PsdRec sm[kFoldG][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  PsdRec a = rec_identity();
  if (k < N) {
    for (long long f = (long long)blockIdx.y * kFoldG + g; f < nb; f += (long long)kPsdFoldRows * kFoldG) {
      const float p = sxx[f * N + k];
      a.sum += (double)p;
      a.mx = np_max(a.mx, p);
      a.mn = np_min(a.mn, p);
    }
  }
  sm[g][lane] = a;
  __syncthreads();
  if (g == 0 && k < N) {
    PsdRec* out = rows + (long long)blockIdx.y * N + k;
    PsdRec r = first ? rec_identity() : *out;
#pragma unroll
    for (int q = 0; q < kFoldG; ++q) rec_fold(r, sm[q][lane]);
    *out = r;
  }
}

__global__ __launch_bounds__(kMergeT) void psd_traces_merge(const PsdRec* __restrict__ rows, long long nrows,
                                                            int N, long long nframes, double* __restrict__ mean,
                                                            float* __restrict__ mx, float* __restrict__ mn) {
  __shared__ PsdRec sm[kMergeG][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  PsdRec a = rec_identity();
  if (k < N) {
#pragma unroll 4
    for (long long r = g; r < nrows; r += kMergeG) rec_fold(a, rows[r * N + k]);
  }
  sm[g][lane] = a;
  __syncthreads();
  if (g == 0 && k < N) {
    for (int q = 1; q < kMergeG; ++q) rec_fold(a, sm[q][lane]);
    const bool bad = a.mx != a.mx || a.mn != a.mn || a.sum != a.sum;      // the record's NaN flag
    if (mean) mean[k] = bad ? __builtin_nan("") : a.sum / (double)nframes;
    if (mx) mx[k] = bad ? __builtin_nanf("") : a.mx;
    if (mn) mn[k] = bad ? __builtin_nanf("") : a.mn;
  }
}

// A wave of a TF-thread block gets 512 / (TF / 256) registers.  Two frames of
// a pair and the accumulators are 8 E of them beside the engine's own (about
// 120); where that does not fit, one frame at a time (6 E).
template <class P>
constexpr bool pairs_fit() { return 8 * P::E + 120 <= 512 / ((P::TF + 255) / 256); }

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
int resident_blocks(K kernel, int block) {
  int per = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, block, 0) != hipSuccess || per < 1) per = 1;
  return per;
}

int cu_count() {
  static thread_local int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
  }
  return cus;
}

// (frames per step, resident blocks per CU) of the in-LDS kernel for N.
hipError_t traces_geom(int N, int* step, int* per) {
  if (N == 8192) {                       // the x4 and the plain instantiation: the smaller of the two
    static const int pa = resident_blocks(psd_traces_pair<Plan8192i, true, true>, Plan8192i::TF);
    static const int pb = resident_blocks(psd_traces_pair<Plan8192, false, true>, Plan8192::TF);
    *step = 2; *per = pa < pb ? pa : pb;
    return hipSuccess;
  }
  VSIG_TRACES_SWITCH(N, {
    if constexpr (PL::TF >= 256) {
      constexpr bool PAIR = pairs_fit<PL>();
      static const int p = resident_blocks(psd_traces_pair<PL, false, PAIR>, PL::TF);
      *step = PAIR ? 2 : 1; *per = p;
    } else {
      static const int p = resident_blocks(psd_traces_split<PL>, block_threads<PL>());
      *step = block_threads<PL>() / PL::TF; *per = p;
    }
  });
  return hipSuccess;
}

}  // namespace

bool psd_traces_in_lds(long long N) { return N >= 64 && N <= 8192 && (N & (N - 1)) == 0; }

int psd_traces_table(int N, bool* two_level) {
  *two_level = psd_plan_threads(N) < 256;
  return N;
}

PsdTracesPlan psd_traces_plan(long long N, long long nframes) {
  PsdTracesPlan p{0, 0, 0};
  if (nframes < 1 || N < 1) return p;
  if (!psd_traces_in_lds(N)) {           // fold route: frames interleaved over the rows
    p.blocks = kPsdFoldRows; p.step = 1; p.fpb = 0;
    return p;
  }
  int step = 0, per = 0;
  if (traces_geom((int)N, &step, &per) != hipSuccess) return p;
  const long long units = (nframes + step - 1) / step;
  const long long maxb = (long long)cu_count() * per;
  long long upb = (units + maxb - 1) / maxb;
  const long long least = units < kMinUnits ? units : kMinUnits;
  if (upb < least) upb = least;
  p.blocks = (units + upb - 1) / upb;    // no empty block
  p.step = step;
  p.fpb = upb * step;
  return p;
}

hipError_t launch_psd_traces(int N, const float2* x, long long stride, const float* win, int nperseg,
                             long long hop, float scale, long long nframes, int shift, const float2* tw,
                             PsdRec* rows, hipStream_t st) {
  const PsdTracesPlan p = psd_traces_plan(N, nframes);
  if (p.blocks < 1 || p.fpb < 1 || p.blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const long long upb = p.fpb / p.step;
  // 8192 points: launch_psd's x4 condition takes the interleaved plan and its
  // 16-byte loads; otherwise the plain plan (the same radices and table), whose
  // element-wise loads leave room for the accumulators
  if (N == 8192 && stride == 1 && nperseg == N && hop % 2 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
      (reinterpret_cast<uintptr_t>(win) & 7) == 0) {
    hipLaunchKernelGGL((psd_traces_pair<Plan8192i, true, true>), dim3((unsigned)p.blocks), dim3(Plan8192i::TF), 0,
                       st, x, stride, win, nperseg, hop, scale, rows, nframes, shift, tw, upb);
    return hipGetLastError();
  }
  VSIG_TRACES_SWITCH(N, {
    if constexpr (PL::TF >= 256) {
      hipLaunchKernelGGL((psd_traces_pair<PL, false, pairs_fit<PL>()>), dim3((unsigned)p.blocks), dim3(PL::TF),
                         0, st, x, stride, win, nperseg, hop, scale, rows, nframes, shift, tw, upb);
    } else {
      hipLaunchKernelGGL(psd_traces_split<PL>, dim3((unsigned)p.blocks), dim3(block_threads<PL>()), 0, st, x,
                         stride, win, nperseg, hop, scale, rows, nframes, shift, tw, upb);
    }
  });
  return hipGetLastError();
}

hipError_t launch_psd_traces_fold(const float* sxx, long long nb, long long N, int first, PsdRec* rows,
                                  hipStream_t st) {
  if (nb < 1 || N < 1 || N > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(psd_traces_fold, dim3((unsigned)((N + 63) / 64), kPsdFoldRows), dim3(kFoldT), 0, st, sxx,
                     nb, (int)N, first, rows);
  return hipGetLastError();
}

hipError_t launch_psd_traces_merge(const PsdRec* rows, long long nrows, long long N, long long nframes,
                                   double* mean, float* mx, float* mn, hipStream_t st) {
  if (nrows < 1 || N < 1 || N > 0x7fffffffLL || nframes < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(psd_traces_merge, dim3((unsigned)((N + 63) / 64)), dim3(kMergeT), 0, st, rows, nrows,
                     (int)N, nframes, mean, mx, mn);
  return hipGetLastError();
}

}  // namespace vsig
