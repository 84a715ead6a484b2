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
#include "psd_traces_run.hpp"

namespace vsig {

namespace {

constexpr int kMinUnits = kTracesMinUnits;
constexpr int kMergeT = 1024, kMergeG = kMergeT / 64;   // merge: 64 bins x 16 row groups
constexpr int kFoldT = 256, kFoldG = kFoldT / 64;       // fold: 64 bins x 4 frame groups

// Block b owns the steps [b * upb, min((b + 1) * upb, units)) of
// traces_pair_run (psd_traces_run.hpp).
template <class P, bool X4, bool PAIR>
__global__ __launch_bounds__(P::TF) void psd_traces_pair(
    const float2* __restrict__ x, long long stride, const float* __restrict__ win, int nperseg,
    long long hop, float scale, PsdRec* __restrict__ rows, long long nframes, int shift,
    const float2* __restrict__ tw, long long upb) {
  constexpr int F = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float2 lds[lds_size<P>()];
  const long long units = (nframes + F - 1) / F;
  const long long u0 = (long long)blockIdx.x * upb;
  const long long u1 = u0 + upb < units ? u0 + upb : units;
  traces_pair_run<P, X4, PAIR>(x, stride, win, nperseg, hop, scale, rows + (long long)blockIdx.x * P::N, nframes,
                               shift, tw, u0, u1, lds);
}

// Block b owns the steps [b * upb, ...) of traces_split_run.
template <class P>
__global__ __launch_bounds__(block_threads<P>(), (P::E <= 16 ? 2 : 1)) void psd_traces_split(
    const float2* __restrict__ x, long long stride, const float* __restrict__ win, int nperseg,
    long long hop, float scale, PsdRec* __restrict__ rows, long long nframes, int shift,
    const float2* __restrict__ tw, long long upb) {
  constexpr int FPB = block_threads<P>() / P::TF;
  __shared__ __attribute__((aligned(16))) float2 lds[traces_split_lds<P>()];
  const long long units = (nframes + FPB - 1) / FPB;
  const long long u0 = (long long)blockIdx.x * upb;
  const long long u1 = u0 + upb < units ? u0 + upb : units;
  traces_split_run<P>(x, stride, win, nperseg, hop, scale, rows + (long long)blockIdx.x * P::N, nframes, shift,
                      tw, u0, u1, lds);
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
