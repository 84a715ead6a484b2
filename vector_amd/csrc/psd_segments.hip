// Segmented spectrum traces and band measurement (gfx950): the per-bin mean /
// max-hold / min-hold of the block PSD over the frames of every segment of a
// table, in one launch (vsig_psd_segments_run), and each averaged spectrum's
// power, centroid, peak and occupied band (vsig_band_measure_run).  The
// definitions are in include/vsig.h.
//
// P[s][m][k] is the float32 value psd.hip stores for the frame at sample
// start[s] + m * hop, by the same expression on the outputs of the same engine
// calls: the kernels here run psd_traces.hip's own block body
// (psd_traces_run.hpp) and differ only in which frames a block owns.
//
//   psd_segments_pair    nfft 4096, 8192 (the plain plans: a frame at an
//                        arbitrary start is 8-byte aligned only)
//   psd_segments_split   nfft 64 .. 2048
//                        Block b reads {x0, nframes} from the block table the
//                        host built (vsig_psd_segments_create): a contiguous
//                        run of frames of one segment, into record row b.  A
//                        lane group or the second frame of a pair past the
//                        run's last frame touches no accumulator.
//   psd_segments_merge   a segment's rows [r0, r1) are contiguous; a lane per
//                        bin folds them in a fixed order and stores
//                        sum / nframes (double), max, min; a segment with no
//                        frame (r0 == r1) gets NaN.
//   band_measure         a block per row, staged through LDS in tiles: every
//                        thread sums a contiguous chunk of 16 bins in ascending
//                        order, the chunk sums are scanned by lane shuffles, and
//                        a second pass over the same sums finds where the
//                        cumulative sum crosses the two targets.
//
// No atomics; the grids are functions of (nfft, the table, the device) and of
// (nrows, nbins): the same input gives the same bytes on every run.
#include "psd_traces_run.hpp"

namespace vsig {

namespace {

constexpr int kSegMergeT = 1024;             // merge: 64 bins x up to 16 row groups
constexpr int kSegMergeFew = 8;              // rows a segment has at most for the 4-group launch
constexpr int kBandT = 256, kBandC = 16, kBandTile = kBandT * kBandC;

template <class P, bool PAIR>
__global__ __launch_bounds__(P::TF) void psd_segments_pair(
    const float2* __restrict__ x, const float* __restrict__ win, int nperseg, long long hop, float scale,
    PsdRec* __restrict__ rows, int shift, const float2* __restrict__ tw, const PsdSegBlock* __restrict__ blocks) {
  constexpr int F = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float2 lds[lds_size<P>()];
  const PsdSegBlock b = blocks[blockIdx.x];
  traces_pair_run<P, false, PAIR>(x + b.x0, 1, win, nperseg, hop, scale, rows + (long long)blockIdx.x * P::N,
                                  b.nframes, shift, tw, 0, (b.nframes + F - 1) / F, lds);
}

template <class P>
__global__ __launch_bounds__(block_threads<P>(), (P::E <= 16 ? 2 : 1)) void psd_segments_split(
    const float2* __restrict__ x, const float* __restrict__ win, int nperseg, long long hop, float scale,
    PsdRec* __restrict__ rows, int shift, const float2* __restrict__ tw, const PsdSegBlock* __restrict__ blocks) {
  constexpr int FPB = block_threads<P>() / P::TF;
  __shared__ __attribute__((aligned(16))) float2 lds[traces_split_lds<P>()];
  const PsdSegBlock b = blocks[blockIdx.x];
  traces_split_run<P>(x + b.x0, 1, win, nperseg, hop, scale, rows + (long long)blockIdx.x * P::N, b.nframes,
                      shift, tw, 0, (b.nframes + FPB - 1) / FPB, lds);
}

// Block j: segment j / (N / 64), bins 64 (j % (N / 64)) ...; row group g (of
// blockDim.x / 64) folds the rows r0 + g, r0 + g + G, ..., then the groups in
// order.
__global__ __launch_bounds__(kSegMergeT) void psd_segments_merge(
    const PsdRec* __restrict__ rows, const PsdSegRows* __restrict__ segs, int N, double* __restrict__ mean,
    float* __restrict__ mx, float* __restrict__ mn) {
  __shared__ PsdRec sm[kSegMergeT / 64][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, G = blockDim.x >> 6;
  const int per = N / 64;
  const long long s = blockIdx.x / per;
  const int k = (int)(blockIdx.x % per) * 64 + lane;
  const PsdSegRows sr = segs[s];
  PsdRec a = rec_identity();
#pragma unroll 4
  for (long long r = sr.r0 + g; r < sr.r1; r += G) rec_fold(a, rows[r * N + k]);
  sm[g][lane] = a;
  __syncthreads();
  if (g == 0) {
    for (int q = 1; q < G; ++q) rec_fold(a, sm[q][lane]);
    const bool bad = sr.nframes < 1 || a.mx != a.mx || a.mn != a.mn || a.sum != a.sum;
    const long long o = s * N + k;
    if (mean) mean[o] = bad ? __builtin_nan("") : a.sum / (double)sr.nframes;
    if (mx) mx[o] = bad ? __builtin_nanf("") : a.mx;
    if (mn) mn[o] = bad ? __builtin_nanf("") : a.mn;
  }
}

// A block per row, the row in tiles of kBandTile bins staged through LDS (the
// loads coalesced, a pad every kBandC doubles against bank conflicts).  Thread
// t owns the kBandC contiguous bins t * kBandC ... of every tile and sums them
// in ascending order; the chunk sums are scanned inside each wave (a fixed
// tree of lane shuffles), the four wave totals and the tiles' totals added in
// ascending order.  c[k] = (that prefix of k's chunk) + (the chunk up to k).
// Every thread carries the running totals (the same operations on the same
// values in all of them).  Pass 0 gives the total, the centroid and the peak;
// pass 1 repeats the same sums -- so the same values -- and finds the first k
// at which c reaches each target.  The prefix of a chunk and the end of the
// chunk before it associate their additions differently, so c may step back
// by an ulp there and c[nbins - 1] may sit an ulp under the total: a target no
// c[k] reaches (a tail below that ulp) is given to bin nbins - 1.
__device__ __forceinline__ int band_pad(int i) { return i + (i / kBandC); }

__global__ __launch_bounds__(kBandT) void band_measure(const double* __restrict__ rows, int nbins, long long ld,
                                                       double tail, BandRec* __restrict__ out) {
  constexpr int kWaves = kBandT / 64;
  __shared__ double buf[kBandTile + kBandTile / kBandC];
  __shared__ double wtot[kWaves], wws[kWaves], wmax[kWaves];
  __shared__ int warg[kWaves], wnan[kWaves], wlo[kWaves], whi[kWaves];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const double* row = rows + (long long)blockIdx.x * ld;
  int lo = 0x7fffffff, hi = 0x7fffffff;                // this thread's first crossings (pass 1)
  double tlo = 0.0, thi = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    double c = 0.0, w = 0.0, pk = -__builtin_inf();    // the running totals, the same in every thread
    int pa = -1, bad = 0;
    for (long long base = 0; base < nbins; base += kBandTile) {
#pragma unroll
      for (int j = 0; j < kBandC; ++j) {
        const int i = t + kBandT * j;
        buf[band_pad(i)] = base + i < nbins ? row[base + i] : 0.0;
      }
      __syncthreads();
      double s = 0.0, ws = 0.0, m = -__builtin_inf();
      int arg = -1, nan = 0;
      const int i0 = t * kBandC;
#pragma unroll
      for (int i = 0; i < kBandC; ++i) {
        if (base + i0 + i < nbins) {
          const double v = buf[band_pad(i0 + i)];
          s += v;
          ws += (double)(base + i0 + i) * v;
          nan |= v != v;
          if (v > m) { m = v; arg = (int)(base + i0 + i); }        // the first maximum of the chunk
        }
      }
      double inc = s;                                  // inclusive scan of the chunk sums in the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const double u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
      }
      double ex = __shfl_up(inc, 1, 64);
      if (lane == 0) ex = 0.0;
      if (!pass) {                                     // lane 0: the wave's weighted sum, first maximum, NaN flag
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
          ws += __shfl_down(ws, d, 64);
          const double om = __shfl_down(m, d, 64);
          const int oa = __shfl_down(arg, d, 64);
          nan |= __shfl_down(nan, d, 64);
          // a lane holds the maximum of the lanes l, l + d, l + 2d, ...: a tie goes to the lower bin
          if (om > m || (om == m && oa >= 0 && (arg < 0 || oa < arg))) { m = om; arg = oa; }
        }
        if (lane == 0) { wws[wv] = ws; wmax[wv] = m; warg[wv] = arg; wnan[wv] = nan; }
      }
      if (lane == 63) wtot[wv] = inc;
      __syncthreads();
      double pre = c;
#pragma unroll
      for (int j = 0; j < kWaves; ++j) {
        if (j == wv) pre = c;                          // the waves before this one
        c += wtot[j];
        if (!pass) {
          w += wws[j];
          bad |= wnan[j];
          if (wmax[j] > pk) { pk = wmax[j]; pa = warg[j]; }
        }
      }
      pre += ex;
      if (pass) {
        double run = 0.0;
#pragma unroll
        for (int i = 0; i < kBandC; ++i) {
          if (base + i0 + i < nbins) {
            run += buf[band_pad(i0 + i)];
            const double ck = pre + run;
            if (lo == 0x7fffffff && ck >= tlo) lo = (int)(base + i0 + i);
            if (hi == 0x7fffffff && ck >= thi) hi = (int)(base + i0 + i);
          }
        }
      }
      __syncthreads();                                 // before the next tile overwrites buf and the wave totals
    }
    if (pass == 0) {
      const bool ok = !bad && c > 0.0;
      if (t == 0) {
        BandRec r;
        r.power = c;
        r.centroid = ok ? w / c : __builtin_nan("");
        r.peak = ok ? pk : __builtin_nan("");
        r.peak_bin = ok ? pa : -1;
        r.lo_bin = r.hi_bin = -1;
        r.flags = (bad ? 1 : 0) | (c > 0.0 ? 0 : 2);
        out[blockIdx.x] = r;
      }
      if (!ok) return;                                 // uniform over the block
      tlo = tail * c;
      thi = (1.0 - tail) * c;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int ol = __shfl_down(lo, d, 64), oh = __shfl_down(hi, d, 64);
    lo = ol < lo ? ol : lo;
    hi = oh < hi ? oh : hi;
  }
  if (lane == 0) { wlo[wv] = lo; whi[wv] = hi; }
  __syncthreads();
  if (t == 0) {
    for (int j = 1; j < kWaves; ++j) {
      lo = wlo[j] < lo ? wlo[j] : lo;
      hi = whi[j] < hi ? whi[j] : hi;
    }
    out[blockIdx.x].lo_bin = lo == 0x7fffffff ? nbins - 1 : lo;
    out[blockIdx.x].hi_bin = hi == 0x7fffffff ? nbins - 1 : hi;
  }
}

}  // namespace

hipError_t psd_segments_geom(int N, int* step, long long* max_blocks) {
  int per = 0;
  VSIG_TRACES_SWITCH(N, {
    if constexpr (PL::TF >= 256) {
      constexpr bool PAIR = pairs_fit<PL>();
      static const int p = resident_blocks(psd_segments_pair<PL, PAIR>, PL::TF);
      *step = PAIR ? 2 : 1; per = p;
    } else {
      static const int p = resident_blocks(psd_segments_split<PL>, block_threads<PL>());
      *step = block_threads<PL>() / PL::TF; per = p;
    }
  });
  *max_blocks = (long long)cu_count() * per;
  return hipSuccess;
}

hipError_t launch_psd_segments(int N, const float2* x, const float* win, int nperseg, long long hop,
                               float scale, int shift, const float2* tw, const PsdSegBlock* blocks,
                               long long nblocks, PsdRec* rows, hipStream_t st) {
  if (nblocks < 1 || nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  VSIG_TRACES_SWITCH(N, {
    if constexpr (PL::TF >= 256) {
      hipLaunchKernelGGL((psd_segments_pair<PL, pairs_fit<PL>()>), dim3((unsigned)nblocks), dim3(PL::TF), 0, st,
                         x, win, nperseg, hop, scale, rows, shift, tw, blocks);
    } else {
      hipLaunchKernelGGL(psd_segments_split<PL>, dim3((unsigned)nblocks), dim3(block_threads<PL>()), 0, st, x,
                         win, nperseg, hop, scale, rows, shift, tw, blocks);
    }
  });
  return hipGetLastError();
}

hipError_t launch_psd_segments_merge(const PsdRec* rows, const PsdSegRows* segs, long long nseg, int N,
                                     long long max_rows, double* mean, float* mx, float* mn, hipStream_t st) {
  if (nseg < 1 || N < 64 || N % 64 || nseg * (N / 64) > 0x7fffffffLL) return hipErrorInvalidValue;
  // many short segments: 4 row groups a block; long ones: 16 (a function of the table alone)
  const int threads = max_rows <= kSegMergeFew ? 256 : kSegMergeT;
  hipLaunchKernelGGL(psd_segments_merge, dim3((unsigned)(nseg * (N / 64))), dim3(threads), 0, st, rows, segs, N,
                     mean, mx, mn);
  return hipGetLastError();
}

hipError_t launch_band_measure(const double* rows, long long nrows, int nbins, long long ld, double tail,
                               BandRec* out, hipStream_t st) {
  if (nrows < 1 || nrows > 0x7fffffffLL || nbins < 1 || ld < nbins) return hipErrorInvalidValue;
  hipLaunchKernelGGL(band_measure, dim3((unsigned)nrows), dim3(kBandT), 0, st, rows, nbins, ld, tail, out);
  return hipGetLastError();
}

}  // namespace vsig
