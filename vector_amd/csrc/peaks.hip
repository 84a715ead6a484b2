// Peak list (gfx950): every index i of an array with m[i] = |a[i]| >= thr that
// is the first maximum of m over [i - d, i + d] (clipped to the array), in
// ascending order (vsig_peaks_dev; packet instances in a stored correlation).
//
//   peaks_tile   one pass over the array, 16-byte loads: {max, first index}
//                of every tile of kPeaksTile elements into a table, and of
//                each block's tiles into a partial; the partials' fixed-order
//                reduce (launch_partial_finalize) gives max / argmax for the
//                relative threshold and the info record.
//   peaks_mark   count pass: the instances of every tile whose maximum
//                reaches thr (the others cost one table read).
//                d < tile:  the tile and a halo of d magnitudes in LDS; each
//                  element >= thr looks outward, nearest first and both sides
//                  in turn, for an element that beats it (larger, or equal
//                  with a lower index) and stops at the first one.  With r(i)
//                  the distance to that element (capped at d), elements with
//                  r >= x are more than x apart, so all scans with r in
//                  [x, 2x) cost O(n) and all scans O(n log d).
//                d >= tile: only a tile's first maximum can be an instance
//                  (it beats the rest of its tile).  The block checks it
//                  against the table for the whole tiles inside the window,
//                  nearest first (128 a side per step, stop at the first
//                  hit: O((n / tile) log d) over all tiles by the same
//                  argument), then against the raw array for the window's
//                  two partial end tiles (< 2 tiles of elements per tile).
//   peaks_scan   exclusive scan of the counts of the mark pass's blocks (32
//                tiles each; one block scans them) and the info record; a
//                tile's offset is its block's plus the counts before it.
//   peaks_mark   emit pass: each tile stores its records at its offset, so
//                the list is ascending, the same bytes on every run, and a
//                full buffer holds the lowest-index instances.
//
// NaN: a NaN magnitude compares false everywhere, so it is never an instance,
// never beats a neighbour and never becomes a tile's maximum (a tile of
// nothing but NaN has maximum -1 at its first index).
#include <climits>

#include "block_ops.hpp"

namespace vsig {

namespace {

constexpr int PT = 256;                      // threads per block
constexpr int PE = kPeaksTile / PT;          // elements per thread and tile
constexpr int PG = 32;                       // tiles per block of the mark passes
constexpr int PW = PT / 64;

// VEC: a is 16-byte aligned (whole tiles by 16-byte loads; the last, partial
// tile and unaligned arrays element by element).
template <class T, bool VEC>
__global__ __launch_bounds__(PT) void peaks_tile(const T* __restrict__ a, long long n, long long ntiles,
                                                 PeakPartial* __restrict__ tab,
                                                 PeakPartial* __restrict__ bpart) {
  constexpr int EPV = 16 / sizeof(T), NV = kPeaksTile / (PT * EPV);
  __shared__ FirstMax slots[2][PW];          // alternate between tiles: one barrier a tile is enough
  int par = 0;
  double bm = -2.0;                          // thread 0: the block's tiles so far
  long long bi = LLONG_MAX;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1) {
    const long long base = tile * kPeaksTile;
    double m = -1.0;
    long long mi = LLONG_MAX;
    if (VEC && base + kPeaksTile <= n) {
      const Pack16<T>* pv = reinterpret_cast<const Pack16<T>*>(a + base);
      Pack16<T> pk[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) pk[j] = pv[j * PT + threadIdx.x];
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int q = 0; q < EPV; ++q)
          betterd(m, mi, (double)mag(pk[j].e[q]), base + (long long)(j * PT + threadIdx.x) * EPV + q);
    } else {
#pragma unroll
      for (int e = 0; e < PE; ++e) {
        const long long g = base + e * PT + threadIdx.x;
        if (g < n) betterd(m, mi, (double)mag(a[g]), g);
      }
    }
    FirstMax v{m, mi};
    block_fold<PW>(v, slots[par]);
    if (threadIdx.x == 0) {
      if (v.i == LLONG_MAX) v.i = base;      // nothing but NaN
      PeakPartial r;
      r.max2 = v.m; r.idx = v.i; r.sum_abs = 0.0; r.sum_abs2 = 0.0;
      tab[tile] = r;
      betterd(bm, bi, v.m, v.i);
    }
  }
  if (threadIdx.x == 0) {                    // every block has at least one tile
    PeakPartial r;
    r.max2 = bm; r.idx = bi; r.sum_abs = 0.0; r.sum_abs2 = 0.0;
    bpart[blockIdx.x] = r;
  }
}

struct PeaksArgs {
  const void* a;
  long long n, d, ntiles, cap;
  double thr;
  int relative;
  const PeakPartial* tab;      // per tile {max, first index}
  const PeakPartial* rec;      // their reduction
  int* counts;                 // per tile instance count
  long long* goff;             // per block of PG tiles: their count, then (scanned) their offset
  PeakInst* out;
};

// Is (v, g), the first maximum of tile t, beaten by an element of its window
// outside tile t?  Block-cooperative; d >= kPeaksTile.
template <class T>
__device__ bool beaten_outside(const PeaksArgs& A, long long t, double v, long long g) {
  const T* a = static_cast<const T*>(A.a);
  const long long lo = g - A.d > 0 ? g - A.d : 0;
  const long long hi = g + A.d < A.n - 1 ? g + A.d : A.n - 1;
  // whole tiles inside the window: jl .. t-1 and t+1 .. jr
  const long long jl = (lo + kPeaksTile - 1) / kPeaksTile;
  const long long jr = hi == A.n - 1 ? A.ntiles - 1 : (hi + 1) / kPeaksTile - 1;
  const long long NL = t - jl, NR = jr - t;
  const long long steps = NL > NR ? NL : NR;
  const int side = threadIdx.x >> 7, i = threadIdx.x & 127;
  for (long long s = 0; s < steps; s += 128) {
    int hit = 0;
    if (side == 0) {
      if (s + i < NL) hit = A.tab[t - 1 - (s + i)].max2 >= v;
    } else {
      if (s + i < NR) hit = A.tab[t + 1 + (s + i)].max2 > v;
    }
    if (__syncthreads_or(hit)) return true;
  }
  // the partial tiles at the window's ends
  int hit = 0;
  for (long long q = lo + threadIdx.x; q < jl * kPeaksTile; q += PT) hit |= (double)mag(a[q]) >= v;
  for (long long q = (jr + 1) * kPeaksTile + threadIdx.x; q <= hi; q += PT) hit |= (double)mag(a[q]) > v;
  return __syncthreads_or(hit) != 0;
}

template <class T, bool EMIT>
__global__ __launch_bounds__(PT) void peaks_mark(PeaksArgs A) {
  __shared__ double L[3 * kPeaksTile];
  __shared__ int wcnt[PE][PW], woff[PE][PW], stot;
  __shared__ unsigned char live[PG];
  __shared__ int tcnt[PG];                               // count pass: the tiles' counts
  __shared__ long long toff[PG];                         // emit pass: the tiles' offsets
  const T* a = static_cast<const T*>(A.a);
  const double thr = A.relative ? __dmul_rn(A.thr, A.rec->max2) : A.thr;
  const long long t0 = (long long)blockIdx.x * PG;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x < PG) {
    const long long t = t0 + threadIdx.x;
    bool lv = false;
    if (EMIT) {
      // the tile's offset: the block's, plus the counts of the tiles before it
      const int c = t < A.ntiles ? A.counts[t] : 0;
      int x = c;
#pragma unroll
      for (int off = 1; off < PG; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
      }
      toff[threadIdx.x] = A.goff[blockIdx.x] + (x - c);
      lv = c > 0 && toff[threadIdx.x] < A.cap;
    } else if (t < A.ntiles) {
      lv = A.tab[t].max2 >= thr;
      if (!lv) A.counts[t] = 0;
    }
    live[threadIdx.x] = lv;
    tcnt[threadIdx.x] = 0;
  }
  __syncthreads();
  for (int q = 0; q < PG; ++q) {
    if (!live[q]) continue;                              // the same for the whole block
    const long long t = t0 + q;
    const PeakPartial te = A.tab[t];
    const double tmax = te.max2;
    const long long tidx = te.idx;
    if (A.d >= kPeaksTile) {
      if (EMIT) {
        if (threadIdx.x == 0) {
          PeakInst r;
          r.index = tidx; r.value = tmax;
          A.out[toff[q]] = r;
        }
      } else {
        const bool b = beaten_outside<T>(A, t, tmax, tidx);
        if (threadIdx.x == 0) A.counts[t] = tcnt[q] = b ? 0 : 1;
      }
      continue;
    }
    const int H = (int)A.d;
    const long long ts = t * kPeaksTile;
    for (int i = threadIdx.x; i < kPeaksTile + 2 * H; i += PT) {
      const long long g = ts - H + i;
      L[i] = (g >= 0 && g < A.n) ? (double)mag(a[g]) : -1.0;
    }
    __syncthreads();
    bool fl[PE];
    int rank[PE];
#pragma unroll
    for (int e = 0; e < PE; ++e) {
      const int p = e * PT + threadIdx.x;
      const long long g = ts + p;
      bool c = false;
      if (g < A.n) {
        const double v = L[H + p];
        c = v >= thr;
        if (c) {
          const bool beats = tmax > v || (tmax == v && tidx < g);
          const long long dist = g > tidx ? g - tidx : tidx - g;
          if (beats && dist <= A.d) {
            c = false;
          } else {
            for (int k = 1; k <= H; ++k)
              if (L[H + p - k] >= v || L[H + p + k] > v) { c = false; break; }
          }
        }
      }
      const unsigned long long bal = __ballot(c);
      fl[e] = c;
      rank[e] = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[e][w] = __popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0;
      for (int e = 0; e < PE; ++e)
        for (int x = 0; x < PW; ++x) { woff[e][x] = acc; acc += wcnt[e][x]; }
      stot = acc;
    }
    __syncthreads();
    if (!EMIT) {
      if (threadIdx.x == 0) A.counts[t] = tcnt[q] = stot;
    } else {
      const long long base = toff[q];
#pragma unroll
      for (int e = 0; e < PE; ++e) {
        const long long pos = base + woff[e][w] + rank[e];
        if (fl[e] && pos < A.cap) {
          const int p = e * PT + threadIdx.x;
          PeakInst r;
          r.index = ts + p; r.value = L[H + p];
          A.out[pos] = r;
        }
      }
    }
    __syncthreads();                                     // L, wcnt, woff are reused
  }
  if (!EMIT && threadIdx.x == 0) {                       // tcnt: written by this thread alone
    long long g = 0;
    for (int q = 0; q < PG; ++q) g += tcnt[q];
    A.goff[blockIdx.x] = g;
  }
}

// Exclusive scan in place of the ng per-block counts (one block: a contiguous
// chunk per thread, then a block scan of the chunk sums) and the info record.
__global__ __launch_bounds__(1024) void peaks_scan(long long* __restrict__ goff, long long ng,
                                                   const PeakPartial* __restrict__ rec, double thr,
                                                   int relative, PeaksInfo* __restrict__ info) {
  __shared__ long long ws[16];
  const long long chunk = (ng + 1023) / 1024;
  const long long lo = threadIdx.x * chunk;
  const long long hi = lo + chunk < ng ? lo + chunk : ng;
  long long s = 0;
  for (long long i = lo; i < hi; ++i) s += goff[i];
  long long total;
  long long run = block_scan<16>(s, ws, total);
  for (long long i = lo; i < hi; ++i) {
    const long long v = goff[i];
    goff[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    PeaksInfo r;
    r.count = total;
    r.argmax = rec->idx;
    r.max = rec->max2;
    r.thr_used = relative ? __dmul_rn(thr, rec->max2) : thr;
    *info = r;
  }
}

constexpr int kTileGrid = 4096;              // blocks of the tile pass (<= 8192: a one-block finalize)
long long groups_of(long long nt) { return (nt + PG - 1) / PG; }

struct PeaksScratch {
  PeakPartial *tab, *bpart, *rec;
  long long* goff;
  int* counts;
};
PeaksScratch carve(void* scratch, long long nt) {
  PeaksScratch s;
  s.tab = static_cast<PeakPartial*>(scratch);
  s.bpart = s.tab + nt;
  s.rec = s.bpart + kTileGrid;
  s.goff = reinterpret_cast<long long*>(s.rec + 1);
  s.counts = reinterpret_cast<int*>(s.goff + groups_of(nt));
  return s;
}

template <class T>
hipError_t peaks_t(const void* a, long long n, double thr, int relative, long long d, PeakInst* out,
                   long long cap, PeaksInfo* info, void* scratch, hipStream_t st) {
  const long long nt = (n + kPeaksTile - 1) / kPeaksTile;
  const PeaksScratch s = carve(scratch, nt);
  const unsigned g1 = (unsigned)(nt < kTileGrid ? nt : kTileGrid);
  if ((reinterpret_cast<uintptr_t>(a) & 15) == 0)
    hipLaunchKernelGGL((peaks_tile<T, true>), dim3(g1), dim3(PT), 0, st, static_cast<const T*>(a), n, nt, s.tab, s.bpart);
  else
    hipLaunchKernelGGL((peaks_tile<T, false>), dim3(g1), dim3(PT), 0, st, static_cast<const T*>(a), n, nt, s.tab, s.bpart);
  hipError_t e = launch_partial_finalize(s.bpart, g1, 0, s.rec, nullptr, st);
  if (e != hipSuccess) return e;
  PeaksArgs A;
  A.a = a; A.n = n; A.d = d < n ? d : n; A.ntiles = nt; A.cap = cap;
  A.thr = thr; A.relative = relative;
  A.tab = s.tab; A.rec = s.rec; A.counts = s.counts; A.goff = s.goff; A.out = out;
  const unsigned g2 = (unsigned)groups_of(nt);
  hipLaunchKernelGGL((peaks_mark<T, false>), dim3(g2), dim3(PT), 0, st, A);
  hipLaunchKernelGGL(peaks_scan, dim3(1), dim3(1024), 0, st, s.goff, (long long)g2, s.rec, thr, relative, info);
  if (cap > 0) hipLaunchKernelGGL((peaks_mark<T, true>), dim3(g2), dim3(PT), 0, st, A);
  return hipGetLastError();
}

}  // namespace

size_t peaks_scratch_bytes(long long n) {
  const long long nt = (n + kPeaksTile - 1) / kPeaksTile;
  return (size_t)(nt + kTileGrid + 1) * sizeof(PeakPartial) + (size_t)groups_of(nt) * sizeof(long long) +
         (size_t)nt * sizeof(int);
}

hipError_t launch_peaks(int dtype, const void* a, long long n, double thr, int relative, long long d,
                        PeakInst* out, long long cap, PeaksInfo* info, void* scratch, hipStream_t st) {
  if (n < 1 || d < 0 || cap < 0 || !a || !info || !scratch || (cap > 0 && !out)) return hipErrorInvalidValue;
  return dispatch_dtype(dtype, [&](auto tag) {
    return peaks_t<typename decltype(tag)::type>(a, n, thr, relative, d, out, cap, info, scratch, st);
  });
}

}  // namespace vsig
