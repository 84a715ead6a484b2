// The block primitives of the reduction kernels (gfx950): one fold and one scan
// over a block's threads, in an order that is fixed here and nowhere else.  A
// kernel says what it folds (a value type with shfl_xor and merge), not how;
// "the same bytes on every run" rests on every kernel folding in this order.
// No LDS of their own: the caller passes the slots, so a kernel that folds in
// a loop can alternate two slot rows and keep one barrier per iteration.
// Included by os_common.hpp (and through it by reduce.hip, refine.hip,
// xcorr_bank.hip, match.hip), peaks.hip, runs.hip, region.hip, combine.hip,
// analysis.hip and trace.hip.
//
// The fold's order: lane l takes lane l ^ 32, then ^ 16 ... ^ 1 (both lanes of
// a pair form the same value: v.merge(other), a sum as own + other); lane 0
// of every wave stores its wave's value; after one barrier thread 0 merges
// the waves 1, 2, ... in ascending order into its own.
// The scan's order: an inclusive shift-up scan over each wave's lanes (offsets
// 1, 2 ... 32); lane 63 stores the wave's total; after one barrier every
// thread adds the totals of the waves before its own, in ascending order.
#pragma once
#include "dtype.hpp"

namespace vsig {

// ---------------------------------------------------------------------------
// Fold
// ---------------------------------------------------------------------------
// The first W lanes of a wave among themselves (W a power of two): every one
// of them ends with the value of all W.
template <int W = 64, class V>
__device__ __forceinline__ void wave_fold(V& v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v.merge(v.shfl_xor(off));
}

// A block of NW waves; slots: NW of V in LDS.  Holds a barrier, so every
// thread of the block calls it.  The result is valid in thread 0 alone.
template <int NW, class V>
__device__ __forceinline__ void block_fold(V& v, V* slots) {
  wave_fold(v);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 1; q < NW; ++q) v.merge(slots[q]);
}

// Value types.  The first maximum: larger value, then lower index (betterd).
struct FirstMax {
  double m;
  long long i;
  __device__ __forceinline__ FirstMax shfl_xor(int off) const { return {__shfl_xor(m, off), __shfl_xor(i, off)}; }
  __device__ __forceinline__ void merge(const FirstMax& o) { betterd(m, i, o.m, o.i); }
};

// K doubles, added.
template <int K>
struct Sums {
  double s[K];
  __device__ __forceinline__ Sums shfl_xor(int off) const {
    Sums o;
#pragma unroll
    for (int k = 0; k < K; ++k) o.s[k] = __shfl_xor(s[k], off);
    return o;
  }
  __device__ __forceinline__ void merge(const Sums& o) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += o.s[k];
  }
};

// First and last index and a count.
struct Span {
  long long first, last, count;
  __device__ __forceinline__ Span shfl_xor(int off) const {
    return {__shfl_xor(first, off), __shfl_xor(last, off), __shfl_xor(count, off)};
  }
  __device__ __forceinline__ void merge(const Span& o) {
    first = o.first < first ? o.first : first;
    last = o.last > last ? o.last : last;
    count += o.count;
  }
};

// The first maximum with K sums beside it: m, i and s[K].
template <int K>
struct FirstMaxSums : FirstMax, Sums<K> {
  __device__ __forceinline__ FirstMaxSums shfl_xor(int off) const {
    return {FirstMax::shfl_xor(off), Sums<K>::shfl_xor(off)};
  }
  __device__ __forceinline__ void merge(const FirstMaxSums& o) {
    FirstMax::merge(o);
    Sums<K>::merge(o);
  }
};

// ---------------------------------------------------------------------------
// Scan
// ---------------------------------------------------------------------------
// The sum of v over the threads before this one, and the block's total (T:
// long long, double).  slots: NW of T in LDS, free again after the caller's
// next barrier.  Holds a barrier.
template <int NW, class T>
__device__ __forceinline__ T block_scan(T v, T* slots, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  if (lane == 63) slots[w] = x;
  __syncthreads();
  T before = 0;
  total = 0;
  for (int q = 0; q < NW; ++q) {
    if (q < w) before += slots[q];
    total += slots[q];
  }
  return before + x - v;
}

// p: the maximum of x over the threads before this one, q: the minimum of y
// over those after it; -none / none where there are none.  sx, sy: NW slots
// each.  Holds a barrier.
template <int NW>
__device__ __forceinline__ void block_scan_edges(long long x, long long y, long long none, long long* sx,
                                                 long long* sy, long long& p, long long& q) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long ux = __shfl_up(x, off), dy = __shfl_down(y, off);
    if (lane >= off) x = ux > x ? ux : x;
    if (lane + off < 64) y = dy < y ? dy : y;
  }
  if (lane == 63) sx[w] = x;
  if (lane == 0) sy[w] = y;
  __syncthreads();
  p = __shfl_up(x, 1);
  q = __shfl_down(y, 1);
  if (lane == 0) p = -none;
  if (lane == 63) q = none;
  for (int k = 0; k < NW; ++k) {
    if (k < w) p = sx[k] > p ? sx[k] : p;
    if (k > w) q = sy[k] < q ? sy[k] : q;
  }
}

}  // namespace vsig
