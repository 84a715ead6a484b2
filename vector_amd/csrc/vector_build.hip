// Vector assembly: the periodic-packet accumulate of generate_vector
// (unified_gui.py:1692-1791, main.py:214-284) and its peak normalise.
//
//   vector_build     out[p] = sum over packets (list order), then instances k
//                    (ascending), of y[p - start - k*period] -- the adds numpy's
//                    sequential  vector[a:b] += y  performs on a zeroed complex64
//                    vector, in the same order, so the result is numpy's to the
//                    bit.  Gather form: a block owns 8192 consecutive output
//                    samples, keeps them in registers over every descriptor and
//                    writes each sample once (8 B per sample of HBM traffic;
//                    the packets are re-read from L2).  Optionally folds
//                    max |out| (numpy's complex64 abs) into one device float.
//   normalize_c64    y = x / m with m read from device memory: numpy's
//                    complex64 / float32 (generate_vector's vector / max_val),
//                    unchanged when m is not > 0.
#include <hip/hip_runtime.h>

#include "npabs.hpp"
#include "vsig_kernels.h"

namespace vsig {

typedef float vb_f4 __attribute__((ext_vector_type(4)));

constexpr int kVbThreads = 256;
constexpr int kVbPairs = 16;                                // 16-byte pairs per lane
constexpr int kVbRow = 2 * kVbThreads;                      // samples per pair row (512)
constexpr int kVbTile = kVbRow * kVbPairs;                  // samples per block (8192)

// floor(a / b) for 0 <= a < 2^52, b >= 1: a correctly rounded double quotient
// is within one of it; the products below cannot overflow (q >= 1 => b <= a).
__device__ __forceinline__ long long vb_floordiv(long long a, long long b) {
  long long q = (long long)((double)a / (double)b);
  if (q * b > a) --q;
  else if (b <= a - q * b) ++q;
  return q;
}

// Positions: q = p + head counts from the 16-byte boundary at or before out
// (head = 1 when out is only 8-byte aligned), so pair (q, q + 1), q even, is one
// aligned 16-byte store; q = 0 with head = 1 (p = -1) and p >= n are masked,
// which leaves the odd first / last sample to an 8-byte store.
// Lane t's pair u is q = tile + 2 (t + 256 u).
template <bool LOAD, bool MAX>
__global__ __launch_bounds__(kVbThreads) void vector_build(PlaceBatch pb, float2* __restrict__ out,
                                                           long long n, int head,
                                                           unsigned* __restrict__ maxbits) {
  const int t = threadIdx.x;
  const long long pbase = (long long)blockIdx.x * kVbTile - head;   // p of the tile's q = 0
  const long long tlo = pbase < 0 ? 0 : pbase;                      // the tile's samples [tlo, thi)
  const long long thi = pbase + kVbTile < n ? pbase + kVbTile : n;
  float2 a0[kVbPairs], a1[kVbPairs];
#pragma unroll
  for (int u = 0; u < kVbPairs; ++u) {
    a0[u] = make_float2(0.f, 0.f);
    a1[u] = make_float2(0.f, 0.f);
    if constexpr (LOAD) {                 // a later launch of a long packet list keeps adding
      const long long p0 = pbase + 2 * (t + kVbThreads * u);
      if (p0 >= 0 && p0 + 1 < n) {
        const vb_f4 v = *reinterpret_cast<const vb_f4*>(out + p0);
        a0[u] = make_float2(v.x, v.y);
        a1[u] = make_float2(v.z, v.w);
      } else {
        if (p0 >= 0 && p0 < n) a0[u] = out[p0];
        if (p0 + 1 < n) a1[u] = out[p0 + 1];
      }
    }
  }
  for (int d = 0; d < pb.nd; ++d) {       // block-uniform: descriptors, instances, row range
    const PlaceDesc P = pb.d[d];
    const long long a = thi - 1 - P.start;                 // instances starting inside or before
    if (a < 0) continue;
    long long k_hi = vb_floordiv(a, P.period);
    if (k_hi > P.count - 1) k_hi = P.count - 1;
    const long long c = tlo - P.len - P.start + 1;         // first k with start + k period + len > tlo
    const long long k_lo = c <= 0 ? 0 : vb_floordiv(c - 1, P.period) + 1;
    const float2* __restrict__ y = P.y;
    const unsigned long long len = (unsigned long long)P.len;
    for (long long k = k_lo; k <= k_hi; ++k) {
      const long long rel = P.start + k * P.period - pbase;   // instance start, tile-relative
      const int lo = rel > 0 ? (int)rel : 0;
      const int hi = rel + P.len < kVbTile ? (int)(rel + P.len) : kVbTile;
      const int u_lo = lo / kVbRow, u_hi = (hi - 1) / kVbRow;
#pragma unroll
      for (int u = 0; u < kVbPairs; ++u) {
        if (u >= u_lo && u <= u_hi) {
          const long long i0 = 2 * (t + kVbThreads * u) - rel;
          if ((unsigned long long)i0 < len) {
            const float2 v = y[i0];
            a0[u] = make_float2(a0[u].x + v.x, a0[u].y + v.y);
          }
          if ((unsigned long long)(i0 + 1) < len) {
            const float2 v = y[i0 + 1];
            a1[u] = make_float2(a1[u].x + v.x, a1[u].y + v.y);
          }
        }
      }
    }
  }
  // max |z| of what this lane writes, as the bit pattern of numpy's fp32 abs
  // (non-negative floats order like their bits; a NaN ranks above everything,
  // as np.max propagates it).  |z|^2 in fp32 screens the samples: one more
  // than 1e-5 below the lane's largest |z|^2 so far cannot hold the maximum
  // (both roundings are ~1e-7); a tiny, infinite or NaN |z|^2 is never screened.
  unsigned mb = 0;
  float s_thr = 0.f, s_max = 0.f;
  auto fold = [&](float2 v) {
    const float s = v.x * v.x + v.y * v.y;
    if (!(s < s_thr)) {
      const unsigned b = __float_as_uint(np_cabs(v.x, v.y)) & 0x7fffffffu;
      mb = b > mb ? b : mb;
      if (s > s_max) {
        s_max = s;
        s_thr = s > 1e-30f ? s * (1.f - 1e-5f) : 0.f;
      }
    }
  };
#pragma unroll
  for (int u = 0; u < kVbPairs; ++u) {
    const long long p0 = pbase + 2 * (t + kVbThreads * u);
    const bool ok0 = p0 >= 0 && p0 < n, ok1 = p0 + 1 < n;
    if (ok0 && ok1) {
      const vb_f4 w = {a0[u].x, a0[u].y, a1[u].x, a1[u].y};
      __builtin_nontemporal_store(w, reinterpret_cast<vb_f4*>(out + p0));
    } else {
      if (ok0) out[p0] = a0[u];
      if (ok1) out[p0 + 1] = a1[u];
    }
    if constexpr (MAX) {
      if (ok0) fold(a0[u]);
      if (ok1) fold(a1[u]);
    }
  }
  if constexpr (MAX) {
    __shared__ unsigned wmax[kVbThreads / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned other = (unsigned)__shfl_xor((int)mb, o, 64);
      mb = other > mb ? other : mb;
    }
    if ((t & 63) == 0) wmax[t >> 6] = mb;
    __syncthreads();
    if (t == 0) {
      unsigned m = wmax[0];
#pragma unroll
      for (int w = 1; w < kVbThreads / 64; ++w) m = wmax[w] > m ? wmax[w] : m;
      // the running maximum only grows: a block at or below it has nothing to add
      if (m > __hip_atomic_load(maxbits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxbits, m);
    }
  }
}

// numpy divides a complex64 by a float32 scalar with Smith's formula, which for
// a zero imaginary divisor is a multiply of both parts by the rounded
// reciprocal, after each part has taken the other part times that zero
// (nothing for a finite part, NaN for an infinite or NaN one: with an infinite
// peak the sample that holds it becomes NaN in both parts; see wv_quantize,
// stream_ops.hip).  Same alignment scheme as vector_build when x and y share
// their 16-byte phase (in place: always).
__device__ __forceinline__ float2 np_div_real(float2 v, float r) {
  return make_float2((v.x + v.y * 0.f) * r, (v.y - v.x * 0.f) * r);
}
template <bool V4>
__global__ __launch_bounds__(256) void normalize_c64(const float2* x, long long n,
                                                     const float* __restrict__ maxabs, float2* y,
                                                     int head) {
  const float m = *maxabs;
  const bool on = m > 0.f;
  const float r = on ? __fdiv_rn(1.f, m) : 1.f;
  const long long stride = (long long)gridDim.x * 256;
  if constexpr (V4) {
    const long long npairs = (n + head + 1) / 2;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < npairs; j += stride) {
      const long long p0 = 2 * j - head;
      if (p0 >= 0 && p0 + 1 < n) {
        vb_f4 v = *reinterpret_cast<const vb_f4*>(x + p0);
        if (on) {
          const float2 p = np_div_real(make_float2(v.x, v.y), r), q = np_div_real(make_float2(v.z, v.w), r);
          v = vb_f4{p.x, p.y, q.x, q.y};
        }
        __builtin_nontemporal_store(v, reinterpret_cast<vb_f4*>(y + p0));
      } else {
        if (p0 >= 0 && p0 < n) {
          const float2 v = x[p0];
          y[p0] = on ? np_div_real(v, r) : v;
        }
        if (p0 + 1 < n) {
          const float2 v = x[p0 + 1];
          y[p0 + 1] = on ? np_div_real(v, r) : v;
        }
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
      const float2 v = x[i];
      y[i] = on ? np_div_real(v, r) : v;
    }
  }
}

// ---------------------------------------------------------------- launchers
// One launch of up to kPlacesPerLaunch descriptors over the whole vector;
// load: start from out (a later launch of a longer list); maxabs (last launch
// only): a device float zeroed on the stream before this launch.
hipError_t launch_vector_build(const PlaceBatch& pb, float2* out, long long n, int load,
                               float* maxabs, hipStream_t st) {
  const int head = (int)((reinterpret_cast<uintptr_t>(out) >> 3) & 1);
  const long long g = (n + head + kVbTile - 1) / kVbTile;
  if (g < 1) return hipSuccess;
  if (g > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)g), block(kVbThreads);
  unsigned* mb = reinterpret_cast<unsigned*>(maxabs);
  if (load) {
    if (maxabs) hipLaunchKernelGGL((vector_build<true, true>), grid, block, 0, st, pb, out, n, head, mb);
    else hipLaunchKernelGGL((vector_build<true, false>), grid, block, 0, st, pb, out, n, head, mb);
  } else {
    if (maxabs) hipLaunchKernelGGL((vector_build<false, true>), grid, block, 0, st, pb, out, n, head, mb);
    else hipLaunchKernelGGL((vector_build<false, false>), grid, block, 0, st, pb, out, n, head, mb);
  }
  return hipGetLastError();
}

hipError_t launch_normalize_c64(const float2* x, long long n, const float* maxabs, float2* y,
                                hipStream_t st) {
  const int hx = (int)((reinterpret_cast<uintptr_t>(x) >> 3) & 1);
  const int hy = (int)((reinterpret_cast<uintptr_t>(y) >> 3) & 1);
  if (hx == hy) {
    long long g = ((n + hx + 1) / 2 + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL((normalize_c64<true>), dim3((unsigned)g), dim3(256), 0, st, x, n, maxabs, y, hx);
  } else {
    long long g = (n + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL((normalize_c64<false>), dim3((unsigned)g), dim3(256), 0, st, x, n, maxabs, y, 0);
  }
  return hipGetLastError();
}

}  // namespace vsig
