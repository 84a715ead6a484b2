// The element-type layer of the kernels that take "an array of dtype VSIG_*"
// and work on |a| (gfx950): numpy's |a| of one element, the two compare rules
// of their reductions, 16-byte packs, and the switch from a dtype code to the
// element type.  Included by block_ops.hpp (and through it by os_common.hpp
// and its includers, peaks.hip, runs.hip, region.hip, combine.hip,
// analysis.hip, trace.hip), display.hip and the C-ABI layer (vsig_ctx.hpp).
#pragma once
#include "npabs.hpp"
#include "vsig_kernels.h"

namespace vsig {

// The real type numpy's np.abs of an array of T has.
template <class T> struct Real { using type = double; };
template <> struct Real<float2> { using type = float; };
template <> struct Real<float> { using type = float; };

// np.abs of one element, in the array's precision (widening a float result to
// double is exact).
__device__ __forceinline__ double mag(double2 v) { return np_cabs(v.x, v.y); }
__device__ __forceinline__ float mag(float2 v) { return np_cabs(v.x, v.y); }
__device__ __forceinline__ double mag(double v) { return fabs(v); }
__device__ __forceinline__ float mag(float v) { return fabsf(v); }

// 16 bytes of T, for one 16-byte load.
template <class T> struct alignas(16) Pack16 { T e[16 / sizeof(T)]; };

// Larger value, then lower index: the first maximum.  A NaN compares false, so
// it is never taken.
template <class R>
__device__ __forceinline__ void betterd(R& m, long long& i, R m2, long long i2) {
  if (m2 > m || (m2 == m && i2 < i)) { m = m2; i = i2; }
}

// np.max / np.min of two values: a NaN on either side wins and then stays.
template <class R> __host__ __device__ __forceinline__ R np_max(R a, R b) { return (b > a || b != b) ? b : a; }
template <class R> __host__ __device__ __forceinline__ R np_min(R a, R b) { return (b < a || b != b) ? b : a; }

// f(Elem<T>{}) for the element type T of a dtype code; hipErrorInvalidValue
// for any other code (dispatch_real: the float64 / float32 kernels).
template <class T> struct Elem { using type = T; };

template <class F> hipError_t dispatch_dtype(int dtype, F&& f) {
  switch (dtype) {
    case VSIG_C128: return f(Elem<double2>{});
    case VSIG_C64: return f(Elem<float2>{});
    case VSIG_F64: return f(Elem<double>{});
    case VSIG_F32: return f(Elem<float>{});
    default: return hipErrorInvalidValue;
  }
}
template <class F> hipError_t dispatch_real(int dtype, F&& f) {
  switch (dtype) {
    case VSIG_F64: return f(Elem<double>{});
    case VSIG_F32: return f(Elem<float>{});
    default: return hipErrorInvalidValue;
  }
}

// Host side: is the code one of the four, and its element's size in bytes.
inline bool dtype_ok(int dtype) { return dtype >= VSIG_C128 && dtype <= VSIG_F32; }
inline size_t dtype_bytes(int dtype) {
  return dtype == VSIG_C128 ? 16 : (dtype == VSIG_F32 ? 4 : 8);
}

}  // namespace vsig
