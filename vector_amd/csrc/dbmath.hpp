// normalize_spectrogram's 10 * np.log10(|S| + floor) of one value, in the dtype
// numpy evaluates it in (float32 S with a float32 floor stays float32).  The
// float32 log10 is correctly rounded here; numpy's SIMD log10f is within a
// few ulp of that, so dB values agree to a few ulp (not bit-exact).  Every
// step is an explicitly rounded operation: a caller's following subtraction
// cannot be contracted into the multiply.  Shared by analysis.hip (the dB
// map) and display.hip (the image), so both round alike.  db20_of is the
// amplitude form, 20 * np.log10(|a| + eps), of the line traces (trace.hip):
// the same steps with the other constant.
#pragma once
#include <hip/hip_runtime.h>

namespace vsig {

__device__ __forceinline__ double db_of(double a, double floor_) {
  return __dmul_rn(10.0, log10(__dadd_rn(fabs(a), floor_)));
}
__device__ __forceinline__ float db_of(float a, float floor_) {
  return __fmul_rn(10.f, (float)log10((double)__fadd_rn(fabsf(a), floor_)));
}
__device__ __forceinline__ double db20_of(double a, double eps) {
  return __dmul_rn(20.0, log10(__dadd_rn(fabs(a), eps)));
}
__device__ __forceinline__ float db20_of(float a, float eps) {
  return __fmul_rn(20.f, (float)log10((double)__fadd_rn(fabsf(a), eps)));
}

}  // namespace vsig
