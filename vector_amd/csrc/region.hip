// Region powers (gfx950): validate_transplant_quality's three mean powers
// (utils.py:1546-1552) of two complex64 regions a, b of n samples in one pass,
//   S0 = sum |a|^2,  S1 = sum |b|^2,  S2 = sum |a - b|^2,
// each element formed in float32 exactly as numpy forms np.abs(x) ** 2 on
// complex64 (m = np_cabs, then m * m rounded to float32; a - b per component
// in float32), widened to double and summed in double.
//
//   region_power     grid-stride pass, 16 B read per sample (8 B of each
//                    operand): one fixed-slot partial of three doubles per
//                    block.  Both operands 16-byte aligned after the same
//                    head (0 or 1 sample): 16-byte loads, two samples per
//                    lane and trip, two trips in flight; else 8-byte loads.
//                    The head and an odd last sample go to block 0.
//   region_finalize  one block adds the partials in a fixed order.
//
// The grid is a function of n alone and nothing is accumulated across blocks
// by atomics, so the sums have the same bits on every run over the same
// operands.  a == b is fine: both are only read.
#include "block_ops.hpp"

namespace vsig {

namespace {

constexpr int RT = 256;                      // threads per block
constexpr int RV = 2;                        // samples per lane and trip (one 16-byte load an operand)
constexpr int RW = RT / 64;

using RegionPartial = Sums<3>;               // S0, S1, S2 of a block, folded in block_ops.hpp's order
static_assert(sizeof(RegionPartial) == 24, "three doubles per block");

#pragma clang fp contract(off)

// np.abs(z) ** 2 of one complex64 value, in float32
__device__ __forceinline__ float pw(float re, float im) {
  const float m = np_cabs(re, im);
  return m * m;
}

__device__ __forceinline__ void acc(double* s, float ar, float ai, float br, float bi) {
  const float dr = ar - br, di = ai - bi;    // complex64 subtraction
  s[0] += (double)pw(ar, ai);
  s[1] += (double)pw(br, bi);
  s[2] += (double)pw(dr, di);
}

__device__ __forceinline__ void acc4(double* s, const float4& u, const float4& v) {
  acc(s, u.x, u.y, v.x, v.y);
  acc(s, u.z, u.w, v.z, v.w);
}

// VEC: a + head and b + head are 16-byte aligned (head = 0 or 1).
template <bool VEC>
__global__ __launch_bounds__(RT) void region_power(const float2* __restrict__ a,
                                                   const float2* __restrict__ b, long long n,
                                                   int head, RegionPartial* __restrict__ parts) {
  __shared__ RegionPartial slots[RW];
  RegionPartial part{{0.0, 0.0, 0.0}};
  double* s = part.s;
  const long long stride = (long long)gridDim.x * RT;
  const long long t0 = (long long)blockIdx.x * RT + threadIdx.x;
  if (VEC) {
    const long long body = n - head, nv = body / RV;          // 16-byte units
    const float4* a4 = reinterpret_cast<const float4*>(a + head);
    const float4* b4 = reinterpret_cast<const float4*>(b + head);
    long long p = t0;
    for (; p + stride < nv; p += 2 * stride) {                // two trips in flight
      const float4 u0 = a4[p], v0 = b4[p];
      const float4 u1 = a4[p + stride], v1 = b4[p + stride];
      acc4(s, u0, v0);
      acc4(s, u1, v1);
    }
    if (p < nv) acc4(s, a4[p], b4[p]);
    if (t0 == 0) {                                            // the peeled ends
      if (head) acc(s, a[0].x, a[0].y, b[0].x, b[0].y);
      if (body & 1) acc(s, a[n - 1].x, a[n - 1].y, b[n - 1].x, b[n - 1].y);
    }
  } else {
    for (long long i = t0; i < n; i += stride) {
      const float2 u = a[i], v = b[i];
      acc(s, u.x, u.y, v.x, v.y);
    }
  }
  block_fold<RW>(part, slots);
  if (threadIdx.x == 0) parts[blockIdx.x] = part;
}

__global__ __launch_bounds__(RT) void region_finalize(const RegionPartial* __restrict__ parts,
                                                      int nparts, double* __restrict__ out) {
  __shared__ RegionPartial slots[RW];
  RegionPartial part{{0.0, 0.0, 0.0}};
  for (int i = threadIdx.x; i < nparts; i += RT) part.merge(parts[i]);
  block_fold<RW>(part, slots);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = part.s[k];
  }
}

}  // namespace

// Blocks of the pass over n samples: one per RT * RV samples, at most
// kRegionBlocks (the rest by the grid stride).
static int region_grid(long long n) {
  const long long g = (n + RT * RV - 1) / (RT * RV);
  return (int)(g < 1 ? 1 : g > kRegionBlocks ? kRegionBlocks : g);
}

size_t region_scratch_bytes() { return (size_t)kRegionBlocks * sizeof(RegionPartial); }

hipError_t launch_region_power(const float2* a, const float2* b, long long n, double* sums,
                               void* scratch, hipStream_t st) {
  if (n < 1 || !a || !b || !sums || !scratch) return hipErrorInvalidValue;
  RegionPartial* parts = static_cast<RegionPartial*>(scratch);
  const int grid = region_grid(n);
  // slices of complex64 arrays: 8-byte aligned, 16-byte aligned after the
  // same head only when both start on the same half of a 16-byte unit
  const unsigned long long ma = reinterpret_cast<unsigned long long>(a) & 15;
  const unsigned long long mb = reinterpret_cast<unsigned long long>(b) & 15;
  if (ma == mb && (ma == 0 || ma == 8)) {
    hipLaunchKernelGGL(region_power<true>, dim3(grid), dim3(RT), 0, st, a, b, n, ma ? 1 : 0, parts);
  } else {
    hipLaunchKernelGGL(region_power<false>, dim3(grid), dim3(RT), 0, st, a, b, n, 0, parts);
  }
  hipLaunchKernelGGL(region_finalize, dim3(1), dim3(RT), 0, st, parts, grid, sums);
  return hipGetLastError();
}

}  // namespace vsig
