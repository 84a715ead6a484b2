// Spectrogram image (gfx950): the display tail of the reference's three plot
// sites -- plot_spectrogram (utils.py:429-449, 491-499), adjust_packet_bounds_gui
// (utils.py:1017-1022, 1062), vector_analyzer/spectrogram_analysis.py:56-62 --
// in one pass from Sxx to RGBA bytes.  No dB map is written.
//
// Per output pixel (r, c), pool factors pf, pt >= 1:
//   P  = max |S[i, j]|, i in [max(r pf - median, 0), min((r+1) pf, n_freq)),
//                       j in [c pt, min((c+1) pt, n_time))
//   db = 10 log10(P + floor)          (db_of: rounded as the dB map is)
//   xa = (db - vmin) / (vmax - vmin) * 256, in the input's dtype
//   row = bad if xa is NaN, under if xa < 0, 255 if xa == 256, over if
//         xa > 256, else trunc(xa)    (matplotlib's Normalize + Colormap)
// ndimage.median_filter(db, size=(2, 1)) is max(db[i], db[max(i-1, 0)]) and
// the dB transform is non-decreasing, so the filter is one more row at the
// bottom of the window: the halo.  The maximum propagates NaN, so a NaN
// anywhere in a window gives the bad row.
//
// Geometry.  x is the input's fast axis, y its slow one: x = frequency for
// frame-major memory [n_time][n_freq] (FF), x = time for a C-contiguous
// (n_freq, n_time) array.  A block of 256 threads owns oxb x oyb output
// pixels (oyb = OYB, or a half or a quarter of it while the grid would have
// fewer than 1024 blocks) and walks its x range in chunks of XW inputs:
//   pass 1  lanes along x (16-byte loads when base and ld are 16-byte
//           aligned, else one element a lane; never past a row's end), 4
//           or 8 rows in flight per lane: the maximum over each output row's y
//           window goes to the LDS tile L[OYB][XW + 1]
//   pass 2  each thread folds the x window of its up to NPIX pixels out of L.
//           FF is a transpose: lanes run along y there (the row pitch XW + 1
//           is odd, so the column reads spread over the banks) and the
//           4-byte pixel stores are contiguous along time in both layouts.
// oxb is chosen so that a block's x range, its halo included, is one chunk
// whenever px <= XW - 4.  No atomics and no cross-block hand-off: the same
// input gives the same bytes on every run.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "dbmath.hpp"
#include "dtype.hpp"

namespace vsig {

namespace {

#pragma clang fp contract(off)

constexpr int IT = 256;     // threads per block
constexpr int NPIX = 16;    // output pixels per thread
constexpr int NLUT = 259;   // 256 rows, under, over, bad (matplotlib's _lut order)

template <bool FF> struct Tile;
template <> struct Tile<true> { static constexpr int XW = 64, OYB = 64; };
template <> struct Tile<false> { static constexpr int XW = 256, OYB = 16; };
static_assert(Tile<true>::XW * Tile<true>::OYB == NPIX * IT, "one pixel slot per input cell");
static_assert(Tile<false>::XW * Tile<false>::OYB == NPIX * IT, "one pixel slot per input cell");

struct ImgGeom {
  long long nx, ny, ld;     // input extents along x (fast) and y (slow), leading dimension
  long long onx, ony;       // output extents along x and y
  long long nbx;            // blocks along x
  long long rows, cols;     // output image
  int px, py;               // pool factors along x and y
  int hx, hy;               // the median's one-cell halo below a window, along x or y
  int oxb, oyb;             // output pixels along x and y per block (oyb <= OYB)
  int flip;
};

template <class T, int N> struct Vec;
template <> struct Vec<float, 4> { using type = float4; };
template <> struct Vec<double, 2> { using type = double2; };

template <class T, int N>
__device__ __forceinline__ void load_row(const T* __restrict__ p, bool full, long long left, T* v) {
  if constexpr (N > 1) {
    if (full) {
      using V = typename Vec<T, N>::type;
      const V u = *reinterpret_cast<const V*>(p);
      const T* e = reinterpret_cast<const T*>(&u);
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] = e[k];
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = k < left ? p[k] : T(0);
}

// The maximum of |S| over rows [y0, y1) at N elements from p0 (row y0), RB rows
// in flight per lane.
template <class T, int N, int RB>
__device__ __forceinline__ void column_max(const T* __restrict__ p0, long long ld, long long y0, long long y1,
                                           bool full, long long left, T* m) {
  for (long long y = y0; y < y1; y += RB) {
    T v[RB][N];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      if (y + b < y1) {
        load_row<T, N>(p0 + (y + b - y0) * ld, full, left, v[b]);
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[b][k] = T(0);
      }
    }
#pragma unroll
    for (int b = 0; b < RB; ++b) {
#pragma unroll
      for (int k = 0; k < N; ++k) m[k] = np_max(m[k], mag(v[b][k]));
    }
  }
}

__device__ __forceinline__ float scaled(float db, float vmin, float den) {
  return __fmul_rn(__fdiv_rn(__fsub_rn(db, vmin), den), 256.f);
}
__device__ __forceinline__ double scaled(double db, double vmin, double den) {
  return __dmul_rn(__ddiv_rn(__dsub_rn(db, vmin), den), 256.0);
}

template <class T>
__device__ __forceinline__ int colour_row(T P, T floor_, T vmin, T den) {
  const T xa = scaled(db_of(P, floor_), vmin, den);
  if (xa != xa) return 258;
  if (xa < T(0)) return 256;
  if (xa == T(256)) return 255;
  if (xa > T(256)) return 257;
  return (int)xa;
}

// N: elements per load (16 bytes' worth, or 1)
template <class T, bool FF, int N>
__global__ __launch_bounds__(IT) void spectrogram_image(const T* __restrict__ S, ImgGeom g, T floor_,
                                                        T vmin, T vmax,
                                                        const unsigned int* __restrict__ lut,
                                                        unsigned int* __restrict__ out) {
  constexpr int XW = Tile<FF>::XW, OYB = Tile<FF>::OYB, PITCH = XW + 1;
  constexpr int XL = XW / N, YG = IT / XL;
  __shared__ T L[OYB * PITCH];
  __shared__ unsigned int lut_s[NLUT];
  for (int i = threadIdx.x; i < NLUT; i += IT) lut_s[i] = lut[i];   // read after the loop's barriers

  const long long bx = blockIdx.x % g.nbx, by = blockIdx.x / g.nbx;
  const long long ox0 = bx * g.oxb, oy0 = by * g.oyb;
  const int oxn = (int)(g.onx - ox0 < g.oxb ? g.onx - ox0 : g.oxb);
  const int oyn = (int)(g.ony - oy0 < g.oyb ? g.ony - oy0 : g.oyb);
  const int npix = oxn * oyn;
  long long xb0 = ox0 * g.px - g.hx;
  xb0 = xb0 < 0 ? 0 : xb0;
  xb0 -= xb0 % N;
  long long xb1 = (ox0 + oxn) * g.px;
  xb1 = xb1 > g.nx ? g.nx : xb1;

  T acc[NPIX];
#pragma unroll
  for (int j = 0; j < NPIX; ++j) acc[j] = T(0);

  const int xl = threadIdx.x % XL, yg = threadIdx.x / XL;
  for (long long cx = xb0; cx < xb1; cx += XW) {
    // pass 1: the maximum over each output row's y window, lanes along x
    const long long x = cx + (long long)xl * N;
    const long long left = g.nx - x;                  // elements of the row from x on
    for (int oyl = yg; oyl < oyn && left > 0; oyl += YG) {      // cells past either end are never read back
      T m[N];
#pragma unroll
      for (int k = 0; k < N; ++k) m[k] = T(0);
      {
        const long long oy = oy0 + oyl;
        long long y0 = oy * g.py - g.hy;
        y0 = y0 < 0 ? 0 : y0;
        long long y1 = (oy + 1) * g.py;
        y1 = y1 > g.ny ? g.ny : y1;
        const bool full = left >= N;
        const T* p0 = S + y0 * g.ld + x;
        if (g.py > 4)                                   // wave-uniform: deep windows keep more rows in flight
          column_max<T, N, 8>(p0, g.ld, y0, y1, full, left, m);
        else
          column_max<T, N, 4>(p0, g.ld, y0, y1, full, left, m);
      }
#pragma unroll
      for (int k = 0; k < N; ++k) L[oyl * PITCH + xl * N + k] = m[k];
    }
    __syncthreads();
    // pass 2: the x window of each pixel, out of the tile
#pragma unroll
    for (int j = 0; j < NPIX; ++j) {
      const int p = threadIdx.x + j * IT;
      if (p < npix) {
        const int oxl = FF ? p / oyn : p % oxn, oyl = FF ? p % oyn : p / oxn;
        const long long ox = ox0 + oxl;
        long long a = ox * g.px - g.hx;
        a = a < cx ? cx : a;                          // cx >= 0
        long long b = (ox + 1) * g.px;
        b = b > g.nx ? g.nx : b;
        b = b > cx + XW ? cx + XW : b;
        T m = acc[j];
        for (long long xx = a; xx < b; ++xx) m = np_max(m, L[oyl * PITCH + (int)(xx - cx)]);
        acc[j] = m;
      }
    }
    __syncthreads();
  }

  const T den = vmax - vmin;
#pragma unroll
  for (int j = 0; j < NPIX; ++j) {
    const int p = threadIdx.x + j * IT;
    if (p < npix) {
      const int oxl = FF ? p / oyn : p % oxn, oyl = FF ? p % oyn : p / oxn;
      long long r = FF ? ox0 + oxl : oy0 + oyl;
      const long long c = FF ? oy0 + oyl : ox0 + oxl;
      if (g.flip) r = g.rows - 1 - r;
      out[r * g.cols + c] = lut_s[colour_row<T>(acc[j], floor_, vmin, den)];
    }
  }
}

template <class T, bool FF>
hipError_t image_t(const void* sxx, long long n_freq, long long n_time, long long ld, double floor_,
                   double vmin, double vmax, int median, int flip, int pf, int pt,
                   const unsigned char* lut, unsigned char* rgba, hipStream_t st) {
  constexpr int XW = Tile<FF>::XW, OYB = Tile<FF>::OYB, NV = 16 / (int)sizeof(T);
  ImgGeom g;
  g.nx = FF ? n_freq : n_time;
  g.ny = FF ? n_time : n_freq;
  g.ld = ld;
  g.px = FF ? pf : pt;
  g.py = FF ? pt : pf;
  g.hx = FF && median;
  g.hy = !FF && median;
  g.rows = (n_freq + pf - 1) / pf;
  g.cols = (n_time + pt - 1) / pt;
  g.onx = FF ? g.rows : g.cols;
  g.ony = FF ? g.cols : g.rows;
  g.flip = flip;
  // 16-byte loads need every row to start on a 16-byte boundary
  const bool vec = reinterpret_cast<uintptr_t>(sxx) % 16 == 0 && (ld * (long long)sizeof(T)) % 16 == 0;
  const int n = vec ? NV : 1;
  // a block's x range (oxb px cells, plus the halo rounded down to a load) in one chunk
  long long oxb = (XW - (g.hx ? n : 0)) / g.px;
  if (oxb >= n) oxb -= oxb % n;
  g.oxb = (int)(oxb < 1 ? 1 : oxb);
  g.nbx = (g.onx + g.oxb - 1) / g.oxb;
  // a small image (heavy pooling) in more, shorter blocks: at least ~4 a CU in flight
  g.oyb = OYB;
  while (g.oyb > OYB / 4 && g.nbx * ((g.ony + g.oyb - 1) / g.oyb) < 1024) g.oyb /= 2;
  const long long nby = (g.ony + g.oyb - 1) / g.oyb;
  if (g.nbx > INT_MAX / nby) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(g.nbx * nby));
  const unsigned int* l32 = reinterpret_cast<const unsigned int*>(lut);
  unsigned int* o32 = reinterpret_cast<unsigned int*>(rgba);
  if (vec)
    hipLaunchKernelGGL((spectrogram_image<T, FF, NV>), grid, dim3(IT), 0, st, static_cast<const T*>(sxx), g,
                       (T)floor_, (T)vmin, (T)vmax, l32, o32);
  else
    hipLaunchKernelGGL((spectrogram_image<T, FF, 1>), grid, dim3(IT), 0, st, static_cast<const T*>(sxx), g,
                       (T)floor_, (T)vmin, (T)vmax, l32, o32);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_spectrogram_image(int dtype, const void* sxx, long long n_freq, long long n_time,
                                    int freq_fast, long long ld, double floor_, double vmin, double vmax,
                                    int median, int flip, int pf, int pt, const unsigned char* lut,
                                    unsigned char* rgba, hipStream_t st) {
  if (!sxx || !lut || !rgba || n_freq < 1 || n_time < 1 || pf < 1 || pt < 1 ||
      ld < (freq_fast ? n_freq : n_time))
    return hipErrorInvalidValue;
  return dispatch_real(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return freq_fast ? image_t<T, true>(sxx, n_freq, n_time, ld, floor_, vmin, vmax, median, flip, pf, pt, lut, rgba, st)
                     : image_t<T, false>(sxx, n_freq, n_time, ld, floor_, vmin, vmax, median, flip, pf, pt, lut, rgba, st);
  });
}

}  // namespace vsig
