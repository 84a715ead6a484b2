// Line traces (gfx950): the min / max envelope of |a| per pixel column, for
// the line plots beside every spectrogram (np.abs(signal) over time; the
// magnitude or 20 log10 of a whole-capture spectrum over frequency).
// vsig_trace_envelope_dev; the definition is in include/vsig.h.
//
// m[i] = |a[i]| in the array's precision (np_cabs / fabs), position p reads
// s[p] = m[(p + rot) % n], column c covers `bin` positions from lo + c * bin.
// A window of positions is at most two contiguous runs of the array (it wraps
// once), and every run is read in 16-byte units aligned in memory: whole units
// by one 16-byte load, kTraceLoads of them in flight per lane, the elements
// outside the run ignored; the units that stick out of the array (its first
// and last, when the base is not 16-byte aligned) and arrays off their
// element's alignment element by element.
//
//   trace_cols    bin <= kTraceTile: a block owns floor(tile / bin) whole
//                 columns.  It puts their magnitudes in LDS, then groups of G
//                 lanes (G: the power of two >= bin, at most 64) reduce one
//                 column each by xor shuffles; then a lane per column maps
//                 and stores the envelope (a logarithm in one lane of a
//                 group cost a wave's time: 3.05 ms for 2^28 samples at
//                 bin 64 before this split).
//   trace_chunks  bin > kTraceTile: a column is cut into chunks of whole
//                 tiles, one block per chunk, one record per chunk;
//   trace_merge   a wave per column merges its chunks' records in a fixed
//                 order and stores the mapped envelope and the column's record.
//   trace_info    one block reduces the records (trace_cols' per block,
//                 trace_merge's per column) to the info record.
//
// Everything reduced is a {value, position} pair under "larger (smaller)
// value, then lower position", which is associative and commutative, so the
// first extremum does not depend on the order of the reduction; nothing
// crosses blocks through atomics and the grids are functions of the arguments
// alone: the same input gives the same bytes on every run.  A NaN makes the
// envelope of its column NaN (a sticky flag beside the pairs); it never wins a
// pair, so info over an array with NaN holds the extrema of the rest.
#include <climits>

#include "block_ops.hpp"
#include "dbmath.hpp"

namespace vsig {

namespace {

constexpr int TT = 256;                      // threads per block
constexpr int TW = TT / 64;
constexpr int kTraceLoads = 4;               // 16-byte loads in flight per lane
constexpr long long kTraceChunks = 8192;     // trace_chunks: blocks aimed at

#pragma clang fp contract(off)

__device__ __forceinline__ void clear(double2& v) { v.x = 0.0; v.y = 0.0; }
__device__ __forceinline__ void clear(float2& v) { v.x = 0.f; v.y = 0.f; }
__device__ __forceinline__ void clear(double& v) { v = 0.0; }
__device__ __forceinline__ void clear(float& v) { v = 0.f; }

template <class R> __device__ __forceinline__ R mapped(R e, int kind, double eps) {
  return kind == kTraceDb20 ? db20_of(e, (R)eps) : e;
}

// First maximum and first minimum of what a lane (wave, block, column) has
// seen; the identity loses to every magnitude.
template <class R>
struct Ext {
  R mx, mn;
  long long pmx, pmn;
  int nan;
  __device__ __forceinline__ void init() {
    mx = (R)-1; mn = (R)__builtin_inf(); pmx = LLONG_MAX; pmn = LLONG_MAX; nan = 0;
  }
  __device__ __forceinline__ void take_max(R v, long long p) { betterd(mx, pmx, v, p); }
  __device__ __forceinline__ void take_min(R v, long long p) {
    if (v < mn || (v == mn && p < pmn)) { mn = v; pmn = p; }
  }
  __device__ __forceinline__ void element(R v, long long p) {
    take_max(v, p);
    take_min(v, p);
    nan |= v != v;
  }
  __device__ __forceinline__ void merge(const Ext& o) {
    take_max(o.mx, o.pmx);
    take_min(o.mn, o.pmn);
    nan |= o.nan;
  }
  __device__ __forceinline__ void merge(const TraceRec& r) {
    take_max((R)r.mx, r.pmx);                // records hold widened values of R: exact
    take_min((R)r.mn, r.pmn);
    nan |= (int)r.nan;
  }
  __device__ __forceinline__ Ext shfl_xor(int off) const {
    return {__shfl_xor(mx, off), __shfl_xor(mn, off), __shfl_xor(pmx, off), __shfl_xor(pmn, off),
            __shfl_xor(nan, off)};
  }
  __device__ __forceinline__ TraceRec rec() const {
    TraceRec r;
    r.mn = (double)mn; r.mx = (double)mx; r.pmn = pmn; r.pmx = pmx; r.nan = nan;
    return r;
  }
};

// The block's lanes -> one record, by thread 0.
template <class R>
__device__ __forceinline__ void block_record(Ext<R> e, TraceRec* out) {
  __shared__ Ext<R> slots[TW];
  block_fold<TW>(e, slots);
  if (threadIdx.x == 0) *out = e.rec();
}

struct TraceArgs {
  const void* a;
  long long n, rot, lo, hi, bin, cols;
  long long cpb;               // trace_cols: columns per block
  int group;                   // trace_cols: lanes per column
  long long cpc, chunk;        // trace_chunks: chunks per column, positions per chunk
  int off;                     // elements between the 16-byte boundary below a and a
  int vec;                     // a is on its element's alignment: 16-byte loads
  int kind;
  double eps;
  void *env_min, *env_max;
  TraceRec* recs;              // trace_cols: per block (null: no info); trace_chunks: per chunk
};

// f(k, |a[ia + k]|) for k in [0, len): one contiguous run of the array.
template <class T, class F>
__device__ __forceinline__ void scan_run(const TraceArgs& A, long long ia, long long len, F&& f) {
  constexpr int EPV = 16 / sizeof(T);
  if (len <= 0) return;
  const T* a = static_cast<const T*>(A.a);
  // unit u holds the elements u * EPV - off .. + EPV - 1
  const Pack16<T>* pv = reinterpret_cast<const Pack16<T>*>(reinterpret_cast<const char*>(a) -
                                                            (size_t)A.off * sizeof(T));
  const long long ua = (ia + A.off) / EPV, ub = (ia + len - 1 + A.off) / EPV;
  for (long long u0 = ua + threadIdx.x; u0 <= ub; u0 += (long long)kTraceLoads * TT) {
    Pack16<T> pk[kTraceLoads];
#pragma unroll
    for (int j = 0; j < kTraceLoads; ++j) {
      const long long u = u0 + (long long)j * TT, i0 = u * EPV - A.off;
      if (u > ub) continue;
      if (A.vec && i0 >= 0 && i0 + EPV <= A.n) {
        pk[j] = pv[u];
      } else {
#pragma unroll
        for (int q = 0; q < EPV; ++q) {
          const long long i = i0 + q;
          if (i >= 0 && i < A.n) pk[j].e[q] = a[i]; else clear(pk[j].e[q]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kTraceLoads; ++j) {
      const long long u = u0 + (long long)j * TT, i0 = u * EPV - A.off;
      if (u > ub) continue;
#pragma unroll
      for (int q = 0; q < EPV; ++q) {
        const long long k = i0 + q - ia;
        if (k >= 0 && k < len) f(k, mag(pk[j].e[q]));
      }
    }
  }
}

// f(k, s[pa + k]) for k in [0, len): positions [pa, pa + len) of the (shifted)
// line, len <= n -- the run up to the end of the array, then the run from its
// start.
template <class T, class F>
__device__ __forceinline__ void scan_positions(const TraceArgs& A, long long pa, long long len, F&& f) {
  long long ia = pa + A.rot;
  if (ia >= A.n) ia -= A.n;
  const long long l1 = len < A.n - ia ? len : A.n - ia;
  scan_run<T>(A, ia, l1, f);
  scan_run<T>(A, 0, len - l1, [&](long long k, typename Real<T>::type v) { f(l1 + k, v); });
}

template <class T>
__global__ __launch_bounds__(TT) void trace_cols(TraceArgs A) {
  using R = typename Real<T>::type;
  __shared__ R sm[kTraceTile];
  const long long c0 = (long long)blockIdx.x * A.cpb;          // the block's first column
  const long long pa = A.lo + c0 * A.bin;
  const long long left = A.hi - pa, span = A.cpb * A.bin;      // span <= kTraceTile
  const int len = (int)(left < span ? left : span);
  Ext<R> e;
  e.init();
  scan_positions<T>(A, pa, len, [&](long long k, R v) {
    sm[k] = v;
    e.element(v, pa + k);
  });
  __syncthreads();
  const int G = A.group, gl = threadIdx.x & (G - 1), g = threadIdx.x / G;
  const int bin = (int)A.bin, ncol = (len + bin - 1) / bin;
  R* emin = static_cast<R*>(A.env_min);
  R* emax = static_cast<R*>(A.env_max);
  for (int cb = 0; cb < ncol; cb += TT / G) {                  // the same trips for every lane
    const int c = cb + g;
    R mx = (R)-1, mn = (R)__builtin_inf();
    if (c < ncol) {
      const int qa = c * bin, qe = qa + bin < len ? qa + bin : len;
      for (int k = qa + gl; k < qe; k += G) {
        const R v = sm[k];
        mx = np_max(mx, v);
        mn = np_min(mn, v);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      if (off < G) {                                           // partners stay inside the group
        mx = np_max(mx, __shfl_xor(mx, off));
        mn = np_min(mn, __shfl_xor(mn, off));
      }
    }
    // the column's results go where its first two magnitudes were (its group
    // has read them all); bin == 1: the magnitude is both
    if (c < ncol && gl == 0 && bin > 1) {
      sm[c * bin] = mx;
      sm[c * bin + 1] = mn;
    }
  }
  __syncthreads();
  // the map and the stores, a column per lane: every lane pays a logarithm
  // and a wave's stores are contiguous
  for (int c = threadIdx.x; c < ncol; c += TT) {
    emax[c0 + c] = mapped(sm[c * bin], A.kind, A.eps);
    if (emin) emin[c0 + c] = mapped(sm[c * bin + (bin > 1)], A.kind, A.eps);
  }
  if (A.recs) block_record(e, A.recs + blockIdx.x);
}

template <class T>
__global__ __launch_bounds__(TT) void trace_chunks(TraceArgs A) {
  using R = typename Real<T>::type;
  const long long c = blockIdx.x / A.cpc, j = blockIdx.x % A.cpc;
  // the chunk's positions inside its column, the column's inside the window
  const long long ka = j * A.chunk, kb = ka + A.chunk < A.bin ? ka + A.chunk : A.bin;
  const long long pa = A.lo + c * A.bin + ka;
  long long pb = A.lo + c * A.bin + kb;
  if (pb > A.hi) pb = A.hi;
  Ext<R> e;
  e.init();
  if (ka < kb && pa < pb) scan_positions<T>(A, pa, pb - pa, [&](long long k, R v) { e.element(v, pa + k); });
  block_record(e, A.recs + blockIdx.x);
}

// A wave per column: the column's chunk records -> the envelope and the
// column's record (behind the chunk records).
template <class R>
__global__ __launch_bounds__(TT) void trace_merge(TraceArgs A) {
  const long long c = (long long)blockIdx.x * TW + (threadIdx.x >> 6);
  if (c >= A.cols) return;                                     // whole waves leave
  const int lane = threadIdx.x & 63;
  Ext<R> e;
  e.init();
  for (long long j = lane; j < A.cpc; j += 64) e.merge(A.recs[c * A.cpc + j]);
  wave_fold(e);
  if (lane == 0) {
    R* emin = static_cast<R*>(A.env_min);
    R* emax = static_cast<R*>(A.env_max);
    const R nan = (R)__builtin_nan("");
    emax[c] = mapped(e.nan ? nan : e.mx, A.kind, A.eps);
    if (emin) emin[c] = mapped(e.nan ? nan : e.mn, A.kind, A.eps);
    A.recs[A.cols * A.cpc + c] = e.rec();
  }
}

template <class R>
__global__ __launch_bounds__(TT) void trace_info(const TraceRec* __restrict__ recs, long long nrec, int kind,
                                                 double eps, TraceInfo* __restrict__ info) {
  Ext<R> e;
  e.init();
  for (long long i = threadIdx.x; i < nrec; i += TT) e.merge(recs[i]);
  __shared__ TraceRec tot;
  block_record(e, &tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    TraceInfo r;
    r.argmin = tot.pmn; r.argmax = tot.pmx;
    r.min = (double)mapped((R)tot.mn, kind, eps);
    r.max = (double)mapped((R)tot.mx, kind, eps);
    *info = r;
  }
}

struct TracePlan {
  long long cols, cpb, cpc, chunk, grid, nrec;   // nrec: records the scratch holds
  int group;
  bool by_cols;
};

TracePlan plan_of(long long lo, long long hi, long long bin) {
  TracePlan p{};
  const long long W = hi - lo;
  p.cols = (W + bin - 1) / bin;
  p.by_cols = bin <= kTraceTile;
  if (p.by_cols) {
    p.cpb = kTraceTile / bin;
    p.group = 1;
    while (p.group < bin && p.group < 64) p.group <<= 1;
    p.grid = (p.cols + p.cpb - 1) / p.cpb;
    p.nrec = p.grid;
  } else {
    const long long tiles = (bin + kTraceTile - 1) / kTraceTile;      // per column
    long long want = (kTraceChunks + p.cols - 1) / p.cols;
    p.cpc = want < tiles ? want : tiles;
    p.chunk = ((tiles + p.cpc - 1) / p.cpc) * kTraceTile;             // whole tiles
    p.cpc = (bin + p.chunk - 1) / p.chunk;                            // no empty chunk
    p.grid = p.cols * p.cpc;
    p.nrec = p.grid + p.cols;
  }
  return p;
}

template <class T>
hipError_t trace_t(TraceArgs A, const TracePlan& p, TraceInfo* info, TraceRec* recs, hipStream_t st) {
  using R = typename Real<T>::type;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(A.a);
  A.vec = addr % sizeof(T) == 0;
  A.off = A.vec ? (int)((addr & 15) / sizeof(T)) : 0;
  A.cols = p.cols; A.cpb = p.cpb; A.group = p.group; A.cpc = p.cpc; A.chunk = p.chunk;
  const TraceRec* src;
  long long nsrc;
  if (p.by_cols) {
    A.recs = info ? recs : nullptr;
    hipLaunchKernelGGL(trace_cols<T>, dim3((unsigned)p.grid), dim3(TT), 0, st, A);
    src = recs; nsrc = p.grid;
  } else {
    A.recs = recs;
    hipLaunchKernelGGL(trace_chunks<T>, dim3((unsigned)p.grid), dim3(TT), 0, st, A);
    hipLaunchKernelGGL(trace_merge<R>, dim3((unsigned)((p.cols + TW - 1) / TW)), dim3(TT), 0, st, A);
    src = recs + p.grid; nsrc = p.cols;
  }
  if (info) hipLaunchKernelGGL(trace_info<R>, dim3(1), dim3(TT), 0, st, src, nsrc, A.kind, A.eps, info);
  return hipGetLastError();
}

}  // namespace

size_t trace_scratch_bytes(long long lo, long long hi, long long bin) {
  return (size_t)plan_of(lo, hi, bin).nrec * sizeof(TraceRec);
}

hipError_t launch_trace_envelope(int dtype, const void* a, long long n, int shift, long long lo, long long hi,
                                 long long bin, int kind, double eps, void* env_min, void* env_max,
                                 TraceInfo* info, void* scratch, hipStream_t st) {
  if (n < 1 || lo < 0 || hi > n || lo >= hi || bin < 1 || !a || !env_max || !scratch)
    return hipErrorInvalidValue;
  const TracePlan p = plan_of(lo, hi, bin);
  if (p.grid > 0x7fffffffLL) return hipErrorInvalidValue;
  TraceArgs A{};
  A.a = a; A.n = n; A.rot = shift ? (n + 1) / 2 : 0; A.lo = lo; A.hi = hi; A.bin = bin;
  A.kind = kind; A.eps = eps; A.env_min = env_min; A.env_max = env_max;
  TraceRec* recs = static_cast<TraceRec*>(scratch);
  return dispatch_dtype(dtype, [&](auto tag) {
    return trace_t<typename decltype(tag)::type>(A, p, info, recs, st);
  });
}

}  // namespace vsig
