// Run list (gfx950): every burst of an array.  With m[i] = |a[i]| and
// mask[i] = m[i] >= thr, a run is a maximal interval [start, end] whose ends
// are masked and that holds no stretch of more than max_gap unmasked elements
// (vsig_runs_dev; packets in a smoothed energy trace).  Per index: a masked i
// is a start iff the previous masked index p has i - p > max_gap + 1, an end
// iff the next masked index q has q - i > max_gap + 1; the k-th start pairs
// with the k-th end.
//
//   runs_tile    one pass over the array, 16-byte loads: {max, first index,
//                min, sum} of every tile of kRunsTile elements into a table,
//                {max, first index} of each block's tiles into a partial; the
//                partials' fixed-order reduce (launch_partial_finalize) gives
//                max / argmax for the relative threshold and the info record.
//                With an absolute threshold the pass also stores the mask,
//                one 64-bit word per 64 elements (ballots of the loaded
//                packs, bit-interleaved into element order): the array is
//                then read exactly once.
//   runs_mask    a block per group of RG tiles.  A tile with max < thr has no
//                masked element and one with min >= thr nothing else: both
//                cost one table read.  With a relative threshold, known only
//                now, the mixed tiles alone are read again and their mask
//                words stored.  Per group: first / last masked index, the
//                masked count, and {max, first index, sum} of its tiles.
//   runs_scan_edges  one block: the exclusive prefix maximum of the groups'
//                last and suffix minimum of their first masked index, i.e.
//                p at every group's left edge and q at its right edge.
//   runs_words   a thread per mask word of a group (count pass, then emit
//                pass).  A block-wide prefix maximum / suffix minimum of the
//                words' last / first set bit, seeded with the group's p / q,
//                gives every word its p and q; inside a word the rule is bit
//                arithmetic on the bits that open or close a stretch of ones.
//                max_gap is one compare: no walk, nothing proportional to it.
//   runs_scan_counts  one block: exclusive scan of the groups' start and end
//                counts, the masked total and the info record.
//   runs_stats   a fixed grid striding over the records k < min(count, cap)
//                (count read on the device): max, first argmax and sum of m
//                over [start, end], the run's two end tiles from the array,
//                its whole tiles from the table and whole groups of them
//                from the group records, in a fixed order.
//
// NaN: a NaN magnitude compares false, so it is never masked and never a
// tile's maximum or minimum (a tile holding one may still be classed as all
// masked: such arrays are outside the contract, the writes stay in bounds).
#include <climits>

#include "block_ops.hpp"

namespace vsig {

namespace {

constexpr int RT = 256;                      // threads per block of the passes over the array
constexpr int RE = kRunsTile / RT;           // elements per thread and tile
constexpr int RW = RT / 64;
constexpr int RG = 32;                       // tiles per group
constexpr int RWORDS = kRunsTile / 64;       // mask words per tile
constexpr int RB = RG * RWORDS;              // threads of runs_words: one per mask word
constexpr int RBW = RB / 64;
static_assert(RB == 1024 && RWORDS == 32, "runs_words maps thread >> 5 to the tile, & 31 to the word");
// a mask word has at most 32 starts and 32 ends, a block at most 32 RB of either:
// runs_words scans both counts as the halves of one 64-bit word
static_assert(32LL * RB < (1LL << 31), "a block's start and end counts each fit a 32-bit half");
constexpr long long kNone = 1LL << 60;       // no masked index: p = -kNone, q = +kNone

struct RunTile { double max; long long idx; double min, sum; };
struct RunGroup { double max; long long idx; double sum; };   // a group's tiles together
using StatFold = FirstMaxSums<1>;   // {max, first index, sum} on its way into a group or run record

// 0: nothing masked, 1: everything masked, 2: mixed
__device__ __forceinline__ int tile_class(double mx, double mn, double thr) {
  return mx >= thr ? (mn >= thr ? 1 : 2) : 0;
}
__device__ __forceinline__ long long lmax(long long a, long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long lmin(long long a, long long b) { return a < b ? a : b; }

// Bit i of x (i < 64 / K) to bit K i: K ballots, one per element of a 16-byte
// pack, interleave into mask words of consecutive elements.
template <int K> __device__ __forceinline__ unsigned long long spread(unsigned long long x);
template <> __device__ __forceinline__ unsigned long long spread<1>(unsigned long long x) { return x; }
template <> __device__ __forceinline__ unsigned long long spread<2>(unsigned long long x) {
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  return (x | (x << 1)) & 0x5555555555555555ull;
}
template <> __device__ __forceinline__ unsigned long long spread<4>(unsigned long long x) {
  x = (x | (x << 24)) & 0x000000FF000000FFull;
  x = (x | (x << 12)) & 0x000F000F000F000Full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  return (x | (x << 3)) & 0x1111111111111111ull;
}

// VEC: a is 16-byte aligned (whole tiles by 16-byte loads; the last, partial
// tile and unaligned arrays element by element).  BITS: the threshold is known
// (absolute), so the pass leaves every tile's mask words too and no tile is
// read a second time.
template <class T, bool VEC, bool BITS>
__global__ __launch_bounds__(RT) void runs_tile(const T* __restrict__ a, long long n, long long ntiles,
                                                RunTile* __restrict__ tab, PeakPartial* __restrict__ bpart,
                                                double thr, unsigned long long* __restrict__ bits) {
  constexpr int EPV = 16 / sizeof(T), NV = kRunsTile / (RT * EPV);
  constexpr int LPW = 64 / EPV;                // lanes whose packs fill one mask word
  __shared__ double smx[2][RW], smn[2][RW], ssum[2][RW];
  __shared__ long long si[2][RW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int par = 0;
  double bm = -2.0;                          // thread 0: the block's tiles so far
  long long bi = LLONG_MAX;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1) {
    const long long base = tile * kRunsTile;
    double m = -1.0, mn = HUGE_VAL, s = 0.0;
    long long mi = LLONG_MAX;
    if (VEC && base + kRunsTile <= n) {
      const Pack16<T>* pv = reinterpret_cast<const Pack16<T>*>(a + base);
      Pack16<T> pk[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) pk[j] = pv[j * RT + threadIdx.x];
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        unsigned long long bal[EPV];           // the same in every lane
#pragma unroll
        for (int q = 0; q < EPV; ++q) {
          const double v = (double)mag(pk[j].e[q]);
          betterd(m, mi, v, base + (long long)(j * RT + threadIdx.x) * EPV + q);
          if (v < mn) mn = v;
          s += v;
          if (BITS) bal[q] = __ballot(v >= thr);
        }
        if (BITS) {
          // this wave's packs j: elements 64 EPV (j RW + w) .. of the tile, lane
          // l's at EPV l + q.  The words are formed from values that are the same
          // in every lane (scalar work); lane k stores word k.
          unsigned long long mine = 0;
#pragma unroll
          for (int k = 0; k < EPV; ++k) {
            unsigned long long word = 0;
#pragma unroll
            for (int q = 0; q < EPV; ++q) {
              unsigned long long part = bal[q];
              if constexpr (EPV > 1) part = (part >> (k * LPW)) & ((1ull << LPW) - 1ull);
              word |= spread<EPV>(part) << q;
            }
            if (lane == k) mine = word;
          }
          if (lane < EPV) bits[tile * RWORDS + (j * RW + w) * EPV + lane] = mine;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < RE; ++e) {
        const long long g = base + e * RT + threadIdx.x;
        bool c = false;
        if (g < n) {
          const double v = (double)mag(a[g]);
          betterd(m, mi, v, g);
          if (v < mn) mn = v;
          s += v;
          c = v >= thr;
        }
        if (BITS) {
          const unsigned long long bal = __ballot(c);
          if (lane == 0) bits[tile * RWORDS + e * RW + w] = bal;
        }
      }
    }
    // block_fold's order written out: as a value type of block_ops.hpp the four
    // fields cost the unaligned instantiations a VGPR (profiles/block_ops_ab.md)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double om = __shfl_xor(m, off);
      const long long oi = __shfl_xor(mi, off);
      const double on = __shfl_xor(mn, off);
      betterd(m, mi, om, oi);
      if (on < mn) mn = on;
      s += __shfl_xor(s, off);                 // both lanes of a pair form the same sum
    }
    // the LDS slots alternate between tiles: one barrier a tile is enough
    if (lane == 0) { smx[par][w] = m; si[par][w] = mi; smn[par][w] = mn; ssum[par][w] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < RW; ++q) {
        betterd(m, mi, smx[par][q], si[par][q]);
        if (smn[par][q] < mn) mn = smn[par][q];
        s += ssum[par][q];
      }
      if (mi == LLONG_MAX) mi = base;          // nothing but NaN
      RunTile r;
      r.max = m; r.idx = mi; r.min = mn; r.sum = s;
      tab[tile] = r;
      betterd(bm, bi, m, mi);
    }
  }
  if (threadIdx.x == 0) {                      // every block has at least one tile
    PeakPartial r;
    r.max2 = bm; r.idx = bi; r.sum_abs = 0.0; r.sum_abs2 = 0.0;
    bpart[blockIdx.x] = r;
  }
}

struct RunsArgs {
  const void* a;
  long long n, gap1, ntiles, ngroups, cap;   // gap1 = max_gap + 1
  double thr;
  int relative;
  const RunTile* tab;             // per tile
  RunGroup* gtab;                 // per group
  const PeakPartial* rec;         // max / argmax of the array
  unsigned long long* bits;       // RWORDS mask words per tile (the mixed tiles' alone are used)
  long long *gfirst, *glast, *gcov;   // per group: first / last masked index, masked count
  long long *gp, *gq;             // per group: p at its left edge, q at its right edge
  long long *gcs, *gce;           // per group: starts / ends, then (scanned) their offsets
  RunRec* out;
  RunsInfo* info;
};

__device__ __forceinline__ double thr_of(const RunsArgs& A) {
  return A.relative ? __dmul_rn(A.thr, A.rec->max2) : A.thr;
}

// Mask word `word` of tile t of class cls: nothing, everything up to n, or
// the stored ballots.
__device__ __forceinline__ unsigned long long word_of(const RunsArgs& A, long long t, int word, int cls) {
  if (cls == 2) return A.bits[t * RWORDS + word];
  if (cls == 0) return 0ull;
  const long long v = A.n - (t * kRunsTile + 64 * word);
  return v >= 64 ? ~0ull : (v > 0 ? (1ull << v) - 1ull : 0ull);
}

// BITS: the tile pass left the mask words (absolute threshold); otherwise the
// mixed tiles are read again here.
template <class T, bool BITS>
__global__ __launch_bounds__(RT) void runs_mask(RunsArgs A) {
  __shared__ Span slots[RW];
  __shared__ int scls[RG];
  const T* a = static_cast<const T*>(A.a);
  const double thr = thr_of(A);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long t0 = (long long)blockIdx.x * RG;
  if (threadIdx.x < RG) {
    // the group's tiles side by side: their classes, and {max, first index,
    // sum} of the whole group for the statistics of long runs
    const long long t = t0 + threadIdx.x;
    StatFold v{{-2.0, LLONG_MAX}, {{0.0}}};
    int cls = 0;
    if (t < A.ntiles) {
      const RunTile e = A.tab[t];
      v.m = e.max; v.i = e.idx; v.s[0] = e.sum;
      cls = tile_class(e.max, e.min, thr);
    }
    scls[threadIdx.x] = cls;
    wave_fold<RG>(v);                            // lanes 0 .. RG-1 among themselves
    if (threadIdx.x == 0) {
      RunGroup r;
      r.max = v.m; r.idx = v.i; r.sum = v.s[0];
      A.gtab[blockIdx.x] = r;
    }
  }
  __syncthreads();
  Span sp{kNone, -kNone, 0};                   // this thread's mask words so far
  auto take = [&](unsigned long long B, long long b0) {
    if (B) {
      sp.first = lmin(sp.first, b0 + __builtin_ctzll(B));
      sp.last = lmax(sp.last, b0 + 63 - __builtin_clzll(B));
      sp.count += __popcll(B);
    }
  };
  if (!BITS) {
    for (int q = 0; q < RG; ++q) {
      if (scls[q] != 2) continue;              // the same for the whole block
      const long long t = t0 + q, ts = t * kRunsTile;
#pragma unroll
      for (int e = 0; e < RE; ++e) {
        const long long g = ts + e * RT + threadIdx.x;
        const bool in = g < A.n && (double)mag(a[g]) >= thr;
        const unsigned long long bal = __ballot(in);
        if (lane == 0) A.bits[t * RWORDS + e * RW + w] = bal;   // elements ts + 64 (e RW + w) ..
      }
    }
    __syncthreads();                           // the words are read back below
  }
  for (int i = threadIdx.x; i < RG * RWORDS; i += RT) {
    const long long t = t0 + i / RWORDS;
    const int word = i % RWORDS;
    if (t < A.ntiles) take(word_of(A, t, word, scls[i / RWORDS]), t * kRunsTile + 64 * word);
  }
  block_fold<RW>(sp, slots);
  if (threadIdx.x == 0) {
    A.gfirst[blockIdx.x] = sp.first; A.glast[blockIdx.x] = sp.last; A.gcov[blockIdx.x] = sp.count;
  }
}

// One block: gp[g] = max of glast over the groups before g (-kNone: none),
// gq[g] = min of gfirst over the groups after g (kNone: none).  A contiguous
// chunk of groups per thread, then a block scan of the chunks.
__global__ __launch_bounds__(1024) void runs_scan_edges(const long long* __restrict__ gfirst,
                                                        const long long* __restrict__ glast, long long ng,
                                                        long long* __restrict__ gp, long long* __restrict__ gq) {
  __shared__ long long wl[16], wf[16];
  const long long chunk = (ng + 1023) / 1024;
  const long long lo = lmin(threadIdx.x * chunk, ng);
  const long long hi = lmin(lo + chunk, ng);
  long long x = -kNone, y = kNone;
  for (long long i = lo; i < hi; ++i) { x = lmax(x, glast[i]); y = lmin(y, gfirst[i]); }
  long long p, q;
  block_scan_edges<16>(x, y, kNone, wl, wf, p, q);
  for (long long i = lo; i < hi; ++i) { gp[i] = p; p = lmax(p, glast[i]); }
  for (long long i = hi - 1; i >= lo; --i) { gq[i] = q; q = lmin(q, gfirst[i]); }
}

// The starts (S) or ends of mask word B (elements b0 ..) under the rule; p /
// q: the masked index before / after the word.  f(index) for each, ascending.
template <class F>
__device__ __forceinline__ void word_starts(unsigned long long B, long long b0, long long p, long long gap1, F&& f) {
  unsigned long long S = B & ~(B << 1);        // a start's left neighbour is unmasked
  while (S) {
    const int i = __builtin_ctzll(S);
    S &= S - 1;
    const unsigned long long below = B & ((1ull << i) - 1ull);
    const long long pi = below ? b0 + 63 - __builtin_clzll(below) : p;
    if (b0 + i - pi > gap1) f(b0 + i);
  }
}
template <class F>
__device__ __forceinline__ void word_ends(unsigned long long B, long long b0, long long q, long long gap1, F&& f) {
  unsigned long long E = B & ~(B >> 1);        // an end's right neighbour is unmasked
  while (E) {
    const int i = __builtin_ctzll(E);
    E &= E - 1;
    const unsigned long long above = i == 63 ? 0ull : B >> (i + 1);
    const long long qi = above ? b0 + i + 1 + __builtin_ctzll(above) : q;
    if (qi - (b0 + i) > gap1) f(b0 + i);
  }
}

template <bool EMIT>
__global__ __launch_bounds__(RB) void runs_words(RunsArgs A) {
  __shared__ long long wl[RBW], wf[RBW], wc[RBW];
  __shared__ unsigned short live[RB];
  __shared__ int nlive;
  const int word = threadIdx.x & 31;
  const double thr = thr_of(A);
  // The block owns a contiguous chunk of groups, at most RB of them (the
  // launch sizes the grid so).  A thread per group first sorts out those with
  // no start and no end -- nothing masked, or everything masked with a masked
  // neighbour on either side -- and, emitting, those whose records lie past
  // cap: a sparse mask then costs one read per group.
  const long long chunk = (A.ngroups + gridDim.x - 1) / gridDim.x;
  const long long glo = blockIdx.x * chunk, ghi = lmin(glo + chunk, A.ngroups);
  if (threadIdx.x == 0) nlive = 0;
  __syncthreads();
  if (glo + threadIdx.x < ghi) {
    const long long g = glo + threadIdx.x;
    const long long g0 = g * RG * kRunsTile;
    const long long glen = lmin(A.n - g0, (long long)RG * kRunsTile);
    const long long cov = A.gcov[g];
    if (cov == 0 || (cov == glen && A.gp[g] == g0 - 1 && A.gq[g] == g0 + glen)) {
      if (!EMIT) { A.gcs[g] = 0; A.gce[g] = 0; }
    } else if (!EMIT || A.gcs[g] < A.cap || A.gce[g] < A.cap) {
      live[atomicAdd(&nlive, 1)] = (unsigned short)threadIdx.x;
    }
  }
  __syncthreads();
  const int nl = nlive;
  for (int j = 0; j < nl; ++j) {
    const long long g = glo + live[j];
    const long long t = g * RG + (threadIdx.x >> 5);
    const long long b0 = t * kRunsTile + 64 * word;
    unsigned long long B = 0;
    if (t < A.ntiles) B = word_of(A, t, word, tile_class(A.tab[t].max, A.tab[t].min, thr));
    // p: the last set bit of the words before this one; q: the first of those after it
    long long p, q;
    block_scan_edges<RBW>(B ? b0 + 63 - __builtin_clzll(B) : -kNone, B ? b0 + __builtin_ctzll(B) : kNone, kNone,
                          wl, wf, p, q);
    p = lmax(p, A.gp[g]);
    q = lmin(q, A.gq[g]);
    int cs = 0, ce = 0;
    if (A.gap1 == 1) {
      // max_gap = 0: every stretch of ones opens and closes a run, but for
      // one that goes on in the neighbouring word
      const unsigned long long S = B & ~(B << 1), E = B & ~(B >> 1);
      cs = __popcll(S) - (int)((S & 1ull) != 0 && b0 - p <= 1);
      ce = __popcll(E) - (int)((E >> 63) != 0 && q - (b0 + 63) <= 1);
    } else {
      word_starts(B, b0, p, A.gap1, [&](long long) { ++cs; });
      word_ends(B, b0, q, A.gap1, [&](long long) { ++ce; });
    }
    // the counts of the threads before this one, both in one scan: starts in
    // the low half, ends in the high (a word has at most 32 of either, a block
    // 2^15: neither half carries)
    long long tot;
    const long long before = block_scan<RBW>((long long)cs | ((long long)ce << 32), wc, tot);
    if (!EMIT) {
      if (threadIdx.x == 0) { A.gcs[g] = tot & 0xffffffffll; A.gce[g] = tot >> 32; }
    } else {
      long long ks = A.gcs[g] + (before & 0xffffffffll), ke = A.gce[g] + (before >> 32);
      word_starts(B, b0, p, A.gap1, [&](long long i) { if (ks < A.cap) A.out[ks].start = i; ++ks; });
      word_ends(B, b0, q, A.gap1, [&](long long i) { if (ke < A.cap) A.out[ke].end = i; ++ke; });
    }
    __syncthreads();                             // the LDS slots are reused by the block's next group
  }
}

// One block: exclusive scan in place of the ng per-group start and end
// counts, the masked total and the info record.
__global__ __launch_bounds__(1024) void runs_scan_counts(long long* __restrict__ gcs, long long* __restrict__ gce,
                                                         const long long* __restrict__ gcov, long long ng,
                                                         const PeakPartial* __restrict__ rec, double thr,
                                                         int relative, RunsInfo* __restrict__ info) {
  __shared__ long long w0[16], w1[16], w2[16];
  const long long chunk = (ng + 1023) / 1024;
  const long long lo = lmin(threadIdx.x * chunk, ng);
  const long long hi = lmin(lo + chunk, ng);
  long long s = 0, e = 0, c = 0;
  for (long long i = lo; i < hi; ++i) { s += gcs[i]; e += gce[i]; c += gcov[i]; }
  long long ts, te, tc;
  long long rs = block_scan<16>(s, w0, ts);
  long long re = block_scan<16>(e, w1, te);
  (void)block_scan<16>(c, w2, tc);
  for (long long i = lo; i < hi; ++i) {
    const long long vs = gcs[i], ve = gce[i];
    gcs[i] = rs; gce[i] = re;
    rs += vs; re += ve;
  }
  if (threadIdx.x == 0) {
    RunsInfo r;
    r.count = ts;
    r.covered = tc;
    r.argmax = rec->idx;
    r.max = rec->max2;
    r.thr_used = relative ? __dmul_rn(thr, rec->max2) : thr;
    *info = r;
  }
}

constexpr int kStatsGrid = 2048;

template <class T>
__global__ __launch_bounds__(RT) void runs_stats(RunsArgs A) {
  __shared__ StatFold slots[2][RW];          // alternate between records: one barrier a record is enough
  const T* a = static_cast<const T*>(A.a);
  const long long cnt = A.info->count;
  const long long kmax = cnt < A.cap ? cnt : A.cap;
  int par = 0;
  for (long long k = blockIdx.x; k < kmax; k += gridDim.x, par ^= 1) {
    const long long s = A.out[k].start, e = A.out[k].end;
    if (s < 0 || e >= A.n || s > e) continue;  // cannot happen without NaN; the same for the whole block
    const long long ts = s / kRunsTile, te = e / kRunsTile;
    double m = -1.0, sum = 0.0;
    long long mi = LLONG_MAX;
    const long long le = ts == te ? e : (ts + 1) * kRunsTile - 1;
    for (long long g = s + threadIdx.x; g <= le; g += RT) {
      const double v = (double)mag(a[g]);
      betterd(m, mi, v, g);
      sum += v;
    }
    if (te > ts) {
      // the whole tiles ts + 1 .. te - 1: whole groups of them from the group
      // table, the others from the tile table
      auto tiles = [&](long long lo, long long hi) {
        for (long long t = lo + threadIdx.x; t < hi; t += RT) {
          const RunTile r = A.tab[t];
          betterd(m, mi, r.max, r.idx);
          sum += r.sum;
        }
      };
      const long long ga = (ts + 1 + RG - 1) / RG, gb = te / RG;
      if (ga >= gb) {
        tiles(ts + 1, te);
      } else {
        tiles(ts + 1, ga * RG);
        for (long long gi = ga + threadIdx.x; gi < gb; gi += RT) {
          const RunGroup r = A.gtab[gi];
          betterd(m, mi, r.max, r.idx);
          sum += r.sum;
        }
        tiles(gb * RG, te);
      }
      for (long long g = te * kRunsTile + threadIdx.x; g <= e; g += RT) {
        const double v = (double)mag(a[g]);
        betterd(m, mi, v, g);
        sum += v;
      }
    }
    StatFold v{{m, mi}, {{sum}}};
    block_fold<RW>(v, slots[par]);
    if (threadIdx.x == 0) {
      if (v.i == LLONG_MAX) v.i = s;           // nothing but NaN
      A.out[k].argmax = v.i; A.out[k].max = v.m; A.out[k].sum = v.s[0];
    }
  }
}

constexpr int kTileGrid = 4096;              // blocks of the tile pass (<= 8192: a one-block finalize)
constexpr unsigned kWordsGrid = 512;         // blocks of runs_words, a chunk of the groups each
long long groups_of(long long nt) { return (nt + RG - 1) / RG; }

struct RunsScratch {
  RunTile* tab;
  PeakPartial *bpart, *rec;
  unsigned long long* bits;
  long long* per_group;          // 7 arrays of groups_of(nt)
  RunGroup* gtab;
};
RunsScratch carve(void* scratch, long long nt) {
  RunsScratch s;
  s.tab = static_cast<RunTile*>(scratch);
  s.bpart = reinterpret_cast<PeakPartial*>(s.tab + nt);
  s.rec = s.bpart + kTileGrid;
  s.bits = reinterpret_cast<unsigned long long*>(s.rec + 1);
  s.per_group = reinterpret_cast<long long*>(s.bits + nt * RWORDS);
  s.gtab = reinterpret_cast<RunGroup*>(s.per_group + 7 * groups_of(nt));
  return s;
}

template <class T>
hipError_t runs_t(const void* a, long long n, double thr, int relative, long long max_gap, RunRec* out,
                  long long cap, RunsInfo* info, void* scratch, hipStream_t st) {
  const long long nt = (n + kRunsTile - 1) / kRunsTile, ng = groups_of(nt);
  const RunsScratch s = carve(scratch, nt);
  const unsigned g1 = (unsigned)(nt < kTileGrid ? nt : kTileGrid);
  const T* at = static_cast<const T*>(a);
  const bool vec = (reinterpret_cast<uintptr_t>(a) & 15) == 0;
  // an absolute threshold is known now: the tile pass leaves the mask words
  if (relative) {
    if (vec) hipLaunchKernelGGL((runs_tile<T, true, false>), dim3(g1), dim3(RT), 0, st, at, n, nt, s.tab, s.bpart, thr, s.bits);
    else hipLaunchKernelGGL((runs_tile<T, false, false>), dim3(g1), dim3(RT), 0, st, at, n, nt, s.tab, s.bpart, thr, s.bits);
  } else {
    if (vec) hipLaunchKernelGGL((runs_tile<T, true, true>), dim3(g1), dim3(RT), 0, st, at, n, nt, s.tab, s.bpart, thr, s.bits);
    else hipLaunchKernelGGL((runs_tile<T, false, true>), dim3(g1), dim3(RT), 0, st, at, n, nt, s.tab, s.bpart, thr, s.bits);
  }
  hipError_t e = launch_partial_finalize(s.bpart, g1, 0, s.rec, nullptr, st);
  if (e != hipSuccess) return e;
  RunsArgs A;
  A.a = a; A.n = n; A.gap1 = (max_gap < n ? max_gap : n) + 1; A.ntiles = nt; A.ngroups = ng; A.cap = cap;
  A.thr = thr; A.relative = relative;
  A.tab = s.tab; A.gtab = s.gtab; A.rec = s.rec; A.bits = s.bits;
  A.gfirst = s.per_group; A.glast = A.gfirst + ng; A.gcov = A.glast + ng;
  A.gp = A.gcov + ng; A.gq = A.gp + ng; A.gcs = A.gq + ng; A.gce = A.gcs + ng;
  A.out = out; A.info = info;
  const unsigned g2 = (unsigned)ng;
  if (relative) hipLaunchKernelGGL((runs_mask<T, false>), dim3(g2), dim3(RT), 0, st, A);
  else hipLaunchKernelGGL((runs_mask<T, true>), dim3(g2), dim3(RT), 0, st, A);
  hipLaunchKernelGGL(runs_scan_edges, dim3(1), dim3(1024), 0, st, A.gfirst, A.glast, ng, A.gp, A.gq);
  // runs_words: a chunk of 2 .. RB groups per block, about kWordsGrid blocks
  long long chunk = (ng + kWordsGrid - 1) / kWordsGrid;
  chunk = chunk < 2 ? 2 : (chunk > RB ? RB : chunk);
  const unsigned gw = (unsigned)((ng + chunk - 1) / chunk);
  hipLaunchKernelGGL((runs_words<false>), dim3(gw), dim3(RB), 0, st, A);
  hipLaunchKernelGGL(runs_scan_counts, dim3(1), dim3(1024), 0, st, A.gcs, A.gce, A.gcov, ng, s.rec, thr, relative, info);
  if (cap > 0) {
    hipLaunchKernelGGL((runs_words<true>), dim3(gw), dim3(RB), 0, st, A);
    const unsigned g3 = (unsigned)(cap < kStatsGrid ? cap : kStatsGrid);
    hipLaunchKernelGGL((runs_stats<T>), dim3(g3), dim3(RT), 0, st, A);
  }
  return hipGetLastError();
}

}  // namespace

size_t runs_scratch_bytes(long long n) {
  const long long nt = (n + kRunsTile - 1) / kRunsTile;
  return (size_t)nt * sizeof(RunTile) + (size_t)(kTileGrid + 1) * sizeof(PeakPartial) +
         (size_t)nt * RWORDS * sizeof(unsigned long long) +
         (size_t)groups_of(nt) * (7 * sizeof(long long) + sizeof(RunGroup));
}

hipError_t launch_runs(int dtype, const void* a, long long n, double thr, int relative, long long max_gap,
                       RunRec* out, long long cap, RunsInfo* info, void* scratch, hipStream_t st) {
  if (n < 1 || max_gap < 0 || cap < 0 || !a || !info || !scratch || (cap > 0 && !out)) return hipErrorInvalidValue;
  return dispatch_dtype(dtype, [&](auto tag) {
    return runs_t<typename decltype(tag)::type>(a, n, thr, relative, max_gap, out, cap, info, scratch, st);
  });
}

}  // namespace vsig
