// Internal interface between the C-ABI layer (api_*.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "combine_plan.hpp"

namespace vsig {

// XCD-aware block order.  The dispatcher hands block b to XCD b % 8 and each
// XCD has its own L2, so with the identity mapping the overlap two
// neighbouring overlap-save segments share is fetched from HBM by two
// different L2s.  Remapping gives every XCD one contiguous run of segments
// (a bijection on [0, nb)), so the overlap of b and its successor (dispatched
// at about the same time to the same XCD) hits in L2.
__device__ __forceinline__ long long xcd_remap(long long b, long long nb) {
  const long long q = nb >> 3, r = nb & 7;
  const long long x = b & 7, i = b >> 3;
  return x * q + (x < r ? x : r) + i;
}

// Per-stage effective clock (vsig_clock_*, a diagnostic the bench runs in
// untimed steps after its timed loop).  When a launch gets a sink, wave 0 of
// every 64th block reads the shader clock (s_memtime) and the 100 MHz
// real-time counter (s_memrealtime) at its start and at its end and adds both
// differences into sink[0] / sink[1] by vector atomics; the clock over the
// sampled blocks' lifetimes is then sink[0] / sink[1] x 100 MHz.  With no sink
// (the default) nothing is read and nothing is written.
struct ClockStamp {
  unsigned long long t0 = 0, r0 = 0;
  bool on;
  __device__ __forceinline__ ClockStamp(unsigned long long* sink, unsigned long long blk)
      : on(sink != nullptr && (blk & 63) == 0) {
    if (on) {
      t0 = __builtin_amdgcn_s_memtime();
      r0 = __builtin_amdgcn_s_memrealtime();
      // lgkmcnt(0) alone: the counters' returns are retired here, so the
      // compiler's waits for the kernel's LDS reads stay counted (an SMEM read
      // left pending on one path makes every later LDS wait a full drain)
      __builtin_amdgcn_s_waitcnt(0xC07F);
    }
  }
  __device__ __forceinline__ void done(unsigned long long* sink) const {
    if (on && threadIdx.x < 2) {
      const unsigned long long t1 = __builtin_amdgcn_s_memtime();
      const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
      atomicAdd(sink + threadIdx.x, threadIdx.x == 0 ? t1 - t0 : r1 - r0);
    }
  }
};
// The sink of the launch being issued on this host thread (set by the C-ABI
// layer's per-stage timer when the clock option is on, else null); the launch
// functions pass it to the kernels that take one.
extern thread_local unsigned long long* g_clock_sink;

enum { VSIG_C128 = 0, VSIG_C64 = 1, VSIG_F64 = 2, VSIG_F32 = 3 };

// NCO mixer of apply_frequency_shift (utils.py:120-127): x[gi] * exp(j theta),
// theta = w * (gi / sr) with w = (2 pi) f, formed in double exactly as numpy
// forms it (t = np.arange(n) / sample_rate; (2j*pi*f) * t), reduced modulo 2 pi
// in double (Cody-Waite), rotation in fp32.  Used by mix_c64 and fused into the
// FIR's segment loads (fir.hip).
struct MixArgs {
  double w, sr;
  long long i0;      // global sample index of x[0]
  double wsr;        // w / sr (the fused loads' phase slope)
  // exp(j wsr d_e) for the fused loads' element offsets d_e = 64 e (the
  // 1024-point one-wave plan, 16 elements per lane), formed in double on the
  // host and rounded once to fp32: a lane rotates by exp(j theta(g + t)) once
  // and then by these, so the double-precision phase runs once per segment
  // and lane instead of once per sample.
  float rot[32];     // (cos, sin) interleaved
};
// The fused loads' form: exp(j theta), theta = (w / sr) * gi, one double
// multiply instead of numpy's division then multiply (|difference| <= ~2 ulp
// of theta, e.g. 2e-7 rad at |theta| = 1e9 rad; the standalone mixer keeps
// numpy's order).
// exp(2 pi j rev) for a phase given in revolutions (double): reduced in double
// to a quarter turn q and |g| <= 1/8 turn, then fp32 Taylor polynomials to
// degree 9 / 10 on |2 pi g| <= pi/4 (truncation < 2e-9); no ocml sincosf, whose
// large-argument path keeps a private array in scratch.
__device__ __forceinline__ float2 cis_rev(double rev) {
  const double f = rev - rint(rev);                    // [-1/2, 1/2] turn
  const double q = rint(4.0 * f);                      // quarter turns, -2..2
  const float x = (float)(f - 0.25 * q) * 6.283185307179586f;   // |x| <= pi/4
  const float x2 = x * x;
  const float sn = x * fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, 2.7557319e-6f, -1.9841270e-4f),
                                              8.3333333e-3f), -1.6666667e-1f), 1.0f);
  const float cs = fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, -2.7557319e-7f, 2.4801587e-5f),
                                                    -1.3888889e-3f), 4.1666667e-2f), -0.5f), 1.0f);
  const int qi = ((int)q) & 3;                         // rotate by q quarter turns
  const float c = qi == 0 ? cs : qi == 1 ? -sn : qi == 2 ? -cs : sn;
  const float s = qi == 0 ? sn : qi == 1 ? cs : qi == 2 ? -sn : -cs;
  return make_float2(c, s);
}
// The standalone mixer's sample: numpy's theta to the bit (correctly rounded
// division, then the product), reduced by whole turns in double (Cody-Waite,
// |r| <= pi to ~1e-16), then cis_rev on r in turns: cheap enough to run for
// every sample.
__device__ __forceinline__ float2 mix_at(float2 v, long long gi, double w, double sr) {
  constexpr double kTwoPiHi = 6.28318530717958623200e+00;
  constexpr double kTwoPiLo = 2.44929359829470635445e-16;
  constexpr double kInvTwoPi = 1.59154943091895345608e-01;
  const double t = __ddiv_rn((double)gi, sr);          // np.arange(n) / sample_rate
  const double th = __dmul_rn(w, t);                   // imaginary part of (2j*pi*f) * t
  const double k = rint(th * kInvTwoPi);
  const double r = fma(-k, kTwoPiLo, fma(-k, kTwoPiHi, th));
  const float2 e = cis_rev(r * kInvTwoPi);
  return make_float2(v.x * e.x - v.y * e.y, v.x * e.y + v.y * e.x);
}
__device__ __forceinline__ float2 mix_rot_fast(long long gi, double wsr) {
  constexpr double kInvTwoPi = 1.59154943091895345608e-01;
  return cis_rev((wsr * kInvTwoPi) * (double)gi);
}

// One block's |c| reduction partial (also the layout of the final result).
struct PeakPartial {
  double max2;       // max |c|^2 (kernels on |c|^2) or max |c| (peak_reduce / finalized)
  long long idx;     // index of the first maximum
  double sum_abs;    // sum |c|
  double sum_abs2;   // sum |c|^2
};

// Radices of the plan for N points (N = -1024: the one-wave FIR plan; -512 /
// -256: the decimating FIR's inverse plans).
hipError_t plan_info(int N, int* radices, int* npasses);
// Two-level twiddle table geometry: W_N^m = A[m >> shift] * B[m & (2^shift - 1)],
// A has `hi` entries, B has 2^shift.
hipError_t tw2_info(int N, int* shift, int* hi);

// Spectrum: nfft >= 4096 two frames per block (anchors, fft_pair), smaller
// plans several frames per block (LDS twiddles, split exchange; tw = the
// two-level table, see psd_plan_threads).
hipError_t launch_psd(int N, const float2* x, long long stride, const float* win, int nperseg,
                      long long hop, float scale, float* out, long long nframes, int shift,
                      const float2* tw, hipStream_t st);
// Threads per frame of the spectrum plan for N points (0: no plan): >= 256
// reads the per-pass twiddle table, below the two-level one.
int psd_plan_threads(int N);
hipError_t launch_spectrum_prep(int N, const float2* u, int len, float gain, float2* S,
                                const float2* tw, hipStream_t st);
// psd_traces.hip: per-bin mean / max / min of the PSD over its frames
// (vsig_psd_traces_c64_dev; see the file's header).  One record per bin and
// row; its max is NaN when a NaN was folded (the record's NaN flag).
struct PsdRec { double sum; float mx, mn; };
// In-LDS plans (psd_traces_in_lds): `blocks` rows, block b owns the frames
// [b fpb, (b + 1) fpb), `step` at a time.  Other lengths: the stored batches
// are folded into kPsdFoldRows rows, frames interleaved (step 1, fpb 0).
struct PsdTracesPlan { long long blocks, step, fpb; };
constexpr int kPsdFoldRows = 8;
constexpr int kTracesMinUnits = 4;           // steps a block runs at least (when there are that many)
bool psd_traces_in_lds(long long N);
PsdTracesPlan psd_traces_plan(long long N, long long nframes);
// The twiddle table launch_psd_traces reads for N: its plan key (plan_info's
// convention) and whether it is the two-level table.
int psd_traces_table(int N, bool* two_level);
// rows: psd_traces_plan(N, nframes).blocks * N records; tw: psd_traces_table(N)'s
hipError_t launch_psd_traces(int N, const float2* x, long long stride, const float* win, int nperseg,
                             long long hop, float scale, long long nframes, int shift, const float2* tw,
                             PsdRec* rows, hipStream_t st);
// nb stored frames (frame-major float32 [nb][N]) into rows[kPsdFoldRows][N];
// first: the rows start from the identity
hipError_t launch_psd_traces_fold(const float* sxx, long long nb, long long N, int first, PsdRec* rows,
                                  hipStream_t st);
// rows[nrows][N] -> mean (sum / nframes), max, min; any output may be null
hipError_t launch_psd_traces_merge(const PsdRec* rows, long long nrows, long long N, long long nframes,
                                   double* mean, float* mx, float* mn, hipStream_t st);
// psd_segments.hip: the traces of every segment of a table in one launch
// (vsig_psd_segments_run; see the file's header).  Block b transforms the
// `nframes` frames that start at sample x0 (hop apart) into record row b;
// segment s folds its rows [r0, r1) and divides by its nframes (0: a NaN row).
struct PsdSegBlock { long long x0, nframes; };
struct PsdSegRows { long long r0, r1, nframes; };
// (frames per step, blocks the device holds at once: CUs x resident blocks) of the segmented kernel for N
hipError_t psd_segments_geom(int N, int* step, long long* max_blocks);
// rows: nblocks * N records; tw: psd_traces_table(N)'s
hipError_t launch_psd_segments(int N, const float2* x, const float* win, int nperseg, long long hop,
                               float scale, int shift, const float2* tw, const PsdSegBlock* blocks,
                               long long nblocks, PsdRec* rows, hipStream_t st);
// max_rows: the most rows [r0, r1) any segment has (it picks the block size)
hipError_t launch_psd_segments_merge(const PsdRec* rows, const PsdSegRows* segs, long long nseg, int N,
                                     long long max_rows, double* mean, float* mx, float* mn, hipStream_t st);
// vsig_band_t (include/vsig.h) of every row of rows[nrows][ld], nbins used
struct BandRec { double power, centroid, peak; int peak_bin, lo_bin, hi_bin, flags; };
hipError_t launch_band_measure(const double* rows, long long nrows, int nbins, long long ld, double tail,
                               BandRec* out, hipStream_t st);
// isolate.hip: every segment of a table mixed down and band-filtered in one
// launch (vsig_isolate_run; see the file's header).  One record per 1024-point
// overlap-save frame: its input window starts at capture index x0 (zero fill
// outside [0, n)), its `keep` outputs (circular indices [lo, lo + keep)) go to
// y + y0, multiplied by row `filter` of Hs (F x kIsoM, FFT(h) / kIsoM) after
// the mixer exp(j wsr i) on capture index i.
constexpr int kIsoM = 1024;
struct IsoFrame { long long x0, y0; double wsr; int keep, filter; };
// tw: the one-wave 1024-point plan's table (plan key -1024)
hipError_t launch_isolate(const float2* x, long long n, const float2* Hs, int lo, float2* y,
                          const IsoFrame* frames, long long nframes, const float2* tw, hipStream_t st);
// Decimating FIR in the frequency domain (M = 1024, D = 2 / 4; see fir.hip).
// mix != nullptr: the mixer above applied to every loaded sample (fused).
hipError_t launch_fir_dec(int decim, const float2* x, long long n, long long g0, const float2* Hs,
                          int lo2, long long hop, float2* y, const float2* tw, const float2* twd,
                          hipStream_t st, const MixArgs* mix = nullptr);
// D = 4 at M = 1024 in polyphase form (fir.hip fir_poly_kernel): G = the
// 4 x 256 component filters from Hs (launch_fir_poly_gtable), tw = Plan256's
// table, twd = Plan256d's.
hipError_t launch_fir_poly_gtable(const float2* Hs, float2* G, hipStream_t st);
hipError_t launch_fir_poly(const float2* x, long long n, long long g0, const float2* G, int lo2,
                           long long hop, float2* y, const float2* tw, const float2* twd,
                           hipStream_t st, const MixArgs* mix = nullptr);
// Overlap-save FIR, M in {1024, 4096, 8192, 16384} (mix: M = 1024 only).
hipError_t launch_fir_os(int M, const float2* x, long long n, long long g0, const float2* Hs,
                         int ntaps, long long hop, int decim, float2* y, const float2* tw,
                         hipStream_t st, const MixArgs* mix = nullptr);
// Correlator, M in {4096, 8192, 16384} (16384: half-frame kernel, tw = the
// 8192-point table, wt = W_M^t for t < 512).  SD (M = 16384, hop even,
// xcorr_parity_aligned(s, off)): the template's parity-split table
// (launch_xcorr_parity_table of Ps); the launch then splits its frames by
// sample parity (16-byte segment loads, xcorr_geom's parity geometry).
hipError_t launch_xcorr_os(int M, const float2* s, long long n, const float2* Ps, long long off,
                           long long nout, long long hop, float2* c, int store_mode,
                           PeakPartial* partials, const float2* tw, const float2* wt,
                           hipStream_t st, unsigned* lkeys = nullptr, const float4* SD = nullptr);
hipError_t launch_xcorr_parity_table(int M, const float2* Ps, float4* SD, hipStream_t st);
bool xcorr_parity_aligned(const float2* s, long long off);
// Rows per thread column if the correlator for M can write lane keys
// (lkeys[b TF + m(t)]: thread t's max |c|^2 key, the refine's column
// candidates), else 0.
int xcorr_lane_keys(int M);
// Outputs of wave w of block b of the correlator for M (the refine pass's
// items): ob + wstep w + lstep l + rstep (q % rsub) + stride (q / rsub),
// l < 64, q < Q; plan: the twiddle table's key.  parity: the M = 16384 launch
// with its (S, D) table.
struct XcorrGeom { int waves, Q, stride, plan, wstep, rsub, lstep, rstep; };
hipError_t xcorr_geom(int M, bool parity, XcorrGeom* g);
// xcorr_bank.hip: K templates of one length against one stream, M in {4096,
// 8192, 16384}.  Ps: K spectra of M points; c: K rows of nout (may be null);
// partials[(k nblocks + b) waves + wave], nblocks = ceil(nout / hop), with
// waves and the launched (persistent) grid from xcorr_bank_geom.
hipError_t xcorr_bank_geom(int M, long long nblocks, int* waves, long long* grid);
hipError_t launch_xcorr_bank(int M, const float2* s, long long n, const float2* Ps, int K,
                             long long off, long long nout, long long hop, float2* c,
                             PeakPartial* partials, const float2* tw, hipStream_t st);
// out[k] = the record (max |c|, first index, sums) of group k of nparts partials
hipError_t launch_bank_finalize(const PeakPartial* parts, int K, long long nparts, PeakPartial* out,
                                hipStream_t st);
// match.hip: every pair of K packed packets in one pass (vsig_match_run; see
// the file's header), N in {1024, 4096, 8192, 16384}.  A unit is packet a
// against b0 .. b0 + nb - 1, all > a and < K.
struct MatchUnit { int a, b0, nb, pad; };
// the twiddle table's key for N, and the pair kernel's resident blocks (CUs x blocks per CU)
hipError_t match_geom(int N, int* table_key, long long* resident);
// offsets: K + 1 prefix sums of the lengths; W: K x N workspace; peak / lag: K x K;
// energy: K.  The spectra launch (K blocks), then the pair launch (grid blocks over nunits).
hipError_t launch_match(int N, const float2* packed, const long long* offsets, int K, float2* W,
                        double* energy, const MatchUnit* units, long long nunits, long long grid,
                        float* peak, int* lag, const float2* tw, hipStream_t st);
// combine.hip: coherent averaging of grouped packets (vsig_combine_*; see the
// file's header and combine_plan.hpp for the tables).  estimate: nitems items
// into their partials, then every packet's record (ref null: against the
// representatives in packed, whose own records are a = 1 by definition; f0
// null: 0).  sum: nitems (group, chunk) items write y exactly.
hipError_t launch_combine_estimate(const float2* packed, const float2* ref, const double* f0,
                                   const CombineMember* mem, int K, const CombineItem* items, long long nitems,
                                   CombinePartial* parts, double min_rho, CombineRecord* rec, hipStream_t st);
hipError_t launch_combine_sum(const float2* packed, const CombineMember* mem, const CombineGroup* grp,
                              const int* csr, const CombineItem* items, long long nitems,
                              const CombineRecord* rec, float2* y, hipStream_t st);
#ifdef VSIG_TUNING
// Tuning micro-benchmarks: iters FFTs per frame, frames blocks (key: plan key).
hipError_t launch_fft_bench(int key, float2* io, int frames, int iters, const float2* tw, int twl,
                            hipStream_t st);
hipError_t launch_copy_probe(const float2* x, long long n, float2* y, int variant, int grid,
                             hipStream_t st);
#endif
hipError_t launch_peak_reduce(int dtype, const void* a, long long n, PeakPartial* partials,
                              int nparts, hipStream_t st);
// np.argmax / np.max of an array holding a NaN: rec (peak_reduce's finalized record) gets
// the first NaN's index and a NaN maximum; a record whose sum |a| is not NaN is left alone
hipError_t launch_peak_first_nan(int dtype, const void* a, long long n, PeakPartial* rec, hipStream_t st);
constexpr int kFinalizeTmp = 1024;   // first-level partials of a two-level finalize
// zeroed PeakPartial-sized slots after the kFinalizeTmp records: the
// finalize's counter (first 8 B) and refine_fused's counters (128 B)
constexpr int kCounterRecs = 4;
hipError_t launch_partial_finalize(const PeakPartial* parts, long long nparts, int sqrt_max,
                                   PeakPartial* out, PeakPartial* tmp, hipStream_t st);

// refine.hip: exact re-rank of the |c| peak (see the file's header).
struct RefineArgs {
  const void* a; long long na;      // np.correlate(a, v) operands (device),
  const void* v; long long nv;      //   complex128 if c128 else complex64
  int c128;
  long long nout, F;                // final outputs; o <-> full index F + o
  int rev;                          // kernel raw index -> final nout - 1 - raw
  int from_array;                   // candidates from a stored c64 array c64[nout]
  const float2* c64;
  const PeakPartial* parts;         // or from the fused correlator's wave partials
  long long nparts, hop;
  int waves, Q, stride;             // wave w of block b: ob + wstep w + lstep l + rstep
  int wstep, rsub;                  //   (q % rsub) + stride (q / rsub), l < 64, q < Q
  int lstep, rstep;                 //   (xcorr_geom; 0: the plain map's 1 and 64)
  double eps;                       // fp32 candidate band (relative)
  int blas_threads;                 // OpenBLAS threads of the numpy matched (sums > 10000)
  int cols;                         // > 0: thread-column items from lane keys (Q = 1;
  const unsigned* lkeys;            //   cols rows each), lkeys: 64 per wave partial
  int finalize;                     // finalize the partials here (+ select, one launch):
  PeakPartial* tmp;                 //   kFinalizeTmp first-level records,
  unsigned long long* done;         //   kCounterRecs records' worth of counters,
                                    //   zero between launches
  long long cap;                    // opt-in limit on candidate outputs (0: none)
  void* scratch;                    // refine_scratch_bytes(*this)
  PeakPartial* rec;                 // finalized record (max |c|), updated in place
  void* out128;                     // optional complex128 c to patch (final space)
  unsigned long long wd_ticks;      // fused launch's watchdog, 100 MHz ticks (0: 2 s)
};
// Header of the refine scratch (zeroed before select: by the fused finalize,
// or a memset); the C-ABI layer reads count / status / fault back.
struct RefineKeys {
  unsigned long long count;    // candidate items appended by select
  unsigned long long lo_inv;   // ~(lowest final output an item covers)  (atomic max)
  unsigned long long hi_p1;    // highest final output an item covers + 1 (atomic max)
  unsigned long long status;   // 1: more candidate outputs than the opt-in cap
  unsigned long long done;     // numpy-pass blocks finished (the last one reduces)
  unsigned long long fault;    // sticky: a refine_fused watchdog fired.  Nothing on
                               // the device clears it (the finalize resets status,
                               // not this); vsig_refine_status reports status 3 and
                               // clears it with the launch's counters.
  unsigned long long pad[2];
};
constexpr size_t kRefineKeysBytes = 64;
static_assert(sizeof(RefineKeys) == kRefineKeysBytes, "the items follow the keys at +64 B");
size_t refine_scratch_bytes(const RefineArgs& r);
hipError_t launch_refine(const RefineArgs& r, hipStream_t st);
// numpy's |c| of every output o in [lo, hi] into vals[o - lo] (operands and
// geometry of r; scratch: refine_values_scratch_bytes()); r.rec (optional)
// receives numpy's argmax over the range.
size_t refine_values_scratch_bytes();
hipError_t launch_refine_values(const RefineArgs& r, long long lo, long long hi, double* vals,
                                hipStream_t st);
// reduce.hip: numpy's np.mean(np.abs(a)) and np.std(np.abs(a)) (float64
// pairwise sums over 8192-element buffers, two passes) of an array of dtype
// VSIG_C128 or VSIG_F64 into out[0], out[1] (device); scratch:
// np_stats_scratch_bytes(n).
size_t np_stats_scratch_bytes(long long n);
hipError_t launch_np_stats(int dtype, const void* a, long long n, double* out, void* scratch,
                           hipStream_t st);
// region.hip: sums[0..2] (device) = sum |a|^2, sum |b|^2, sum |a - b|^2 over two
// complex64 regions of n samples, each term numpy's float32 np.abs(x) ** 2,
// summed in double in a fixed order (one partial a block, at most
// kRegionBlocks of them; scratch: region_scratch_bytes()).  a and b are
// 8-byte aligned and may be the same array.
constexpr int kRegionBlocks = 2048;
size_t region_scratch_bytes();
hipError_t launch_region_power(const float2* a, const float2* b, long long n, double* sums,
                               void* scratch, hipStream_t st);
hipError_t launch_convert_c(int to128, const void* x, long long n, void* y, hipStream_t st);

// bigfft.hip: four-step FFT of M = N1 N2 > 16384 points, Bluestein for any
// length (see the file's header).
struct BigIn {                 // operand n of frame f
  const void* src;
  int kind;                    // 0 complex64, 1 complex128, 2 zeros
  long long fstride, estride, nvalid;
  const float2* chirp;         // optional * chirp[n]
  const float* win;            // optional * win[n]
  int conj;                    // conj(x) first (inverse DFT)
  float scale;
};
struct BigOut {                // natural-order result n of frame f
  void* dst;
  int kind;                    // 0 complex64, 1 complex128, 2 float64 real part, 3 complex64 real part,
                               // 4 float32 |X|^2 * scale (PSD), at (n + nout/2) % nout if shift
  long long fstride, nout;
  const float2* chirp;         // optional * chirp[n], then conj
  int conj;
  float scale;
  int shift = 0;
};
void bigfft_split(long long M, int* N1, int* N2);
hipError_t launch_bf_chirp(long long N, long long M, float2* c, float2* b, hipStream_t st);
hipError_t launch_bf_col(int N1, int N2, long long batch, const BigIn& in, float2* tmp,
                         const float2* tw1, const float2* t2, int S, int hiA, hipStream_t st);
hipError_t launch_bf_icol(int N1, int N2, long long batch, float2* tmp, const BigOut& out,
                          const float2* tw1, const float2* t2, int S, int hiA, hipStream_t st);
// mode 3 (natural-order DFT output) stores through *out; the other modes ignore it
hipError_t launch_bf_row(int mode, int N1, int N2, long long batch, float2* tmp, const float2* Bk,
                         const float2* tw2, float scale, float* psd, int shift, hipStream_t st,
                         const BigOut* out = nullptr);
// a frame of N <= kDirectMax points as a direct sum in double (no plan, no chirp)
constexpr int kDirectMax = 512;
hipError_t launch_bf_direct(int N, long long batch, const BigIn& in, const BigOut& out, hipStream_t st);
hipError_t launch_bf_small(int mode, int M, long long batch, const BigIn& in, const BigOut& out,
                           const float2* Bk, const float2* tw, hipStream_t st);
hipError_t launch_resample_spectrum(const float2* X, long long Nx, long long num, float2* Y,
                                    hipStream_t st);
hipError_t launch_channel_mask(const float2* X, long long n, double sr, double center, double lo,
                               double hi, float2* F, hipStream_t st);
// kept bins [ka, kb] (kb < ka: none) of the channel filter by direct double sums;
// part: 256 * (kb - ka + 1) scratch, X: kb - ka + 1
hipError_t launch_channel_direct(int c128, const void* x, long long n, long long ka, long long kb,
                                 double2* part, double2* X, double* y, hipStream_t st);

// pfb.hip: C in {64, 128, 256}, PT in {4, 8, 16}; y frame-major (M x C)
hipError_t launch_pfb(int C, int PT, const float2* x, long long n, const float* h, long long M,
                      float2* y, const float2* tw, hipStream_t st);
hipError_t pfb_plan(int C, int PT, long long M, long long* fpg, long long* groups_per_block,
                    long long* blocks);

// stream_ops.hip
hipError_t launch_mix_c64(const float2* x, long long n, double w, double sr, long long i0, float2* y,
                          hipStream_t st);
hipError_t launch_scale_c64(const float2* x, long long n, float s, float2* y, hipStream_t st);
hipError_t launch_fir_part_accum(const float2* z, long long nz, long long off, int D, long long ny,
                                 int first, float2* y, hipStream_t st);
hipError_t launch_wv_quantize(const float2* x, long long n, float norm, short* out, hipStream_t st);
hipError_t launch_planar_to_c64(int mi_type, const void* re, const void* im, long long n, float2* y,
                                hipStream_t st);
hipError_t launch_c64_to_planar(const float2* x, long long n, float* re, float* im, hipStream_t st);

// vector_build.hip: one packet's placements (instance k at start + k period,
// k < count, every instance inside the vector) and one launch's worth of them,
// carried in the kernel arguments.
struct PlaceDesc {
  const float2* y;
  long long len, start, period, count;
};
constexpr int kPlacesPerLaunch = 16;
struct PlaceBatch {
  PlaceDesc d[kPlacesPerLaunch];
  int nd;
};
hipError_t launch_vector_build(const PlaceBatch& pb, float2* out, long long n, int load,
                               float* maxabs, hipStream_t st);
hipError_t launch_normalize_c64(const float2* x, long long n, const float* maxabs, float2* y,
                                hipStream_t st);

// analysis.hip
hipError_t launch_radix_hist(int dtype, const void* a, long long n, const unsigned long long* prefix,
                             const unsigned long long* mask, int nq, int shift,
                             unsigned long long* hist, hipStream_t st);
struct ThreshPartialH { long long count, first, last; double max; };   // = ThreshPartial
hipError_t launch_thresh_reduce(int dtype, const void* a, long long n, double thr, void* parts,
                                int nparts, hipStream_t st);
long long energy_scan_tiles(long long n);
hipError_t launch_energy_prefix(int dtype, const void* x, long long n, double* sums, double* P,
                                hipStream_t st);
hipError_t launch_boxcar_same(const double* P, long long n, long long w, double* sm, hipStream_t st);
// the same outputs summed directly over each window (an input with a non-finite energy)
hipError_t launch_boxcar_direct(int dtype, const void* x, long long n, long long w, double* sm,
                                hipStream_t st);
hipError_t launch_db_transform(int dtype, const void* a, long long n, double floor_, void* out,
                               hipStream_t st);
hipError_t launch_abs_c64(int dtype, const void* a, long long n, float2* out, hipStream_t st);
hipError_t launch_abs_c128(int dtype, const void* a, long long n, double2* out, hipStream_t st);

// display.hip: Sxx (n_freq x n_time, VSIG_F32 / VSIG_F64; frame-major memory
// when freq_fast, else C-contiguous; ld elements between rows of the fast axis)
// -> ceil(n_freq / pf) x ceil(n_time / pt) RGBA pixels through the 259-row
// colour table lut (see the file's header).  lut and rgba are 4-byte aligned.
hipError_t launch_spectrogram_image(int dtype, const void* sxx, long long n_freq, long long n_time,
                                    int freq_fast, long long ld, double floor_, double vmin, double vmax,
                                    int median, int flip, int pf, int pt, const unsigned char* lut,
                                    unsigned char* rgba, hipStream_t st);

// peaks.hip: the peak list of |a| (threshold + first maximum of a +-d window;
// see the file's header).  thr: absolute, or with `relative` a ratio of
// max |a| multiplied on the device.  out: the first `cap` instances in
// ascending index order (may be null when cap == 0); info: always written.
// scratch: peaks_scratch_bytes(n).
constexpr int kPeaksTile = 2048;
struct PeakInst { long long index; double value; };                          // = vsig_instance_t
struct PeaksInfo { long long count, argmax; double max, thr_used; };         // = vsig_peaks_info_t
size_t peaks_scratch_bytes(long long n);
hipError_t launch_peaks(int dtype, const void* a, long long n, double thr, int relative, long long d,
                        PeakInst* out, long long cap, PeaksInfo* info, void* scratch, hipStream_t st);

// runs.hip: the run list of |a| >= thr (maximal intervals whose ends are
// masked and that hold no more than max_gap unmasked elements in a row; see
// the file's header).  thr / relative / out / cap / info as for launch_peaks.
// scratch: runs_scratch_bytes(n).
constexpr int kRunsTile = 2048;
struct RunRec { long long start, end, argmax; double max, sum; };           // = vsig_run_t
struct RunsInfo { long long count, covered, argmax; double max, thr_used; };  // = vsig_runs_info_t
size_t runs_scratch_bytes(long long n);
hipError_t launch_runs(int dtype, const void* a, long long n, double thr, int relative, long long max_gap,
                       RunRec* out, long long cap, RunsInfo* info, void* scratch, hipStream_t st);

// trace.hip: the min / max envelope of |a| per column of `bin` positions of
// the (optionally fftshifted) line over [lo, hi), and the window's first
// extrema (vsig_trace_envelope_dev; see include/vsig.h).  env_min / info may
// be null.  scratch: trace_scratch_bytes(lo, hi, bin).
constexpr int kTraceTile = 2048;             // positions a block of trace_cols owns at most
constexpr int kTraceAbs = 0, kTraceDb20 = 1;                                 // = VSIG_TRACE_*
struct TraceRec { double mn, mx; long long pmn, pmx, nan; };                 // one block's / column's extrema
struct TraceInfo { long long argmin, argmax; double min, max; };             // = vsig_trace_info_t
size_t trace_scratch_bytes(long long lo, long long hi, long long bin);
hipError_t launch_trace_envelope(int dtype, const void* a, long long n, int shift, long long lo,
                                 long long hi, long long bin, int kind, double eps, void* env_min,
                                 void* env_max, TraceInfo* info, void* scratch, hipStream_t st);

}  // namespace vsig
