/* vsig — MI355X-native vector-signal DSP hot path, C ABI (libvsig.so).
 *
 * The reference (ramiyako/vector) is a pure-Python module whose DSP lives in
 * utils.py and calls numpy/scipy directly; it has no FFI.  Each entry point
 * below replaces one numpy/scipy call the reference makes on its hot path, and
 * is what a ctypes / cffi binding in place of that call would bind
 * (INTEGRATION.md shows the binding):
 *
 *   vsig_psd_*        scipy.signal.spectrogram(..., return_onesided=False,
 *                     detrend=False, scaling='spectrum')      utils.py:281-291
 *                     (+ fftshift of Sxx, utils.py:351, when shift = 1)
 *   vsig_psd_traces_* the mean / max / min of that Sxx over its frames
 *                     (scipy.signal.welch(..., average='mean'), max-hold,
 *                     min-hold) without storing it
 *   vsig_fir_*        np.convolve(x, taps, 'full')[:len(x)] then x[::decim]
 *                     (reference idioms utils.py:802,816 and utils.py:194)
 *   vsig_correlate_*  np.correlate(signal2, signal1, mode) in
 *                     cross_correlate_signals                  utils.py:1284-1285
 *   vsig_xcorr_*      the same, streaming form with a fixed template, fused
 *                     with find_correlation_peak               utils.py:1321-1334
 *   vsig_xcorr_bank_* K templates of one length against one stream in one pass
 *                     (the carrier-offset search; no reference counterpart)
 *   vsig_match_*      every pair of K packets against each other in one pass: peak
 *                     |correlation|, its lag and the energies (which bursts are
 *                     one emitter's; no reference counterpart)
 *   vsig_combine_*    the bursts of one emitter averaged coherently into one packet, with
 *                     a gain, a frequency and an SNR per instance (the clean packet the
 *                     reference's users cut by hand; no reference counterpart)
 *   vsig_peak_*       find_correlation_peak's |c| argmax / mean / std
 *                                                               utils.py:1321-1334
 *
 * Conventions
 *   - complex data is interleaved float32 pairs (numpy complex64 layout);
 *     complex128 only where stated.
 *   - "_dev" functions take device pointers and enqueue on the context's
 *     stream (vsig_set_stream); they do not synchronise.  Host-pointer
 *     functions copy in, compute and copy out synchronously.
 *   - the caller allocates every output; the library never frees caller
 *     memory.  Output sizes follow the formulas in the comments.
 *   - every function returns VSIG_OK (0) or a negative status; nothing throws
 *     across the ABI.  vsig_last_error(ctx) gives a message.
 *   - one context per host thread.
 */
#ifndef VSIG_H
#define VSIG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSIG_OK 0
#define VSIG_E_INVALID -1     /* bad argument (size, mode, null pointer ...) */
#define VSIG_E_HIP -2         /* HIP runtime error */
#define VSIG_E_NOMEM -3       /* device allocation failed */
#define VSIG_E_UNSUPPORTED -4 /* size outside what the kernels implement */
#define VSIG_E_NODEVICE -5    /* no HIP device */
#define VSIG_E_REFINE -6      /* the exact-argmax refine faulted (watchdog, status 3):
                                 the peak record must not be used */

#define VSIG_MODE_VALID 0
#define VSIG_MODE_FULL 1
#define VSIG_MODE_SAME 2

#define VSIG_DTYPE_C128 0
#define VSIG_DTYPE_C64 1
#define VSIG_DTYPE_F64 2
#define VSIG_DTYPE_F32 3

typedef struct vsig_ctx vsig_ctx;
typedef struct vsig_fir vsig_fir;
typedef struct vsig_xcorr vsig_xcorr;
typedef struct vsig_xcorr_bank vsig_xcorr_bank;

/* Result of a |c| peak reduction (find_correlation_peak, utils.py:1321-1334).
 * index: first maximum of |c|; peak: |c[index]|; sums over every element.
 * From the fused correlators (a peak record without a stored c) the sums are
 * fp32 per-thread sums of the fp32 |c|, combined in double: relative error
 * ~1e-7, so the single-pass variance var = sum_abs2/n - (sum_abs/n)^2 carries
 * ~1e-7 x (sum_abs2/n) / var.  find_correlation_peak's confidence formed from
 * them is within 1e-5 of numpy's while var >= 0.05 sum_abs2/n (noise-like
 * |c|: 0.21); below that (a flat |c|: a tone, a tone under weak noise) use
 * vsig_correlate_stats_dev for numpy's own mean / std -- the Python front end
 * (correlate_peak) does exactly that (tests/test_gpu_refine.py, tone under
 * noise at 0-60 dB).  An index of -1 means the record is invalid (a refine
 * fault, VSIG_E_REFINE / vsig_refine_status 3). */
typedef struct vsig_peak_t {
  double peak;
  int64_t index;
  double sum_abs;
  double sum_abs2;
} vsig_peak_t;

int vsig_version(void);
const char* vsig_errstr(int status);

/* ---- context ------------------------------------------------------------- */
int vsig_init(int device, vsig_ctx** out);
void vsig_free(vsig_ctx* ctx);
const char* vsig_last_error(const vsig_ctx* ctx);
/* hip_stream: the hipStream_t to enqueue on; NULL is the default (null)
 * stream.  A new context starts on a private non-blocking stream. */
int vsig_set_stream(vsig_ctx* ctx, void* hip_stream);
/* The hipStream_t the context enqueues on. */
void* vsig_get_stream(vsig_ctx* ctx);
/* Copy bytes between device or host buffers, ordered on the context's stream. */
int vsig_copy_dev(vsig_ctx* ctx, void* dst, const void* src, int64_t bytes);
int vsig_synchronize(vsig_ctx* ctx);
/* Options of the correlators' exact-argmax refine pass (refine.hip):
 *   "refine"          1 (default): after every correlation, the outputs whose
 *                     fp32 |c| lies within the band below the fp32 maximum are
 *                     recomputed by direct sums in double precision, and the
 *                     ones that can be the maximum once more in numpy's own
 *                     operation order (OpenBLAS zdotu + numpy's complex abs),
 *                     in the operands' own precision; the record's peak /
 *                     index are replaced by numpy's -- np.argmax over
 *                     np.abs(np.correlate) in complex128, to the bit;
 *                     0: the fp32 FFT result only -- for the fused correlators
 *                     (M >= 16384) the peak is then |c| with the low 6 mantissa
 *                     bits of |c|^2 replaced by the output's rank in its thread
 *                     (up to 3.8e-6 relative low; near-ties within 2^-17
 *                     decided by that rank, not by the lowest index);
 *   "blas_threads"    OpenBLAS threads of the numpy being matched (default 1;
 *                     the Python front end sets numpy's own): its zdotu splits
 *                     sums of more than 10000 terms into that many chunks;
 *   "refine_eps_ppm"  the band, relative to max |c| (default 1000 = 1e-3; the
 *                     fp32 correlation error is ~1e-8 of |p| |s_segment|);
 *   "refine_cap"      0 (default): no limit -- every candidate output is
 *                     evaluated in numpy's order however many there are (a
 *                     flat |c|, e.g. a tone, puts every full-overlap output in
 *                     the band; those run in refine.hip's dense form, about
 *                     1 ms per 2^20 outputs x 4096 terms); > 0 (>= 4096): an
 *                     explicit limit on candidate outputs -- beyond it the
 *                     record is left as the fp32 pass produced it and
 *                     vsig_refine_status reports status 1;
 *   "refine_watchdog_us" bound on the one-launch refine's two waits (default
 *                     2000000; a test hook: tiny values force a fire, status 3);
 *   "refine_async"    0 (default): the refine runs on the context stream after
 *                     its correlator; 1: the refine of vsig_xcorr_exec_dev runs
 *                     on the context's own refine stream (vsig_refine_stream),
 *                     behind an event after the correlator, so the caller's next
 *                     kernels (e.g. the next chunk's filter) overlap it.  The
 *                     peak record is then complete only on the refine stream:
 *                     read it after vsig_refine_join (the context stream waits
 *                     for the last refine) or order its consumers on
 *                     vsig_refine_stream; the caller must not overwrite the
 *                     correlated stream before that.  The library itself joins
 *                     before it reuses the refine's scratch (any later
 *                     correlation, peak, statistics or staging call), and
 *                     vsig_refine_status / vsig_synchronize wait for it.
 * and of the spectrum traces (vsig_psd_traces_c64_dev):
 *   "psd_traces_batch" 0 (default): frames per stored batch by the 256 MB rule;
 *                     > 0: at most that many (nfft outside the in-LDS plans only).
 * and of the template bank (vsig_xcorr_bank_create): "xcorr_bank_m", see there;
 * and of the all-pairs match (vsig_match_create): "match_grid", see there. */
int vsig_set_option(vsig_ctx* ctx, const char* key, int value);
int vsig_get_option(const vsig_ctx* ctx, const char* key, int* value);
/* The hipStream_t the "refine_async" refine runs on (the context stream when
 * the option is off), and the join: the context stream waits for the last
 * refine (an event; no host synchronisation). */
void* vsig_refine_stream(vsig_ctx* ctx);
int vsig_refine_join(vsig_ctx* ctx);
/* Outcome of the context's last refine pass (synchronises the stream):
 * status 0 refined, 1 skipped (more candidate outputs than a refine_cap set
 * > 0), 2 no pass ran (refine off, or no correlation yet), 3 the one-launch
 * refine's watchdog fired in some pass since the last call (a block waited
 * longer than the "refine_watchdog_us" option, default 2 s, for the published
 * keys: a device fault, never seen in operation).  Status 3 is an error: the
 * record's index is poisoned (-1) and its values must not be used; this call
 * reports it once and clears the refine's counters so the context's next
 * correlation starts clean (vsig_chain_result returns VSIG_E_REFINE instead);
 * candidates =
 * candidate items (thread columns of the M = 16384 / 32768 correlators, waves
 * of the M = 4096 / 8192 ones, 64-output chunks of a stored array). */
int vsig_refine_status(vsig_ctx* ctx, int32_t* status, int64_t* candidates);
/* Hash of the kernel / ABI sources this library was built from (the Python
 * loader compares it with the sources next to it and refuses a stale build). */
const char* vsig_build_id(void);
/* Per-kernel timing with HIP events on the context stream (for bench.py):
 * enable, run, then read the mean duration in ms of each kernel family. */
int vsig_timing_enable(vsig_ctx* ctx, int on);
int vsig_timing_read(vsig_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches);
int vsig_timing_reset(vsig_ctx* ctx);
/* Per-stage effective clock (a diagnostic, for bench.py's untimed clock steps):
 * while enabled (enable zeroes the sums), the FIR, PSD, correlator and PFB
 * kernels sample the shader clock and the 100 MHz real-time counter at the
 * start and end of every 64th block (wave 0); read returns the mean clock in
 * GHz of a kernel family over those blocks' lifetimes (0 if none ran) and the
 * real-time ticks it averaged over. */
int vsig_clock_enable(vsig_ctx* ctx, int on);
int vsig_clock_read(vsig_ctx* ctx, const char* kernel, double* ghz, int64_t* ticks);

/* ---- spectrum: Sxx[f, k] = |sum_{i<nperseg} w[i] x[f*hop + i] e^{-2 pi j k i / nfft}|^2 * scale
 * nfft: any length >= nperseg up to 2^27 (powers of two in [64, 2^28]: in-LDS plans, above
 *   16384 a four-step FFT per frame; other lengths: a direct sum in double up to 512 points,
 *   Bluestein per frame beyond, bigfft.hip);
 * nframes = (n - nperseg) / hop + 1;
 * sxx is frame-major float32 [nframes][nfft] (Sxx of scipy is its transpose);
 * shift = 1 stores bin k at (k + nfft/2) % nfft (np.fft.fftshift).
 * _dev only: stride reads sample i at x[i*stride] (n counts strided samples),
 * which folds create_spectrogram's sig[::factor] (utils.py:194) into the load. */
int vsig_psd_c64_dev(vsig_ctx* ctx, const void* x, int64_t n, int64_t stride, const float* win,
                     int32_t nperseg, int64_t hop, int32_t nfft, float scale, int32_t shift,
                     float* sxx, int64_t nframes);
int vsig_psd_c64(vsig_ctx* ctx, const void* x, int64_t n, const float* win, int32_t nperseg,
                 int64_t hop, int32_t nfft, float scale, int32_t shift, float* sxx,
                 int64_t nframes);

/* ---- spectrum traces: per-bin mean / max-hold / min-hold of Sxx over its frames in one
 * pass (a spectrum analyser's averaged, max-hold and min-hold detectors; the mean is
 * scipy.signal.welch(..., average='mean') with vsig_psd_*'s arguments).  The spectrogram
 * is never stored: the call reads 8 bytes per sample and writes O(nfft).
 * Arguments, validation and the frames are vsig_psd_c64_dev's.  With P[m][k] the float32
 * value vsig_psd_c64_dev stores for frame m, bin k (the same expression on the same
 * transform), at (k + nfft/2) % nfft when shift = 1:
 *   max[k]  = max over m, min[k] = min over m                       float32[nfft]
 *   mean[k] = (sum over m of (double)P[m][k]) / nframes             float64[nfft]
 * The sum is kept in double in registers, records and merge, so the result depends on the
 * launch geometry by about nframes * 2^-53 relative only.  A NaN P[m][k] makes all three
 * outputs of bin k NaN (np.max / np.min / np.mean).  Any output may be NULL (not computed);
 * all three NULL is VSIG_E_INVALID.
 * The call enqueues on the context stream and never synchronises; once its scratch (a
 * grow-only context buffer, bounded by the device's CU count and nfft, not by nframes) is
 * warm it allocates nothing and can be captured into a graph.  No float atomics; the
 * launch geometry is a function of (nfft, nframes) and the device alone, so the same input
 * gives the same bytes on every run.
 * nfft 64 .. 8192 (powers of two): the transform kernels reduce in their epilogue.  Every
 * other nfft vsig_psd_c64_dev accepts (16384 among them: its accumulators fit neither the
 * registers nor the LDS its transform leaves): that route runs in batches of frames into a
 * bounded scratch (256 MB, or at most "psd_traces_batch" frames: a vsig_set_option key,
 * 0 = automatic, the default) and each batch is folded into the same records.
 * vsig_psd_traces_plan: the geometry for (nfft, nframes) on the current device.  In-LDS
 * lengths: `blocks` blocks, block b owns the frames [b * frames_per_block, (b + 1) *
 * frames_per_block) and transforms frames_per_block_step of them at a time.  Other lengths:
 * blocks = the record rows the batches fold into, step 1, frames_per_block 0 (the frames
 * are interleaved over the rows). */
int vsig_psd_traces_c64_dev(vsig_ctx* ctx, const void* x, int64_t n, int64_t stride, const float* win,
                            int32_t nperseg, int64_t hop, int32_t nfft, float scale, int32_t shift,
                            int64_t nframes, double* mean_dev, float* max_dev, float* min_dev);
int vsig_psd_traces_c64(vsig_ctx* ctx, const void* x, int64_t n, const float* win, int32_t nperseg,
                        int64_t hop, int32_t nfft, float scale, int32_t shift, int64_t nframes,
                        double* mean, float* max, float* min);
int vsig_psd_traces_plan(int32_t nfft, int64_t nframes, int64_t* blocks, int64_t* frames_per_block_step,
                         int64_t* frames_per_block);

/* ---- segmented spectrum traces: vsig_psd_traces_c64_dev's three detectors for every
 * segment of a table, in one pass over all their frames (per-burst spectra: the table is
 * what vsig_runs lists).  window (float32[nperseg]), hop, nfft >= nperseg, scale and shift
 * are vsig_psd_c64_dev's; stride is 1.  Table: nseg entries {start, len} in samples with
 * 0 <= start, len >= 0, start + len <= n; segments may touch, overlap, repeat and come in
 * any order.  Segment s has nframes[s] = (len - nperseg) / hop + 1 frames if
 * len >= nperseg, else 0; its frame m covers x[start + m*hop + i], i < nperseg, and
 * P[s][m][k] is the float32 value vsig_psd_c64_dev stores for that frame (the same
 * expression on the same transform).  Row-major outputs, one row of nfft bins a segment:
 *   mean[s][k] = (sum over m of (double)P[s][m][k]) / nframes[s]    float64[nseg][nfft]
 *   max[s][k], min[s][k]: np.max / np.min over m (a NaN stays)      float32[nseg][nfft]
 * A NaN P makes that bin NaN in all three outputs of every segment whose frames hold it
 * and of no other; a segment with no frame gets NaN in its whole row of every output.
 * Samples outside the union of the frames (between segments, past a segment's last whole
 * frame, in a segment shorter than nperseg) are not read.
 * nfft: the powers of two from 64 to 8192; any other is VSIG_E_UNSUPPORTED.
 * vsig_psd_segments_create validates everything, takes the table from the HOST, builds
 *   the block table (a block owns a contiguous run of at most max_run_frames frames of
 *   one segment, transformed frames_per_step at a time; runs are sized so that the blocks
 *   fill the device once, and to at least four steps) and uploads it; it allocates the
 *   plan's own scratch (16 bytes x nfft per block) and may synchronise.
 *   VSIG_E_INVALID, with a message that names the offending segment where there is one:
 *   nseg < 0 or > 2^24, n < 1 or > 2^40, a segment outside [0, n], hop < 1, nperseg < 1,
 *   nfft < nperseg, a NULL ctx / out, a NULL table with nseg > 0.  nseg == 0 is valid.
 * vsig_psd_segments_run takes DEVICE pointers: x (complex64[n], 8-byte aligned), win,
 *   and the outputs, any of which may be NULL (not computed; all three NULL, a NULL x or
 *   win, or a misaligned x: VSIG_E_INVALID before any work is enqueued).  It enqueues on
 *   the context stream, allocates nothing, never synchronises and can be captured into a
 *   graph; a plan with nseg == 0 does nothing.  It reads 8 bytes per frame sample and
 *   writes O(nseg * nfft).  No float atomics; the launch geometry is a function of
 *   (nfft, the table, the device) alone, so the same input gives the same bytes on every
 *   run, and by vsig_psd_traces_c64_dev's argument max and min do not depend on the
 *   geometry at all and the mean by about nframes * 2^-53 relative.
 * vsig_psd_segments_info: the plan's frames (all segments), blocks, frames per step and
 *   the longest run a block is given.
 * vsig_psd_segments_free waits for the context stream, then frees the plan. */
typedef struct vsig_segment_t { int64_t start, len; } vsig_segment_t;
typedef struct vsig_psd_segments vsig_psd_segments;
int vsig_psd_segments_create(vsig_ctx* ctx, const vsig_segment_t* segs /*host*/, int64_t nseg, int64_t n,
                             int32_t nperseg, int64_t hop, int32_t nfft, vsig_psd_segments** out);
void vsig_psd_segments_free(vsig_psd_segments* plan);
int vsig_psd_segments_info(const vsig_psd_segments* plan, int64_t* frames_total, int64_t* blocks,
                           int64_t* frames_per_step, int64_t* max_run_frames);
int vsig_psd_segments_run(vsig_psd_segments* plan, const void* x, const float* win, float scale,
                          int32_t shift, double* mean, float* max, float* min);

/* ---- band measurement: where the power of each of nrows spectra sits.  rows: DEVICE
 * float64, row r at rows + r*ld, nbins <= ld values M[k] >= 0 in ascending frequency
 * (vsig_psd_segments_run's mean with shift = 1; any non-negative rows).  Per row, in
 * double, with c[k] the inclusive cumulative sum of M in ascending k:
 *   power    = total = c[nbins-1]
 *   peak_bin = the first maximum, peak = its value
 *   centroid = (sum of k * M[k]) / total, a fractional bin
 *   lo_bin   = the smallest k with c[k] >= tail * total
 *   hi_bin   = the smallest k with c[k] >= (1 - tail) * total
 * so [lo_bin, hi_bin] holds the fraction 1 - 2 tail of the power (the occupied bandwidth).
 * A row that holds a NaN (flags bit 0) or whose total is not > 0 (flags bit 1): power =
 * the total as summed, centroid = peak = NaN, peak_bin = lo_bin = hi_bin = -1.
 * The sums run in a fixed order that is not np.cumsum's left-to-right one (contiguous
 * chunks of 16 bins, each summed ascending; the chunk sums in a fixed tree): the same
 * input gives the same bytes on every run, and every c[k] and the total are within
 * nbins * 2^-52 * total of the sequential sums -- the indices are those of the sequential
 * sum whenever none of its values lies that close to a target.  lo_bin / hi_bin are the
 * first k at which the c so formed reaches the target (nbins-1 for a target within that
 * rounding of the total).
 * out: DEVICE vsig_band_t[nrows].  The call enqueues on the context stream, allocates
 * nothing and never synchronises (capturable).  VSIG_E_INVALID before any work is
 * enqueued: nrows < 0 or >= 2^31, nbins < 1, ld < nbins, a tail outside (0, 0.5) or NaN,
 * a NULL ctx / rows / out, rows or out not 8-byte aligned.  nrows == 0 does nothing. */
typedef struct vsig_band_t {
  double power;      /* sum of the row */
  double centroid;   /* power-weighted mean bin */
  double peak;       /* the largest value */
  int32_t peak_bin;  /* its first bin */
  int32_t lo_bin;    /* first bin at which the cumulative sum reaches tail * power */
  int32_t hi_bin;    /* ... (1 - tail) * power */
  int32_t flags;     /* bit 0: a NaN in the row; bit 1: power not > 0 */
} vsig_band_t;
int vsig_band_measure_run(vsig_ctx* ctx, const double* rows, int64_t nrows, int32_t nbins, int64_t ld,
                          double tail, vsig_band_t* out);

/* ---- burst isolation: every segment of a table mixed down to baseband and band-filtered,
 * all segments in one launch (the inverse of what vsig_vector_build_dev assembles; the
 * table is what vsig_runs lists, the frequencies what vsig_band_measure_run finds).
 * x: the capture, complex64[n]; sr the sample rate; T = ntaps, odd, d = (T-1)/2.  Segment
 * s = {start, len, freq, filter} covers the capture indices [lo, hi) = [start, start+len)
 * with 0 <= lo < hi <= n and uses row `filter` of the taps (real float32, F rows of T):
 *   u_s[i] = x[i] * exp(-2j*pi*freq*i/sr)              phase origin = capture index 0
 *   z_s[j] = sum_{m<T} h[m] * u_s[lo + j + d - m],  j in [0, len),  u_s = 0 outside [0, n)
 * i.e. the whole capture mixed by -freq, a linear-phase filter with its group delay
 * removed ("same" alignment), then the slice: the filter sees the capture's own samples
 * on both sides of the segment, zeros only beyond the capture's ends, and overlapping or
 * repeated segments of one frequency agree sample for sample.  The phase is formed as
 * theta = (w/sr)*i with w = -2*pi*freq, reduced in double, rotated in fp32 (the fused
 * mixer's form, vsig_fir_exec_mix_dev); freq == 0 is not rotated at all.  The packed
 * output y holds z_0, z_1, ... back to back: z_s starts at offsets[s], offsets the prefix
 * sums of len.  Segments may touch, overlap, repeat and come in any order.
 * Work runs in 1024-point overlap-save frames of hop = 1025 - T outputs, each segment
 * cut into ceil(len / hop) frames of its own (two frames a workgroup, which may belong to
 * different segments and filters); a frame reads x[g + d - (T-1) .. + 1024) for its first
 * output's capture index g, clipped to [0, n).
 * Non-finite input: a NaN or Inf sample makes every output of every frame whose window
 * holds it non-finite and changes no bit of any other frame's outputs.
 * ntaps: odd, 3 .. 511 (hop 1022 .. 514); an odd ntaps above 511 is VSIG_E_UNSUPPORTED.
 * vsig_isolate_create validates everything, takes the table and the taps from the HOST,
 *   builds the F x 1024 filter spectra and the frame table (32 bytes a frame) on the
 *   device and may synchronise.  VSIG_E_INVALID, with a message that names the offending
 *   segment where there is one: nseg < 0 or > 2^24, n < 1 or > 2^40, a segment with
 *   len < 1 or outside [0, n), a filter index outside [0, nfilters), a non-finite freq,
 *   nfilters outside [1, 4096], an even ntaps or one below 3, sr not finite or not > 0, a
 *   non-finite tap, a NULL ctx / out / taps, a NULL table with nseg > 0.  nseg == 0 is valid.
 * vsig_isolate_info: the packed output's length, the frames, the workgroups, the hop.
 * vsig_isolate_offsets: the nseg + 1 prefix sums into a HOST array.
 * vsig_isolate_run takes DEVICE pointers: x (complex64[n]) and y (complex64[out_total]),
 *   both 8-byte aligned, not overlapping (a NULL or misaligned pointer: VSIG_E_INVALID
 *   before any work is enqueued).  It enqueues on the context stream, allocates nothing,
 *   never synchronises and can be captured into a graph; a plan with nseg == 0 does
 *   nothing.  x is read inside [0, n) only, y written at [0, out_total) exactly, each
 *   element once.  No atomics; the grid is a function of the table alone, so the same
 *   input gives the same bytes on every run.
 * vsig_isolate_free waits for the context stream, then frees the plan. */
typedef struct vsig_isolate_seg_t {
  int64_t start;    /* first capture index of the output range */
  int64_t len;      /* outputs */
  double freq;      /* the centre mixed down to 0, Hz (same unit as sr) */
  int32_t filter;   /* row of taps */
  int32_t pad;
} vsig_isolate_seg_t;
typedef struct vsig_isolate vsig_isolate;
int vsig_isolate_create(vsig_ctx* ctx, const vsig_isolate_seg_t* segs /*host*/, int64_t nseg, int64_t n,
                        const float* taps /*host float[nfilters*ntaps]*/, int32_t nfilters, int32_t ntaps,
                        double sr, vsig_isolate** out);
void vsig_isolate_free(vsig_isolate* plan);
int vsig_isolate_info(const vsig_isolate* plan, int64_t* out_total, int64_t* frames, int64_t* blocks,
                      int64_t* hop);
int vsig_isolate_offsets(const vsig_isolate* plan, int64_t* offsets /*host, nseg + 1*/);
int vsig_isolate_run(vsig_isolate* plan, const void* x, void* y);

/* ---- FIR: y[g] = sum_{m<ntaps} h[m] x[g*decim - m] (x = 0 outside [0, n)),
 * g in [0, ceil(n/decim)).  Taps complex64 on the host (real taps: imag = 0);
 * any ntaps >= 1 (np.convolve's contract, utils.py:802,816): up to 8192 one
 * overlap-save pass, beyond that 8192-tap parts run undecimated and summed with
 * their delays (a scratch of n samples). */
int vsig_fir_create(vsig_ctx* ctx, const void* taps, int32_t ntaps, int32_t decim, vsig_fir** out);
void vsig_fir_free(vsig_fir* fir);
/* Overlap-save block size M chosen for the taps (0 for a null handle). */
int vsig_fir_block(const vsig_fir* fir);
int vsig_fir_exec_dev(vsig_fir* fir, const void* x, int64_t n, void* y, int64_t ny);
/* Time-chunk form: x points at nhist history samples (the previous chunk's
 * last samples, the left halo) followed by the n samples to filter; y gets the
 * ceil(n/decim) outputs of those n samples, exactly as if the whole stream
 * had been filtered at once. */
int vsig_fir_exec_hist_dev(vsig_fir* fir, const void* x, int64_t nhist, int64_t n, void* y,
                           int64_t ny);
/* The same with the NCO mixer of apply_frequency_shift (utils.py:120-127)
 * fused into the FIR's loads: filters x[i] * exp(2j*pi*freq_shift*t_i),
 * t_i = (i0 + i) / sample_rate, i0 = global sample index of x[0] (the first
 * history sample), i.e. vsig_mix_c64_dev then vsig_fir_exec_hist_dev in one
 * pass.  freq_shift == 0: plain filter.  Needs the default FIR variant and
 * the 1024-point block (ntaps <= 256); else VSIG_E_UNSUPPORTED (mix first). */
int vsig_fir_exec_mix_dev(vsig_fir* fir, const void* x, int64_t nhist, int64_t n, void* y,
                          int64_t ny, double freq_shift, double sample_rate, int64_t i0);
int vsig_fir_c64(vsig_ctx* ctx, const void* x, int64_t n, const float* taps, int32_t ntaps,
                 int32_t decim, void* y, int64_t ny);
/* ---- streaming correlation with a fixed template p of L samples (any L >= 1;
 * L > 8192 runs as one pass per 8192-sample chunk, accumulated in c):
 * c[o] = sum_{k<L} s[o - off + k] conj(p[k]), mode VALID (off = 0, nout = n-L+1)
 * or FULL (off = L-1, nout = n+L-1).  c may be NULL (peak only).  peak_dev: a
 * device vsig_peak (may be NULL); peak = max |c|, sums over all nout outputs;
 * the peak / index are refined (see "refine" above).
 * Templates of 2049 .. 8192 samples run fastest where s - off is 16-byte
 * aligned (VALID: s itself; FULL: an odd L): the kernel then loads sample
 * pairs (parity split); any 8-byte aligned s is accepted and
 * gives the same record at the float bar. */
int vsig_xcorr_create(vsig_ctx* ctx, const void* tmpl, int64_t L, vsig_xcorr** out);
void vsig_xcorr_free(vsig_xcorr* xc);
int vsig_xcorr_exec_dev(vsig_xcorr* xc, const void* s, int64_t n, int32_t mode, void* c,
                        vsig_peak_t* peak_dev);

/* ---- template bank: K templates p_k of one length L (1 <= K <= 4096,
 * 1 <= L <= 4096) against one stream in one pass (xcorr_bank.hip):
 * c_k[o] = sum_{j<L} s[o - off + j] conj(p_k[j]), the stream transformed once
 * per block and its spectrum multiplied with the K template spectra in turn.
 * Serves the frequency search (one reference mixed at K offsets) and any
 * "which of these K packets, and where" question.
 * Record k is the UNREFINED fp32 result -- no exact re-rank runs on a bank
 * whatever the "refine" option says: index = the first maximum of the fp32
 * |c_k|^2, peak = its square root, the sums in double over per-wave fp32
 * partials (what "refine" = 0 gives a single template at M <= 8192).  A NaN
 * |c|^2 is never the maximum, and makes its own record's sums NaN.  The same
 * call gives the same bits twice, and record / row k does not depend on the
 * other templates of the bank.
 * Block size M: 4096 for L <= 1024, else 8192 (measured); the
 * option "xcorr_bank_m" (0: that rule; 4096 / 8192 / 16384 with L <= M / 2)
 * overrides it for banks created afterwards -- a measurement hook. */
/* tmpls: HOST complex64[K][L], row-major.  Spectra via make_spectrum, one per row. */
int vsig_xcorr_bank_create(vsig_ctx* ctx, const void* tmpls, int32_t K, int64_t L,
                           vsig_xcorr_bank** out);
/* the same from a DEVICE complex64[K][L] (the rows may be freed once the call returns) */
int vsig_xcorr_bank_create_dev(vsig_ctx* ctx, const void* tmpls_dev, int32_t K, int64_t L,
                               vsig_xcorr_bank** out);
void vsig_xcorr_bank_free(vsig_xcorr_bank* bank);
/* mode VALID / FULL as vsig_xcorr_exec_dev.  c: device complex64[K][nout] or NULL.
 * peaks_dev: device vsig_peak_t[K] (required).  Enqueued on the context stream, no sync. */
int vsig_xcorr_bank_exec_dev(vsig_xcorr_bank* bank, const void* s, int64_t n, int32_t mode, void* c,
                             vsig_peak_t* peaks_dev);
/* the geometry the exec will use, for tests and tools: M, hop (outputs per block),
 * nblocks = ceil(nout / hop), and the launched (persistent) grid: a launched block
 * walks blocks b, b + grid, ... */
int vsig_xcorr_bank_plan(const vsig_xcorr_bank* bank, int64_t n, int32_t mode, int32_t* M,
                         int64_t* hop, int64_t* nblocks, int64_t* grid);

/* ---- all-pairs burst similarity: which of K packets are the same packet sent again, and at
 * what offset (match.hip).  Packets p_0 .. p_{K-1}, complex64, lengths 1 <= L_k <= 8192,
 * packed back to back (p_k starts at the prefix sum of the lengths before it):
 *   E_k     = sum_j |p_k[j]|^2
 *   c_ab[l] = sum_j p_a[j + l] * conj(p_b[j]),  l in [-(L_b - 1), L_a - 1]
 *             (np.correlate(p_a, p_b, 'full'), l = index - (L_b - 1))
 *   peak[a,b] = max_l |c_ab[l]|,  lag[a,b] = the smallest l that attains it
 * so lag[a,b] = l says that p_b's first sample lines up with p_a[l], and
 * rho = peak / sqrt(E_a E_b) is in [0, 1].  For a < b the device computes the pair as
 * written; (b,a) is its mirror: the same peak bits and lag[b,a] = -lag[a,b].  The diagonal
 * is peak[a,a] = E_a rounded to float32, lag 0.  peak and lag are K x K row-major.
 * The transform length N is the smallest of 1024 / 4096 / 8192 / 16384 with
 * N >= 2 max(L_k) - 1.  One launch transforms every packet once into a K x N workspace the
 * plan owns (and writes E and the diagonal), a second walks units (a, up to 8 consecutive
 * b > a) on a persistent grid: the spectrum of a stays in registers, each b costs one
 * spectrum product, one transform and the first maximum of the fp32 |c|^2 over the pair's
 * valid lags only -- K + K(K-1)/2 transforms.  peak is v_sqrt of that maximum (1 ulp).
 * Special values are decided from the energies (each a double sum, in a fixed order, of
 * the fp32 |p|^2): if E_a or E_b is not finite (a NaN or Inf sample, or |p|^2 above
 * FLT_MAX) the pair's peak is NaN and its lag 0, the diagonal included; if either is 0 the
 * peak is 0 and the lag 0; every other pair's bytes are what they are without such a
 * packet in the list.  The fp32 |c|^2 itself overflows where sqrt(E_a E_b) reaches
 * 1.8e19 (sqrt(FLT_MAX)): constant-modulus packets of 8192 samples from an amplitude of
 * about 4.7e7, of 512 samples from 1.9e8; the spectra (|P| <= L max|p|) and their product
 * over N stay below that bound.  Past it a pair's peak is Inf or NaN and its lag
 * arbitrary; underflow (sqrt(E_a E_b) below ~1e-19) loses the peak to 0 the same way.
 * vsig_match_create validates everything before it touches the device, takes the lengths
 *   from the HOST, builds the offsets and the unit table on the device and may
 *   synchronise.  VSIG_E_INVALID: a NULL ctx / lens / out, K outside [1, 4096], a length
 *   below 1; VSIG_E_UNSUPPORTED: a length above 8192; the message names the offending
 *   packet.  The context option "match_grid" (0, the default: as many workgroups as the
 *   device holds at once; > 0: at most that many) caps the launched grid of plans created
 *   afterwards -- a measurement and test hook, so that one workgroup walks many units at a
 *   small K; it changes no output byte.
 * vsig_match_info: N, the pairs K(K-1)/2, the units, the launched grid, the workspace bytes.
 * vsig_match_run takes DEVICE pointers: packed (complex64[sum of lens], 8-byte aligned),
 *   peak (float[K*K]), lag (int32[K*K]), both 4-byte aligned, energy (double[K], 8-byte
 *   aligned); a NULL or misaligned pointer is VSIG_E_INVALID before any work is enqueued.
 *   It enqueues on the context stream, allocates nothing, never synchronises and can be
 *   captured into a graph.  packed is read at [0, sum of lens) only; peak, lag and energy
 *   are written exactly, each element once.  No atomics and a fixed walk order: the same
 *   input gives the same bytes on every run and from every plan, and a pair's record does
 *   not depend on the other packets of the list or on K, as long as a < b is kept and the
 *   list's longest packet asks for the same N.
 * vsig_match_free waits for the context stream, then frees the plan. */
typedef struct vsig_match vsig_match;
int vsig_match_create(vsig_ctx* ctx, const int64_t* lens /*host, K*/, int32_t K, vsig_match** out);
void vsig_match_free(vsig_match* plan);
int vsig_match_info(const vsig_match* plan, int32_t* N, int64_t* pairs, int64_t* units, int64_t* grid,
                    int64_t* workspace_bytes);
int vsig_match_run(vsig_match* plan, const void* packed, float* peak, int32_t* lag, double* energy);

/* ---- coherent averaging of an emitter's repeats: the bursts vsig_match_run found to be one
 * packet sent again, summed into one packet of up to M times the SNR, with a per-instance
 * SNR from the same sums (no reference counterpart).  K packets p_k (complex64, lengths
 * L_k >= 1) packed back to back; G groups; group[k] in [-1, G) (-1: not combined); lag[k] =
 * d_k, the match's lag[k, rep]: the representative's sample j lines up with p_k[j + d_k];
 * rep[g] a member of g with d = 0.  y_g, group g's output, has the representative's length
 * L_g and lives in its sample frame; the outputs are packed back to back in group order
 * (vsig_combine_offsets).  All ranges half open.
 * Estimate of member k against a reference v of length L_g and a prior frequency f0_k
 * (cycles per sample): the overlap is lo = max(0, -d_k), hi = min(L_g, L_k - d_k), n = hi -
 * lo; h = n / 2 (integer), m = lo + (n - 1) / 2;
 *   z[j] = p_k[j + d_k] * exp(-2j*pi*f0_k*(j - m)) * conj(v[j]),  j in [lo, hi)
 *   A1 = sum z over the first h samples, A2 over the rest; Ep1, Ep2 the same sums of
 *   |p_k[j + d_k]|^2, Ev1, Ev2 of |v[j]|^2;  Ep = Ep1 + Ep2, Ev = Ev1 + Ev2
 *   phi  = arg(A2 conj(A1))  (0 when A1 == 0 or A2 == 0)
 *   freq = f0_k + phi / (pi n)               the halves' centres are n / 2 apart
 *   B    = A1 exp(+j phi/2) + A2 exp(-j phi/2)
 *   a    = B / Ev                            the complex gain at the overlap's centre
 *   rho  = |B| / sqrt(Ep Ev)
 *   res  = Ep - (|A1|^2 / Ev1 + |A2|^2 / Ev2)     a term whose Ev is 0 is dropped
 * used = n > 0, every sum finite, Ev > 0 and rho >= min_rho (an all-zero member has rho
 * 0/0 and is not used); otherwise a = 0, freq = f0_k, rho = 0 (NaN if a sum is not
 * finite).  n, m, Ep, Ev and res are written as computed either way; a packet in group -1
 * has used = 0, n = 0, freq = f0_k and every other field 0.  With ref == NULL the reference
 * is the representative inside packed, and the representative's own record is a = 1, freq =
 * 0, rho = 1, res = 0, used = 1 by definition (Ep = Ev = its energy).
 * Sum (maximum-ratio combining), j in [0, L_g):
 *   y_g[j] = sum_k conj(a_k) exp(-2j*pi*freq_k*(j - m_k)) p_k[j + d_k] / sum_k |a_k|^2
 * both sums over the used members of g that cover j (0 <= j + d_k < L_k), in ascending k;
 * 0 where none does.  freq == 0 and a == 1 multiply nothing and a denominator of 1 divides
 * nothing, so a group of one member gives back its packet's bytes.
 * Arithmetic: the products of the estimate are fp32 (uncontracted: p against itself has an
 * imaginary part of exactly 0), widened to double and added in double in a fixed order in
 * chunks of S = 2048 samples of the overlap (vsig_combine_info's chunk), one fixed-slot
 * partial a chunk in the plan's workspace, then per member in chunk order; the rotations
 * are fp32 on a phase formed in double; the sum accumulates in fp32.  No atomics: a record
 * is a function of its member, its reference, f0 and S, an output sample of its group's
 * members, and neither depends on K, on the other groups or on the grid.
 * vsig_combine_create validates everything before it touches the device, takes all four
 *   lists from the HOST, builds the member, group and item tables on the device and may
 *   synchronise.  VSIG_E_INVALID, the message naming the offending packet or group: a NULL
 *   pointer, K outside [1, 4096], G outside [1, K], a length below 1, a group id outside
 *   [-1, G), a representative that is not a member of its group or whose lag is not 0;
 *   VSIG_E_UNSUPPORTED: 2^31 packed samples or more.  A lag beyond every length is valid
 *   (no overlap).
 * vsig_combine_info: the packed output's length, S, the estimate items (one per member and
 *   chunk of its overlap), the sum items (one per group and chunk of 512 samples of its
 *   output) and the workspace bytes (64 an estimate item).
 * vsig_combine_offsets: the G + 1 prefix sums of the outputs into a HOST array.
 * vsig_combine_estimate and vsig_combine_sum take DEVICE pointers, all 8-byte aligned:
 *   packed (complex64[sum of lens]), ref (NULL, or complex64[out_total] in the output
 *   layout), f0 (NULL = 0, or double[K]), records ([K]), y (complex64[out_total]); a NULL
 *   packed / records / y, a misaligned pointer or a NaN min_rho is VSIG_E_INVALID before
 *   any work is enqueued.  They enqueue on the context stream, allocate nothing, never
 *   synchronise and can be captured into a graph.  Inputs are read inside their extents
 *   only; estimate writes every record whole (80 bytes, pad 0), sum every element of y
 *   once.  Every address is formed from the plan's tables, never from a record's fields.
 *   Two estimates of one plan share its workspace: they run in stream order.
 * vsig_combine_free waits for the context stream, then frees the plan. */
typedef struct vsig_combine_member_t {
  double a_re, a_im; /* complex gain against the reference at the overlap's centre */
  double freq;       /* cycles per sample */
  double m;          /* the overlap's centre lo + (n - 1) / 2, in the group's frame */
  double rho;        /* normalised correlation with the reference, in [0, 1] */
  double Ep, Ev;     /* the member's and the reference's energy over the overlap */
  double res;        /* Ep minus what the two-half fit explains */
  int64_t n;         /* overlap, samples */
  int32_t used;      /* 1: part of the sum */
  int32_t pad;
} vsig_combine_member_t;
typedef struct vsig_combine vsig_combine;
int vsig_combine_create(vsig_ctx* ctx, const int64_t* lens /*host, K*/, const int32_t* group /*host, K, -1 = none*/,
                        const int64_t* lag /*host, K*/, int32_t K, const int32_t* rep /*host, G*/, int32_t G,
                        vsig_combine** out);
void vsig_combine_free(vsig_combine* plan);
int vsig_combine_info(const vsig_combine* plan, int64_t* out_total, int32_t* chunk /*S*/, int64_t* est_items,
                      int64_t* sum_items, int64_t* workspace_bytes);
int vsig_combine_offsets(const vsig_combine* plan, int64_t* offsets /*host, G + 1*/);
int vsig_combine_estimate(vsig_combine* plan, const void* packed, const void* ref, const double* f0,
                          double min_rho, vsig_combine_member_t* records);
int vsig_combine_sum(vsig_combine* plan, const void* packed, const vsig_combine_member_t* records, void* y);

/* ---- general correlation, np.correlate(a, v, mode) semantics for any length
 * order (cross_correlate_signals, utils.py:1279-1285): output length full
 * na+nv-1, valid |na-nv|+1, same max(na, nv).  The FFT pass runs in complex64;
 * dtype VSIG_DTYPE_C128 takes complex128 operands (converted for the FFT pass,
 * kept for the refine pass), out_dtype VSIG_DTYPE_C128 writes c as complex128
 * with the refined outputs patched in (exact near the peak, fp32 accuracy
 * elsewhere).  The shorter operand up to 8192 samples runs as one streaming
 * pass; longer ones as a sum over 8192-sample chunks of it (one pass per
 * chunk, accumulated in c -- a device scratch c when c is NULL).  All pointers
 * device (dev) or host.  The _c64 forms are dtype = out_dtype = C64. */
int vsig_correlate_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t na, const void* v,
                       int64_t nv, int32_t mode, int32_t out_dtype, void* c, vsig_peak_t* peak_dev);
int vsig_correlate(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t na, const void* v,
                   int64_t nv, int32_t mode, int32_t out_dtype, void* c, vsig_peak_t* peak);
int vsig_correlate_c64_dev(vsig_ctx* ctx, const void* a, int64_t na, const void* v, int64_t nv,
                           int32_t mode, void* c, vsig_peak_t* peak_dev);
int vsig_correlate_c64(vsig_ctx* ctx, const void* a, int64_t na, const void* v, int64_t nv,
                       int32_t mode, void* c, vsig_peak_t* peak);

/* ---- transforms of any length (bigfft.hip; complex64 arithmetic).
 * vsig_dft_dev, vsig_resample_dev and vsig_filter_channel_dev run a power of
 * two from 256 to 16384 points as one in-LDS transform of that length, a power
 * of two from 2^15 to 2^28 points as one four-step FFT of that length on the
 * in-LDS engine, every other length up to 512 points (the powers of two below
 * 256 included) as the sum itself in double precision, and every other length
 * from 513 to 2^27 points as a Bluestein / chirp-z convolution of M >= 2n - 1
 * points.
 * vsig_dft_dev: batch frames of n contiguous samples, y[f][k] = sum_j x[f][j]
 *   e^{-+2 pi i jk/n} (inverse: + and 1/n, numpy.fft's convention).
 * vsig_resample_dev: scipy.signal.resample(x, num) as resample_signal calls it
 *   (utils.py:107-118): spectrum of x, its bins copied / the Nyquist bin split
 *   or folded into num bins, inverse transform, * num / n; y complex64[num]
 *   (real_input: imaginary part 0, scipy's rfft path).
 * vsig_filter_channel_dev: split_channels.filter_channel (vector_analyzer/
 *   split_channels.py:15-44) as written, CENTER_FREQ 5230 MHz: brick-wall mask
 *   on fftfreq(n, 1/sr) * sr + CENTER_FREQ, the negative half replaced by the
 *   conjugate mirror of the masked non-negative half, inverse FFT, real part
 *   (y float64[n]).  Odd n > 1: VSIG_E_INVALID (numpy's shape mismatch). */
int vsig_dft_dev(vsig_ctx* ctx, int32_t dtype, const void* x, int64_t n, int64_t batch,
                 int32_t inverse, int32_t out_dtype, void* y);
int vsig_resample_dev(vsig_ctx* ctx, int32_t dtype, const void* x, int64_t n, int64_t num,
                      int32_t real_input, void* y);
int vsig_filter_channel_dev(vsig_ctx* ctx, int32_t dtype, const void* x, int64_t n,
                            double center_freq, double sample_rate, double bandwidth, double* y);

/* ---- |c| reduction in double precision over an array of dtype VSIG_DTYPE_*:
 * index of the first max of |c|, the max, sum |c|, sum |c|^2. */
int vsig_peak_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, vsig_peak_t* peak_dev);
int vsig_peak(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, vsig_peak_t* peak);
/* find_correlation_peak's mean_corr / std_corr (utils.py:1329-1330) exactly as
 * numpy forms them: np.mean(np.abs(a)) and np.std(np.abs(a)) in float64, by
 * numpy's pairwise summation over 8192-element buffers (two passes).
 * stats_dev: device double[2] = {mean, std}.  dtype VSIG_DTYPE_C128 or
 * VSIG_DTYPE_F64 (cross_correlate_signals' output is complex128). */
int vsig_abs_stats_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, double* stats_dev);
/* The same statistics of |np.correlate(a, v, mode)| without the correlation
 * array: every output evaluated in numpy's operation order (the refine pass's
 * dense form; O(nout x min(na, nv)) fp64 FMAs, about 1 ms per 2^20 outputs x
 * 4096 terms) -- the exact confidence for a flat |c|, where the fused
 * correlators' fp32 sums cannot resolve numpy's rounding-noise std. */
int vsig_correlate_stats_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t na, const void* v,
                             int64_t nv, int32_t mode, double* stats_dev);
/* validate_transplant_quality's three mean powers (utils.py:1546-1552) in one
 * pass over two complex64 regions: sums_dev = device double[3] =
 * { sum |a|^2, sum |b|^2, sum |a-b|^2 }, each |.|^2 formed in float32 as numpy
 * forms np.abs(x)**2, summed in double in a fixed order.  Enqueued on the
 * context stream, no synchronisation; the same operands give the same bits on
 * every run.  a and b are 8-byte aligned (any slice of a complex64 array) and
 * may be the same array.  n < 1, a NULL pointer or an operand off an 8-byte
 * boundary: VSIG_E_INVALID. */
int vsig_region_power_dev(vsig_ctx* ctx, const void* a, const void* b, int64_t n, double* sums_dev);

/* ---- stream ops either side of the chain.
 * vsig_mix_c64_dev: y[i] = x[i] * exp(j w (i0 + i) / sr) — apply_frequency_shift
 *   (utils.py:120-127) with w = 2*pi*freq_shift as numpy forms it.
 * vsig_scale_c64_dev: y = x * s (transplant_packet_in_vector power scale,
 *   utils.py:1481-1496).
 * vsig_wv_quantize_dev: SMU-WV int16 I/Q interleave of mat2wv
 *   (vector_analyzer/mat_to_wv_converter.py:28-50); norm > 0 divides by norm
 *   first (bNormalize, norm = max |x|); out holds 2n int16.
 * vsig_planar_to_c64_dev: MAT v5 real / imaginary planes of storage type
 *   mi_type (miINT8 1 .. miDOUBLE 9, miINT64 12, miUINT64 13; im may be NULL)
 *   -> complex64 (load_packet, utils.py:48-86).
 * vsig_c64_to_planar_dev: complex64 -> float32 planes (save_vector,
 *   utils.py:659-670). */
int vsig_mix_c64_dev(vsig_ctx* ctx, const void* x, int64_t n, double w, double sr, int64_t i0,
                     void* y);
int vsig_scale_c64_dev(vsig_ctx* ctx, const void* x, int64_t n, float s, void* y);
int vsig_wv_quantize_dev(vsig_ctx* ctx, const void* x, int64_t n, float norm, int16_t* out);
int vsig_planar_to_c64_dev(vsig_ctx* ctx, int32_t mi_type, const void* re, const void* im,
                           int64_t n, void* y);
int vsig_c64_to_planar_dev(vsig_ctx* ctx, const void* x, int64_t n, float* re, float* im);

/* ---- vector assembly: generate_vector's insert loop and peak normalise
 * (unified_gui.py:1692-1791, older form main.py:214-284).
 * vsig_vector_build_dev: out (device complex64[n], 8-byte aligned) = the
 *   zeroed vector after  vector[a:b] += y  for every place in list order and
 *   every instance k = 0 .. count-1 at a = start + k*period, b = a + len
 *   (unified_gui.py:1756-1769): the same fp32 adds in the same order, numpy's
 *   result to the bit.  places is a host array (read before the call returns);
 *   each y is the packet as inserted (already mixed).  Every place needs
 *   y != NULL, len >= 1, period >= 1, count >= 0, start >= 0 and, when
 *   count >= 1, start + (count-1)*period + len <= n (the reference inserts no
 *   cut-off instance); n <= 2^40.  Anything else: VSIG_E_INVALID before any
 *   work is enqueued.  No places, or every count 0: out is all zeros.
 *   maxabs_dev (may be NULL): a device float that receives
 *   np.max(np.abs(out)) (numpy's complex64 abs; unified_gui.py:1779).
 * vsig_normalize_c64_dev: y = x / m, m = *maxabs_dev read on the device, as
 *   numpy divides a complex64 array by a float32 (unified_gui.py:1780-1781);
 *   y = x when m is not > 0.  y may be x.
 * Both enqueue on the context stream and never synchronise (capturable). */
typedef struct vsig_packet_place {
  const void* y;      /* device complex64[len], as inserted */
  int64_t len, start, period, count;   /* instance k at start + k*period, k < count */
} vsig_packet_place;
int vsig_vector_build_dev(vsig_ctx* ctx, const vsig_packet_place* places /*host*/, int32_t nplaces,
                          void* out, int64_t n, float* maxabs_dev /*may be NULL*/);
int vsig_normalize_c64_dev(vsig_ctx* ctx, const void* x, int64_t n, const float* maxabs_dev, void* y);

/* ---- polyphase channelizer (BASELINE config 4; no reference counterpart,
 * nearest analogue vector_analyzer/split_channels.py:15-44):
 * y[m*nchan + k] = sum_p z_m[p] e^{-2 pi j k p / nchan},
 * z_m[p] = sum_q h[q*nchan + p] x[(m + q)*nchan + p];
 * nchan in {64, 128, 256}, ntaps = {4, 8, 16} * nchan,
 * nframes = (n - ntaps) / nchan + 1; y frame-major (nframes x nchan). */
int vsig_pfb_c64_dev(vsig_ctx* ctx, const void* x, int64_t n, const float* h, int32_t ntaps,
                     int32_t nchan, void* y, int64_t nframes);
/* the geometry the call will use, for tests and tools: a launched block holds
 * groups_per_block lane groups, group g of the grid owns the frames
 * [g * frames_per_group, (g + 1) * frames_per_group); blocks = the grid for nframes.
 * No context needed.  Another nchan / ntaps than above: VSIG_E_UNSUPPORTED. */
int vsig_pfb_plan(int32_t nchan, int32_t ntaps, int64_t nframes, int64_t* frames_per_group,
                  int64_t* groups_per_block, int64_t* blocks);

/* ---- analysis (normalize_spectrogram utils.py:356-404, find_packet_start /
 * detect_packet_bounds utils.py:784-825).  All operate on |a|.
 * vsig_select_dev: k-th smallest |a| for up to 4 0-based ranks (host output;
 *   np.percentile / np.median are interpolations of these).
 * vsig_threshold_dev: count / first / last index of |a| >= thr and max |a|.
 * vsig_boxcar_energy_dev: sm = np.convolve(np.abs(x)**2, ones(w)/w, 'same')
 *   in double (x of any VSIG_DTYPE; sm: max(n, w) doubles on the device).
 * vsig_db_dev: out = 10 log10(|a| + floor), F32 -> float32 math and output,
 *   F64 -> double (numpy's promotion in normalize_spectrogram).
 * vsig_abs_c64_dev / vsig_abs_c128_dev: out = |a| + 0j as complex64 / complex128
 *   (a of any VSIG_DTYPE; np.abs as numpy forms it). */
int vsig_select_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, const int64_t* ranks,
                    int32_t nranks, double* values);
int vsig_threshold_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, double thr,
                       int64_t* count, int64_t* first, int64_t* last, double* maxval);
int vsig_boxcar_energy_dev(vsig_ctx* ctx, int32_t dtype, const void* x, int64_t n, int64_t w,
                           double* sm);
int vsig_db_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, double floor_, void* out);
int vsig_abs_c64_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, void* out);
int vsig_abs_c128_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, void* out);

/* ---- display image: the pixels the reference's three plot sites draw --
 * plot_spectrogram (utils.py:429-449, 491-499: percentiles 5 / 95, the
 * (2, 1) median filter, turbo / inferno), adjust_packet_bounds_gui
 * (utils.py:1017-1022, 1062: 10 / 95, viridis, rows flipped) and
 * vector_analyzer/spectrogram_analysis.py:56-62 (10 / 95, viridis) -- from
 * Sxx in one pass, with no dB map in between.
 * sxx: n_freq x n_time values of dtype VSIG_DTYPE_F32 or VSIG_DTYPE_F64;
 *   freq_fast != 0: frame-major memory, element (i, j) at sxx[j*ld + i]
 *   (ld >= n_freq); freq_fast == 0: C-contiguous, (i, j) at sxx[i*ld + j]
 *   (ld >= n_time).  ld counts elements, so a slice along either axis is
 *   rendered in place.  Rows that start on 16-byte boundaries (base and
 *   ld * itemsize multiples of 16) are read with 16-byte loads.
 * Pixel (r, c) of the ceil(n_freq / pool_f) x ceil(n_time / pool_t) image:
 *   P  = max |sxx(i, j)| over i in [max(r*pool_f - (median != 0), 0),
 *        min((r+1)*pool_f, n_freq)), j in [c*pool_t, min((c+1)*pool_t, n_time))
 *        (the median filter of size (2, 1) is the maximum of rows i-1 and i,
 *        row 0 with itself; peak-hold pooling has no reference counterpart);
 *        a NaN anywhere in the window makes P NaN;
 *   db = 10 log10(P + floor), rounded as vsig_db_dev rounds it;
 *   xa = (db - vmin) / (vmax - vmin) * 256 in the input's dtype (matplotlib's
 *        Normalize); table row: bad if xa is NaN, under if xa < 0, 255 if
 *        xa == 256, over if xa > 256, else trunc(xa) (Colormap.__call__).
 * lut_dev: 259 x 4 bytes on the device -- rows 0..255, under, over, bad
 *   (matplotlib's _lut order); rgba_dev: rows * cols * 4 bytes, C-contiguous
 *   [rows][cols][4]; with flip_freq output row r holds frequency block
 *   rows - 1 - r.  Both 4-byte aligned.
 * Enqueued on the context stream, no synchronisation; the same input gives
 * the same bytes on every run.  A NULL pointer, an extent or pool factor
 * below 1, ld below the fast extent, another dtype, a misaligned table or
 * image, vmax <= vmin (also after rounding to float for F32) or a level that
 * is not finite: VSIG_E_INVALID. */
int vsig_spectrogram_image_dev(vsig_ctx* ctx, int32_t dtype, const void* sxx, int64_t n_freq,
                               int64_t n_time, int32_t freq_fast, int64_t ld, double floor_,
                               double vmin, double vmax, int32_t median, int32_t flip_freq,
                               int32_t pool_f, int32_t pool_t, const uint8_t* lut_dev,
                               uint8_t* rgba_dev);

/* ---- peak list: every packet instance in a stored correlation (or the peaks
 * of any array of dtype VSIG_DTYPE_*), where the entry points above stop at
 * the one global argmax.  With m[i] = |a[i]| as vsig_peak_dev forms it
 * (numpy's abs in the array's precision, widened to double), index i is an
 * instance iff m[i] >= thr and i is the FIRST maximum of m over
 * [max(0, i - min_distance), min(n - 1, i + min_distance)]; in numpy
 * lo + np.argmax(m[lo:hi+1]) == i.  So two instances are more than
 * min_distance apart, min_distance = 0 is plain threshold compaction, a flat
 * array has the one instance 0, and a peak with a higher neighbour within
 * min_distance is dropped even if that neighbour is dropped too (a maximum
 * filter, not a greedy selection).  thr is absolute, or with relative != 0 a
 * ratio: thr_used = thr * max(m), one double multiply on the device.
 * out: the instances in ascending index order, at most cap records (the cap
 *   lowest-index ones when there are more); may be NULL when cap == 0 (count
 *   only).  Records past min(count, cap) are not written.
 * info: always written; count is the exact number of instances whatever cap.
 * The same input gives the same bytes on every run.  Cost: one pass over the
 * array plus O(n log min_distance) compares in the worst case (every element
 * above thr), nothing proportional to n * min_distance.
 * n < 1, n > 2^40, cap < 0, min_distance < 0, a NULL a / info, a NULL out with
 * cap > 0, an unknown dtype or a NaN thr: VSIG_E_INVALID before any work is
 * enqueued.  Arrays that hold NaN are outside the contract: a NaN element is
 * never an instance and never suppresses one, and all writes stay inside
 * out[0..cap) and info.
 * vsig_peaks_dev enqueues on the context stream, allocates nothing once its
 * scratch is warm for n and never synchronises (capturable).  vsig_peaks takes
 * host pointers (a, out, info) and returns when they are filled.
 * vsig_peaks_tile: the kernels' tile length (elements); min_distance below it
 * and from it upward take different paths. */
typedef struct vsig_instance_t {
  int64_t index;
  double value;      /* |a[index]| */
} vsig_instance_t;
typedef struct vsig_peaks_info_t {
  int64_t count;     /* instances in the array */
  int64_t argmax;    /* index of the first max of |a| */
  double max;        /* max |a| */
  double thr_used;   /* the threshold applied */
} vsig_peaks_info_t;
int vsig_peaks_tile(void);
int vsig_peaks_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, double thr,
                   int32_t relative, int64_t min_distance, vsig_instance_t* out_dev, int64_t cap,
                   vsig_peaks_info_t* info_dev);
int vsig_peaks(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
               int64_t min_distance, vsig_instance_t* out, int64_t cap, vsig_peaks_info_t* info);

/* ---- run list: every burst of an array, where vsig_threshold_dev stops at the
 * first and last index above the threshold.  With m[i] = |a[i]| as
 * vsig_peak_dev forms it (numpy's abs in the array's precision, widened to
 * double; any VSIG_DTYPE_*) and mask[i] = m[i] >= thr, a run is a maximal
 * interval [start, end] (end inclusive) whose two ends are in the mask and in
 * which no stretch of more than max_gap consecutive elements is outside it.
 * Per index: a masked i is a start iff the previous masked index p (or -inf)
 * has i - p > max_gap + 1, an end iff the next masked index q (or +inf) has
 * q - i > max_gap + 1; the k-th start pairs with the k-th end.  In numpy:
 *   idx = np.flatnonzero(m >= thr); brk = np.flatnonzero(np.diff(idx) > max_gap + 1)
 *   start = idx[np.r_[0, brk + 1]]; end = idx[np.r_[brk, idx.size - 1]]
 * So max_gap = 0 gives the plain runs of the mask, any max_gap >= n at most
 * the one run [first, last] of vsig_threshold_dev, and start[0] / end[-1]
 * never depend on max_gap.  thr is absolute, or with relative != 0 a ratio:
 * thr_used = thr * max(m), one double multiply on the device.
 * Per run: max / argmax the first maximum of m over [start, end] (gaps
 *   included), sum = the sum of m over [start, end] in double, in a fixed order.
 * out: the runs in ascending order, at most cap records (the cap lowest-index
 *   ones when there are more); may be NULL when cap == 0 (count only).
 *   Records past min(count, cap) are not written.
 * info: always written; count is the exact number of runs whatever cap,
 *   covered the number of masked elements, argmax / max those of the array.
 * The same input gives the same bytes on every run.  Cost: one pass over the
 * array, a second read of the tiles that hold both masked and unmasked
 * elements, and per run its two end tiles; nothing proportional to max_gap.
 * n < 1, n > 2^40, cap < 0, max_gap < 0, a NULL a / info, a NULL out with
 * cap > 0, an unknown dtype or a NaN thr: VSIG_E_INVALID before any work is
 * enqueued.  Arrays that hold NaN are outside the contract: a NaN element is
 * not masked, and all writes stay inside out[0..cap) and info.
 * vsig_runs_dev enqueues on the context stream, allocates nothing once its
 * scratch is warm for n and never synchronises (capturable).  vsig_runs takes
 * host pointers (a, out, info) and returns when they are filled.
 * vsig_runs_tile: the kernels' tile length (elements). */
typedef struct vsig_run_t {
  int64_t start;     /* first index of the run */
  int64_t end;       /* last index of the run (inclusive) */
  int64_t argmax;    /* index of the first max of |a| over [start, end] */
  double max;        /* that maximum */
  double sum;        /* sum of |a| over [start, end] */
} vsig_run_t;
typedef struct vsig_runs_info_t {
  int64_t count;     /* runs in the array */
  int64_t covered;   /* elements with |a| >= thr_used */
  int64_t argmax;    /* index of the first max of |a| */
  double max;        /* max |a| */
  double thr_used;   /* the threshold applied */
} vsig_runs_info_t;
int vsig_runs_tile(void);
int vsig_runs_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
                  int64_t max_gap, vsig_run_t* out_dev, int64_t cap, vsig_runs_info_t* info_dev);
int vsig_runs(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, double thr, int32_t relative,
              int64_t max_gap, vsig_run_t* out, int64_t cap, vsig_runs_info_t* info);

/* ---- line traces: the lines the reference draws beside every spectrogram --
 * np.abs(signal) over time (utils.py:551-554, 853-856, 939, 1090) and the
 * magnitude, or 20 log10 of it, of a whole-capture spectrum over frequency
 * (vector_analyzer/spectrogram_analysis.py:9-30, analyze_channels.py:6-25,
 * analyze_vectors.py:17-40, display_vectors.py:26-35, mat_analyzer.py:202-215)
 * -- reduced on the device to what a plot axis can show: a min / max envelope
 * per pixel column.
 * m[i] = |a[i]| exactly as vsig_peak_dev forms it: for complex input numpy's
 *   abs in the array's own precision (npabs.hpp), for real input fabs.  dtype
 *   is any VSIG_DTYPE_*.
 * Position p in [0, n) reads s[p] = m[(p + rot) % n]; with shift != 0
 *   rot = (n + 1) / 2, which is np.fft.fftshift for even and odd n; without,
 *   rot = 0.
 * cols = ceil((hi - lo) / bin); column c covers p in
 *   [lo + c*bin, min(lo + (c+1)*bin, hi)).
 * E_min[c] / E_max[c]: the minimum / maximum of s over the column; a NaN
 *   anywhere in the column makes both NaN (np.min / np.max of that column).
 * Stored, by kind:
 *   VSIG_TRACE_ABS   E itself;
 *   VSIG_TRACE_DB20  20 * log10(E + eps) of the envelope values: the map is
 *     applied to the 2 * cols results, not per element (log10 and + eps are
 *     monotone, so the envelope of the mapped line is the mapped envelope).
 *     Every step is rounded in the output dtype, as vsig_db_dev rounds
 *     (dbmath.hpp db20_of beside db_of); E + eps == 0 gives -inf.
 *   At bin = 1 this is the reference's line itself, otherwise its envelope.
 * Output dtype follows the input: C64 / F32 give float32, C128 / F64 float64.
 * env_min_dev / env_max_dev hold cols values each; env_min_dev may be NULL
 *   (bin = 1, where the two planes are equal, or a max-only trace).
 * info (may be NULL), over [lo, hi): argmax / argmin are the first position p
 *   of the maximum / minimum of s, in the shifted coordinate and not offset by
 *   lo; max / min are the stored (mapped) values there.  Arrays that hold NaN
 *   are outside info's contract; all writes stay inside the three outputs.
 * The call enqueues on the context stream, never synchronises, allocates
 * nothing once its scratch is warm for (n, cols), is capturable, and gives the
 * same bytes for the same input on every run.  a may be any slice of an array
 * at its element's natural alignment (16-byte loads are used from the first
 * 16-byte boundary on).
 * n < 1, n > 2^40, lo < 0, hi > n, lo >= hi, bin < 1, a NULL a or env_max_dev,
 * an unknown dtype or kind, eps < 0 or not finite: VSIG_E_INVALID before any
 * work is enqueued. */
#define VSIG_TRACE_ABS  0   /* |a| */
#define VSIG_TRACE_DB20 1   /* 20 log10(|a| + eps) */
typedef struct vsig_trace_info_t {
  int64_t argmin, argmax;
  double min, max;
} vsig_trace_info_t;
int vsig_trace_envelope_dev(vsig_ctx* ctx, int32_t dtype, const void* a, int64_t n, int32_t shift,
                            int64_t lo, int64_t hi, int64_t bin, int32_t kind, double eps,
                            void* env_min_dev /* may be NULL */, void* env_max_dev,
                            vsig_trace_info_t* info_dev /* may be NULL */);

/* ---- time-chunk shard of the streaming chain (chain.hip; the C form of
 * vector_amd/shard.py StreamChain; reference precedent: the
 * overlapped chunking of heavy_packet_optimizer.py:114-152).  Rank r of world
 * owns input samples [r n, (r+1) n) of one capture; per step: left halo
 * (hist = ntaps-1 input samples rounded up to a multiple of 16, so that the
 * FIR's segments start on 128-byte lines: the last hist samples of rank r-1;
 * world > 1 needs n >= hist) -> FIR + decimate -> right halo (L-1
 * filtered samples from rank r+1) -> PSD (nfft, hop nfft) -> valid
 * correlation with the template + exact peak -> all-gather of the 32-byte
 * peak records.  Results equal one chain over the whole capture.
 * n must be a multiple of nfft * decim; taps / tmpl complex64 host arrays;
 * window float32[nfft] host; psd_scale = 1 / sum(window)^2 for 'spectrum'
 * scaling; tmpl = NULL: no sync stage. */
typedef struct vsig_chain_config {
  int64_t n_local;
  const void* taps;
  int32_t ntaps;
  int32_t decim;
  int32_t nfft;
  const float* window;
  float psd_scale;
  const void* tmpl;
  int64_t L;
} vsig_chain_config;

/* How ranks exchange: sendrecv sends send_bytes of device memory to rank dst
 * and receives recv_bytes into recv from rank src (dst / src < 0: none),
 * ordered on hip_stream; allgather gathers `bytes` from every rank into recv
 * (world * bytes, rank order).  Return 0 on success. */
typedef struct vsig_transport {
  void* user;
  int (*sendrecv)(void* user, const void* send, int64_t send_bytes, int32_t dst, void* recv,
                  int64_t recv_bytes, int32_t src, void* hip_stream);
  int (*allgather)(void* user, const void* send, void* recv, int64_t bytes, void* hip_stream);
} vsig_transport;

typedef struct vsig_chain vsig_chain;
/* tr may be NULL for world = 1.  The chain enqueues on ctx's stream. */
int vsig_chain_create(vsig_ctx* ctx, const vsig_chain_config* cfg, int32_t rank, int32_t world,
                      const vsig_transport* tr, vsig_chain** out);
void vsig_chain_free(vsig_chain* chain);
const char* vsig_chain_last_error(const vsig_chain* chain);
/* Device complex64[n_local]: this rank's input chunk (fill before a step). */
void* vsig_chain_input(vsig_chain* chain);
int vsig_chain_step(vsig_chain* chain);
/* The global peak of the last step (index in the whole filtered, decimated
 * capture; sums over all nout outputs); synchronises. */
int vsig_chain_result(vsig_chain* chain, vsig_peak_t* peak, int64_t* nout);
/* This rank's filtered stream (complex64[n]) and spectra (frame-major float32
 * [nframes][nfft]) on the device. */
const void* vsig_chain_filtered(const vsig_chain* chain, int64_t* n);
const float* vsig_chain_spectra(const vsig_chain* chain, int64_t* nframes);

/* RCCL over xGMI as the transport (librccl resolved at run time: an RCCL
 * already in the process -- e.g. torch's -- is shared; VSIG_RCCL_LIB names
 * another).  comm is an ncclComm_t; vsig_rccl_comm_init makes one per rank
 * from a unique id that rank 0 creates and the launcher distributes. */
int vsig_rccl_available(void);
int vsig_rccl_unique_id(char id[128]);
int vsig_rccl_comm_init(int32_t world, int32_t rank, const char id[128], int32_t device, void** comm);
int vsig_rccl_comm_destroy(void* comm);
int vsig_rccl_transport(void* comm, vsig_transport* out);

/* In-process loopback transport: ranks as host threads of one process (one
 * context each), halos copied device to device -- several ranks on one GPU
 * for tests, or ranks on the GPUs of one process. */
typedef struct vsig_loopback vsig_loopback;
int vsig_loopback_create(int32_t world, vsig_loopback** out);
void vsig_loopback_free(vsig_loopback* lb);
int vsig_loopback_transport(vsig_loopback* lb, int32_t rank, vsig_transport* out);

#ifdef __cplusplus
}
#endif
#endif /* VSIG_H */
