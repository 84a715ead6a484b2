// Coherent averaging of an emitter's repeats (gfx950): K packets p_k packed
// back to back, G groups of them, every member k with a lag d_k against its
// group's representative (whose sample j lines up with p_k[j + d_k]).  Group
// g's output y_g lives in its representative's sample frame, [0, L_g).
//
//   combine_estimate_kernel  an item is (member, chunk of S = kCombineChunk
//     samples of its overlap [lo, lo + n) with the frame).  Against the
//     reference v (the representative, or a caller's y) and a prior frequency
//     f0 (cycles per sample) it forms, with m = lo + (n - 1) / 2 and h = n / 2,
//       z[j] = p_k[j + d_k] exp(-2 pi i f0 (j - m)) conj(v[j])
//     and the chunk's share of six sums: A1 = sum z over the overlap's first h
//     samples, A2 over the rest, and the same two sums of |p_k|^2 and |v|^2.
//     Products are fp32 (contraction off, so p against itself gives |p|^2 and an
//     imaginary part of exactly 0), widened to double and added in double in a
//     fixed order: per thread in element order, then the block's threads by
//     block_fold (block_ops.hpp).  The rotation is cis_rev on a phase formed
//     in double, once per sample; f0 == 0 rotates nothing.  One fixed-slot
//     partial per item; the items of one stretch of the reference are adjacent
//     in the table, so it comes from L2 after its first read.
//   combine_finalize_kernel  one thread per packet adds its partials in chunk
//     order and writes the member record: phi = arg(A2 conj A1), freq = f0 +
//     phi / (pi n), the gain a and the correlation rho at the overlap's centre,
//     the energies and the residual (see include/vsig.h).
//   combine_sum_kernel       an item is (group, chunk of kCombineSumChunk = 512
//     outputs); a thread owns two of them and walks the group's members in
//     ascending order:
//       y[j] = sum_k conj(a_k) exp(-2 pi i freq_k (j - m_k)) p_k[j + d_k] / sum_k |a_k|^2
//     over the used members that cover j, numerator and denominator in fp32,
//     written once.  freq == 0 and a == 1 multiply nothing, the first term is
//     stored, not added to zero, and a denominator of 1 divides nothing: a
//     group of one member gives back its packet's bytes.
//
// No atomics; a record is a function of its member, its reference, f0 and S, an
// output sample of its group's members; neither depends on K, the other groups
// or the grid.  Member loads are 8-byte loads (d_k shifts them by any number of
// samples).  Every address comes from the plan's tables, never from a record.
#include "block_ops.hpp"

namespace vsig {

namespace {

constexpr int CT = 256;                          // threads per block
constexpr int CV = kCombineChunk / CT;           // samples per thread and item
constexpr int SV = kCombineSumChunk / CT;        // outputs per thread and sum item
static_assert(kCombineChunk % CT == 0 && kCombineSumChunk % CT == 0, "a chunk is a whole number of block strides");
constexpr int CW = CT / 64;

#pragma clang fp contract(off)

__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__global__ __launch_bounds__(CT) void combine_estimate_kernel(
    const float2* __restrict__ packed, const float2* __restrict__ ref, const double* __restrict__ f0,
    const CombineMember* __restrict__ mem, const CombineItem* __restrict__ items,
    CombinePartial* __restrict__ parts) {
  const CombineItem it = items[blockIdx.x];
  const CombineMember mb = mem[it.id];
  const float2* __restrict__ v = ref ? ref + mb.ro : packed + mb.rp;
  const float2* __restrict__ p = packed + mb.off;
  const double fk = f0 ? f0[it.id] : 0.0;
  const long long h = mb.n / 2;
  const double mc = (double)mb.lo + 0.5 * (double)(mb.n - 1);
  const long long c0 = (long long)it.chunk * kCombineChunk;          // within the overlap
  const long long cend = mb.n < c0 + kCombineChunk ? mb.n : c0 + kCombineChunk;
  float2 x[CV], r[CV];
#pragma unroll
  for (int i = 0; i < CV; ++i) {
    const long long q = c0 + threadIdx.x + i * CT;
    x[i] = r[i] = make_float2(0.f, 0.f);
    if (q < cend) {
      x[i] = p[mb.lo + q + mb.d];              // in [0, len): lo >= -d, lo + n <= len - d
      r[i] = v[mb.lo + q];                     // in [0, L_g): lo + n <= L_g
    }
  }
  Sums<8> acc{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
  double* s = acc.s;
#pragma unroll
  for (int i = 0; i < CV; ++i) {
    const long long q = c0 + threadIdx.x + i * CT;
    float2 xr = x[i];
    if (fk != 0.0) xr = cmulf(xr, cis_rev(-fk * ((double)(mb.lo + q) - mc)));
    const double zr = (double)(xr.x * r[i].x + xr.y * r[i].y);
    const double zi = (double)(xr.y * r[i].x - xr.x * r[i].y);
    const double ep = (double)(x[i].x * x[i].x + x[i].y * x[i].y);
    const double ev = (double)(r[i].x * r[i].x + r[i].y * r[i].y);
    const bool in = q < cend, first = in && q < h, rest = in && !first;
    s[0] += first ? zr : 0.0;
    s[1] += first ? zi : 0.0;
    s[2] += rest ? zr : 0.0;
    s[3] += rest ? zi : 0.0;
    s[4] += first ? ep : 0.0;
    s[5] += rest ? ep : 0.0;
    s[6] += first ? ev : 0.0;
    s[7] += rest ? ev : 0.0;
  }
  __shared__ Sums<8> slots[CW];
  block_fold<CW>(acc, slots);
  if (threadIdx.x == 0)
    parts[mb.slot + it.chunk] = CombinePartial{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
}

__global__ __launch_bounds__(CT) void combine_finalize_kernel(
    const CombinePartial* __restrict__ parts, const CombineMember* __restrict__ mem, int K,
    const double* __restrict__ f0, double min_rho, int first_pass, CombineRecord* __restrict__ rec) {
  const int k = blockIdx.x * CT + threadIdx.x;
  if (k >= K) return;
  const CombineMember mb = mem[k];
  double a1r = 0.0, a1i = 0.0, a2r = 0.0, a2i = 0.0, ep1 = 0.0, ep2 = 0.0, ev1 = 0.0, ev2 = 0.0;
  for (int c = 0; c < mb.nchunks; ++c) {
    const CombinePartial q = parts[mb.slot + c];
    a1r += q.a1r; a1i += q.a1i; a2r += q.a2r; a2i += q.a2i;
    ep1 += q.ep1; ep2 += q.ep2; ev1 += q.ev1; ev2 += q.ev2;
  }
  const double fk = f0 ? f0[k] : 0.0;
  const double ep = ep1 + ep2, ev = ev1 + ev2;
  CombineRecord r;
  r.n = mb.n;
  r.m = mb.n > 0 ? (double)mb.lo + 0.5 * (double)(mb.n - 1) : 0.0;
  r.ep = ep;
  r.ev = ev;
  r.pad = 0;
  if (first_pass && mb.is_rep) {                 // the frame itself, by definition
    r.a_re = 1.0; r.a_im = 0.0; r.freq = 0.0; r.rho = 1.0; r.res = 0.0; r.used = 1;
    rec[k] = r;
    return;
  }
  const bool fin = isfinite(a1r) && isfinite(a1i) && isfinite(a2r) && isfinite(a2i) && isfinite(ep) && isfinite(ev);
  double phi = 0.0;
  if ((a1r != 0.0 || a1i != 0.0) && (a2r != 0.0 || a2i != 0.0))
    phi = atan2(a2i * a1r - a2r * a1i, a2r * a1r + a2i * a1i);
  double sn, cs;
  sincos(0.5 * phi, &sn, &cs);
  const double br = (a1r * cs - a1i * sn) + (a2r * cs + a2i * sn);
  const double bi = (a1r * sn + a1i * cs) + (a2i * cs - a2r * sn);
  const double rho = sqrt(br * br + bi * bi) / sqrt(ep * ev);
  double fit = 0.0;
  if (ev1 > 0.0) fit += (a1r * a1r + a1i * a1i) / ev1;
  if (ev2 > 0.0) fit += (a2r * a2r + a2i * a2i) / ev2;
  r.res = ep - fit;
  const bool used = mb.n > 0 && fin && ev > 0.0 && rho >= min_rho;
  r.used = used ? 1 : 0;
  r.a_re = used ? br / ev : 0.0;
  r.a_im = used ? bi / ev : 0.0;
  r.freq = used ? fk + phi / (3.14159265358979323846 * (double)mb.n) : fk;
  r.rho = used ? rho : fin ? 0.0 : __builtin_nan("");
  rec[k] = r;
}

__global__ __launch_bounds__(CT) void combine_sum_kernel(
    const float2* __restrict__ packed, const CombineMember* __restrict__ mem,
    const CombineGroup* __restrict__ grp, const int* __restrict__ csr,
    const CombineItem* __restrict__ items, const CombineRecord* __restrict__ rec, float2* __restrict__ y) {
  const CombineItem it = items[blockIdx.x];
  const CombineGroup g = grp[it.id];
  const long long j0 = (long long)it.chunk * kCombineSumChunk + threadIdx.x;
  float2 num[SV];
  float den[SV];
  bool any[SV];
#pragma unroll
  for (int i = 0; i < SV; ++i) { num[i] = make_float2(0.f, 0.f); den[i] = 0.f; any[i] = false; }
  for (int q = g.m0; q < g.m1; ++q) {
    const int k = csr[q];
    const CombineRecord r = rec[k];
    if (!r.used) continue;
    const CombineMember mb = mem[k];
    const bool unit_a = r.a_re == 1.0 && r.a_im == 0.0, unit_f = r.freq == 0.0;
    const float2 w = make_float2((float)r.a_re, -(float)r.a_im);
    const float w2 = w.x * w.x + w.y * w.y;
    const float2* __restrict__ p = packed + mb.off;
    float2 x[SV];
    bool ok[SV];
#pragma unroll
    for (int i = 0; i < SV; ++i) {
      const long long j = j0 + i * CT, idx = j + mb.d;
      ok[i] = j < g.len && idx >= 0 && idx < mb.len;
      x[i] = ok[i] ? p[idx] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < SV; ++i) {
      if (!ok[i]) continue;
      float2 t = x[i];
      if (!unit_f) t = cmulf(t, cis_rev(-r.freq * ((double)(j0 + i * CT) - r.m)));
      if (!unit_a) t = cmulf(t, w);
      num[i] = any[i] ? make_float2(num[i].x + t.x, num[i].y + t.y) : t;
      den[i] += w2;
      any[i] = true;
    }
  }
#pragma unroll
  for (int i = 0; i < SV; ++i) {
    const long long j = j0 + i * CT;
    if (j >= g.len) continue;
    float2 o = num[i];
    if (!(den[i] > 0.f)) o = make_float2(0.f, 0.f);                // no used member covers j
    else if (den[i] != 1.f) o = make_float2(o.x / den[i], o.y / den[i]);
    y[g.ro + j] = o;
  }
}

}  // namespace

hipError_t launch_combine_estimate(const float2* packed, const float2* ref, const double* f0,
                                   const CombineMember* mem, int K, const CombineItem* items, long long nitems,
                                   CombinePartial* parts, double min_rho, CombineRecord* rec, hipStream_t st) {
  if (!packed || !mem || !rec || K < 1 || nitems < 0 || nitems > 0x7fffffffLL || (nitems > 0 && (!items || !parts)))
    return hipErrorInvalidValue;
  if (nitems > 0)
    hipLaunchKernelGGL(combine_estimate_kernel, dim3((unsigned)nitems), dim3(CT), 0, st, packed, ref, f0, mem,
                       items, parts);
  hipLaunchKernelGGL(combine_finalize_kernel, dim3((unsigned)((K + CT - 1) / CT)), dim3(CT), 0, st,
                     (const CombinePartial*)parts, mem, K, f0, min_rho, ref ? 0 : 1, rec);
  return hipGetLastError();
}

hipError_t launch_combine_sum(const float2* packed, const CombineMember* mem, const CombineGroup* grp,
                              const int* csr, const CombineItem* items, long long nitems,
                              const CombineRecord* rec, float2* y, hipStream_t st) {
  if (!packed || !mem || !grp || !csr || !items || !rec || !y || nitems < 1 || nitems > 0x7fffffffLL)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(combine_sum_kernel, dim3((unsigned)nitems), dim3(CT), 0, st, packed, mem, grp, csr, items,
                     rec, y);
  return hipGetLastError();
}

}  // namespace vsig
