// The tables of a combine plan (vsig_combine_create): plain host C++ with no
// HIP in it, shared by the kernels (combine.hip), the C-ABI layer
// (api_combine.hip) and the stand-alone check of this logic
// (tools/probes/combine_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace vsig {

constexpr int kCombineChunk = 2048;          // S: samples of one estimate item
// outputs of one sum item: 2 a thread.  Measured at 512 x 16384 in 32 groups, estimate + sum +
// estimate: 0.119 ms at 2048 (256 blocks for 256 CUs), 0.106 at 1024, 0.097 at 512
constexpr int kCombineSumChunk = 512;
constexpr int kCombineMaxK = 4096;
constexpr long long kCombineMaxTotal = 1LL << 31;   // packed samples, exclusive
constexpr long long kCombineLagClamp = 1LL << 40;   // |lag| beyond every length: no overlap either way

// Packet k: p_k = packed[off, off + len); its overlap with its group's frame is
// j in [lo, lo + n), where it supplies p_k[j + d].  rp / ro: the group's
// representative in packed, the group's output in y.  Its nchunks partials
// start at slot.  g < 0: in no group (n = 0, no items).
struct CombineMember {
  long long off, len, d, lo, n, rp, ro, slot;
  int g, nchunks, is_rep, pad;
};
// Group g: y_g = y[ro, ro + len), its members csr[m0, m1) in ascending order.
struct CombineGroup {
  long long ro, len;
  int m0, m1;
};
// An estimate item is (member, chunk of its overlap), a sum item (group, chunk of its output).
struct CombineItem { int id, chunk; };
// One estimate item's sums: A1, A2, Ep1, Ep2, Ev1, Ev2.
struct CombinePartial { double a1r, a1i, a2r, a2i, ep1, ep2, ev1, ev2; };
// = vsig_combine_member_t (include/vsig.h)
struct CombineRecord {
  double a_re, a_im, freq, m, rho, ep, ev, res;
  long long n;
  int used, pad;
};

struct CombineTables {
  std::vector<CombineMember> mem;            // K
  std::vector<CombineGroup> grp;             // G
  std::vector<int> csr;                      // grouped packets, group by group
  std::vector<CombineItem> est, sum;
  std::vector<long long> out_offsets;        // G + 1
  long long total = 0;                       // packed samples
};

// Validates the lists and fills t.  0, or -1 (an invalid argument) / -4 (an
// unsupported size) with the reason in msg.  No pointer may be null.
inline int combine_tables(const int64_t* lens, const int32_t* group, const int64_t* lag, int32_t K,
                          const int32_t* rep, int32_t G, CombineTables* t, std::string* msg) {
  constexpr long long S = kCombineChunk;
  if (K < 1 || K > kCombineMaxK) {
    *msg = "combine: K must be in [1, " + std::to_string(kCombineMaxK) + "]";
    return -1;
  }
  if (G < 1 || G > K) {
    *msg = "combine: G must be in [1, K]";
    return -1;
  }
  long long total = 0;
  for (int k = 0; k < K; ++k) {
    if (lens[k] < 1) {
      *msg = "combine: packet " + std::to_string(k) + " has length " + std::to_string(lens[k]) + " (need >= 1)";
      return -1;
    }
    if (lens[k] >= kCombineMaxTotal || (total += lens[k]) >= kCombineMaxTotal) {
      *msg = "combine: the packed list reaches 2^31 samples at packet " + std::to_string(k);
      return -4;
    }
    if (group[k] < -1 || group[k] >= G) {
      *msg = "combine: packet " + std::to_string(k) + " names group " + std::to_string(group[k]) +
             ", outside [-1, " + std::to_string(G) + ")";
      return -1;
    }
  }
  for (int g = 0; g < G; ++g) {
    const int r = rep[g];
    if (r < 0 || r >= K || group[r] != g) {
      *msg = "combine: group " + std::to_string(g) + "'s representative " + std::to_string(r) +
             " is not one of its members";
      return -1;
    }
    if (lag[r] != 0) {
      *msg = "combine: group " + std::to_string(g) + "'s representative " + std::to_string(r) + " has lag " +
             std::to_string(lag[r]) + " (need 0)";
      return -1;
    }
  }
  t->total = total;
  t->out_offsets.assign((size_t)G + 1, 0);
  for (int g = 0; g < G; ++g) t->out_offsets[g + 1] = t->out_offsets[g] + lens[rep[g]];
  std::vector<long long> off((size_t)K + 1, 0);
  for (int k = 0; k < K; ++k) off[k + 1] = off[k] + lens[k];
  // the members' list of every group, in ascending packet order
  t->grp.assign(G, CombineGroup{0, 0, 0, 0});
  for (int k = 0; k < K; ++k)
    if (group[k] >= 0) ++t->grp[group[k]].m1;                 // counts first
  int at = 0;
  for (int g = 0; g < G; ++g) {
    const int cnt = t->grp[g].m1;
    t->grp[g] = {t->out_offsets[g], (long long)lens[rep[g]], at, at};
    at += cnt;
  }
  t->csr.assign(at, 0);
  for (int k = 0; k < K; ++k)
    if (group[k] >= 0) t->csr[t->grp[group[k]].m1++] = k;
  // members, their overlaps and partial slots
  t->mem.assign(K, CombineMember{});
  long long slot = 0;
  for (int k = 0; k < K; ++k) {
    CombineMember& m = t->mem[k];
    m.off = off[k];
    m.len = lens[k];
    m.g = group[k];
    m.d = std::max(-kCombineLagClamp, std::min(kCombineLagClamp, (long long)lag[k]));
    m.slot = slot;
    if (m.g < 0) continue;
    const long long Lg = lens[rep[m.g]];
    const long long lo = std::max(0LL, -m.d), hi = std::min(Lg, m.len - m.d);
    m.lo = hi > lo ? lo : 0;
    m.n = hi > lo ? hi - lo : 0;
    m.rp = off[rep[m.g]];
    m.ro = t->out_offsets[m.g];
    m.is_rep = rep[m.g] == k;
    m.nchunks = (int)((m.n + S - 1) / S);
    slot += m.nchunks;
  }
  // estimate items: within a group by the reference chunk they start in, then
  // by member, so the items that read one stretch of the reference are adjacent
  t->est.clear();
  t->est.reserve((size_t)slot);
  for (int g = 0; g < G; ++g) {
    const size_t first = t->est.size();
    for (int q = t->grp[g].m0; q < t->grp[g].m1; ++q)
      for (int c = 0; c < t->mem[t->csr[q]].nchunks; ++c) t->est.push_back({t->csr[q], c});
    std::stable_sort(t->est.begin() + first, t->est.end(), [&](const CombineItem& a, const CombineItem& b) {
      const long long ra = (t->mem[a.id].lo + a.chunk * S) / S, rb = (t->mem[b.id].lo + b.chunk * S) / S;
      return ra < rb;
    });
  }
  t->sum.clear();
  for (int g = 0; g < G; ++g)
    for (long long c = 0; c * kCombineSumChunk < t->grp[g].len; ++c) t->sum.push_back({g, (int)c});
  return 0;
}

}  // namespace vsig
