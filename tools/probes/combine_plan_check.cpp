// Stand-alone check of the combine plan's host logic (combine_plan.hpp: the
// validation, the member and group tables, the CSR lists, the item tables),
// meant to be built with the host sanitizers; no device, no HIP:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/probes/combine_plan_check.cpp -o combine_plan_check && ./combine_plan_check
// Random lists (every refusal among them) are built and every table entry is
// checked against the invariants the kernels rely on for their addresses.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../vector_amd/csrc/combine_plan.hpp"

using namespace vsig;

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);        \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

static void check_tables(const std::vector<int64_t>& lens, const std::vector<int32_t>& group,
                         const std::vector<int64_t>& lag, const std::vector<int32_t>& rep, const CombineTables& t) {
  const int K = (int)lens.size(), G = (int)rep.size();
  const long long S = kCombineChunk;
  REQUIRE((int)t.mem.size() == K && (int)t.grp.size() == G && (int)t.out_offsets.size() == G + 1);
  long long off = 0, slots = 0;
  for (int k = 0; k < K; ++k) {
    const CombineMember& m = t.mem[k];
    REQUIRE(m.off == off && m.len == lens[k] && m.g == group[k] && m.slot == slots);
    off += lens[k];
    if (m.g < 0) {
      REQUIRE(m.n == 0 && m.nchunks == 0);
      continue;
    }
    const long long Lg = lens[rep[m.g]];
    REQUIRE(m.n >= 0 && m.nchunks == (m.n + S - 1) / S && m.ro == t.out_offsets[m.g]);
    REQUIRE(m.is_rep == (rep[m.g] == k));
    if (m.n > 0) {       // every estimate load: p[lo + q + d], v[lo + q] for q < n
      REQUIRE(m.lo >= 0 && m.lo + m.n <= Lg && m.lo + m.d >= 0 && m.lo + m.n + m.d <= m.len);
      REQUIRE(m.d == lag[k]);
      // the overlap is maximal
      REQUIRE(m.lo == 0 || m.lo + m.d == 0);
      REQUIRE(m.lo + m.n == Lg || m.lo + m.n + m.d == m.len);
    }
    if (m.is_rep) REQUIRE(m.n == Lg && m.lo == 0 && m.d == 0);
    slots += m.nchunks;
  }
  REQUIRE(off == t.total && (long long)t.est.size() == slots);
  std::vector<int> seen((size_t)slots, 0);
  int prev_g = -1;
  long long prev_r = -1;
  for (const CombineItem& it : t.est) {
    REQUIRE(it.id >= 0 && it.id < K);
    const CombineMember& m = t.mem[it.id];
    REQUIRE(it.chunk >= 0 && it.chunk < m.nchunks && !seen[m.slot + it.chunk]++);
    const long long r = (m.lo + it.chunk * S) / S;
    if (m.g != prev_g) {                                          // by group, then by reference chunk
      REQUIRE(m.g > prev_g);
      prev_r = -1;
    }
    REQUIRE(r >= prev_r);
    prev_r = r;
    prev_g = m.g;
  }
  size_t si = 0;
  int at = 0;
  for (int g = 0; g < G; ++g) {
    const CombineGroup& q = t.grp[g];
    REQUIRE(q.ro == t.out_offsets[g] && q.len == lens[rep[g]] && q.m0 == at && q.m1 > q.m0);
    for (int i = q.m0; i < q.m1; ++i) {
      REQUIRE(i < (int)t.csr.size() && group[t.csr[i]] == g && (i == q.m0 || t.csr[i] > t.csr[i - 1]));
    }
    at = q.m1;
    for (long long c = 0; c * kCombineSumChunk < q.len; ++c, ++si) REQUIRE(si < t.sum.size() && t.sum[si].id == g && t.sum[si].chunk == c);
  }
  REQUIRE(si == t.sum.size() && at == (int)t.csr.size());
}

int main() {
  std::mt19937_64 rng(12345);
  auto uni = [&](long long lo, long long hi) { return (long long)(rng() % (unsigned long long)(hi - lo + 1)) + lo; };
  int ok = 0, refused = 0;
  for (int trial = 0; trial < 3000; ++trial) {
    const int K = (int)uni(1, 40), G = (int)uni(1, K);
    std::vector<int64_t> lens(K), lag(K);
    std::vector<int32_t> group(K), rep(G);
    const long long lmax = trial % 3 == 0 ? 3 * kCombineChunk + 7 : 50;
    for (int k = 0; k < K; ++k) {
      lens[k] = uni(1, lmax);
      group[k] = (int32_t)uni(-1, G - 1);
      const long long r = uni(0, 9);
      lag[k] = r == 0 ? (uni(0, 1) ? 1 : -1) * uni(1LL << 39, 1LL << 62) : r < 4 ? uni(-lmax - 2, lmax + 2) : uni(-20, 20);
    }
    for (int g = 0; g < G; ++g) {       // mostly valid representatives
      rep[g] = (int32_t)uni(0, K - 1);
      if (uni(0, 30) != 0) { group[rep[g]] = g; lag[rep[g]] = 0; }
    }
    for (int g = 0; g < G; ++g)         // a later group may have taken an earlier one's representative
      if (uni(0, 30) != 0 && group[rep[g]] != g)
        for (int k = 0; k < K; ++k)
          if (group[k] == g) { rep[g] = k; lag[k] = 0; break; }
    if (uni(0, 40) == 0) lens[uni(0, K - 1)] = uni(-2, 0);
    if (uni(0, 40) == 0) group[uni(0, K - 1)] = (int32_t)(uni(0, 1) ? G : -2);
    CombineTables t;
    std::string msg;
    const int rc = combine_tables(lens.data(), group.data(), lag.data(), K, rep.data(), G, &t, &msg);
    if (rc) {
      REQUIRE((rc == -1 || rc == -4) && !msg.empty());
      ++refused;
      continue;
    }
    check_tables(lens, group, lag, rep, t);
    ++ok;
  }
  // the size limits
  {
    CombineTables t;
    std::string msg;
    std::vector<int64_t> lens = {1LL << 30, 1LL << 30}, lag = {0, 0};
    std::vector<int32_t> group = {0, 0}, rep = {0};
    REQUIRE(combine_tables(lens.data(), group.data(), lag.data(), 2, rep.data(), 1, &t, &msg) == -4);
    lens = {(1LL << 31) - 2, 1};
    REQUIRE(combine_tables(lens.data(), group.data(), lag.data(), 2, rep.data(), 1, &t, &msg) == 0);
    REQUIRE(t.total == (1LL << 31) - 1 && t.est.size() == (size_t)(((1LL << 31) - 2 + kCombineChunk - 1) / kCombineChunk) + 1);
    lens = {INT64_MAX, INT64_MAX};
    REQUIRE(combine_tables(lens.data(), group.data(), lag.data(), 2, rep.data(), 1, &t, &msg) == -4);
    REQUIRE(combine_tables(lens.data(), group.data(), lag.data(), 0, rep.data(), 1, &t, &msg) == -1);
    REQUIRE(combine_tables(lens.data(), group.data(), lag.data(), 2, rep.data(), 3, &t, &msg) == -1);
  }
  std::printf("combine plan: %d lists checked, %d refused\n", ok, refused);
  REQUIRE(ok > 500 && refused > 50);
  return 0;
}
