// C-ABI layer: all-pairs burst similarity of a packed packet list (vsig_match_*).
#include "vsig_ctx.hpp"

constexpr int kMatchMaxK = 4096;
constexpr long long kMatchMaxL = 8192;
constexpr int kMatchMaxTile = 8;           // partners of one a per unit at most
constexpr long long kMatchUnitsPerBlock = 4;

// The smallest in-LDS plan with N >= 2 L - 1.
static int match_size(long long L) {
  for (int N : {1024, 4096, 8192}) if (N >= 2 * L - 1) return N;
  return 16384;
}

// Partners per unit.  A unit saves one spectrum load in two for each partner
// after its first, so 8 already reaches 9 / 16 of the loads of tile 1; what
// the tile must not do is leave resident blocks without work.  It is held to
// pairs / (4 resident blocks): every block then walks 4 units or more, and the
// rows near a = K - 1, whose units are shorter than the tile, come last in the
// fixed order, where short units even the blocks' ends out.
static int match_tile(long long pairs, long long resident) {
  const long long t = pairs / (kMatchUnitsPerBlock * (resident < 1 ? 1 : resident));
  return (int)(t < 1 ? 1 : t > kMatchMaxTile ? kMatchMaxTile : t);
}

int vsig_match_create(vsig_ctx* c, const int64_t* lens, int32_t K, vsig_match** out) {
  if (!c || !lens || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  if (K < 1 || K > kMatchMaxK)
    return fail(c, VSIG_E_INVALID, "match: K must be in [1, " + std::to_string(kMatchMaxK) + "]");
  long long lmax = 0;
  for (int k = 0; k < K; ++k) {
    if (lens[k] < 1)
      return fail(c, VSIG_E_INVALID, "match: packet " + std::to_string(k) + " has length " +
                                         std::to_string(lens[k]) + " (need >= 1)");
    if (lens[k] > kMatchMaxL)
      return fail(c, VSIG_E_UNSUPPORTED, "match: packet " + std::to_string(k) + " has length " +
                                             std::to_string(lens[k]) + ", above " + std::to_string(kMatchMaxL));
    lmax = lens[k] > lmax ? lens[k] : lmax;
  }
  std::unique_ptr<vsig_match> p(new vsig_match(c));
  p->K = K;
  p->N = match_size(lmax);
  p->pairs = (long long)K * (K - 1) / 2;
  std::vector<long long> offsets((size_t)K + 1, 0);
  for (int k = 0; k < K; ++k) offsets[k + 1] = offsets[k] + lens[k];
  p->total = offsets[K];
  int key = 0, rc;
  long long resident = 1;
  if (vsig::match_geom(p->N, &key, &resident) != hipSuccess)
    return fail(c, VSIG_E_UNSUPPORTED, "match: transform length");
  p->tile = match_tile(p->pairs, resident);
  std::vector<vsig::MatchUnit> units;
  units.reserve((size_t)(p->pairs / p->tile + K));
  for (int a = 0; a + 1 < K; ++a)
    for (int b0 = a + 1; b0 < K; b0 += p->tile)
      units.push_back({a, b0, K - b0 < p->tile ? K - b0 : p->tile, 0});
  p->nunits = (long long)units.size();
  p->grid = p->nunits < resident ? p->nunits : resident;
  if (c->match_grid > 0 && p->grid > c->match_grid) p->grid = c->match_grid;
  if ((rc = get_twiddles(c, key, &p->tw))) return rc;
  HIPCHK(c, p->W.alloc((size_t)K * p->N * sizeof(float2)));
  rc = upload(c, p->offsets, offsets.data(), offsets.size());
  if (!rc && p->nunits) rc = upload(c, p->units, units.data(), units.size());
  (void)hipStreamSynchronize(c->stream);           // the host tables go out of scope
  if (rc) return rc;
  *out = p.release();
  return VSIG_OK;
}

void vsig_match_free(vsig_match* p) { delete p; }

int vsig_match_info(const vsig_match* p, int32_t* N, int64_t* pairs, int64_t* units, int64_t* grid,
                    int64_t* workspace_bytes) {
  if (!p) return VSIG_E_INVALID;
  if (!N || !pairs || !units || !grid || !workspace_bytes) return fail(p->ctx, VSIG_E_INVALID, "null pointer");
  *N = p->N; *pairs = p->pairs; *units = p->nunits; *grid = p->grid;
  *workspace_bytes = (int64_t)p->W.bytes();
  return VSIG_OK;
}

int vsig_match_run(vsig_match* p, const void* packed, float* peak, int32_t* lag, double* energy) {
  if (!p) return VSIG_E_INVALID;
  vsig_ctx* c = p->ctx;
  if (!packed || !peak || !lag || !energy) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!aligned8(packed, energy)) return fail(c, VSIG_E_INVALID, "packed and energy must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(peak) | reinterpret_cast<uintptr_t>(lag)) & 3)
    return fail(c, VSIG_E_INVALID, "peak and lag must be 4-byte aligned");
  Timed t(c, "match");
  return HIPRC(c, vsig::launch_match(p->N, (const float2*)packed, p->offsets.as<long long>(), p->K,
                                     p->W.as<float2>(), energy, p->units.as<vsig::MatchUnit>(), p->nunits,
                                     p->grid, peak, lag, p->tw, c->stream));
}
