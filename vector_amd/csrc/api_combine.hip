// C-ABI layer: coherent averaging of an emitter's repeats (vsig_combine_*).
#include "vsig_ctx.hpp"

static_assert(sizeof(vsig_combine_member_t) == sizeof(vsig::CombineRecord) && sizeof(vsig_combine_member_t) == 80,
              "vsig_combine_member_t");
static_assert(offsetof(vsig_combine_member_t, n) == offsetof(vsig::CombineRecord, n) &&
              offsetof(vsig_combine_member_t, used) == offsetof(vsig::CombineRecord, used), "vsig_combine_member_t");

int vsig_combine_create(vsig_ctx* c, const int64_t* lens, const int32_t* group, const int64_t* lag, int32_t K,
                        const int32_t* rep, int32_t G, vsig_combine** out) {
  if (!c || !lens || !group || !lag || !rep || !out) return fail(c, VSIG_E_INVALID, "null pointer");
  *out = nullptr;
  vsig::CombineTables t;
  std::string msg;
  if (const int rc = vsig::combine_tables(lens, group, lag, K, rep, G, &t, &msg))
    return fail(c, rc == -4 ? VSIG_E_UNSUPPORTED : VSIG_E_INVALID, msg);
  std::unique_ptr<vsig_combine> p(new vsig_combine(c));
  p->K = K;
  p->G = G;
  p->total = t.total;
  p->offsets = t.out_offsets;
  p->out_total = t.out_offsets[G];
  p->est_items = (long long)t.est.size();
  p->sum_items = (long long)t.sum.size();
  HIPCHK(c, p->parts.alloc((size_t)p->est_items * sizeof(vsig::CombinePartial)));
  int rc = upload(c, p->mem, t.mem.data(), t.mem.size());
  if (!rc) rc = upload(c, p->grp, t.grp.data(), t.grp.size());
  if (!rc) rc = upload(c, p->csr, t.csr.data(), t.csr.size());
  if (!rc) rc = upload(c, p->est, t.est.data(), t.est.size());
  if (!rc) rc = upload(c, p->sum, t.sum.data(), t.sum.size());
  (void)hipStreamSynchronize(c->stream);           // the host tables go out of scope
  if (rc) return rc;
  *out = p.release();
  return VSIG_OK;
}

void vsig_combine_free(vsig_combine* p) { delete p; }

int vsig_combine_info(const vsig_combine* p, int64_t* out_total, int32_t* chunk, int64_t* est_items,
                      int64_t* sum_items, int64_t* workspace_bytes) {
  if (!p) return VSIG_E_INVALID;
  if (!out_total || !chunk || !est_items || !sum_items || !workspace_bytes)
    return fail(p->ctx, VSIG_E_INVALID, "null pointer");
  *out_total = p->out_total; *chunk = vsig::kCombineChunk; *est_items = p->est_items; *sum_items = p->sum_items;
  *workspace_bytes = (int64_t)p->parts.bytes();
  return VSIG_OK;
}

int vsig_combine_offsets(const vsig_combine* p, int64_t* offsets) {
  if (!p) return VSIG_E_INVALID;
  if (!offsets) return fail(p->ctx, VSIG_E_INVALID, "null pointer");
  for (size_t g = 0; g < p->offsets.size(); ++g) offsets[g] = p->offsets[g];
  return VSIG_OK;
}

int vsig_combine_estimate(vsig_combine* p, const void* packed, const void* ref, const double* f0, double min_rho,
                          vsig_combine_member_t* records) {
  if (!p) return VSIG_E_INVALID;
  vsig_ctx* c = p->ctx;
  if (!packed || !records) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!aligned8(packed, ref) || !aligned8(f0, records))
    return fail(c, VSIG_E_INVALID, "packed, ref, f0 and records must be 8-byte aligned");
  if (min_rho != min_rho) return fail(c, VSIG_E_INVALID, "combine: min_rho is NaN");
  Timed t(c, "combine_estimate");
  return HIPRC(c, vsig::launch_combine_estimate(
                      (const float2*)packed, (const float2*)ref, f0, p->mem.as<vsig::CombineMember>(), p->K,
                      p->est.as<vsig::CombineItem>(), p->est_items, p->parts.as<vsig::CombinePartial>(), min_rho,
                      reinterpret_cast<vsig::CombineRecord*>(records), c->stream));
}

int vsig_combine_sum(vsig_combine* p, const void* packed, const vsig_combine_member_t* records, void* y) {
  if (!p) return VSIG_E_INVALID;
  vsig_ctx* c = p->ctx;
  if (!packed || !records || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (!aligned8(packed, records) || !aligned8(y))
    return fail(c, VSIG_E_INVALID, "packed, records and y must be 8-byte aligned");
  Timed t(c, "combine_sum");
  return HIPRC(c, vsig::launch_combine_sum((const float2*)packed, p->mem.as<vsig::CombineMember>(),
                                           p->grp.as<vsig::CombineGroup>(), p->csr.as<int>(),
                                           p->sum.as<vsig::CombineItem>(), p->sum_items,
                                           reinterpret_cast<const vsig::CombineRecord*>(records), (float2*)y,
                                           c->stream));
}
