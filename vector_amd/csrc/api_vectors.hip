// C-ABI layer: element-wise stream operations (mix, scale, quantize, planar
// conversions), test-vector assembly and its normalisation, and the
// spectrogram image.
#include "vsig_ctx.hpp"

// What the element-wise entry points refuse; n == 0 then launches nothing.
static int elementwise_check(vsig_ctx* c, bool operands, int64_t n) {
  if (!operands) return fail(c, VSIG_E_INVALID, "null pointer");
  return n < 0 ? fail(c, VSIG_E_INVALID, "n < 0") : VSIG_OK;
}

// ---------------------------------------------------------------- stream ops
int vsig_mix_c64_dev(vsig_ctx* c, const void* x, int64_t n, double w, double sr, int64_t i0,
                     void* y) {
  if (!c || !x || !y) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0 || !(sr != 0.0)) return fail(c, VSIG_E_INVALID, "need n >= 0 and sample_rate != 0");
  if (n == 0) return VSIG_OK;
  return HIPRC(c, vsig::launch_mix_c64((const float2*)x, n, w, sr, i0, (float2*)y, c->stream));
}

int vsig_scale_c64_dev(vsig_ctx* c, const void* x, int64_t n, float s, void* y) {
  const int rc = elementwise_check(c, c && x && y, n);
  if (rc || n == 0) return rc;
  return HIPRC(c, vsig::launch_scale_c64((const float2*)x, n, s, (float2*)y, c->stream));
}

int vsig_wv_quantize_dev(vsig_ctx* c, const void* x, int64_t n, float norm, int16_t* out) {
  const int rc = elementwise_check(c, c && x && out, n);
  if (rc || n == 0) return rc;
  return HIPRC(c, vsig::launch_wv_quantize((const float2*)x, n, norm, (short*)out, c->stream));
}

int vsig_planar_to_c64_dev(vsig_ctx* c, int32_t mi_type, const void* re, const void* im, int64_t n,
                           void* y) {
  const int rc = elementwise_check(c, c && re && y, n);
  if (rc || n == 0) return rc;
  const hipError_t e = vsig::launch_planar_to_c64(mi_type, re, im, n, (float2*)y, c->stream);
  if (e == hipErrorInvalidValue) return fail(c, VSIG_E_UNSUPPORTED, "MAT storage type");
  return HIPRC(c, e);
}

int vsig_c64_to_planar_dev(vsig_ctx* c, const void* x, int64_t n, float* re, float* im) {
  const int rc = elementwise_check(c, c && x && re && im, n);
  if (rc || n == 0) return rc;
  return HIPRC(c, vsig::launch_c64_to_planar((const float2*)x, n, re, im, c->stream));
}

// ---------------------------------------------------------------- vector assembly
int vsig_vector_build_dev(vsig_ctx* c, const vsig_packet_place* places, int32_t nplaces, void* out,
                          int64_t n, float* maxabs_dev) {
  if (!c || !out || (nplaces > 0 && !places)) return fail(c, VSIG_E_INVALID, "null pointer");
  if (nplaces < 0 || n < 0) return fail(c, VSIG_E_INVALID, "need nplaces >= 0 and n >= 0");
  if (n > (1LL << 40)) return fail(c, VSIG_E_INVALID, "n above 2^40");
  if (!aligned8(out)) return fail(c, VSIG_E_INVALID, "out must be 8-byte aligned");
  for (int32_t i = 0; i < nplaces; ++i) {
    const vsig_packet_place& p = places[i];
    const std::string who = "place " + std::to_string(i) + ": ";
    if (!p.y) return fail(c, VSIG_E_INVALID, who + "null packet pointer");
    if (!aligned8(p.y)) return fail(c, VSIG_E_INVALID, who + "packet must be 8-byte aligned");
    if (p.len < 1) return fail(c, VSIG_E_INVALID, who + "len must be >= 1");
    if (p.period < 1) return fail(c, VSIG_E_INVALID, who + "period must be >= 1");
    if (p.count < 0) return fail(c, VSIG_E_INVALID, who + "count must be >= 0");
    if (p.start < 0) return fail(c, VSIG_E_INVALID, who + "start must be >= 0");
    // start + (count-1) period + len <= n without overflow
    if (p.count >= 1 && (p.start > n || p.len > n - p.start ||
                         p.count - 1 > (n - p.start - p.len) / p.period))
      return fail(c, VSIG_E_INVALID, who + "an instance ends past the vector");
  }
  if (maxabs_dev) HIPCHK(c, hipMemsetAsync(maxabs_dev, 0, sizeof(float), c->stream));
  if (n == 0) return VSIG_OK;
  // successive launches of kPlacesPerLaunch descriptors keep the add order:
  // each later one starts from what the earlier ones wrote
  vsig::PlaceBatch pb{};
  int launches = 0;
  for (int32_t i = 0; i < nplaces; ++i) {
    const vsig_packet_place& p = places[i];
    if (p.count == 0) continue;
    if (pb.nd == vsig::kPlacesPerLaunch) {
      HIPCHK(c, vsig::launch_vector_build(pb, (float2*)out, n, launches > 0, nullptr, c->stream));
      ++launches;
      pb.nd = 0;
    }
    pb.d[pb.nd++] = vsig::PlaceDesc{(const float2*)p.y, p.len, p.start, p.period, p.count};
  }
  return HIPRC(c, vsig::launch_vector_build(pb, (float2*)out, n, launches > 0, maxabs_dev, c->stream));
}

int vsig_normalize_c64_dev(vsig_ctx* c, const void* x, int64_t n, const float* maxabs_dev, void* y) {
  if (!c || !x || !y || !maxabs_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (n < 0) return fail(c, VSIG_E_INVALID, "n < 0");
  if (!aligned8(x, y)) return fail(c, VSIG_E_INVALID, "x and y must be 8-byte aligned");
  if (n == 0) return VSIG_OK;
  return HIPRC(c, vsig::launch_normalize_c64((const float2*)x, n, maxabs_dev, (float2*)y, c->stream));
}

// ---------------------------------------------------------------- display image
int vsig_spectrogram_image_dev(vsig_ctx* c, int32_t dtype, const void* sxx, int64_t n_freq,
                               int64_t n_time, int32_t freq_fast, int64_t ld, double floor_,
                               double vmin, double vmax, int32_t median, int32_t flip_freq,
                               int32_t pool_f, int32_t pool_t, const uint8_t* lut_dev,
                               uint8_t* rgba_dev) {
  if (!c || !sxx || !lut_dev || !rgba_dev) return fail(c, VSIG_E_INVALID, "null pointer");
  if (dtype != VSIG_DTYPE_F32 && dtype != VSIG_DTYPE_F64)
    return fail(c, VSIG_E_INVALID, "spectrogram image: dtype must be VSIG_DTYPE_F32 or VSIG_DTYPE_F64");
  if (n_freq < 1 || n_time < 1) return fail(c, VSIG_E_INVALID, "empty input");
  if (pool_f < 1 || pool_t < 1) return fail(c, VSIG_E_INVALID, "spectrogram image: pool factors must be >= 1");
  if (ld < (freq_fast ? n_freq : n_time))
    return fail(c, VSIG_E_INVALID, "spectrogram image: ld is below the fast extent");
  if ((reinterpret_cast<uintptr_t>(lut_dev) | reinterpret_cast<uintptr_t>(rgba_dev)) & 3)
    return fail(c, VSIG_E_INVALID, "spectrogram image: table and image must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(sxx) & (dtype == VSIG_DTYPE_F32 ? 3 : 7))
    return fail(c, VSIG_E_INVALID, "spectrogram image: sxx is not aligned to its dtype");
  if (!std::isfinite(vmin) || !std::isfinite(vmax) || !(vmax > vmin) ||
      (dtype == VSIG_DTYPE_F32 && !((float)vmax > (float)vmin && std::isfinite((float)vmax) &&
                                    std::isfinite((float)vmin))))
    return fail(c, VSIG_E_INVALID, "spectrogram image: need finite levels with vmax > vmin");
  Timed t(c, "spectrogram_image");
  return HIPRC(c, vsig::launch_spectrogram_image(dtype, sxx, n_freq, n_time, freq_fast != 0, ld, floor_, vmin,
                                                 vmax, median != 0, flip_freq != 0, pool_f, pool_t, lut_dev,
                                                 rgba_dev, c->stream));
}
