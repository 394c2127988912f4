// diag.hip -- device self-tests of the wave-level primitives the tile passes rely on, and of the sort / scan / binning
// building blocks (thin wrappers of the library's own launchers).
#include "gslm_tile.hpp"

namespace gslm {

// in: [64 lanes][8 values] (value-major per lane); out[lane] = primitive result of that lane.
__global__ void k_selftest(int which, const float* __restrict__ in, float* __restrict__ out) {
  const int lane = threadIdx.x;
  if (which == 0) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = in[lane * 8 + k];
    out[lane] = wave_reduce8_t(v, lane);
  } else {
    out[lane] = wave_sum_lane63(in[lane * 8]);
  }
}

}  // namespace gslm

extern "C" int gslm_selftest(int32_t which, const float* in, float* out, void* stream) {
  hipLaunchKernelGGL(gslm::k_selftest, dim3(1), dim3(64), 0, (hipStream_t)stream, which, in, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    gslm::set_error(std::string("selftest launch: ") + hipGetErrorString(e));
    return GSLM_ERR_HIP;
  }
  return GSLM_OK;
}

extern "C" int gslm_selftest_scan(const uint32_t* in, uint32_t* out, int64_t n, int32_t force_top, void* tmp,
                                  size_t tmp_bytes, uint32_t* total, void* stream) {
  if (n < 0 || (n > 0 && (!in || !out || !tmp || !total))) {
    gslm::set_error("selftest_scan: n < 0 or NULL buffer");
    return GSLM_ERR_INVALID;
  }
  if (tmp_bytes < gslm::scan_tmp_bytes(n)) {
    gslm::set_error("selftest_scan: tmp below 8 ceil(n / 2048) + 64 bytes rounded up to 256");
    return GSLM_ERR_CAPACITY;
  }
  return gslm::exclusive_scan_u32(in, nullptr, out, n, static_cast<uint32_t*>(tmp), total, (hipStream_t)stream,
                                  force_top ? 0 : gslm::SCAN_INLINE_MAX_BLOCKS);
}

extern "C" int gslm_selftest_scan_dual(const uint32_t* in, const uint32_t* idx, const uint32_t* in_b, uint32_t* out_a,
                                       uint32_t* out_b, int64_t n, int32_t force_top, void* tmp, size_t tmp_bytes,
                                       uint32_t* total_a, uint32_t* total_b, void* stream) {
  if (n < 0 || !total_a || !total_b || (n > 0 && (!in || !out_a || !out_b || !tmp)) ||
      (n > 0 && (idx != nullptr) == (in_b != nullptr))) {
    gslm::set_error("selftest_scan_dual: n < 0, NULL buffer, or not exactly one of idx and in_b");
    return GSLM_ERR_INVALID;
  }
  if (tmp_bytes < gslm::scan_tmp_bytes(n)) {
    gslm::set_error("selftest_scan_dual: tmp below 8 ceil(n / 2048) + 64 bytes rounded up to 256");
    return GSLM_ERR_CAPACITY;
  }
  return gslm::exclusive_scan_u32_dual(in, idx, out_a, out_b, n, static_cast<uint32_t*>(tmp), total_a, total_b,
                                       (hipStream_t)stream, in_b, force_top ? 0 : gslm::SCAN_INLINE_MAX_BLOCKS);
}

extern "C" size_t gslm_selftest_sort_hist_bytes(int64_t n, int32_t payload) {
  return gslm::sort_hist_bytes(n > 0 ? n : 0, payload != 0);
}

extern "C" int gslm_selftest_sort(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t* p0, uint32_t* p1,
                                  int64_t n, int32_t end_bit, int32_t iota_values, int32_t key_range,
                                  const uint32_t* last_gather, const uint32_t* n_dev, void* hist, size_t hist_bytes,
                                  int32_t* result_in_alt, void* stream) {
  if (n < 0 || end_bit < 1 || end_bit > 32) {
    gslm::set_error("selftest_sort: n < 0 or end_bit outside 1..32");
    return GSLM_ERR_INVALID;
  }
  if (!k0 || !k1 || !v1 || (!v0 && !iota_values) || !hist || !result_in_alt) {
    gslm::set_error("selftest_sort: NULL key, value, hist or result_in_alt buffer");
    return GSLM_ERR_INVALID;
  }
  if ((p0 != nullptr) != (p1 != nullptr)) {
    gslm::set_error("selftest_sort: a payload buffer without its ping-pong partner");
    return GSLM_ERR_INVALID;
  }
  if (hist_bytes < gslm::sort_hist_bytes(n, p0 != nullptr)) {
    gslm::set_error("selftest_sort: hist below gslm_selftest_sort_hist_bytes(n, payload)");
    return GSLM_ERR_CAPACITY;
  }
  bool alt = false;
  const int st = gslm::radix_sort_pairs(k0, v0, k1, v1, n, end_bit, static_cast<uint32_t*>(hist), &alt,
                                        (hipStream_t)stream, iota_values != 0, last_gather, n_dev, p0, p1,
                                        key_range != 0);
  *result_in_alt = alt ? 1 : 0;
  return st;
}

extern "C" int gslm_selftest_ranges(const uint32_t* keys, int64_t n, int32_t ntiles, const uint32_t* n_dev,
                                    uint32_t* n_out, uint32_t* ranges, void* stream) {
  if (n < 0 || n > 0xFFFFFFFFll || ntiles < 1 || !ranges || (n > 0 && !keys) || (n_out && !n_dev)) {
    gslm::set_error("selftest_ranges: n outside [0, 2^32), ntiles < 1, NULL buffer, or n_out without n_dev");
    return GSLM_ERR_INVALID;
  }
  if (reinterpret_cast<uintptr_t>(keys) % 16 || reinterpret_cast<uintptr_t>(ranges) % 8) {
    gslm::set_error("selftest_ranges: keys not 16-byte or ranges not 8-byte aligned");
    return GSLM_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  GSLM_HIP_CHECK(hipMemsetAsync(ranges, 0, (size_t)ntiles * sizeof(uint2), s));
  return gslm::launch_ranges(n, keys, reinterpret_cast<uint2*>(ranges), n_dev, n_out, s);
}

extern "C" int gslm_selftest_tile_order(const uint32_t* ranges, const uint32_t* cost, int32_t ntiles, int32_t form,
                                        uint32_t* order, void* stream) {
  if (ntiles < 1 || (form != gslm::TILE_ORDER_FLAT && form != gslm::TILE_ORDER_XCD) || !order || (!ranges && !cost)) {
    gslm::set_error("selftest_tile_order: ntiles < 1, form outside {0, 1}, NULL order, or neither ranges nor cost");
    return GSLM_ERR_INVALID;
  }
  if (reinterpret_cast<uintptr_t>(ranges) % 8) {
    gslm::set_error("selftest_tile_order: ranges not 8-byte aligned");
    return GSLM_ERR_INVALID;
  }
  return gslm::launch_tile_order_form(form, ntiles, reinterpret_cast<const uint2*>(ranges), order, cost,
                                      (hipStream_t)stream);
}
