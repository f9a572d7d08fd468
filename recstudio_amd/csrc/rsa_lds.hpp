// What the kernels that keep a small matrix in dynamic LDS share (rsa_midx.hip, rsa_lsh.hip): the row padding, the LDS budget
// and its per-kernel grant, and the dot product's accumulation order.
#pragma once
#include <atomic>

#include "rsa_common.hpp"
#include "rsa_launch.hpp"

namespace rsa {

constexpr int CPAD = 4;                 // floats of padding per matrix row in LDS: one ds_read_b128 width
constexpr int64_t LDS_STATIC_LIMIT = 64 << 10, LDS_LIMIT = 160 << 10;

// four interleaved FMA chains (elements i % 4, ascending i) ...
__device__ __forceinline__ void fma4(float4& acc, const float4& a, const float4& b) {
  acc.x = __fmaf_rn(a.x, b.x, acc.x);
  acc.y = __fmaf_rn(a.y, b.y, acc.y);
  acc.z = __fmaf_rn(a.z, b.z, acc.z);
  acc.w = __fmaf_rn(a.w, b.w, acc.w);
}
// ... summed (x + y) + (z + w)
__device__ __forceinline__ float sum4(const float4& a) { return (a.x + a.y) + (a.z + a.w); }

// dynamic LDS above 64 KB has to be granted per kernel and device: asked for once, and again only for a larger size
template <auto kern>
static int allow_lds(int64_t bytes, const char* who) {
  constexpr int MAX_DEV = 64;
  static std::atomic<int64_t> granted[MAX_DEV];            // zero-initialised: nothing granted yet
  if (bytes <= LDS_STATIC_LIMIT) return RSA_OK;
  int dev = 0;
  RSA_CHECK_HIP(hipGetDevice(&dev), who);
  if (dev >= 0 && dev < MAX_DEV && granted[dev].load(std::memory_order_relaxed) >= bytes) return RSA_OK;
  RSA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), who);
  if (dev >= 0 && dev < MAX_DEV) granted[dev].store(bytes, std::memory_order_relaxed);
  return RSA_OK;
}

}  // namespace rsa
