// What the kernels that walk a CSR row with ascending ids share (rsa_knn.hip, rsa_ease.hip).
#pragma once
#include "rsa_common.hpp"

namespace rsa {

// first position in [a, b) of the ascending ids whose value is >= v
__device__ __forceinline__ int64_t knn_lower_bound(const int32_t* __restrict__ ids, int64_t a, int64_t b, int32_t v) {
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    if (ids[mid] < v) a = mid + 1; else b = mid;
  }
  return a;
}

}  // namespace rsa
