// The host launch layer of librecstudio_amd.so: how an entry point turns run-time values into template arguments, sizes a
// grid, decides how rows are loaded, and sizes / places a workspace.  Host code only.
#pragma once
#include <type_traits>

#include "rsa_common.hpp"

namespace rsa {

#define RSA_CHECK_HIP(call, who)                                                 \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                      \
      rsa::set_error("%s: %s", who, hipGetErrorString(e_));                      \
      return RSA_ERR_HIP;                                                        \
    }                                                                            \
  } while (0)

// ---------------------------------------------------------------- run-time value -> template argument
// Calls f(std::integral_constant<int, V>) for the V of the list that equals v and returns true; false (and no call) when v is
// not in the list.  The list is the caller's: only the kernels it names for these values are instantiated.
template <int... Vs, class F>
static inline bool dispatch_int(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// The embedding width: f receives D with D() == dim.  A false return is the caller's RSA_ERR_UNSUPPORTED.
template <int... Dims, class F>
static inline bool dispatch_dim(int dim, F&& f) {
  return dispatch_int<Dims...>(dim, static_cast<F&&>(f));
}

// f(std::true_type) or f(std::false_type); nests for several flags.
template <class F>
static inline void dispatch_bool(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// ---------------------------------------------------------------- policies
// streaming (nontemporal) row loads once the table cannot live in the 256 MB Infinity Cache
static inline bool streams_past_cache(int64_t rows, int64_t dim) {
  return (size_t)rows * (size_t)dim * sizeof(float) > (512ull << 20);
}

// ceil(work / per_block) workgroups, at most `cap` (the kernels behind it stride over the rest)
static inline unsigned grid_1d(int64_t work, int64_t per_block, int64_t cap) {
  const int64_t blocks = (work + per_block - 1) / per_block;
  return (unsigned)(blocks > cap ? cap : blocks);
}

// The owner walks (rsa_owner.hip) give a query 1, 2 or 4 waves by the 64-slot tiles it has on average; a 256-thread workgroup
// then holds 4, 2 or 1 queries.
struct WalkGeometry {
  int wpq_log2;
  unsigned blocks;
};
constexpr int OWNER_WALK_GRID_CAP = 4096;
static_assert(OWNER_WALK_GRID_CAP <= LOSS_MAX_GRID, "the owner BPR walk reduces its loss with reduce_mean_loss");
static inline WalkGeometry owner_walk_geometry(int64_t slots, int64_t n_queries) {
  const int64_t tiles_per_query = slots / (n_queries > 0 ? n_queries : 1) / 64;
  const int wpq_log2 = tiles_per_query >= 8 ? 2 : (tiles_per_query >= 3 ? 1 : 0);
  return WalkGeometry{wpq_log2, grid_1d(n_queries, 4 >> wpq_log2, OWNER_WALK_GRID_CAP)};
}

// ---------------------------------------------------------------- workspaces
static inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// One description per workspace: a function takes its regions from a Carver in order.  Run over a null base it sizes the
// workspace (bytes()), run over the caller's pointer it places the regions -- the two cannot disagree.  Every region starts
// on a 256-byte boundary, the first one at the base rounded UP: the sizes the entry points report carry 256 bytes or more
// of slack beyond bytes() for that.
class Carver {
 public:
  explicit Carver(void* base) : base_(reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + 255) & ~(uintptr_t)255)) {}
  template <class T>
  T* take(int64_t count) {       // null when sizing
    const int64_t at = align256(bytes_);
    bytes_ = at + count * (int64_t)sizeof(T);
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  int64_t bytes() const { return bytes_; }      // the end of the last region

 private:
  char* base_;
  int64_t bytes_ = 0;
};

}  // namespace rsa
