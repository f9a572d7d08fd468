// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of recstudio_amd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/recstudio_amd.h"

namespace rsa {

constexpr int WAVE = 64;

// ---------------------------------------------------------------- error plumbing (host)
void set_error(const char* fmt, ...);
#define RSA_CHECK_ARG(cond, ...)                \
  do {                                          \
    if (!(cond)) {                              \
      rsa::set_error(__VA_ARGS__);              \
      return RSA_ERR_ARG;                       \
    }                                           \
  } while (0)
#define RSA_CHECK_LAUNCH(what)                                                   \
  do {                                                                           \
    hipError_t e_ = hipGetLastError();                                           \
    if (e_ != hipSuccess) {                                                      \
      rsa::set_error("%s: launch failed: %s", what, hipGetErrorString(e_));      \
      return RSA_ERR_HIP;                                                        \
    }                                                                            \
  } while (0)

// Versioned argument blocks (include/recstudio_amd.h, ABI 9): copy min(caller's size, ours) bytes of `src` into the
// zero-filled `dst` -- fields the caller's header did not have read as 0 / null, fields ours does not have are ignored.
template <class T>
static inline int load_args(T& dst, const T* src, const char* who) {
  RSA_CHECK_ARG(src != nullptr, "%s: args is null", who);
  const int64_t sz = *reinterpret_cast<const int64_t*>(src);
  RSA_CHECK_ARG(sz >= 16 && sz <= (1 << 16), "%s: args->size = %lld (set it to sizeof the argument struct)", who, (long long)sz);
  __builtin_memset(&dst, 0, sizeof(T));
  __builtin_memcpy(&dst, src, (size_t)sz < sizeof(T) ? (size_t)sz : sizeof(T));
  dst.size = (int64_t)sizeof(T);
  return RSA_OK;
}

// ---------------------------------------------------------------- Philox4x32-10
// Random123 Philox4x32 with 10 rounds: the generator behind torch's device
// distributions (rocRAND philox4x32_10_engine::ten_rounds).
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
    const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += W0;
    k.y += W1;
  }
  return c;
}

// State of one torch distribution call, see include/recstudio_amd.h ("Philox state").
struct PhiloxCall {
  uint64_t seed;
  uint64_t offset4;        // generator offset / 4 (torch offsets are multiples of 4)
  uint32_t grid_threads;   // G
  uint64_t elem_base;      // element index of this launch's element 0 inside the (global) torch call
};

// ---------------------------------------------------------------- caller-owned reduction scratch
// Layout of the rsa_scratch_bytes() block (zero-filled once by the caller):
//   [0]     NaN / inf flag word of the in-kernel loss reduction (cleared by the kernel that read it)
//   [64]    valid-row counter of the BCE losses (reset by a memset before each use)
//   [256]   64-bit {arrivals in bits 56..63, 2^-34 fixed-point loss sum in bits 0..55} words of the in-kernel loss
//           reduction: the top word, then 32 sub-words 128 bytes apart (zero again after EVERY launch, whatever the
//           losses were; 4.2 KB of the 16 KB reserved here)
//   [256 + 4 * SCRATCH_MAX_GRID]   256 stage-1 partials of rsa_mean_rows
constexpr int SCRATCH_MAX_GRID = 4096;
constexpr int64_t SCRATCH_COUNTER = 0, SCRATCH_BCE_COUNT = 64, SCRATCH_FUSED_PARTIALS = 256,
                  SCRATCH_MEAN_PARTIALS = 256 + 4 * SCRATCH_MAX_GRID, SCRATCH_BYTES = SCRATCH_MEAN_PARTIALS + 4 * 256;

// Raw philox draw for output element li of a call whose per-draw unroll is UNROLL
// (4: 32-bit ints and floats, 2: 64-bit ints).  Returns the 4 words and the
// component index the element owns.
template <int UNROLL>
__device__ __forceinline__ uint4 philox_for_element(const PhiloxCall& pc, uint64_t li, int& comp) {
  li += pc.elem_base;
  uint64_t idx, j;
  if (li < pc.grid_threads) {   // common case: every element on its own subsequence, first draw
    idx = li;
    j = 0;
  } else if ((li >> 32) == 0) {  // 32-bit quotient (the 64-bit one is a ~100-instruction subroutine, once per element)
    j = (uint32_t)li / pc.grid_threads;
    idx = li - j * pc.grid_threads;
  } else {
    j = li / pc.grid_threads;
    idx = li - j * pc.grid_threads;
  }
  const uint64_t k = j / UNROLL;
  comp = (int)(j - k * UNROLL);
  const uint64_t ctr = pc.offset4 + k;
  const uint4 c = make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)idx, (uint32_t)(idx >> 32));
  const uint2 key = make_uint2((uint32_t)pc.seed, (uint32_t)(pc.seed >> 32));
  return philox4x32_10(c, key);
}

__device__ __forceinline__ uint32_t pick(const uint4& v, int comp) {
  return comp == 0 ? v.x : comp == 1 ? v.y : comp == 2 ? v.z : v.w;
}

// == element li of torch.randint(low, low+range, ..., device='cuda')
__device__ __forceinline__ int64_t torch_randint_element(const PhiloxCall& pc, uint64_t li, uint64_t range,
                                                         int64_t low) {
  int comp;
  if (range >= (1ull << 28)) {   // ATen random_from_to_kernel: 64-bit draws above 2^28
    const uint4 v = philox_for_element<2>(pc, li, comp);
    const uint64_t r = comp == 0 ? (((uint64_t)v.x << 32) | v.y) : (((uint64_t)v.z << 32) | v.w);
    return (int64_t)(r % range) + low;
  }
  const uint4 v = philox_for_element<4>(pc, li, comp);
  return (int64_t)(pick(v, comp) % (uint32_t)range) + low;      // range < 2^28 here: a 32-bit remainder, not the 64-bit subroutine
}

// == element li of torch.rand(..., device='cuda', dtype=float32)
__device__ __forceinline__ float torch_rand_element(const PhiloxCall& pc, uint64_t li) {
  int comp;
  const uint4 v = philox_for_element<4>(pc, li, comp);
  const float inv = 2.3283064e-10f;                       // 2^-32 (rocRAND uniform_distribution)
  const float u = __fmaf_rn((float)pick(v, comp), inv, inv);   // product exact => == mul then add
  return u == 1.0f ? 0.0f : u;                            // torch uniform_kernel bound flip
}

// ---------------------------------------------------------------- inverse-CDF lookup
// First index i in [0, n_items) with table[i] >= u, found inside the cut-point
// bucket [guide[b], guide[b+1]] of b = floor(u * 2^guide_log2); clamped to n_items-1.
template <int STRIDE = 1>
__device__ __forceinline__ int32_t cdf_lower_bound(const float* __restrict__ table,
                                                   const int32_t* __restrict__ guide, int64_t n_items,
                                                   int guide_log2, float u) {
  const int32_t K = 1 << guide_log2;
  int32_t b = (int32_t)(u * (float)K);    // exact: power-of-two scale
  b = b < 0 ? 0 : (b > K - 1 ? K - 1 : b);
  int32_t lo = guide[b], hi = guide[b + 1];   // answer in [lo, hi]
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (table[(size_t)mid * STRIDE] < u) lo = mid + 1; else hi = mid;
  }
  return lo > (int32_t)(n_items - 1) ? (int32_t)(n_items - 1) : lo;
}

// Direct-lookup form of the same search.  One self-contained 16-byte entry per guide bucket b, with
// lo = guide[b], hi = guide[b+1] (so the answer lies in [lo, hi]):
//   x = lo, sign bit set when hi - lo >= 2 (bucket holds two or more CDF boundaries: binary search needed)
//   y = table[lo], or +inf when hi == lo          z = pop_prob[min(lo, N-1)]       w = pop_prob[min(lo+1, N-1)]
// Direct buckets (hi - lo <= 1, the common case with a fine guide) resolve id AND probability from this
// single read -- one HBM line per sampled id instead of three dependent round trips (guide -> table ->
// pop_prob): id = lo + (y < u).  Same comparisons as the binary search, same index.
constexpr uint32_t LUT_SEARCH_BIT = 0x80000000u;

__device__ __forceinline__ int32_t lut_bucket(int guide_log2, float u) {
  const int32_t K = 1 << guide_log2;
  const int32_t b = (int32_t)(u * (float)K);     // exact: power-of-two scale
  return b < 0 ? 0 : (b > K - 1 ? K - 1 : b);
}

// resolve a draw u given its (already loaded) bucket entry e0 = lut[lut_bucket(u)]
template <int STRIDE>
__device__ __forceinline__ int32_t cdf_resolve_lut(const float4 e0, const float4* __restrict__ lut,
                                                   const float* __restrict__ cdf, const float* __restrict__ prob,
                                                   int prob_stride, int64_t n_items, int guide_log2, float u,
                                                   float& pr) {
  const int32_t b = lut_bucket(guide_log2, u);
  const uint32_t x = __float_as_uint(e0.x);
  int32_t lo = (int32_t)(x & ~LUT_SEARCH_BIT);
  const int32_t last = (int32_t)(n_items - 1);
  if (!(x & LUT_SEARCH_BIT)) {
    const bool up = e0.y < u;
    pr = up ? e0.w : e0.z;
    const int32_t id = lo + (up ? 1 : 0);
    return id > last ? last : id;
  }
  // Bucket with >= 2 boundaries.  The answer is lo + #{i : cdf[lo+i] < u} (the CDF is non-decreasing, so the
  // predicate holds on a prefix): probe the next PROBE entries with loads issued together -- one more round
  // trip instead of a chain of dependent binary-search probes -- and only buckets with more than PROBE
  // boundaries below u (rare with ~1 item per bucket) continue with the binary search in [lo+PROBE, hi].
  constexpr int PROBE = 4;
  float c[PROBE], q[PROBE];
#pragma unroll
  for (int i = 0; i < PROBE; ++i) {
    const int32_t j = lo + i > last ? last : lo + i;
    c[i] = cdf[(size_t)j * STRIDE];
    q[i] = STRIDE == 2 ? cdf[(size_t)j * STRIDE + 1] : 0.f;     // interleaved {cdf, prob}: the same 8-byte load
  }
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < PROBE; ++i) cnt += (lo + i <= last && c[i] < u) ? 1 : 0;   // prefix count
  if (cnt < PROBE) {
    lo += cnt;
    lo = lo > last ? last : lo;
    if (STRIDE == 2 && prob == cdf + 1) {
      pr = cnt == 0 ? q[0] : cnt == 1 ? q[1] : cnt == 2 ? q[2] : q[3];
      if (lo == last) pr = prob[(size_t)last * prob_stride];    // clamped index: re-read (edge only)
    } else {
      pr = prob[(size_t)lo * prob_stride];
    }
    return lo;
  }
  lo += PROBE;
  int32_t hi = (int32_t)(__float_as_uint(lut[b + 1].x) & ~LUT_SEARCH_BIT);
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (cdf[(size_t)mid * STRIDE] < u) lo = mid + 1; else hi = mid;
  }
  lo = lo > last ? last : lo;
  pr = prob[(size_t)lo * prob_stride];
  return lo;
}

template <int STRIDE>
__device__ __forceinline__ int32_t cdf_lookup_lut(const float4* __restrict__ lut, const float* __restrict__ cdf,
                                                  const float* __restrict__ prob, int prob_stride, int64_t n_items,
                                                  int guide_log2, float u, float& pr) {
  return cdf_resolve_lut<STRIDE>(lut[lut_bucket(guide_log2, u)], lut, cdf, prob, prob_stride, n_items, guide_log2, u,
                                 pr);
}

// Bucket-line form (layout: include/recstudio_amd.h, rsa_fused_args.cdf_lines): one 128-byte line per bucket,
//   words 0..11  cdf[12]     the bucket's first distinct CDF values, then (when fewer than 12) the first entry ABOVE the
//                            bucket, then +inf
//   words 12..23 prob[12]    pop_prob of those entries
//   words 24..29 delta[12]   uint16 each: id = base + delta
//   word  30     base        id of slot 0
//   word  31     count       distinct values inside the bucket (may exceed 12); -1: ids too far apart for 16-bit deltas
// k = #{cdf[i] < u} is the answer's slot: the entry above the bucket compares >= u, so k never points past it.  Only
// k == 12 (more than 12 distinct values, all below u) and count == -1 fall back to a binary search of `table`
// between this line's and the next line's base.  Same comparisons as torch.searchsorted, same index; one HBM line.
constexpr int LINE_SLOTS = 12;
__device__ __forceinline__ int32_t lines_bucket(int lines_log2, float u) { return lut_bucket(lines_log2, u); }

__device__ __forceinline__ int32_t cdf_lookup_line(const float* __restrict__ lines, int lines_log2,
                                                   const float* __restrict__ cdf, int cdf_stride,
                                                   const float* __restrict__ prob, int prob_stride, int64_t n_items,
                                                   float u, float& pr) {
  const float* line = lines + (size_t)lines_bucket(lines_log2, u) * 32;
  const float4* l4 = reinterpret_cast<const float4*>(line);
  const float4 c0 = l4[0], c1 = l4[1], c2 = l4[2];                       // four loads of ONE line, issued together
  const int2 tail = *reinterpret_cast<const int2*>(line + 30);
  const int k = (c0.x < u) + (c0.y < u) + (c0.z < u) + (c0.w < u) + (c1.x < u) + (c1.y < u) + (c1.z < u) + (c1.w < u) +
                (c2.x < u) + (c2.y < u) + (c2.z < u) + (c2.w < u);
  if (tail.y >= 0 && k < LINE_SLOTS) {
    pr = line[12 + k];
    const uint32_t w = __float_as_uint(line[24 + (k >> 1)]);
    return tail.x + (int32_t)((k & 1) ? (w >> 16) : (w & 0xffffu));
  }
  // rare: > 12 distinct values in the bucket and u above the first 12, or a line whose ids do not fit 16-bit deltas
  int32_t lo = tail.x, hi = __float_as_int(line[32 + 30]);               // base of the next line (a sentinel line closes the table)
  const int32_t last = (int32_t)(n_items - 1);
  hi = hi > last ? last : hi;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (cdf[(size_t)mid * cdf_stride] < u) lo = mid + 1; else hi = mid;
  }
  lo = lo > last ? last : lo;
  pr = prob[(size_t)lo * prob_stride];
  return lo;
}

// ---------------------------------------------------------------- 32-bit division by a launch constant
// x / d for 32-bit x by ONE 32-bit multiply-high and a correction: with magic = floor(2^32 / d) (d == 1: 2^32 - 1) the
// estimate floor(x * magic / 2^32) is the quotient or one below it (x * magic / 2^32 > x / d - x / 2^32 > x / d - 1).  The
// routing kernel divides four times per element (query of an element, owner of an id, modulo of the uniform draw): the
// 64-bit forms (a 64 x 64 multiply-high is four quarter-rate multiplies, a 64-bit % a ~150-instruction subroutine)
// were most of its time.
struct Div32 {
  uint32_t d, magic;
  __device__ __forceinline__ uint32_t div(uint32_t x) const {
    const uint32_t q = __umulhi(x, magic);
    return (x - q * d >= d) ? q + 1 : q;
  }
  __device__ __forceinline__ uint32_t mod(uint32_t x) const { return x - div(x) * d; }
};
inline Div32 make_div32(uint64_t d) {
  Div32 v;
  v.d = (uint32_t)d;
  v.magic = d <= 1 ? 0xffffffffu : (uint32_t)((1ull << 32) / d);
  return v;
}

// a key of the sharded exchange is (query << 32) | local row, negative for an empty slot
__device__ __forceinline__ int64_t key_query(int64_t k) { return (k >> 32) & 0x7fffffffll; }
__device__ __forceinline__ int64_t key_row(int64_t k) { return k & 0xffffffffll; }

// ---------------------------------------------------------------- wave helpers
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {   // all lanes of each WIDTH-group get the sum
#pragma unroll
  for (int m = WIDTH / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  return __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, a.x * b.x)));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// Inverse CDF of the popularity sampler for a draw u, by the best structure the caller supplied (P: any parameter
// struct with the fields table, pop_prob, table_prob, lut, lines, guide, n_items, guide_log2, lines_log2): bucket lines
// (one HBM line), direct-lookup table (+ one 4-wide probe), or the guide table + binary search.  All return
// torch.searchsorted(table, u) clamped to n_items-1 and the id's probability.
template <typename P>
__device__ __forceinline__ int32_t lookup_popular(const P& p, float u, float& pr) {
  if (p.lines != nullptr) {
    if (p.table_prob) return cdf_lookup_line(p.lines, p.lines_log2, p.table_prob, 2, p.table_prob + 1, 2, p.n_items, u, pr);
    return cdf_lookup_line(p.lines, p.lines_log2, p.table, 1, p.pop_prob, 1, p.n_items, u, pr);
  }
  if (p.lut != nullptr) {   // direct lookup: one round trip for id AND probability in the common case
    if (p.table_prob)
      return cdf_lookup_lut<2>(reinterpret_cast<const float4*>(p.lut), p.table_prob, p.table_prob + 1, 2, p.n_items,
                               p.guide_log2, u, pr);
    return cdf_lookup_lut<1>(reinterpret_cast<const float4*>(p.lut), p.table, p.pop_prob, 1, p.n_items, p.guide_log2, u, pr);
  }
  int32_t id;
  if (p.table_prob) {       // interleaved {cdf, prob}: the search and the probability share cache lines
    id = cdf_lower_bound<2>(p.table_prob, p.guide, p.n_items, p.guide_log2, u);
    pr = p.table_prob[2 * (size_t)id + 1];
  } else {
    id = cdf_lower_bound<1>(p.table, p.guide, p.n_items, p.guide_log2, u);
    pr = p.pop_prob[id];
  }
  return id;
}

// loss = mean of the per-query losses, in the SAME launch, with ONE device-scope atomic per workgroup and no
// second phase: every workgroup adds {its share of the mean as a 2^-34 fixed-point integer, 1 arrival} to one 64-bit
// word (bits 0..55 sum, bits 56..63 arrivals); integer addition is associative, so the total is bit-reproducible
// whatever the arrival order.  The workgroup whose add returns gridDim.x - 1 earlier arrivals holds the complete sum
// (returned value + its own share), writes the mean and resets the word.  A NaN / inf partial (SampledSoftmax with a
// padded positive, loss_func.py:88-89) first sets a sticky flag word with a RETURNING atomic and only then arrives
// (the arrival is made to depend on the returned value), and the last workgroup reads the flags through a pointer
// that depends on its own returned arrival count -- so the flag is visible whenever the arrival is.  No fences: a
// release / acquire pair at workgroup exit writes back / invalidates the whole XCD L2 (measured: +90 us per launch);
// the first version exchanged float partials and counted arrivals with a second, dependent atomic -- two memory
// round trips in every workgroup's tail, 7.5 us of a 43 us launch at B = 4096.
// The words hold each workgroup's share of the MEAN (its loss sum / n_queries) at 2^-34 resolution, so the range does
// not depend on the batch size.  A share at or above LOSS_SHARE_CAP = 2^10 - 2^-35 (or NaN / inf) saturates to +inf / NaN
// through the flag word; every other share rounds to an integer below 2^44, and LOSS_MAX_GRID = 4096 of them (the
// largest grid of any caller: static_asserts at the launch sites) total less than 2^56, so the 56-bit sum field cannot
// carry into the arrival count: the result is the mean (any mean below 2^10 * grid whose shares stay under the cap; a
// mean below 2^11 needs two workgroups with about half each), or +inf / NaN, never another finite number, and the
// words are zero after every launch.  Quantisation: every share is rounded to nearest, <= grid * 2^-35 absolute
// (6e-8 at 2048 workgroups, before the one fp32 rounding of the result).  The 8-bit count holds the <= 128 members of
// a sub-word and the <= 32 sub-words of the top word.  The first layout (2^-38 resolution, count at bit 50) held totals
// below 2^12 only: a mean in [2^12, 2^10 * grid) with every share under the cap carried into the count, one workgroup
// took itself for the last an arrival early, wrote a wrong finite loss, and the true last arrival left its {1, sum}
// in the scratch for the next launch.  Totals must be >= 0 (every loss on this path is).
// Two levels: workgroup b adds to sub-word b % 32 (the sub-words sit in different 128-byte lines), and the workgroup
// that completes a sub-word forwards its total to the top word -- atomics on ONE address are performed one after the
// other at the memory side (~8 ns each), and at B = 4096 all 1024 workgroups finish together: a single word cost an
// 8 us tail on a 37 us launch.
constexpr int LOSS_FRAC_BITS = 34, LOSS_COUNT_SHIFT = 56, LOSS_SUBWORDS = 32;
constexpr int LOSS_SHARE_BITS = 10;                  // a share below 2^10 - 2^-35 is added, anything else saturates
constexpr int LOSS_MAX_GRID = SCRATCH_MAX_GRID;      // the largest grid a caller of reduce_mean_loss may launch
constexpr double LOSS_SHARE_CAP = (double)(1 << LOSS_SHARE_BITS) - 1.0 / (double)(1ll << (LOSS_FRAC_BITS + 1));
constexpr int loss_log2_ceil(long long v) { return v <= 1 ? 0 : 1 + loss_log2_ceil((v + 1) / 2); }
static_assert(LOSS_FRAC_BITS + LOSS_SHARE_BITS + loss_log2_ceil(LOSS_MAX_GRID) <= LOSS_COUNT_SHIFT,
              "reduce_mean_loss: LOSS_MAX_GRID capped shares must not carry out of the sum field");
static_assert((LOSS_MAX_GRID + LOSS_SUBWORDS - 1) / LOSS_SUBWORDS < (1 << (64 - LOSS_COUNT_SHIFT)) &&
                  LOSS_SUBWORDS < (1 << (64 - LOSS_COUNT_SHIFT)),
              "reduce_mean_loss: the arrival count of a sub-word / of the top word must fit above the sum field");
__device__ __forceinline__ void reduce_mean_loss(float wave_loss, float* __restrict__ loss_out,
                                                 unsigned int* __restrict__ flag_word,
                                                 float* __restrict__ loss_partials, int64_t n_queries) {
  __shared__ float s_red[16];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  if (lane == 0) s_red[wave] = wave_loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float part = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) part += s_red[w];
    unsigned long long* words = reinterpret_cast<unsigned long long*>(loss_partials);     // 8-byte aligned (offset 256)
    constexpr unsigned long long FIELD = (1ull << LOSS_COUNT_SHIFT) - 1, ONE = 1ull << LOSS_COUNT_SHIFT;
    const double share = (double)part / (double)n_queries;       // this workgroup's share of the mean
    const bool bad = !(fabs(share) < LOSS_SHARE_CAP);            // NaN, inf or out of the fixed-point range
    const long long fixed = bad ? 0ll : __double2ll_rn(share * (double)(1ll << LOSS_FRAC_BITS));
    unsigned long long add = ((unsigned long long)fixed & FIELD) + ONE;
    if (bad) {
      const unsigned int old = __hip_atomic_fetch_or(flag_word, part != part ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("; the arrival waits for the flag" : "+v"(add) : "v"(old));
    }
    const unsigned j = blockIdx.x % LOSS_SUBWORDS;
    const unsigned members = (gridDim.x - j + LOSS_SUBWORDS - 1) / LOSS_SUBWORDS;
    const unsigned n_sub = gridDim.x < LOSS_SUBWORDS ? gridDim.x : LOSS_SUBWORDS;
    unsigned long long* sub = words + 16 * (1 + j);      // 128 bytes apart; words[0] is the top word
    const unsigned long long prev = __hip_atomic_fetch_add(sub, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((prev >> LOSS_COUNT_SHIFT) == (unsigned long long)(members - 1)) {
      const unsigned long long sub_total = (prev + add) & FIELD;
      __hip_atomic_store(sub, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // leave the scratch zeroed
      const unsigned long long add2 = sub_total + ONE;
      const unsigned long long prev2 = __hip_atomic_fetch_add(words, add2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((prev2 >> LOSS_COUNT_SHIFT) == (unsigned long long)(n_sub - 1)) {
        const unsigned long long total = (prev2 + add2) & FIELD;
        float loss = (float)((double)total / (double)(1ll << LOSS_FRAC_BITS));
        unsigned int* fw = flag_word;
        asm volatile("; the flags are read after the last arrival" : "+v"(fw) : "v"(prev2));
        const unsigned int flags = __hip_atomic_load(fw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (flags & 1u) loss = NAN;
        else if (flags & 2u) loss = INFINITY;
        loss_out[0] = loss;
        __hip_atomic_store(words, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (flags) __hip_atomic_store(fw, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

}  // namespace rsa
